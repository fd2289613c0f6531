"""ph_table_create_parquet on the device: every array of the loaded table against the table ph_table_create_arrow builds over
pq.read_table of the same file and columns, on the same context — type, scale, data with the zeroed padding, presence and bits of the
validity bitmap, dictionary, offsets, bytes, min / max, order and run statistics, narrowed copies. The files are tests/parquet_cases.py's
(the CPU tests pin the host twin on the same ones). Then overrides against the host twin, column selection, every refusal and malformed
file (same code, no table, the context usable afterwards), and TPC-H at SF0.01 written as Parquet."""
import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
pq = pytest.importorskip("pyarrow.parquet")

import oracle_lib as O  # noqa: E402
import parquet_cases as C  # noqa: E402
from plan_amd import hip, loader, queries, tpch, tpchgen  # noqa: E402

pytestmark = pytest.mark.gpu

ROW_PAD = C.ROW_PAD
OK, EINVAL, EUNSUPPORTED, EOVERFLOW = hip.PH_OK, hip.PH_EINVAL, hip.PH_EUNSUPPORTED, hip.PH_EOVERFLOW


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("parquet_cases")


@pytest.fixture(scope="module")
def cases(files):
    return C.generate(files)


def pages_of(data, column):
    return loader.parquet_pages(data, column)


def outcome(f, *a):
    """the call's value, or the code it refuses with (a VARCHAR column has no range statistics, in either table)"""
    try:
        return f(*a)
    except hip.PlanHipError as e:
        return ("refused", e.code)


def assert_tables_equal(ctx, t, ref, n):
    """every device array of t against ref's (the Arrow route's)"""
    assert t.nrows == ref.nrows == n and t.ncols == ref.ncols
    padded = (n + ROW_PAD - 1) // ROW_PAD * ROW_PAD
    for k in range(t.ncols):
        a, b = t.col(k), ref.col(k)
        assert (a.type, a.scale) == (b.type, b.scale), k
        assert t.dicts[k] == ref.dicts[k], k
        if n == 0:
            continue
        assert bool(a.validity) == bool(b.validity), k
        if a.validity:
            assert ctx.download(hip.vp(a.validity), np.uint8, padded // 8).tobytes() == ctx.download(hip.vp(b.validity), np.uint8, padded // 8).tobytes(), k
        if a.type == hip.PH_STR:
            oa, ob = ctx.download(hip.vp(a.data), np.int32, n + 1), ctx.download(hip.vp(b.data), np.int32, n + 1)
            assert np.array_equal(oa, ob) and a.aux_bytes == b.aux_bytes == oa[n], k
            if a.aux_bytes:
                assert ctx.download(hip.vp(a.aux), np.uint8, int(a.aux_bytes)).tobytes() == ctx.download(hip.vp(b.aux), np.uint8, int(b.aux_bytes)).tobytes(), k
        else:
            dt = hip.NP_TYPES[a.type]
            assert ctx.download(hip.vp(a.data), dt, padded).tobytes() == ctx.download(hip.vp(b.data), dt, padded).tobytes(), k
        assert outcome(hip.table_col_range_of, t, k) == outcome(hip.table_col_range_of, ref, k), k
        assert outcome(hip.table_col_stats, t, k) == outcome(hip.table_col_stats, ref, k), k
        assert outcome(t.col_run_len, k) == outcome(ref.col_run_len, k), k
        assert outcome(t.col_narrow, k) == outcome(ref.col_narrow, k), k
    assert t.narrow_bytes() == ref.narrow_bytes()


def load_and_compare(ctx, path, columns=None, source=None):
    """columns: names in the order wanted (a name may repeat)"""
    tbl = pq.read_table(path)
    names = list(columns) if columns is not None else tbl.column_names
    as_text = lambda col: col.combine_chunks().view(pa.string()) if pa.types.is_binary(col.type) else col  # noqa: E731  (the Arrow route takes utf8 only)
    arrow = pa.Table.from_arrays([as_text(tbl.column(c)) for c in names], names=["c%d" % i for i in range(len(names))])
    t = loader.table_from_parquet_device(ctx, path if source is None else source, columns)
    ref = loader.table_from_arrow_c(ctx, arrow)
    try:
        assert t.column_names == names
        assert_tables_equal(ctx, t, ref, tbl.num_rows)
        return [(t.col(k).type, len(t.dicts[k]), bool(t.col(k).validity)) for k in range(t.ncols)]
    finally:
        t.free()
        ref.free()


MATRIX = ["matrix_v1", "matrix_v2", "matrix_pages13", "matrix_pages37_v2", "matrix_pages37_v1_plain", "matrix_plain_v2", "matrix_decint_3groups",
          "matrix_3groups_pages37", "matrix_fallback", "matrix_fallback_v2_3groups", "matrix_dict_some"]


@pytest.mark.parametrize("name", MATRIX)
def test_matrix_equals_the_arrow_route(ctx, cases, name):
    kinds = load_and_compare(ctx, cases[name].path)
    names = cases[name].table.column_names
    by = dict(zip(names, kinds))
    assert by["s300_n"][0] == by["s300_r"][0] == hip.PH_STR and by["s40_n"][:2] == by["s40_r"][:2] == (hip.PH_CODE8, 40)
    assert all(by[n][2] == n.endswith("_n") for n in names)        # a bitmap exactly where NULLs are


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 63, 64, 65, ROW_PAD - 1, ROW_PAD + 1])
def test_small_row_counts(ctx, cases, n):
    c = cases["rows_%d" % n]
    load_and_compare(ctx, c.path)
    load_and_compare(ctx, c.path, source=c.data)                    # bytes instead of a path


@pytest.mark.parametrize("name", ["nulls_v1", "nulls_v2_plain"])
def test_null_patterns(ctx, cases, name):
    kinds = dict(zip(cases[name].table.column_names, load_and_compare(ctx, cases[name].path)))
    assert kinds["all_null"][2] and not kinds["none_null"][2] and kinds["last_page"][2] and kinds["rle_then_alt"][2]
    assert kinds["s_all_null"] == (hip.PH_CODE8, 0, True) and kinds["s_none_null"] == (hip.PH_CODE8, 50, False) and kinds["s_alt"] == (hip.PH_CODE8, 50, True)


@pytest.mark.parametrize("name", ["dict_widths", "dict_widths_pages37_v2", "dict_width17"])
def test_dictionary_index_widths(ctx, cases, name):
    load_and_compare(ctx, cases[name].path)


@pytest.mark.parametrize("plain", ["", "_plain"])
@pytest.mark.parametrize("kind,want", [("256_nulls", (hip.PH_CODE8, 256, True)), ("256_empty_nulls", (hip.PH_STR, 0, True)), ("257", (hip.PH_STR, 0, False)),
                                       ("empty", (hip.PH_CODE8, 2, True)), ("long", (hip.PH_STR, 0, True)), ("straddle", (hip.PH_CODE8, 17, True))])
def test_varchar_encodings(ctx, cases, kind, want, plain):
    kinds = load_and_compare(ctx, cases["varchar_" + kind + plain].path)
    assert kinds[0] == want


@pytest.mark.parametrize("plain", ["", "_plain"])
def test_varchar_value_with_a_nul_byte_stays_offsets_and_bytes(ctx, cases, plain):
    """The text path's rule (a dictionary entry is a C string). ph_table_create_arrow has no such rule — it cuts the entry at the NUL — so
    this column is compared with pyarrow's values themselves; the column beside it with the Arrow route as everywhere else."""
    c = cases["varchar_nul_byte" + plain]
    load_and_compare(ctx, c.path, ["t"])
    _v, valid, strs = C.expected_column(pq.read_table(c.path).column("s"))
    t = loader.table_from_parquet_device(ctx, c.path, ["s"])
    try:
        col, n = t.col(0), len(strs)
        assert col.type == hip.PH_STR and t.dicts[0] == []
        off = ctx.download(hip.vp(col.data), np.int32, n + 1)
        byts = ctx.download(hip.vp(col.aux), np.uint8, int(col.aux_bytes)).tobytes()
        assert [byts[off[i]:off[i + 1]] for i in range(n)] == strs and b"\0" in byts
        bits = np.unpackbits(ctx.download(hip.vp(col.validity), np.uint8, ROW_PAD // 8), bitorder="little")
        assert np.array_equal(bits[:n].astype(bool), valid) and not bits[n:].any()
    finally:
        t.free()


def test_unannotated_byte_array_is_varchar(ctx, cases):
    assert load_and_compare(ctx, cases["binary"].path)[0] == (hip.PH_CODE8, 3, True)


def test_column_selection_and_order(ctx, cases):
    path = cases["matrix_3groups_pages37"].path
    load_and_compare(ctx, path, ["s40_n", "d15_r", "i32_n"])
    load_and_compare(ctx, path, ["i64_n", "s300_n", "i64_n", "s300_n"])
    with pytest.raises(KeyError):
        loader.table_from_parquet_device(ctx, path, ["nope"])
    # only the requested columns are judged: the INT32 column beside a DOUBLE and a list
    refused = C.refusals(cases["matrix_v1"].path.rsplit("/", 1)[0])
    load_and_compare(ctx, refused["double"][0], ["i", "s"])


def test_overrides_equal_the_host_twin(ctx, cases):
    c = cases["matrix_decint_3groups"]
    names = c.table.column_names
    data = c.data
    n = c.table.num_rows
    padded = (n + ROW_PAD - 1) // ROW_PAD * ROW_PAD
    wanted = [("i32_n", hip.PH_I64, 0), ("i32_r", hip.PH_DEC64, 3), ("i64_n", hip.PH_DEC64, 18), ("i64_r", hip.PH_I64, 0), ("d15_n", hip.PH_DEC64, 2)]
    t = loader.table_from_parquet_device(ctx, data, [w[0] for w in wanted], {w[0]: (w[1], w[2]) for w in wanted})
    try:
        for k, (cname, typ, scale) in enumerate(wanted):
            col = t.col(k)
            assert (col.type, col.scale) == (typ, scale), cname
            v, valid, _o, _b = hip.parquet_read_column_host(data, names.index(cname), typ, scale)
            got = ctx.download(hip.vp(col.data), hip.NP_TYPES[typ], padded)
            assert np.array_equal(got[:n].astype(np.int64), v) and not got[n:].any(), cname
            assert bool(col.validity) == (not valid.all())
            if col.validity:
                bits = np.unpackbits(ctx.download(hip.vp(col.validity), np.uint8, padded // 8), bitorder="little")
                assert np.array_equal(bits[:n].astype(bool), valid) and not bits[n:].any()
    finally:
        t.free()
    # PH_I32 over INT64: narrows when the values fit, PH_EOVERFLOW naming the column when they do not
    small = cases["dict_widths"]
    t = loader.table_from_parquet_device(ctx, small.path, ["d2"], {"d2": (hip.PH_I32, 0)})
    try:
        got = ctx.download(hip.vp(t.col(0).data), np.int32, small.table.num_rows)
        assert t.col(0).type == hip.PH_I32 and np.array_equal(got.astype(np.int64), C.expected_column(small.table.column("d2"))[0])
    finally:
        t.free()
    with pytest.raises(hip.PlanHipError) as e:
        loader.table_from_parquet_device(ctx, data, ["i32_n", "i64_r"], {"i64_r": (hip.PH_I32, 0)})
    assert e.value.code == EOVERFLOW and "i64_r" in str(e.value)
    for cname, typ, scale in [("i32_n", hip.PH_DATE, 0), ("i32_n", hip.PH_DEC64, 19), ("date_n", hip.PH_I32, 0), ("d15_r", hip.PH_I64, 0), ("d15_r", hip.PH_DEC64, 3),
                              ("s40_n", hip.PH_I32, 0), ("i64_r", 99, 0)]:
        with pytest.raises(hip.PlanHipError) as e:
            loader.table_from_parquet_device(ctx, data, [cname], {cname: (typ, scale)})
        assert e.value.code == EINVAL and cname in str(e.value)
    load_and_compare(ctx, c.path, ["i32_n"])


def test_refusals_and_malformed_files_leave_the_context_usable(ctx, cases, files):
    good = cases["rows_65"]

    def refused(data, code, columns=None, word=None):
        with pytest.raises(hip.PlanHipError) as e:
            loader.table_from_parquet_device(ctx, data, columns)
        assert e.value.code == code, str(e.value)
        if word:
            assert word in str(e.value), str(e.value)
        return str(e.value)
    for name, (path, cname, word) in C.refusals(files).items():
        msg = refused(open(path, "rb").read(), EUNSUPPORTED, [cname], word)
        assert cname in msg, (name, msg)
    refused(open(C.refusals(files)["double"][0], "rb").read(), EUNSUPPORTED)          # every column: the DOUBLE is judged
    for name, bad in C.truncations(cases["matrix_decint_3groups"].data).items():
        refused(bad, EINVAL)
    load_and_compare(ctx, good.path)
    for name, (orig, bad, column) in C.patched(files, pages_of).items():
        msg = refused(bad, EINVAL, word="row group 0, page")
        assert "column %d (" % column in msg, (name, msg)
        t = loader.table_from_parquet_device(ctx, orig)            # the file the patch started from loads, on the same context
        t.free()
    load_and_compare(ctx, good.path)


def test_lowest_failing_page_is_named(ctx, files):
    """two bad pages in one column: the message names the first"""
    src = C.patch_sources(files)["levels"].data
    pages = [p for p in pages_of(src, 0) if p["kind"] == 0]
    assert len(pages) == 3
    bad = bytearray(src)
    for p in pages[1:]:
        bad[p["data_pos"] + 4] = 0x7f if bad[p["data_pos"] + 4] & 1 == 0 else 0xff
    with pytest.raises(hip.PlanHipError) as e:
        loader.table_from_parquet_device(ctx, bytes(bad))
    with pytest.raises(hip.PlanHipError) as h:
        hip.parquet_read_column_host(bytes(bad), 0)
    assert e.value.code == h.value.code == EINVAL and "page 1:" in str(e.value) and "page 1:" in str(h.value)


# ---------------------------------------------------------------- TPC-H at SF0.01 written as Parquet

def arrow_of(name, src):
    """the generator's columns as the Arrow table a Parquet writer gets: DATE date32, DECIMAL decimal128(15, 2), VARCHAR strings"""
    import decimal
    arrays, names = [], []
    for cname, typ, scale, dic in tpch.SCHEMA[name]:
        if typ == hip.PH_STR:
            if cname + "_off" not in src:                     # a column the fixture does not hold: a filler, as in the .tbl test
                arr = pa.array(["x"] * len(src[tpch.SCHEMA[name][0][0]]), pa.string())
            else:
                off, byts = src[cname + "_off"], src[cname + "_bytes"].tobytes()
                arr = pa.array([byts[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)], pa.string())
        elif typ == hip.PH_CODE8:
            arr = pa.array(np.array(dic)[src[cname]].tolist(), pa.string())
        elif typ == hip.PH_DEC64:
            arr = pa.array([decimal.Decimal(int(v)).scaleb(-scale) for v in src[cname].tolist()], pa.decimal128(15, scale))
        elif typ == hip.PH_DATE:
            arr = pa.array(src[cname].astype(np.int32), pa.int32()).cast(pa.date32())
        else:
            arr = pa.array(src[cname])
        arrays.append(arr)
        names.append(cname)
    return pa.Table.from_arrays(arrays, names=names)


@pytest.fixture(scope="module")
def tpch_files(sf001, files):
    out = {}
    for name in ("lineitem", "orders", "customer"):
        path = str(files / (name + ".parquet"))
        pq.write_table(arrow_of(name, sf001[name]), path, compression="NONE", row_group_size=25000, data_page_size=64 << 10)
        out[name] = path
    return out


@pytest.mark.parametrize("name", ["lineitem", "orders", "customer"])
def test_tpch_tables_are_byte_identical_to_the_arrow_route(ctx, tpch_files, name):
    load_and_compare(ctx, tpch_files[name])


def test_q1_over_parquet_loaded_lineitem_equals_the_oracle(ctx, tpch_files, sf001):
    L = sf001["lineitem"]
    names = ["l_quantity", "l_extendedprice", "l_discount", "l_tax", "l_returnflag", "l_linestatus", "l_shipdate"]      # test_loader.py's order
    t = loader.table_from_parquet_device(ctx, tpch_files["lineitem"], names)
    direct = queries.lineitem_table(ctx, L)
    try:
        assert t.dicts[4] == tpchgen.RETURNFLAG_DICT and t.dicts[5] == tpchgen.LINESTATUS_DICT
        p, pd = queries.q1_plan(ctx, t), queries.q1_plan(ctx, direct)
        p.run()
        r = p.fetch()
        want = O.q1(L, queries.q1_shipdate_cutoff())
        assert r["ngroups"] == len(want) == 4
        for g, w in enumerate(want):
            assert tuple(r["keys"][g]) == (w.returnflag, w.linestatus)
            assert r["sum"][g][0] == w.sum_qty.value() and r["sum"][g][1] == w.sum_base_price.unscaled(2)
            assert r["sum"][g][2] == w.sum_disc_price.unscaled(4) and r["sum"][g][3] == w.sum_charge.unscaled(6)
            assert r["count"][g][7] == w.count_order
        assert p.bytes_per_row == pd.bytes_per_row < 34
        assert t.narrow_bytes() == direct.narrow_bytes() > 0
        p.free()
        pd.free()
    finally:
        t.free()
        direct.free()


def test_q3_over_from_parquet_equals_the_generated_database(ctx, tpch_files, sf001):
    db_pq = tpch.Database.from_parquet(ctx, tpch_files)
    db_gen = tpch.Database(ctx, sf001)
    try:
        out = []
        for db in (db_pq, db_gen):
            res = []
            for topk in (10, 0):
                p = tpch.q3_plan(db, topk=topk)
                p.run()
                r = p.fetch()
                p.free()
                groups = [(int(r["keys"][g][0]), r["sum"][g][0], int(r["keys"][g][1]), int(r["keys"][g][2])) for g in range(r["ngroups"])]
                res.append((r["ngroups"], sorted(groups), tpch.q3_top(r)))
            out.append(res)
        assert out[0] == out[1] and out[0][1][0] > 10
    finally:
        db_pq.free()
        db_gen.free()
