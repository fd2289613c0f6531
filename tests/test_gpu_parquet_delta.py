"""Delta-encoded pages decoded on the device (PH_PARQUET_DELTA). Every array of the table ph_table_create_parquet_ex builds from the files of
tests/delta_cases.py against the table ph_table_create_arrow builds over pq.read_table of the same file (the comparison of
tests/test_gpu_parquet_load.py), and against the same rows written PLAIN and loaded at flags 0; ph_delta_decode over every crafted and
refused stream in one call against the host twin, with canaries around the destinations; overrides, refusals and one-byte patches (the
host twin's code and message, no table, the context usable afterwards); TPC-H lineitem at SF0.01 written with delta encodings."""
import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
pq = pytest.importorskip("pyarrow.parquet")

import delta_cases as D  # noqa: E402
import oracle_lib as O  # noqa: E402
from test_gpu_parquet_load import assert_tables_equal  # noqa: E402
from plan_amd import hip, loader, queries, tpch  # noqa: E402

pytestmark = pytest.mark.gpu

OK, EINVAL, EUNSUPPORTED, EOVERFLOW, ECAPACITY = hip.PH_OK, hip.PH_EINVAL, hip.PH_EUNSUPPORTED, hip.PH_EOVERFLOW, hip.PH_ECAPACITY
DELTA, SNAPPY = hip.PH_PARQUET_DELTA, hip.PH_PARQUET_SNAPPY
CANARY = 3            # values between two destinations of the raw decoder


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("delta_cases")


@pytest.fixture(scope="module")
def cases(files):
    return D.generate(files)


def pages_of(data, column):
    return loader.parquet_pages(data, column)


def load_and_compare(ctx, path, flags, columns=None):
    tbl = pq.read_table(path)
    names = list(columns) if columns is not None else tbl.column_names
    arrow = pa.Table.from_arrays([tbl.column(c) for c in names], names=["c%d" % i for i in range(len(names))])
    t = loader.table_from_parquet_device(ctx, path, columns, flags=flags)
    ref = loader.table_from_arrow_c(ctx, arrow)
    try:
        assert t.column_names == names
        assert_tables_equal(ctx, t, ref, tbl.num_rows)
        return [(t.col(k).type, len(t.dicts[k]), bool(t.col(k).validity)) for k in range(t.ncols)]
    finally:
        t.free()
        ref.free()


def compare_with_the_plain_file(ctx, files, name, case, flags):
    plain = D.plain_twin(files, name, case.table)
    assert {p["encoding"] for k in range(case.table.num_columns) for p in pages_of(plain.data, k)} == {0}
    t = loader.table_from_parquet_device(ctx, case.path, flags=flags)
    u = loader.table_from_parquet_device(ctx, plain.path)
    try:
        assert_tables_equal(ctx, t, u, case.table.num_rows)
        return t.column_names, [(t.col(k).type, len(t.dicts[k]), bool(t.col(k).validity)) for k in range(t.ncols)]
    finally:
        t.free()
        u.free()


# a value with a NUL byte stays offsets + bytes here and is cut by the Arrow route (tests/test_gpu_parquet_load.py): that file is compared with
# its PLAIN twin only
ARROW_ROUTE = [n for n in D.CASE_NAMES if n != "strings_nul_byte"]


@pytest.mark.parametrize("name", ARROW_ROUTE)
def test_delta_file_equals_the_arrow_route(ctx, cases, name):
    if name not in cases:
        pytest.skip("this pyarrow has no Snappy codec to write the file with")
    c, more = cases[name]
    kinds = dict(zip(c.table.column_names, load_and_compare(ctx, c.path, DELTA | more)))
    if name.startswith("matrix") or name.startswith("dictionary"):
        assert kinds["s300_n"][0] == kinds["s300_r"][0] == hip.PH_STR and kinds["s40_n"][:2] == kinds["s40_r"][:2] == (hip.PH_CODE8, 40)
        assert all(kinds[n][2] == n.endswith("_n") for n in kinds)
    want = {"strings_256_nulls": (hip.PH_CODE8, 256, True), "strings_256_empty_nulls": (hip.PH_STR, 0, True), "strings_257": (hip.PH_STR, 0, False),
            "strings_empty": (hip.PH_CODE8, 2, True), "strings_long": (hip.PH_STR, 0, True), "strings_all_null": (hip.PH_CODE8, 0, True),
            "strings_one_value": (hip.PH_CODE8, 1, False)}
    if name in want:
        assert kinds["s"] == want[name]
    if name == "count_0_nullable":
        assert kinds == {"i32": (hip.PH_I32, 0, True), "i64": (hip.PH_I64, 0, True), "s": (hip.PH_CODE8, 0, True)}


@pytest.mark.parametrize("name", ["matrix_v1", "matrix_pages37_v2", "matrix_3groups_snappy", "widths_v1", "widths_v2_pages37", "count_513_nullable", "count_257_required",
                                  "strings_nul_byte", "strings_long", "strings_257"])
def test_delta_file_equals_the_plain_file_at_flags_0(ctx, cases, files, name):
    if name not in cases:
        pytest.skip("this pyarrow has no Snappy codec to write the file with")
    c, more = cases[name]
    names, kinds = compare_with_the_plain_file(ctx, files, name, c, DELTA | more)
    if name == "strings_nul_byte":
        assert kinds[names.index("s")][0] == hip.PH_STR and kinds[names.index("t")][:2] == (hip.PH_CODE8, 3)


def test_selection_and_bytes_as_the_source(ctx, cases):
    c, _m = cases["matrix_pages37_v1"]
    load_and_compare(ctx, c.path, DELTA, ["s40_n", "d15_r", "i32_n", "s40_n", "date_n"])
    t = loader.table_from_parquet_device(ctx, c.data, ["i64_r"], flags=DELTA)
    try:
        assert np.array_equal(ctx.download(hip.vp(t.col(0).data), np.int64, c.table.num_rows), c.table.column("i64_r").to_numpy())
    finally:
        t.free()


def test_overrides(ctx, cases):
    c, _m = cases["overrides"]
    data, names = c.data, c.table.column_names
    types = {"i32": (hip.PH_I64, 0), "small64": (hip.PH_I32, 0), "small64_n": (hip.PH_DEC64, 3)}
    t = loader.table_from_parquet_device(ctx, c.path, ["i32", "small64", "small64_n", "big64"], types=types, flags=DELTA)
    try:
        n = c.table.num_rows
        assert [(t.col(k).type, t.col(k).scale) for k in range(4)] == [(hip.PH_I64, 0), (hip.PH_I32, 0), (hip.PH_DEC64, 3), (hip.PH_I64, 0)]
        for k, (col, typ) in enumerate((("i32", hip.PH_I64), ("small64", hip.PH_I32), ("small64_n", hip.PH_DEC64), ("big64", 0))):
            want, _valid, _o, _b = hip.parquet_read_column_host(data, names.index(col), typ, 3 if typ == hip.PH_DEC64 else 0, flags=DELTA)
            got = ctx.download(hip.vp(t.col(k).data), hip.NP_TYPES[t.col(k).type], n)
            assert np.array_equal(got.astype(np.int64), want), col
    finally:
        t.free()
    with pytest.raises(hip.PlanHipError) as e:
        loader.table_from_parquet_device(ctx, c.path, ["big64"], types={"big64": (hip.PH_I32, 0)}, flags=DELTA)
    with pytest.raises(hip.PlanHipError) as h:
        hip.parquet_read_column_host(data, names.index("big64"), hip.PH_I32, 0, flags=DELTA)
    assert e.value.code == EOVERFLOW and str(e.value).split(": ", 2)[2] == str(h.value).split(": ", 2)[2]
    load_and_compare(ctx, c.path, DELTA)


# ---------------------------------------------------------------- raw streams

def test_raw_streams_in_one_call_equal_the_host_twin(ctx):
    valid, invalid = D.valid_streams(), D.invalid_streams()
    jobs = [(name, stream, bits, -1, True) for name, stream, bits in valid]
    jobs += [(name, stream, bits, -1 if expected is None else expected, True) for name, stream, bits, expected, _w, _u in invalid]
    jobs += [(name + "_with_a_tail", stream + b"\x55\xaa\x55", bits, -1, False) for name, stream, bits in valid[:6]]
    jobs.append(("room_one_short", valid[0][1], 64, -1, True))
    room = [len(D.decode(stream, bits)[0]) if k < len(valid) or k >= len(valid) + len(invalid) else 700 for k, (_n, stream, bits, _e, _x) in enumerate(jobs)]
    room[-1] -= 1
    got, whole, pos = hip.delta_decode(ctx, [(stream, bits, expected, exact, r) for (_n, stream, bits, expected, exact), r in zip(jobs, room)], canary=CANARY)
    mask = np.ones(len(whole), bool)
    for (status, vals, count, _c), p in zip(got, pos):
        if status == OK:
            mask[p:p + count] = False
    for k, ((name, stream, bits, expected, exact), (status, vals, count, consumed)) in enumerate(zip(jobs, got)):
        s = hip.DeltaStream(0, len(stream), bits, int(exact), expected, 0, room[k], 0, 0, 0, 0)
        out = np.zeros(max(room[k], 1), np.int64)
        rc = hip.lib().ph_delta_decode_host(bytes(stream), hip.vp(out.ctypes.data), hip.ctypes.byref(s))
        assert (status, count, consumed) == (rc, s.count, s.consumed), name
        if rc == OK:
            assert vals.tolist() == out[:count].tolist() == D.decode(stream, bits)[0], name
    assert [g[0] for g in got[:len(valid)]] == [OK] * len(valid)
    assert [g[0] for g in got[len(valid):len(valid) + len(invalid)]] == [EUNSUPPORTED if u else EINVAL for *_r, u in invalid]
    assert [g[0] for g in got[len(valid) + len(invalid):]] == [OK] * 6 + [ECAPACITY]
    # nothing is written outside the destinations of the streams that decoded; a refused stream writes inside its own room at most
    for (status, _v, _c, _u), p, r in zip(got, pos, room):
        if status != OK:
            mask[p:p + r] = False
    assert (whole[mask] == hip.DELTA_CANARY).all(), "values outside the destinations were written"
    assert hip.delta_decode(ctx, [])[0] == []


# ---------------------------------------------------------------- refusals

def test_refusals_and_patches_leave_the_context_usable(ctx, cases, files):
    good, _m = cases["count_65_nullable"]

    def refused(data, code, flags, word, columns=None):
        with pytest.raises(hip.PlanHipError) as e:
            loader.table_from_parquet_device(ctx, data, columns, flags=flags)
        assert e.value.code == code and word in str(e.value), str(e.value)
        return str(e.value)
    refused(good.data, EUNSUPPORTED, 0, "DELTA_BINARY_PACKED values; PLAIN and RLE_DICTIONARY only")       # without the flag: as before
    refused(good.data, EUNSUPPORTED, SNAPPY, "DELTA_BINARY_PACKED values; PLAIN and RLE_DICTIONARY only")
    for flags in (2, 3, 6, 7, 8):
        assert "PH_PARQUET_DELTA" in refused(good.data, EINVAL, flags, "flags")
    for name, (path, col, enc) in D.unsupported_files(files).items():
        refused(open(path, "rb").read(), EUNSUPPORTED, DELTA, enc + " values", [col])
    for name, (orig, bad, column, page) in D.patched(files, pages_of).items():
        msg = refused(bad, EINVAL, DELTA, "row group 0, page %d:" % page)
        assert "column %d (" % column in msg, (name, msg)
        with pytest.raises(hip.PlanHipError) as h:
            hip.parquet_read_column_host(bad, column, flags=DELTA)
        assert msg.split(": ", 2)[2] == str(h.value).split(": ", 2)[2], name      # the host twin says the same behind its own name
        t = loader.table_from_parquet_device(ctx, orig, flags=DELTA)              # the file the patch started from loads, on the same context
        t.free()
    both, _column = D.two_bad_pages(files, pages_of)
    assert "page 1:" in refused(both, EINVAL, DELTA, "fewer or more values")
    load_and_compare(ctx, good.path, DELTA)


# ---------------------------------------------------------------- TPC-H lineitem at SF0.01 written with delta encodings

def arrow_of(name, src):
    """the generator's columns as the Arrow table a Parquet writer gets (tests/test_gpu_parquet_snappy.py)"""
    import decimal
    arrays, names = [], []
    for cname, typ, scale, dic in tpch.SCHEMA[name]:
        if typ == hip.PH_STR:
            if cname + "_off" not in src:
                arr = pa.array(["x%d" % (i % 300) for i in range(len(src[tpch.SCHEMA[name][0][0]]))], pa.string())
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
def lineitem_files(sf001, files):
    table = arrow_of("lineitem", sf001["lineitem"])
    # (the resident lineitem carries no l_comment: a text column of dbgen's length range stands in for it, and is compared as a column)
    rng = np.random.default_rng(17)
    words = ["furiously", "regular", "deposits", "sleep", "quickly", "ironic", "packages", "along", "the", "blithely", "final", "accounts"]
    comment = [" ".join(words[j] for j in rng.integers(0, len(words), int(k)))[:43] for k in rng.integers(2, 8, table.num_rows)]
    table = table.append_column("l_comment", pa.array(comment, pa.string()))
    strings = [f.name for f in table.schema if pa.types.is_string(f.type)]
    flags = [n for n in strings if n != "l_comment"]                       # dictionary pages for the low-cardinality strings
    enc = {f.name: "DELTA_BINARY_PACKED" for f in table.schema if f.name not in strings}
    enc["l_comment"] = "DELTA_LENGTH_BYTE_ARRAY"
    out = {}
    for kind, kw in (("plain", dict(use_dictionary=flags)), ("delta", dict(use_dictionary=flags, column_encoding=enc)),
                     ("delta_snappy", dict(use_dictionary=flags, column_encoding=enc, compression="SNAPPY"))):
        if kind.endswith("snappy") and not pa.Codec.is_available("snappy"):
            continue
        path = str(files / ("lineitem_%s.parquet" % kind))
        kw.setdefault("compression", "NONE")
        pq.write_table(table, path, store_decimal_as_integer=True, row_group_size=25000, data_page_size=64 << 10, **kw)
        out[kind] = path
    return out


def q1_and_q6(ctx, db, path, flags):
    """both results as text, and Q1's rows"""
    p = tpch.q1_plan(db)
    p.run()
    r = p.fetch()
    p.free()
    n = r["ngroups"]
    q1 = (n, [tuple(k) for k in r["keys"][:n]], [list(s) for s in r["sum"][:n]], [list(c) for c in r["count"][:n]])
    t = loader.table_from_parquet_device(ctx, path, ["l_quantity", "l_extendedprice", "l_discount", "l_tax", "l_returnflag", "l_linestatus", "l_shipdate"], flags=flags)
    try:
        p = queries.q6_plan(ctx, t)
        p.run()
        r6 = p.fetch()
        p.free()
    finally:
        t.free()
    return repr(q1) + "\n" + repr(r6["sum"][0][0]), q1, r6["sum"][0][0]


def test_q1_and_q6_over_delta_lineitem_equal_the_plain_file_and_the_oracle(ctx, lineitem_files, sf001):
    encs = {c: {p["encoding"] for p in pages_of(open(lineitem_files["delta"], "rb").read(), c) if p["kind"] != 2}
            for c in ("l_orderkey", "l_shipdate", "l_extendedprice", "l_comment", "l_returnflag")}
    assert encs == {"l_orderkey": {5}, "l_shipdate": {5}, "l_extendedprice": {5}, "l_comment": {6}, "l_returnflag": {8}}
    texts = {}
    for kind, path in lineitem_files.items():
        flags = 0 if kind == "plain" else DELTA | (SNAPPY if kind.endswith("snappy") else 0)
        db = tpch.Database.from_parquet(ctx, {"lineitem": path}, flags=flags)
        try:
            if kind != "plain":
                plain = tpch.Database.from_parquet(ctx, {"lineitem": lineitem_files["plain"]})
                try:
                    assert_tables_equal(ctx, db.t("lineitem"), plain.t("lineitem"), len(sf001["lineitem"]["l_quantity"]))
                finally:
                    plain.free()
                t = loader.table_from_parquet_device(ctx, path, ["l_comment", "l_orderkey"], flags=flags)
                u = loader.table_from_parquet_device(ctx, lineitem_files["plain"], ["l_comment", "l_orderkey"])
                try:
                    assert_tables_equal(ctx, t, u, t.nrows)
                    assert t.col(0).type == hip.PH_STR
                finally:
                    t.free()
                    u.free()
            texts[kind], q1, q6 = q1_and_q6(ctx, db, path, flags)
        finally:
            db.free()
    assert all(t == texts["plain"] for t in texts.values()) and len(texts) >= 2
    want = O.q1(sf001["lineitem"], queries.q1_shipdate_cutoff())
    assert q1[0] == len(want) == 4
    for g, w in enumerate(want):
        assert q1[1][g] == (w.returnflag, w.linestatus) and q1[2][g][0] == w.sum_qty.value() and q1[2][g][1] == w.sum_base_price.unscaled(2)
        assert q1[2][g][3] == w.sum_charge.unscaled(6) and q1[3][g][7] == w.count_order
    rc, d = O.q6(sf001["lineitem"], *queries.q6_constants())
    assert rc == 0 and q6 == d.unscaled(4)
    with pytest.raises(hip.PlanHipError) as e:                    # the flag is what lets the file in
        tpch.Database.from_parquet(ctx, {"lineitem": lineitem_files["delta"]})
    assert e.value.code == EUNSUPPORTED and "DELTA_BINARY_PACKED" in str(e.value)
