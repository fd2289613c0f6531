"""Front-coded pages decoded on the device (DELTA_BYTE_ARRAY, PH_PARQUET_DELTA_BYTE_ARRAY). Every array of the table
ph_table_create_parquet_ex builds from the files of tests/dba_cases.py against the table ph_table_create_arrow builds over pq.read_table of
the same file, and against the same rows written PLAIN and loaded at flags 0; ph_delta_byte_array_decode over every crafted and refused
section in one call against the host twin, with canaries around both destinations; refusals and one-byte patches (the host twin's code and
message, no table, the context usable afterwards); a corrupt front-coded page beside a corrupt compressed one; TPC-H lineitem at SF0.01
with its VARCHAR columns front-coded."""
import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
pq = pytest.importorskip("pyarrow.parquet")

import dba_cases as B  # noqa: E402
import oracle_lib as O  # noqa: E402
from test_gpu_parquet_delta import arrow_of  # noqa: E402
from test_gpu_parquet_load import assert_tables_equal  # noqa: E402
from plan_amd import hip, loader, queries, tpch  # noqa: E402

pytestmark = pytest.mark.gpu

OK, EINVAL, EUNSUPPORTED, ECAPACITY = hip.PH_OK, hip.PH_EINVAL, hip.PH_EUNSUPPORTED, hip.PH_ECAPACITY
DBA, DELTA, SNAPPY = hip.PH_PARQUET_DELTA_BYTE_ARRAY, hip.PH_PARQUET_DELTA, hip.PH_PARQUET_SNAPPY
CANARY = 5            # values / bytes between two destinations of the raw decoder


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("dba_cases")


@pytest.fixture(scope="module")
def cases(files):
    return B.generate(files)


def pages_of(data, column):
    return loader.parquet_pages(data, column)


def kinds_of(t):
    return [(t.col(k).type, len(t.dicts[k]), bool(t.col(k).validity)) for k in range(t.ncols)]


def load_and_compare(ctx, files, name, case, flags, columns=None, arrow_route=True):
    """the front-coded file against the Arrow route over pq.read_table and against its PLAIN twin at flags 0 -> {column: (type, dictionary
    entries, has a bitmap)}"""
    tbl = pq.read_table(case.path)
    names = list(columns) if columns is not None else tbl.column_names
    as_text = lambda col: col.combine_chunks().view(pa.string()) if pa.types.is_binary(col.type) else col  # noqa: E731  (the Arrow route takes utf8 only)
    t = loader.table_from_parquet_device(ctx, case.path, columns, flags=flags)
    try:
        assert t.column_names == names
        if arrow_route:
            ref = loader.table_from_arrow_c(ctx, pa.Table.from_arrays([as_text(tbl.column(c)) for c in names], names=["c%d" % i for i in range(len(names))]))
            try:
                assert_tables_equal(ctx, t, ref, tbl.num_rows)
            finally:
                ref.free()
        plain = B.plain_twin(files, name, case.table)
        assert {p["encoding"] for k in range(case.table.num_columns) for p in pages_of(plain.data, k)} <= {0}
        u = loader.table_from_parquet_device(ctx, plain.path, columns)
        try:
            assert_tables_equal(ctx, t, u, tbl.num_rows)
        finally:
            u.free()
        return dict(zip(names, kinds_of(t)))
    finally:
        t.free()


@pytest.mark.parametrize("name", B.CASE_NAMES)
def test_front_coded_file_equals_the_arrow_route_and_the_plain_file(ctx, cases, files, name):
    if name not in cases:
        pytest.skip("this pyarrow has no codec to write the file with")
    c, more = cases[name]
    # (a value with a NUL byte stays offsets + bytes here and is cut by the Arrow route: compared with its PLAIN twin only)
    kinds = load_and_compare(ctx, files, name.split("_snappy")[0].split("_lz4")[0].split("_gzip")[0].split("_zstd")[0], c, DBA | more, arrow_route="nul_byte" not in name)
    if name.startswith("matrix") or name.startswith("beside"):
        assert kinds["sorted_r"] == (hip.PH_STR, 0, False) and kinds["sorted_n"] == (hip.PH_STR, 0, True)
        assert kinds["same_r"] == (hip.PH_CODE8, 1, False) and kinds["s40_n"] == (hip.PH_CODE8, 40, True) and kinds["gaps_r"][:2] == (hip.PH_CODE8, 8)
    want = {"shape_256": (hip.PH_CODE8, 256, False), "shape_257": (hip.PH_STR, 0, False), "shape_all_null": (hip.PH_CODE8, 0, True), "shape_one_value": (hip.PH_CODE8, 1, False),
            "shape_long": (hip.PH_STR, 0, True), "shape_nul_byte": (hip.PH_STR, 0, False), "count_0_nullable": (hip.PH_CODE8, 0, True)}
    if name in want:
        assert kinds["s" if name.startswith("shape") else "sorted"] == want[name]


def test_selection_and_bytes_as_the_source(ctx, cases, files):
    c, _m = cases["matrix_pages37_v1"]
    load_and_compare(ctx, files, "matrix_pages37_v1", c, DBA, ["sorted_n", "i64", "gaps_r", "sorted_n", "text_n"])
    t = loader.table_from_parquet_device(ctx, c.data, ["sorted_r"], flags=DBA)
    try:
        n = c.table.num_rows
        off = ctx.download(hip.vp(t.col(0).data), np.int32, n + 1)
        assert ctx.download(hip.vp(t.col(0).aux), np.uint8, int(off[n])).tobytes() == "".join(c.table.column("sorted_r").to_pylist()).encode()
    finally:
        t.free()


# ---------------------------------------------------------------- raw sections

def test_raw_sections_in_one_call_equal_the_host_twin(ctx):
    valid, invalid = B.valid_sections(), B.invalid_sections()
    jobs = [(name, data, -1, len(vals), sum(len(v) for v in vals)) for name, data, vals in valid]
    jobs += [(name, data, -1 if expected is None else expected, 70000 if "bomb" in name else 700, 1 << 16) for name, data, expected, _w, _c in invalid]
    name, data, vals = valid[2]
    jobs.append(("lengths_room_one_short", data, -1, len(vals) - 1, sum(len(v) for v in vals)))
    jobs.append(("bytes_room_one_short", data, len(vals), len(vals), sum(len(v) for v in vals) - 1))
    jobs.append(("no_room", data, -1, 0, 0))
    got, lens, byts = hip.delta_byte_array_decode(ctx, [j[1:] for j in jobs], canary=CANARY)
    lmask, bmask = np.ones(len(lens), bool), np.ones(len(byts), bool)
    for (name, data, expected, lroom, broom), g in zip(jobs, got):
        s = hip.DbaStream(0, len(data), expected, 0, lroom, 0, broom, 0, 0, 0, 0, 0)
        hl, hb = np.zeros(max(lroom, 1), np.int32), np.zeros(max(broom, 1), np.uint8)
        rc = hip.lib().ph_delta_byte_array_decode_host(bytes(data), hip.vp(hl.ctypes.data), hip.vp(hb.ctypes.data), hip.ctypes.byref(s))
        assert (g.status, g.sub, g.count, g.total_bytes, g.consumed) == (rc, s.sub, s.count, s.total_bytes, s.consumed), name
        if rc == OK:
            assert lens[g.len_pos:g.len_pos + g.count].tolist() == hl[:s.count].tolist(), name
            assert byts[g.byte_pos:g.byte_pos + g.total_bytes].tobytes() == hb[:s.total_bytes].tobytes() == b"".join(B.decode(data)), name
            lmask[g.len_pos:g.len_pos + g.count] = False
            bmask[g.byte_pos:g.byte_pos + g.total_bytes] = False
    assert [g.status for g in got[:len(valid)]] == [OK] * len(valid)
    assert [g.status for g in got[len(valid):len(valid) + len(invalid)]] == [EUNSUPPORTED if c == "EUNSUPPORTED" else EINVAL for *_r, c in invalid]
    assert [g.status for g in got[-3:]] == [ECAPACITY] * 3 and [g.total_bytes for g in got[-3:]] == [0, sum(len(v) for v in vals), 0]
    # nothing is written outside the destinations of the sections that decoded; a refused section writes nothing at all
    assert (lens[lmask] == hip.DBA_CANARY * 0x01010101).all() and (byts[bmask] == hip.DBA_CANARY).all(), "values outside the destinations were written"
    assert hip.delta_byte_array_decode(ctx, [])[0] == []


# ---------------------------------------------------------------- refusals

def test_refusals_and_patches_leave_the_context_usable(ctx, cases, files):
    good, _m = cases["count_65_nullable"]

    def refused(data, code, flags, word, columns=None):
        with pytest.raises(hip.PlanHipError) as e:
            loader.table_from_parquet_device(ctx, data, columns, flags=flags)
        assert e.value.code == code and word in str(e.value), str(e.value)
        return str(e.value)
    refused(good.data, EUNSUPPORTED, 0, "DELTA_BYTE_ARRAY values; PLAIN and RLE_DICTIONARY only")           # without the flag: as before
    refused(good.data, EUNSUPPORTED, DELTA | SNAPPY, "DELTA_BYTE_ARRAY values of a BYTE_ARRAY column; PLAIN, RLE_DICTIONARY, DELTA_BINARY_PACKED")
    for flags in (2048, 1024 | 2, 512):
        msg = refused(good.data, EINVAL, flags, "flags")
        assert "PH_PARQUET_DELTA_BYTE_ARRAY" in msg and msg.endswith("and PH_PARQUET_ZSTD are defined")
    for name, (path, col, enc, phys) in B.unsupported_files(files).items():
        assert phys is None or phys in refused(open(path, "rb").read(), EUNSUPPORTED, DBA | DELTA, enc + " values", [col])
    for name, (orig, bad, column, page, word) in B.patched(files, pages_of).items():
        msg = refused(bad, EINVAL, DBA, "row group 0, page %d:" % page)
        assert "column %d (" % column in msg and word in msg, (name, msg)
        with pytest.raises(hip.PlanHipError) as h:
            hip.parquet_read_column_host(bad, column, flags=DBA)
        assert msg.split(": ", 2)[2] == str(h.value).split(": ", 2)[2], name      # the host twin says the same behind its own name
        t = loader.table_from_parquet_device(ctx, orig, flags=DBA)                # the file the patch started from loads, on the same context
        t.free()
    both, _column = B.two_bad_pages(files, pages_of)
    assert "page 1:" in refused(both, EINVAL, DBA, "fewer or more values")
    load_and_compare(ctx, files, "count_65_nullable", good, DBA)


def test_a_corrupt_front_coded_page_and_a_corrupt_compressed_page_name_the_lower(ctx, files):
    mixed = B.front_and_compressed(files, lambda d, k: loader.parquet_pages(d, k, codecs=True))
    if mixed is None:
        pytest.skip("this pyarrow has no Snappy codec to write the file with")
    data, s_page, z_page = mixed
    for columns, want in ((["s", "z"], ("column 0 (s)", "page %d:" % s_page, "fewer or more values")), (["z", "s"], ("column 1 (z)", "page %d:" % z_page, "corrupt SNAPPY"))):
        with pytest.raises(hip.PlanHipError) as e:
            loader.table_from_parquet_device(ctx, data, columns, flags=DBA | SNAPPY)
        assert e.value.code == EINVAL and all(w in str(e.value) for w in want), str(e.value)
        with pytest.raises(hip.PlanHipError) as h:
            hip.parquet_read_column_host(data, 0 if columns[0] == "s" else 1, flags=DBA | SNAPPY)
        assert str(e.value).split(": ", 2)[2] == str(h.value).split(": ", 2)[2]


# ---------------------------------------------------------------- TPC-H lineitem at SF0.01 with its VARCHAR columns front-coded

@pytest.fixture(scope="module")
def lineitem_files(sf001, files):
    table = arrow_of("lineitem", sf001["lineitem"])
    rng = np.random.default_rng(17)
    words = ["furiously", "regular", "deposits", "sleep", "quickly", "ironic", "packages", "along", "the", "blithely", "final", "accounts"]
    comment = [" ".join(words[j] for j in rng.integers(0, len(words), int(k)))[:43] for k in rng.integers(2, 8, table.num_rows)]
    table = table.append_column("l_comment", pa.array(comment, pa.string()))
    strings = [f.name for f in table.schema if pa.types.is_string(f.type)]
    out = {}
    for kind, kw in (("plain", dict(use_dictionary=False)), ("front", dict(use_dictionary=False, column_encoding={n: "DELTA_BYTE_ARRAY" for n in strings}))):
        path = str(files / ("lineitem_%s.parquet" % kind))
        pq.write_table(table, path, store_decimal_as_integer=True, row_group_size=25000, data_page_size=64 << 10, compression="NONE", **kw)
        out[kind] = path
    return out, strings


def q1_and_q6(ctx, db, path, flags):
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


def test_q1_and_q6_over_front_coded_lineitem_equal_the_plain_file_and_the_oracle(ctx, lineitem_files, sf001):
    paths, strings = lineitem_files
    data = open(paths["front"], "rb").read()
    assert len(strings) >= 5 and all({p["encoding"] for p in pages_of(data, c)} == {B.E_DELTA_BYTE_ARRAY} for c in strings)
    texts = {}
    for kind, path in paths.items():
        flags = 0 if kind == "plain" else DBA
        db = tpch.Database.from_parquet(ctx, {"lineitem": path}, flags=flags)
        try:
            if kind != "plain":
                plain = tpch.Database.from_parquet(ctx, {"lineitem": paths["plain"]})
                try:
                    assert_tables_equal(ctx, db.t("lineitem"), plain.t("lineitem"), len(sf001["lineitem"]["l_quantity"]))
                finally:
                    plain.free()
                t = loader.table_from_parquet_device(ctx, path, ["l_comment", "l_shipmode"], flags=flags)
                u = loader.table_from_parquet_device(ctx, paths["plain"], ["l_comment", "l_shipmode"])
                try:
                    assert_tables_equal(ctx, t, u, t.nrows)
                    assert t.col(0).type == hip.PH_STR and t.col(1).type == hip.PH_CODE8
                finally:
                    t.free()
                    u.free()
            texts[kind], q1, q6 = q1_and_q6(ctx, db, path, flags)
        finally:
            db.free()
    assert texts["front"] == texts["plain"]
    want = O.q1(sf001["lineitem"], queries.q1_shipdate_cutoff())
    assert q1[0] == len(want) == 4
    for g, w in enumerate(want):
        assert q1[1][g] == (w.returnflag, w.linestatus) and q1[2][g][0] == w.sum_qty.value() and q1[2][g][1] == w.sum_base_price.unscaled(2)
        assert q1[2][g][3] == w.sum_charge.unscaled(6) and q1[3][g][7] == w.count_order
    rc, d = O.q6(sf001["lineitem"], *queries.q6_constants())
    assert rc == 0 and q6 == d.unscaled(4)
    with pytest.raises(hip.PlanHipError) as e:                    # the flag is what lets the file in
        tpch.Database.from_parquet(ctx, {"lineitem": paths["front"]})
    assert e.value.code == EUNSUPPORTED and "DELTA_BYTE_ARRAY" in str(e.value)
