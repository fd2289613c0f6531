"""SNAPPY pages decompressed on the device. ph_snappy_decompress over the crafted streams of tests/snappy_cases.py and over Codec.compress
output, all in one call each, against pyarrow's Snappy — the same bytes, the same refusals, nothing written around a destination. Then
ph_table_create_parquet_ex with PH_PARQUET_SNAPPY: every array of the loaded table against the table ph_table_create_arrow builds over
pq.read_table of the same file (the comparison of tests/test_gpu_parquet_load.py), the refusals and one-byte patches (same code and message
as the host twin, no table, the context usable afterwards), and TPC-H at SF0.01 written with Snappy."""
import pytest

pa = pytest.importorskip("pyarrow")
pq = pytest.importorskip("pyarrow.parquet")
if not pa.Codec.is_available("snappy"):
    pytest.skip("this pyarrow has no Snappy codec", allow_module_level=True)

import oracle_lib as O  # noqa: E402
import snappy_cases as S  # noqa: E402
from parquet_codec_helpers import arrow_of, assert_tables_equal, run_streams  # noqa: E402
from plan_amd import hip, loader, queries, tpch, tpchgen  # noqa: E402

pytestmark = pytest.mark.gpu

OK, EINVAL, EUNSUPPORTED = hip.PH_OK, hip.PH_EINVAL, hip.PH_EUNSUPPORTED
SNAPPY = hip.PH_PARQUET_SNAPPY
CODEC = pa.Codec("snappy")


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("snappy_cases")


@pytest.fixture(scope="module")
def cases(files):
    return S.generate(files)


def pages_of(data, column):
    return loader.parquet_pages(data, column, codecs=True)


def theirs(stream, n):
    try:
        return CODEC.decompress(stream, decompressed_size=n).to_pybytes()
    except Exception:  # noqa: BLE001
        return None


def test_crafted_streams_in_one_call(ctx):
    valid = [(name, stream, len(out)) for name, stream, out in S.valid_streams()]
    streams = valid + S.invalid_streams() + S.stricter_streams()
    got = run_streams(ctx, hip.snappy_decompress, streams)
    for (name, stream, out), g in zip(S.valid_streams(), got):
        assert theirs(stream, len(out)) == out and g == out, name
    for (name, stream, n), g in zip(S.invalid_streams(), got[len(valid):]):
        assert theirs(stream, n) is None and g is None, name
    for (name, _stream, _n), g in zip(S.stricter_streams(), got[len(valid) + len(S.invalid_streams()):]):
        assert g is None, name                                  # (a preamble below the expected length: refused here, see snappy_cases.py)
    # the same outcomes as the host twin
    for (name, stream, n), g in zip(streams, got):
        try:
            h = hip.snappy_decompress_host(stream, n)
        except hip.PlanHipError:
            h = None
        assert g == h, name


def test_compressor_output_in_one_call(ctx):
    inputs = S.roundtrip_inputs()
    streams = [(name, CODEC.compress(data).to_pybytes(), len(data)) for name, data in inputs]
    cut = [(name + "_cut", s[:-1], n) for name, s, n in streams if n > 64][:6] + [(name + "_more", s + b"\0", n) for name, s, n in streams if n > 64][:6]
    got = run_streams(ctx, hip.snappy_decompress, streams + cut)
    for (name, data), g in zip(inputs, got):
        assert g == data, name
    assert all(g is None for g in got[len(streams):])


def test_no_streams_and_bad_arguments(ctx):
    assert hip.snappy_decompress(ctx, [], [])[0] == []
    got = run_streams(ctx, hip.snappy_decompress, [("empty_stream", b"", 0), ("empty", b"\0", 0)])
    assert got == [None, b""]                                    # no preamble is no stream


# ---------------------------------------------------------------- Parquet

def load_and_compare(ctx, path, columns=None, source=None):
    tbl = pq.read_table(path)
    names = list(columns) if columns is not None else tbl.column_names
    arrow = pa.Table.from_arrays([tbl.column(c) for c in names], names=["c%d" % i for i in range(len(names))])
    t = loader.table_from_parquet_device(ctx, path if source is None else source, columns, flags=SNAPPY)
    ref = loader.table_from_arrow_c(ctx, arrow)
    try:
        assert t.column_names == names
        assert_tables_equal(ctx, t, ref, tbl.num_rows)
        return [(t.col(k).type, len(t.dicts[k]), bool(t.col(k).validity)) for k in range(t.ncols)]
    finally:
        t.free()
        ref.free()


@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_snappy_file_equals_the_arrow_route(ctx, cases, name):
    c = cases[name]
    kinds = dict(zip(c.table.column_names, load_and_compare(ctx, c.path)))
    if name.startswith("matrix"):
        assert kinds["s300_n"][0] == kinds["s300_r"][0] == hip.PH_STR and kinds["s40_n"][:2] == kinds["s40_r"][:2] == (hip.PH_CODE8, 40)
        assert all(kinds[n][2] == n.endswith("_n") for n in kinds)
    if name.startswith("nulls"):
        assert kinds["all_null"][2] and not kinds["none_null"][2] and kinds["s_all_null"] == (hip.PH_CODE8, 0, True) and kinds["s_alt"] == (hip.PH_CODE8, 50, True)
    if name.startswith("text"):
        assert kinds == {"t_r": (hip.PH_CODE8, 12, False), "t_n": (hip.PH_CODE8, 12, True)}


def test_selection_bytes_and_an_uncompressed_file_with_the_flag(ctx, cases, files):
    c = cases["matrix_v1_dict_3groups_pages37"]
    load_and_compare(ctx, c.path, ["s40_n", "d15_r", "i32_n", "s40_n"])
    load_and_compare(ctx, c.path, ["i64_r"], source=c.data)
    plain = S.P._write(files, "sn_none_gpu", cases["rows_65"].table)
    load_and_compare(ctx, plain.path)


def test_refusals_and_patches_leave_the_context_usable(ctx, cases, files):
    good = cases["rows_65"]

    def refused(data, code, flags, word):
        with pytest.raises(hip.PlanHipError) as e:
            loader.table_from_parquet_device(ctx, data, flags=flags)
        assert e.value.code == code and word in str(e.value), str(e.value)
        return str(e.value)
    refused(good.data, EUNSUPPORTED, 0, "SNAPPY")                # without the flag: as before
    refused(good.data, EINVAL, 2, "flags")
    for name, (orig, bad, column, page) in S.patched(files, pages_of).items():
        msg = refused(bad, EINVAL, SNAPPY, "row group 0, page %d:" % page)
        assert "column %d (" % column in msg, (name, msg)
        with pytest.raises(hip.PlanHipError) as h:
            hip.parquet_read_column_host(bad, column, flags=SNAPPY)
        assert msg.split(": ", 2)[2] == str(h.value).split(": ", 2)[2], name      # the host twin says the same behind its own name
        t = loader.table_from_parquet_device(ctx, orig, flags=SNAPPY)    # the file the patch started from loads, on the same context
        t.free()
    both, _column = S.two_bad_pages(files, pages_of)
    assert "page 1:" in refused(both, EINVAL, SNAPPY, "corrupt SNAPPY stream")
    # a corrupt dictionary page and a corrupt data page of one column: planhip.h's order of pages, the host twin's answer
    for column, page in ((0, 2), (1, 0)):
        bad = S.bad_dictionary_and_data_page(files, pages_of, column)
        with pytest.raises(hip.PlanHipError) as e:
            loader.table_from_parquet_device(ctx, bad, ["k", "s"][column:column + 1], flags=SNAPPY)
        with pytest.raises(hip.PlanHipError) as h:
            hip.parquet_read_column_host(bad, column, flags=SNAPPY)
        assert e.value.code == EINVAL and ("page %d: a corrupt SNAPPY stream" % page) in str(e.value), (column, str(e.value))
        assert str(e.value).split(": ", 2)[2] == str(h.value).split(": ", 2)[2]
    load_and_compare(ctx, good.path)


def test_a_gzip_file_is_refused_with_the_flag_too(ctx, files):
    if not pa.Codec.is_available("gzip"):
        pytest.skip("this pyarrow has no GZIP codec to write the file with")
    with pytest.raises(hip.PlanHipError) as e:
        loader.table_from_parquet_device(ctx, open(S.write_gzip(files), "rb").read(), flags=SNAPPY)
    assert e.value.code == EUNSUPPORTED and "GZIP" in str(e.value) and "(i)" in str(e.value)


# ---------------------------------------------------------------- TPC-H at SF0.01 written with Snappy

@pytest.fixture(scope="module")
def tpch_files(sf001, files):
    out = {}
    for codec in ("NONE", "SNAPPY"):
        for name in ("lineitem", "orders", "customer"):
            path = str(files / ("sn_%s_%s.parquet" % (name, codec.lower())))
            pq.write_table(arrow_of(name, sf001[name]), path, compression=codec, row_group_size=25000, data_page_size=64 << 10)
            out[name, codec] = path
    return out


def test_q1_over_snappy_lineitem_equals_the_uncompressed_file_and_the_oracle(ctx, tpch_files, sf001):
    names = ["l_quantity", "l_extendedprice", "l_discount", "l_tax", "l_returnflag", "l_linestatus", "l_shipdate"]
    t = loader.table_from_parquet_device(ctx, tpch_files["lineitem", "SNAPPY"], names, flags=SNAPPY)
    u = loader.table_from_parquet_device(ctx, tpch_files["lineitem", "NONE"], names)
    try:
        assert_tables_equal(ctx, t, u, len(sf001["lineitem"]["l_quantity"]))
        assert t.dicts[4] == tpchgen.RETURNFLAG_DICT and t.dicts[5] == tpchgen.LINESTATUS_DICT
        res = []
        for tab in (t, u):
            p = queries.q1_plan(ctx, tab)
            p.run()
            r = p.fetch()
            res.append((r["ngroups"], [tuple(k) for k in r["keys"][:r["ngroups"]]], [list(s) for s in r["sum"][:r["ngroups"]]], [list(c) for c in r["count"][:r["ngroups"]]]))
            p.free()
        assert res[0] == res[1]
        want = O.q1(sf001["lineitem"], queries.q1_shipdate_cutoff())
        assert res[0][0] == len(want) == 4
        for g, w in enumerate(want):
            assert res[0][1][g] == (w.returnflag, w.linestatus) and res[0][2][g][0] == w.sum_qty.value() and res[0][3][g][7] == w.count_order
    finally:
        t.free()
        u.free()


def test_q3_over_snappy_files_equals_the_uncompressed_files(ctx, tpch_files):
    db_sn = tpch.Database.from_parquet(ctx, {n: tpch_files[n, "SNAPPY"] for n in ("lineitem", "orders", "customer")}, flags=SNAPPY)
    db_un = tpch.Database.from_parquet(ctx, {n: tpch_files[n, "NONE"] for n in ("lineitem", "orders", "customer")})
    try:
        out = []
        for db in (db_sn, db_un):
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
        db_sn.free()
        db_un.free()
