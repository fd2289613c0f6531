"""LZ4_RAW pages decompressed on the device. ph_lz4_decompress over the crafted blocks of tests/lz4_cases.py — valid, corrupt, the two
lists on which this decoder and liblz4 differ — and over Codec.compress output, one call each, at odd destination alignments between
canaries, against the host twin. Then ph_table_create_parquet_ex with PH_PARQUET_LZ4_RAW: every array of the loaded table against the host
twin's columns and against the table the same rows give when written uncompressed and loaded at flags 0, the mixed-codec and delta files,
the one-byte patches (same code, page and message as the host twin, the context usable afterwards), and TPC-H at SF0.01 written with
LZ4_RAW."""
import numpy as np
import pytest

import pyarrow as pa
import pyarrow.parquet as pq

import lz4_cases as L
import oracle_lib as O
from parquet_codec_helpers import arrow_of, assert_tables_equal, groups_of, load_and_compare, plain, run_streams
from plan_amd import hip, loader, queries, tpch

pytestmark = pytest.mark.gpu

OK, EINVAL, EUNSUPPORTED = hip.PH_OK, hip.PH_EINVAL, hip.PH_EUNSUPPORTED
SNAPPY, DELTA, LZ4_RAW = hip.PH_PARQUET_SNAPPY, hip.PH_PARQUET_DELTA, hip.PH_PARQUET_LZ4_RAW
CODEC = pa.Codec("lz4_raw")


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("lz4_cases")


@pytest.fixture(scope="module")
def cases(files):
    return L.generate(files)


def pages_of(data, column):
    return loader.parquet_pages(data, column, codecs=True)


def twin(stream, n):
    """the host twin's answer: the bytes, or None for PH_EINVAL"""
    try:
        return hip.lz4_decompress_host(stream, n)
    except hip.PlanHipError as e:
        assert e.code == EINVAL
        return None


def test_crafted_blocks_in_one_call(ctx):
    valid = [(name, stream, len(out)) for name, stream, out in L.valid_streams()]
    lenient = [(name, stream, len(out)) for name, stream, out in L.lenient_streams()]
    bad = [c[:3] for c in L.invalid_streams() + L.stricter_streams()]
    # the straddling block once at each alignment of its source: a one-byte block in front of it shifts it by one
    (sname, sstream, sout), _marks = L.straddling_stream()
    shifted = []
    for k in range(16):
        shifted += [("shift_%d" % k, b"\x10s", 1), ("%s_at_%d" % (sname, k), sstream, len(sout))]
    streams = valid + lenient + bad + shifted
    got = run_streams(ctx, hip.lz4_decompress, streams)
    for (name, _stream, out), g in zip(L.valid_streams() + L.lenient_streams(), got):
        assert g == out, name
    for (name, _stream, _n), g in zip(bad, got[len(valid) + len(lenient):]):
        assert g is None, name
    for (name, _stream, n), g in zip(shifted, got[len(valid) + len(lenient) + len(bad):]):
        assert g == (b"s" if n == 1 else sout), name
    for (name, stream, n), g in zip(streams[:len(valid) + len(lenient) + len(bad)], got):   # byte-equal to the host twin, status[i] its code
        assert g == twin(stream, n), name


def test_compressor_output_in_one_call(ctx):
    inputs = L.roundtrip_inputs()
    streams = [(name, CODEC.compress(data).to_pybytes(), len(data)) for name, data in inputs]
    big = [(name, s, n) for name, s, n in streams if n > 64]
    cut = [(name + "_cut", s[:-1], n) for name, s, n in big][:6] + [(name + "_more", s + b"\0", n) for name, s, n in big][:6] + \
          [(name + "_short", s, n + 1) for name, s, n in big][:6] + [(name + "_past", s, n - 1) for name, s, n in big][:6]
    got = run_streams(ctx, hip.lz4_decompress, streams + cut)
    for (name, data), g in zip(inputs, got):
        assert g == data, name
    assert all(g is None for g in got[len(streams):])


def test_no_blocks_and_empty_blocks(ctx):
    assert hip.lz4_decompress(ctx, [], [])[0] == []
    got = run_streams(ctx, hip.lz4_decompress, [("no_bytes_for_none", b"", 0), ("empty", b"\0", 0), ("no_bytes_for_one", b"", 1), ("impossible", b"\x1f\x00\x01\x00\xff", 255 * 5 + 1)])
    assert got == [b"", b"", None, None]


# ---------------------------------------------------------------- Parquet

@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_lz4_file_equals_the_uncompressed_file_and_the_host_twin(ctx, cases, files, name):
    c = cases[name]
    kinds = dict(zip(c.table.column_names, load_and_compare(ctx, c, LZ4_RAW, files)))
    if name.startswith("matrix"):
        assert kinds["s300_n"][0] == kinds["s300_r"][0] == hip.PH_STR and kinds["s40_n"][:2] == kinds["s40_r"][:2] == (hip.PH_CODE8, 40)
        assert all(kinds[n][2] == n.endswith("_n") for n in kinds)
    if name.startswith("nulls"):
        assert kinds["all_null"][2] and not kinds["none_null"][2] and kinds["s_all_null"] == (hip.PH_CODE8, 0, True) and kinds["s_alt"] == (hip.PH_CODE8, 50, True)
    if name.startswith("text"):
        assert kinds == {"t_r": (hip.PH_CODE8, 12, False), "t_n": (hip.PH_CODE8, 12, True)}


@pytest.mark.parametrize("name", ["mixed_codecs", "delta_v1", "delta_v2"])
def test_mixed_codecs_and_delta_pages_in_lz4_chunks(ctx, files, name):
    c, more = L.flagged_files(files)[name]
    load_and_compare(ctx, c, LZ4_RAW | more, files)
    load_and_compare(ctx, c, LZ4_RAW | SNAPPY | DELTA, files)
    with pytest.raises(hip.PlanHipError) as e:                    # the other flag alone does not do
        loader.table_from_parquet_device(ctx, c.data, flags=LZ4_RAW if name == "mixed_codecs" else DELTA)
    assert e.value.code == EUNSUPPORTED


def test_selection_and_an_uncompressed_file_with_the_flag(ctx, cases, files):
    c = cases["matrix_v1_dict_3groups_pages37"]
    names = ["s40_n", "d15_r", "i32_n", "s40_n"]
    t = loader.table_from_parquet_device(ctx, c.path, names, flags=LZ4_RAW)
    plain = L.P._write(files, "lz_none_gpu", c.table)
    ref = loader.table_from_parquet_device(ctx, plain.path, names, flags=LZ4_RAW)    # word 16 on an uncompressed file reads as flags 0
    ref0 = loader.table_from_parquet_device(ctx, plain.path, names)
    try:
        assert_tables_equal(ctx, t, ref, c.table.num_rows)
        assert_tables_equal(ctx, ref, ref0, c.table.num_rows)
    finally:
        t.free()
        ref.free()
        ref0.free()


def test_refusals_and_patches_leave_the_context_usable(ctx, cases, files):
    good = cases["rows_65"]

    def refused(data, code, flags, word):
        with pytest.raises(hip.PlanHipError) as e:
            loader.table_from_parquet_device(ctx, data, flags=flags)
        assert e.value.code == code and word in str(e.value), str(e.value)
        return str(e.value)
    for flags in (0, SNAPPY, SNAPPY | DELTA):
        refused(good.data, EUNSUPPORTED, flags, "LZ4_RAW pages")     # without the flag: refused
    for flags in (2, 8, 18, 32):
        refused(good.data, EINVAL, flags, "PH_PARQUET_LZ4_RAW")
    for name, (orig, bad, column, page, word) in L.patched(files, pages_of).items():
        msg = refused(bad, EINVAL, LZ4_RAW, "row group 0, page %d:" % page)
        assert "column %d (" % column in msg and word in msg, (name, msg)
        with pytest.raises(hip.PlanHipError) as h:
            hip.parquet_read_column_host(bad, column, flags=LZ4_RAW)
        assert h.value.code == EINVAL and msg.split(": ", 2)[2] == str(h.value).split(": ", 2)[2], name   # the host twin says the same behind its own name
        t = loader.table_from_parquet_device(ctx, orig, flags=LZ4_RAW)   # the file the patch started from loads, on the same context
        t.free()
    both, column = L.two_bad_pages(files, pages_of)
    msg = refused(both, EINVAL, LZ4_RAW, "page 1: a corrupt LZ4_RAW stream")
    with pytest.raises(hip.PlanHipError) as h:
        hip.parquet_read_column_host(both, column, flags=LZ4_RAW)
    assert msg.split(": ", 2)[2] == str(h.value).split(": ", 2)[2]
    gz = L.P._write(files, "lz_refuse_gzip_gpu", pa.table({"i": pa.array(np.arange(100, dtype=np.int32))}), compression="GZIP")
    assert "(i)" in refused(gz.data, EUNSUPPORTED, LZ4_RAW, "GZIP pages")
    load_and_compare(ctx, good, LZ4_RAW, files)


# ---------------------------------------------------------------- TPC-H at SF0.01 written with LZ4_RAW

@pytest.fixture(scope="module")
def tpch_files(sf001, files):
    out = {}
    for name in ("lineitem", "orders", "customer"):
        table = arrow_of(name, sf001[name])
        for codec in ("NONE", "LZ4_RAW"):
            path = str(files / ("lz_%s_%s.parquet" % (name, codec.lower())))
            pq.write_table(table, path, compression=codec, row_group_size=25000, data_page_size=64 << 10)
            out[name, codec] = path
    return out


def test_q1_and_q6_over_lz4_files_equal_the_uncompressed_files(ctx, tpch_files, sf001):
    tables = ("lineitem", "orders", "customer")
    db_lz = tpch.Database.from_parquet(ctx, {n: tpch_files[n, "LZ4_RAW"] for n in tables}, flags=LZ4_RAW)
    db_un = tpch.Database.from_parquet(ctx, {n: tpch_files[n, "NONE"] for n in tables})
    names = ["l_quantity", "l_extendedprice", "l_discount", "l_tax", "l_returnflag", "l_linestatus", "l_shipdate"]
    t = loader.table_from_parquet_device(ctx, tpch_files["lineitem", "LZ4_RAW"], names, flags=LZ4_RAW)
    u = loader.table_from_parquet_device(ctx, tpch_files["lineitem", "NONE"], names)
    try:
        for n in tables:
            assert_tables_equal(ctx, db_lz.t(n), db_un.t(n), db_un.rows(n))
        q1 = []
        for db in (db_lz, db_un):
            p = tpch.q1_plan(db)
            p.run()
            q1.append(plain(p.fetch()))
            p.free()
        assert q1[0] == q1[1] and q1[0]["ngroups"] == 4
        q6 = []
        for tab in (t, u):
            p = queries.q6_plan(ctx, tab)
            p.run()
            q6.append(p.fetch()["sum"][0][0])
            p.free()
        rc, d = O.q6(sf001["lineitem"], *queries.q6_constants())
        assert rc == 0 and q6[0] == q6[1] == d.unscaled(4)
        p = queries.q1_plan(ctx, t)
        p.run()
        r = groups_of(p.fetch())
        p.free()
        want = O.q1(sf001["lineitem"], queries.q1_shipdate_cutoff())
        assert r[0] == len(want) == 4
        for g, w in enumerate(want):
            assert r[1][g] == (w.returnflag, w.linestatus) and r[2][g][0] == w.sum_qty.value() and r[3][g][7] == w.count_order
    finally:
        t.free()
        u.free()
        db_lz.free()
        db_un.free()
