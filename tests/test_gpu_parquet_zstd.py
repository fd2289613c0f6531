"""ZSTD pages decompressed on the device. ph_zstd_decompress over the crafted streams of tests/zstd_cases.py — valid, corrupt, the list
on which this decoder is stricter than libzstd — and over libzstd's output, one call each, at odd destination alignments between canaries,
against the host twin; the block whose streams cross the input windows at all sixteen source alignments. Then ph_table_create_parquet_ex
with PH_PARQUET_ZSTD: every array of the loaded table against the host twin's columns and against the table the same rows give when
written uncompressed and loaded at flags 0, the mixed-codec and delta files, the patches (same code, page and message as the host twin,
the context usable afterwards), and TPC-H at SF0.01 written with ZSTD. A corrupt stream is an input the decoder refuses before a byte
moves: tests/test_zstd_reference.py runs the same source on the host over the same streams."""
import numpy as np
import pytest

import pyarrow as pa
import pyarrow.parquet as pq

import oracle_lib as O
import zstd_cases as Z
from parquet_codec_helpers import arrow_of, assert_tables_equal, groups_of, load_and_compare, plain, run_streams
from plan_amd import hip, loader, queries, tpch

pytestmark = pytest.mark.gpu

OK, EINVAL, EUNSUPPORTED = hip.PH_OK, hip.PH_EINVAL, hip.PH_EUNSUPPORTED
SNAPPY, DELTA, LZ4_RAW, GZIP = hip.PH_PARQUET_SNAPPY, hip.PH_PARQUET_DELTA, hip.PH_PARQUET_LZ4_RAW, hip.PH_PARQUET_GZIP
ZSTD = getattr(hip, "PH_PARQUET_ZSTD", 256)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("zstd_cases")


@pytest.fixture(scope="module")
def cases(files):
    return Z.generate(files)


def pages_of(data, column):
    return loader.parquet_pages(data, column, codecs=True)


def twin(stream, n):
    """the host twin's answer: the bytes, or None for PH_EINVAL"""
    try:
        return hip.zstd_decompress_host(stream, n)
    except hip.PlanHipError as e:
        assert e.code == EINVAL
        return None


def test_crafted_streams_in_one_call(ctx):
    valid = [(name, stream, len(out)) for name, stream, out in Z.valid_streams()]
    bad = [c[:3] for c in Z.invalid_streams() + Z.stricter_streams() if c[2] < 1 << 20]
    # the straddling block once at each alignment of its source: a small frame in front of it shifts it by an odd number of bytes each time
    sname, sstream, sout = Z.straddling_stream()
    one, _o = Z.one_frame(lambda f: f.raw(b"s", last=True), did_bytes=1 if len(sstream) % 2 == 0 else 2)
    assert (len(one) + len(sstream)) % 2 == 1
    shifted = []
    for k in range(16):
        shifted += [("shift_%d" % k, one, 1), ("%s_at_%d" % (sname, k), sstream, len(sout))]
    streams = valid + bad + shifted
    assert len({sum(len(s) for _n, s, _e in streams[:i]) % 16 for i in range(len(streams) - 31, len(streams), 2)}) == 16
    got = run_streams(ctx, hip.zstd_decompress, streams)
    for (name, _stream, out), g in zip(Z.valid_streams(), got):
        assert g == out, name
    for (name, _stream, _n), g in zip(bad, got[len(valid):]):
        assert g is None, name
    for (name, _stream, n), g in zip(shifted, got[len(valid) + len(bad):]):
        assert g == (b"s" if n == 1 else sout), name
    for (name, stream, n), g in zip(streams[:len(valid) + len(bad)], got):   # byte-equal to the host twin, status[i] its code
        assert g == twin(stream, n), name


def test_libzstd_output_cut_extended_and_mis_sized_in_one_call(ctx):
    streams = [(name, s, len(data)) for name, s, data in Z.pyarrow_streams()]
    few = [c for c in streams if c[0].endswith(("level_1", "level_19"))]
    cut = [(name + "_cut", s[:-1], n) for name, s, n in few] + [(name + "_more", s + b"\0", n) for name, s, n in few] + \
          [(name + "_short", s, n + 1) for name, s, n in few] + [(name + "_past", s, n - 1) for name, s, n in few]
    got = run_streams(ctx, hip.zstd_decompress, streams + cut)
    for (name, _s, data), g in zip(Z.pyarrow_streams(), got):
        assert g == data, name
    assert all(g is None for g in got[len(streams):])


def test_no_streams_and_empty_streams(ctx):
    assert hip.zstd_decompress(ctx, [], [])[0] == []
    empty, _o = Z.one_frame(lambda f: f.raw(b"", last=True))
    got = run_streams(ctx, hip.zstd_decompress, [("no_bytes_for_none", b"", 0), ("empty_frame", empty, 0), ("no_bytes_for_one", b"", 1), ("eight_bytes", empty[:8], 0),
                                                 ("impossible", empty, 32768 * 9 + 1)])
    assert got == [b"", b"", None, None, None]


# ---------------------------------------------------------------- Parquet

@pytest.mark.parametrize("name", Z.CASE_NAMES)
def test_zstd_file_equals_the_uncompressed_file_and_the_host_twin(ctx, cases, files, name):
    c = cases[name]
    kinds = dict(zip(c.table.column_names, load_and_compare(ctx, c, ZSTD, files)))
    if name.startswith("matrix"):
        assert kinds["s300_n"][0] == kinds["s300_r"][0] == hip.PH_STR and kinds["s40_n"][:2] == kinds["s40_r"][:2] == (hip.PH_CODE8, 40)
        assert all(kinds[n][2] == n.endswith("_n") for n in kinds)


@pytest.mark.parametrize("name", ["mixed_codecs", "delta_v1", "delta_v2"])
def test_mixed_codecs_and_delta_pages_in_zstd_chunks(ctx, files, name):
    c, more = Z.flagged_files(files)[name]
    load_and_compare(ctx, c, ZSTD | more, files)
    load_and_compare(ctx, c, ZSTD | GZIP | LZ4_RAW | SNAPPY | DELTA, files)
    with pytest.raises(hip.PlanHipError) as e:                    # the other flag alone does not do
        loader.table_from_parquet_device(ctx, c.data, flags=ZSTD if name == "mixed_codecs" else DELTA)
    assert e.value.code == EUNSUPPORTED


def test_selection_and_an_uncompressed_file_with_the_flag(ctx, cases, files):
    c = cases["matrix_v1_dict_3groups_pages37"]
    names = ["s40_n", "d15_r", "i32_n", "s40_n"]
    t = loader.table_from_parquet_device(ctx, c.path, names, flags=ZSTD)
    unc = Z.P._write(files, "zs_none_gpu", c.table)
    ref = loader.table_from_parquet_device(ctx, unc.path, names, flags=ZSTD)      # word 256 on an uncompressed file reads as flags 0
    ref0 = loader.table_from_parquet_device(ctx, unc.path, names)
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
    for flags in (0, SNAPPY, SNAPPY | DELTA, LZ4_RAW, GZIP, SNAPPY | LZ4_RAW | GZIP | DELTA):
        refused(good.data, EUNSUPPORTED, flags, "ZSTD pages")        # without the flag: refused
    for flags in (256 | 2, 512, 256 | 32, 256 | 128):
        refused(good.data, EINVAL, flags, "PH_PARQUET_ZSTD")
    for name, (orig, bad, column, page, word) in Z.patched(files, pages_of).items():
        msg = refused(bad, EINVAL, ZSTD, "row group 0, page %d:" % page)
        assert "column %d (" % column in msg and word in msg, (name, msg)
        with pytest.raises(hip.PlanHipError) as h:
            hip.parquet_read_column_host(bad, column, flags=ZSTD)
        assert h.value.code == EINVAL and msg.split(": ", 2)[2] == str(h.value).split(": ", 2)[2], name   # the host twin says the same behind its own name
        t = loader.table_from_parquet_device(ctx, orig, flags=ZSTD)   # the file the patch started from loads, on the same context
        t.free()
    both, column = Z.two_bad_pages(files, pages_of)
    msg = refused(both, EINVAL, ZSTD, "page 1: a corrupt ZSTD stream")
    with pytest.raises(hip.PlanHipError) as h:
        hip.parquet_read_column_host(both, column, flags=ZSTD)
    assert msg.split(": ", 2)[2] == str(h.value).split(": ", 2)[2]
    if pa.Codec.is_available("brotli"):
        br = Z.P._write(files, "zs_refuse_brotli_gpu", pa.table({"i": pa.array(np.arange(100, dtype=np.int32))}), compression="BROTLI")
        assert "(i)" in refused(br.data, EUNSUPPORTED, ZSTD | GZIP, "only UNCOMPRESSED, GZIP and ZSTD pages are decoded")
    load_and_compare(ctx, good, ZSTD, files)


# ---------------------------------------------------------------- TPC-H at SF0.01 written with ZSTD

@pytest.fixture(scope="module")
def tpch_files(sf001, files):
    out = {}
    for name in ("lineitem", "orders", "customer"):
        table = arrow_of(name, sf001[name])
        for codec in ("NONE", "ZSTD"):
            path = str(files / ("zs_%s_%s.parquet" % (name, codec.lower())))
            pq.write_table(table, path, compression=codec, row_group_size=25000, data_page_size=64 << 10)
            out[name, codec] = path
    return out


def test_q1_and_q6_over_zstd_files_equal_the_uncompressed_files(ctx, tpch_files, sf001):
    tables = ("lineitem", "orders", "customer")
    db_zs = tpch.Database.from_parquet(ctx, {n: tpch_files[n, "ZSTD"] for n in tables}, flags=ZSTD)
    db_un = tpch.Database.from_parquet(ctx, {n: tpch_files[n, "NONE"] for n in tables})
    names = ["l_quantity", "l_extendedprice", "l_discount", "l_tax", "l_returnflag", "l_linestatus", "l_shipdate"]
    t = loader.table_from_parquet_device(ctx, tpch_files["lineitem", "ZSTD"], names, flags=ZSTD)
    u = loader.table_from_parquet_device(ctx, tpch_files["lineitem", "NONE"], names)
    try:
        for n in tables:
            assert_tables_equal(ctx, db_zs.t(n), db_un.t(n), db_un.rows(n))
        q1 = []
        for db in (db_zs, db_un):
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
        db_zs.free()
        db_un.free()
