"""What the GPU tests of the compressed Parquet pages (test_gpu_parquet_snappy.py, _lz4.py, _gzip.py, _codecs.py) share: the raw-stream call
between canaries, the comparison of two resident tables array by array and of a loaded table with the host twin's columns, and TPC-H's
generator columns as the Arrow table a Parquet writer gets. A plain module: no fixtures, no test."""
import numpy as np
import pyarrow as pa

import parquet_cases as P
from plan_amd import hip, loader, tpch

ROW_PAD = P.ROW_PAD
CANARY = 37           # bytes between two destinations: odd, so that destinations begin on every alignment


def run_streams(ctx, decompress, streams):
    """[(name, stream, expected length)] through ONE call of `decompress` (hip.snappy_decompress / lz4_decompress / gzip_decompress) ->
    [bytes or None]; the canaries and the zeros of refused streams are checked"""
    got, whole, pos = decompress(ctx, [s for _n, s, _e in streams], [e for _n, _s, e in streams], canary=CANARY)
    mask = np.ones(len(whole), bool)
    for (name, _s, e), p, g in zip(streams, pos, got):
        mask[p:p + e] = False
        if g is None:
            assert not whole[p:p + e].any(), name               # a refused stream leaves zeros
    assert (whole[mask] == 0xA5).all(), "bytes outside the destinations were written"
    assert len({p % 16 for p in pos}) > 8 or len(pos) < 16     # (the destinations begin on many alignments)
    return got


def outcome(f, *a):
    """the call's value, or the code it refuses with (a VARCHAR column has no range statistics, in either table)"""
    try:
        return f(*a)
    except hip.PlanHipError as e:
        return ("refused", e.code)


def assert_tables_equal(ctx, t, ref, n):
    """every device array of t against ref's: values, validity, dictionaries, statistics and narrowed copies"""
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


def assert_equals_host_twin(ctx, t, data, flags, n):
    """the loaded columns against ph_parquet_read_column_host_ex of the same bytes: values, validity, strings (through the dictionary
    where the column was encoded)"""
    if n == 0:
        return
    padded = (n + ROW_PAD - 1) // ROW_PAD * ROW_PAD
    for k in range(t.ncols):
        col = t.col(k)
        v, valid, off, byts = hip.parquet_read_column_host(data, k, flags=flags)
        assert bool(col.validity) == (not valid.all()), k
        if col.validity:
            bits = np.unpackbits(ctx.download(hip.vp(col.validity), np.uint8, padded // 8), bitorder="little")
            assert np.array_equal(bits[:n].astype(bool), valid) and not bits[n:].any(), k
        if v is not None:
            got = ctx.download(hip.vp(col.data), hip.NP_TYPES[col.type], padded)
            assert np.array_equal(got[:n].astype(np.int64), v) and not got[n:].any(), k
            continue
        strs = [byts[off[i]:off[i + 1]] for i in range(n)]
        if col.type == hip.PH_STR:
            o = ctx.download(hip.vp(col.data), np.int32, n + 1)
            b = ctx.download(hip.vp(col.aux), np.uint8, int(col.aux_bytes)).tobytes() if col.aux_bytes else b""
            assert np.array_equal(o, off) and b == byts, k
        else:
            assert col.type == hip.PH_CODE8, k
            codes = ctx.download(hip.vp(col.data), np.uint8, n)
            d = [s.encode("utf-8", "surrogateescape") for s in t.dicts[k]]
            assert all(d[codes[i]] == strs[i] for i in range(n) if valid[i]), k


def load_and_compare(ctx, case, flags, files):
    """the file on the device at `flags` against the host twin and against the same rows written uncompressed and loaded at flags 0"""
    data = case.data
    n = case.table.num_rows
    plain_file = P._write(files, "plain_of_" + case.name, case.table)
    t = loader.table_from_parquet_device(ctx, data, flags=flags)
    ref = loader.table_from_parquet_device(ctx, plain_file.path)
    try:
        assert t.column_names == ref.column_names == case.table.column_names
        assert_tables_equal(ctx, t, ref, n)
        assert_equals_host_twin(ctx, t, data, flags, n)
        return [(t.col(k).type, len(t.dicts[k]), bool(t.col(k).validity)) for k in range(t.ncols)]
    finally:
        t.free()
        ref.free()


def arrow_of(name, src):
    """the generator's columns as the Arrow table a Parquet writer gets: DATE date32, DECIMAL decimal128(15, 2), VARCHAR strings"""
    import decimal
    arrays, names = [], []
    for cname, typ, scale, dic in tpch.SCHEMA[name]:
        if typ == hip.PH_STR:
            if cname + "_off" not in src:                     # a column the fixture does not hold: a filler
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


def groups_of(r):
    g = r["ngroups"]
    return g, [tuple(k) for k in r["keys"][:g]], [list(s) for s in r["sum"][:g]], [list(c) for c in r["count"][:g]]


def plain(r):
    """a plan's fetched result as plain Python values"""
    return {k: np.asarray(v).tolist() for k, v in r.items()}
