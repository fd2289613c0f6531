"""Parquet load path: an uncompressed lineitem Parquet file -> resident table through ph_table_create_parquet (column chunks decoded
on the device), against pq.read_table + ph_table_create_arrow on the same file and columns.

  python scripts/bench_parquet_load.py [--gb 1.0] [--warmup 3] [--runs 10] [--arrow-runs 5] [--out FILE] [--device-only] [--file PATH]
                                       [--compression {none,snappy,lz4_raw,gzip,zstd}] [--encoding {plain,delta,delta_byte_array}] [--comment]

The rows are the SF0.01 lineitem (every SCHEMA column, a filler comment) repeated to about --gb gigabytes of CSV-equivalent text and
written once by pyarrow, uncompressed, dictionary pages on for the VARCHAR columns only. Reported (medians over the timed runs, one
JSON line):
  parquet_e2e_ms / _gbps   wall time of loader.table_from_parquet_device over all columns (footer, upload of the chunks, kernels, column
                           finishing; the call returns synchronised); GB/s of FILE bytes
  h2d_ms / _gbps           the same chunk bytes through ph_dev_upload alone: the bound
  q1_e2e_ms                the same load taking only Q1's seven columns (what pruning buys: the other chunks never cross PCIe)
  arrow_e2e_ms             pq.read_table (16 threads) + loader.table_from_arrow_c over the same file and columns
--compression snappy writes the same table with compression="SNAPPY" and loads it with PH_PARQUET_SNAPPY (the pages are decompressed on the
device); the line then also holds "compression", and "uncompressed_bytes": what the same chunks take uncompressed (the writer's
total_uncompressed_size), beside "file_bytes", the file as written. GB/s stay those of FILE bytes. The default, none, prints what it always did.
--compression lz4_raw does the same with compression="LZ4_RAW" (Parquet codec 7, what pyarrow also writes for "LZ4") and PH_PARQUET_LZ4_RAW.
--compression gzip does the same with compression="GZIP" (codec 2, zlib's default level) and PH_PARQUET_GZIP.
--compression zstd does the same with compression="ZSTD" (codec 6, libzstd's default level) and PH_PARQUET_ZSTD; the line then also holds
"zstd_stats": what the host twin counted over every page's stream (sections, literal bytes, sequences, match bytes, and the share of match
bytes whose offset lies beyond the kernel's ring of 32 KiB).
--encoding delta writes the integer, date and decimal columns DELTA_BINARY_PACKED (decimals stored as integers, which the encoding needs) and
loads the file with PH_PARQUET_DELTA; the VARCHAR columns keep their dictionary pages. In the same sitting the file the script writes by
default (PLAIN, uncompressed) is loaded with the same protocol, and the line holds "encoding", "plain_file_bytes", "plain_parquet_e2e_ms",
"plain_q1_e2e_ms" and "delta_over_plain" (median load time of the delta file over the PLAIN file's) beside the delta file's own figures.
--skip-plain leaves that second file out (a profiler run: the page kernels of both files share their names).
--comment adds an l_comment text column of dbgen's length range to the file (the resident lineitem has none): PLAIN BYTE_ARRAY by default,
DELTA_LENGTH_BYTE_ARRAY with --encoding delta. The two options compose with --compression.
--encoding delta_byte_array writes the VARCHAR columns (and with --comment the comment column) DELTA_BYTE_ARRAY, Parquet's front coding, with
use_dictionary off for them, the other columns PLAIN, and loads the file with PH_PARQUET_DELTA_BYTE_ARRAY. In the same sitting the PLAIN file
and the --encoding delta file of the same rows are loaded with the same protocol: "plain_file_bytes", "plain_parquet_e2e_ms",
"delta_file_bytes", "delta_parquet_e2e_ms", "front_over_plain" and "front_over_delta" (medians) stand beside the front-coded file's figures.
The per-kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python scripts/bench_parquet_load.py --device-only` run.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plan_amd import hip, loader, tpch, tpchgen  # noqa: E402

Q1_COLUMNS = ["l_quantity", "l_extendedprice", "l_discount", "l_tax", "l_returnflag", "l_linestatus", "l_shipdate"]
CSV_BYTES_PER_ROW = 135        # scripts/bench_csv_load.py's text: what "a gigabyte of rows" means here


def lineitem_arrow(L, reps, comment=False):
    import pyarrow as pa
    arrays, names = [], []
    n = len(L["l_orderkey"])
    if comment:
        rng = np.random.default_rng(17)
        words = ["furiously", "regular", "deposits", "sleep", "quickly", "ironic", "packages", "along", "the", "blithely", "final", "accounts"]
        text = [" ".join(words[j] for j in rng.integers(0, len(words), int(k)))[:43] for k in rng.integers(2, 8, n)]
        arrays.append(pa.chunked_array([pa.array(text, pa.string())] * reps))
        names.append("l_comment")
    for cname, typ, scale, dic in tpch.SCHEMA["lineitem"]:
        if typ == hip.PH_CODE8:
            arr = pa.DictionaryArray.from_arrays(pa.array(L[cname].astype(np.int32)), pa.array(dic, pa.string())).cast(pa.string())
        elif typ == hip.PH_STR:
            arr = pa.array(["regular deposits haggle x"] * n, pa.string())
        elif typ == hip.PH_DEC64:
            wide = np.zeros((n, 2), np.int64)
            wide[:, 0] = L[cname]
            wide[:, 1] = L[cname] >> 63
            arr = pa.Array.from_buffers(pa.decimal128(15, scale), n, [None, pa.py_buffer(wide.tobytes())])
        elif typ == hip.PH_DATE:
            arr = pa.array(L[cname].astype(np.int32), pa.int32()).cast(pa.date32())
        else:
            arr = pa.array(L[cname])
        arrays.append(pa.chunked_array([arr] * reps))
        names.append(cname)
    return pa.Table.from_arrays(arrays, names=names)


def timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--arrow-runs", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--file", help="where the Parquet file is written (default: a temporary file)")
    ap.add_argument("--device-only", action="store_true", help="the device path alone (for a profiler run)")
    ap.add_argument("--compression", choices=["none", "snappy", "lz4_raw", "gzip", "zstd"], default="none",
                    help="the codec the file is written with (snappy: loaded with PH_PARQUET_SNAPPY; lz4_raw: with PH_PARQUET_LZ4_RAW; gzip: with PH_PARQUET_GZIP; zstd: with PH_PARQUET_ZSTD)")
    ap.add_argument("--encoding", choices=["plain", "delta", "delta_byte_array"], default="plain",
                    help="delta: integer, date and decimal columns DELTA_BINARY_PACKED, loaded with PH_PARQUET_DELTA; delta_byte_array: the VARCHAR columns front-coded, loaded with PH_PARQUET_DELTA_BYTE_ARRAY")
    ap.add_argument("--skip-plain", action="store_true", help="with --encoding delta / delta_byte_array: do not load the PLAIN file beside it (for a profiler run, whose kernels share names)")
    ap.add_argument("--comment", action="store_true", help="add an l_comment text column (PLAIN, or DELTA_LENGTH_BYTE_ARRAY with --encoding delta)")
    a = ap.parse_args()
    import pyarrow as pa
    import pyarrow.parquet as pq

    cols = [c for c, _t, _s, _d in tpch.SCHEMA["lineitem"]]
    L = tpchgen.lineitem((1, 100), columns=[c for c, t, _s, _d in tpch.SCHEMA["lineitem"] if t != hip.PH_STR])
    n1 = len(L["l_orderkey"])
    reps = max(1, round(a.gb * 1e9 / (n1 * CSV_BYTES_PER_ROW)))
    nrows = n1 * reps
    tmp = None
    path = a.file
    if path is None:
        tmp = tempfile.NamedTemporaryFile(suffix=".parquet", delete=False)
        path = tmp.name
        tmp.close()
    varchar = [c for c, t, _s, _d in tpch.SCHEMA["lineitem"] if t in (hip.PH_CODE8, hip.PH_STR)]
    snappy, lz4_raw, gzip, zstd = a.compression == "snappy", a.compression == "lz4_raw", a.compression == "gzip", a.compression == "zstd"
    delta, front = a.encoding == "delta", a.encoding == "delta_byte_array"
    flags = (hip.PH_PARQUET_SNAPPY if snappy else 0) | (hip.PH_PARQUET_LZ4_RAW if lz4_raw else 0) | (hip.PH_PARQUET_GZIP if gzip else 0) | (hip.PH_PARQUET_ZSTD if zstd else 0) | \
            (hip.PH_PARQUET_DELTA if delta else 0) | (hip.PH_PARQUET_DELTA_BYTE_ARRAY if front else 0)
    table = lineitem_arrow(L, reps, a.comment)
    if a.comment:
        cols = ["l_comment"] + cols
    delta_knobs = {"store_decimal_as_integer": True,
                   "column_encoding": {c: "DELTA_LENGTH_BYTE_ARRAY" if c == "l_comment" else "DELTA_BINARY_PACKED" for c in cols if c not in varchar}}
    more, dictionary = {}, varchar
    if delta:
        more = delta_knobs
    if front:                                  # no dictionary pages for the VARCHAR columns: they are front-coded, and so is the comment
        dictionary = False
        more = {"column_encoding": {c: "DELTA_BYTE_ARRAY" for c in varchar + (["l_comment"] if a.comment else [])}}
    pq.write_table(table, path, compression="SNAPPY" if snappy else "LZ4_RAW" if lz4_raw else "GZIP" if gzip else "ZSTD" if zstd else "NONE", use_dictionary=dictionary,
                   row_group_size=1 << 20, **more)
    data = open(path, "rb").read()
    plain_data = delta_data = None
    if (delta or front) and not a.skip_plain:  # the file the script writes by default, for the same sitting
        pq.write_table(table, path, compression="NONE", use_dictionary=varchar, row_group_size=1 << 20)
        plain_data = open(path, "rb").read()
    if front and not a.skip_plain:             # and the --encoding delta file
        pq.write_table(table, path, compression="NONE", use_dictionary=varchar, row_group_size=1 << 20, **delta_knobs)
        delta_data = open(path, "rb").read()
    del table
    nbytes = len(data)
    ctx = hip.Ctx(0)
    res = {"bench": "parquet_load", "file_bytes": nbytes, "csv_equivalent_bytes": nrows * CSV_BYTES_PER_ROW, "rows": nrows, "columns": len(cols),
           "varchar_dictionary_columns": varchar, "warmup": a.warmup, "runs": a.runs}
    if snappy or lz4_raw or gzip or zstd:
        md = pq.ParquetFile(pa.BufferReader(data)).metadata
        res["compression"] = a.compression
        res["uncompressed_bytes"] = sum(md.row_group(g).column(k).total_uncompressed_size for g in range(md.num_row_groups) for k in range(md.num_columns))

    if zstd and not a.device_only:
        tot = [0, 0, 0, 0, 0]
        for k in range(len(cols)):
            for p in loader.parquet_pages(data, k, codecs=True):
                if p["compressed"]:
                    lv = p["rep_levels_bytes"] + p["def_levels_bytes"]
                    st = hip.zstd_stream_stats_host(data[p["data_pos"] + lv:p["data_pos"] + p["data_bytes"]], p["uncompressed_bytes"] - lv)
                    tot = [tot[0] + 1] + [x + y for x, y in zip(tot[1:], st)]
        res["zstd_stats"] = {"sections": tot[0], "literal_bytes": tot[1], "sequences": tot[2], "match_bytes": tot[3], "match_bytes_beyond_ring": tot[4],
                             "beyond_ring_share": round(tot[4] / max(tot[3], 1), 4)}
    if delta or front:
        res["encoding"] = a.encoding
    if a.comment:
        res["comment_column"] = True

    def device_load(columns=None, source=None, how=None):
        t = loader.table_from_parquet_device(ctx, data if source is None else source, columns, flags=flags if how is None else how)
        assert t.nrows == nrows
        t.free()
    if plain_data is not None:
        ps = timed(lambda: device_load(None, plain_data, 0), a.warmup, a.runs)
        res["plain_file_bytes"] = len(plain_data)
        res["plain_parquet_e2e_ms"] = [round(x * 1e3, 2) for x in ps]
        if not a.device_only:
            res["plain_q1_e2e_ms"] = [round(x * 1e3, 2) for x in timed(lambda: device_load(Q1_COLUMNS, plain_data, 0), a.warmup, a.runs)]
    if delta_data is not None:
        ds = timed(lambda: device_load(None, delta_data, hip.PH_PARQUET_DELTA), a.warmup, a.runs)
        res["delta_file_bytes"] = len(delta_data)
        res["delta_parquet_e2e_ms"] = [round(x * 1e3, 2) for x in ds]
    s = timed(device_load, a.warmup, a.runs)
    if plain_data is not None:
        res["front_over_plain" if front else "delta_over_plain"] = round(statistics.median(s) / statistics.median(ps), 3)
    if delta_data is not None:
        res["front_over_delta"] = round(statistics.median(s) / statistics.median(ds), 3)
    res["parquet_e2e_ms"] = [round(x * 1e3, 2) for x in s]
    res["parquet_e2e_gbps"] = round(nbytes / statistics.median(s) / 1e9, 3)
    res["parquet_rows_per_s"] = round(nrows / statistics.median(s))
    if not a.device_only:
        q1 = timed(lambda: device_load(Q1_COLUMNS), a.warmup, a.runs)
        res["q1_e2e_ms"] = [round(x * 1e3, 2) for x in q1]
        dev = ctx.alloc(nbytes)

        def upload():
            hip.check(hip.lib().ph_dev_upload(ctx.h, dev, data, hip.i64(nbytes)))   # synchronises before it returns
        h2d = timed(upload, a.warmup, a.runs)
        ctx.free(dev)
        res["h2d_ms"] = [round(x * 1e3, 2) for x in h2d]
        res["h2d_gbps"] = round(nbytes / statistics.median(h2d) / 1e9, 3)
        res["parquet_after_upload_share"] = round(1 - statistics.median(h2d) / statistics.median(s), 3)
        pa.set_cpu_count(16)
        pa.set_io_thread_count(16)

        def arrow_load():
            t = loader.table_from_arrow_c(ctx, pq.read_table(pa.BufferReader(data), columns=cols, use_threads=True))
            assert t.nrows == nrows
            t.free()
        ar = timed(arrow_load, 1, a.arrow_runs)
        res["arrow_runs"] = a.arrow_runs
        res["arrow_e2e_ms"] = [round(x * 1e3, 2) for x in ar]
        res["device_over_arrow"] = round(statistics.median(ar) / statistics.median(s), 2)
    ctx.close()
    if tmp is not None:
        os.unlink(path)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
