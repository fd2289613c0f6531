"""ph_table_concat: resident pieces of lineitem -> one resident table on the device, against a device-to-device copy of the same bytes
and against the route a user had before (one Parquet file holding all the rows through ph_table_create_parquet).

  python scripts/bench_table_concat.py [--gb 1.0] [--warmup 3] [--runs 10] [--pieces 4,1024] [--comment] [--only N] [--out FILE]

The rows are the SF0.01 lineitem (every SCHEMA column) repeated to about --gb gigabytes of CSV-equivalent text (about 7.4 M rows at 1.0),
as scripts/bench_parquet_load.py builds them. The pieces are row ranges of that table, each loaded through
loader.table_from_parquet_device from a Parquet buffer of its own. Reported (medians over the timed runs, one JSON line):
  concat_ms[N]       wall time of ph_table_concat over N equal pieces (the call returns synchronised; freeing the result is not timed)
  d2d_ms             a device-to-device copy of table_bytes, the bytes of the result's column arrays: the bound for moving them once
  concat_gbps[N] / d2d_gbps   bytes read plus bytes written (2 x table_bytes) per second
  parquet_e2e_ms     loader.table_from_parquet_device of the one file with all rows (upload, decode, finishing)
  pieces_hi_over_lo  concat_ms of the largest piece count over the smallest: launches and read-backs do not depend on the count
  result_types       the result's column types (5 = PH_CODE8, 8 = PH_STR), and code_columns_identical: whether the pieces' dictionaries
                     were identical (codes copied) or merged (codes rewritten)
--comment adds an l_comment text column (PH_STR in every piece: the VARCHAR path with its scan and byte copy).
--only N runs ph_table_concat over N pieces and nothing else timed: for `rocprofv3 --kernel-trace --stats`, whose table then shows how
much of the call the concatenation kernels take and how much ph::table_finish_column's statistics and narrowing kernels.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_parquet_load import CSV_BYTES_PER_ROW, lineitem_arrow, timed  # noqa: E402
from plan_amd import hip, loader, tpch, tpchgen  # noqa: E402

ROW_PAD = 8192


def table_bytes(t):
    """bytes of the table's column arrays as allocated: data, validity, VARCHAR bytes (narrowed copies not counted)"""
    padded = (max(t.nrows, 1) + ROW_PAD - 1) // ROW_PAD * ROW_PAD
    total = 0
    for k in range(t.ncols):
        c = t.col(k)
        total += (padded + 1) * 4 + int(c.aux_bytes) if c.type == hip.PH_STR else padded * hip.NP_TYPES[c.type]().itemsize
        total += padded // 8 if c.validity else 0
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--pieces", default="4,1024")
    ap.add_argument("--comment", action="store_true")
    ap.add_argument("--only", type=int, default=0, help="concatenate this many pieces and time nothing else (a profiler run)")
    ap.add_argument("--out")
    a = ap.parse_args()
    import pyarrow as pa
    import pyarrow.parquet as pq

    L = tpchgen.lineitem((1, 100), columns=[c for c, t, _s, _d in tpch.SCHEMA["lineitem"] if t != hip.PH_STR])
    n1 = len(L["l_orderkey"])
    reps = max(1, round(a.gb * 1e9 / (n1 * CSV_BYTES_PER_ROW)))
    nrows = n1 * reps
    table = lineitem_arrow(L, reps, a.comment).combine_chunks()
    varchar = [c for c, t, _s, _d in tpch.SCHEMA["lineitem"] if t in (hip.PH_CODE8, hip.PH_STR)]

    def parquet_of(tbl):
        sink = pa.BufferOutputStream()
        pq.write_table(tbl, sink, compression="NONE", use_dictionary=varchar, row_group_size=1 << 20)
        return sink.getvalue().to_pybytes()

    ctx = hip.Ctx(0)
    counts = [a.only] if a.only else [int(x) for x in a.pieces.split(",")]
    res = {"bench": "table_concat", "rows": nrows, "columns": table.num_columns, "comment_column": bool(a.comment), "warmup": a.warmup, "runs": a.runs}

    def pieces_of(n):
        bounds = [nrows * k // n for k in range(n + 1)]
        return [loader.table_from_parquet_device(ctx, parquet_of(table.slice(lo, hi - lo))) for lo, hi in zip(bounds, bounds[1:])]

    concat_ms = {}
    for n in counts:
        parts = pieces_of(n)
        times, h = [], None
        for k in range(a.warmup + a.runs):
            if h is not None:
                hip.lib().ph_table_free(h)                 # (not timed: hipFree waits for the device)
            t0 = time.perf_counter()
            h = hip.table_concat(ctx, parts)
            if k >= a.warmup:
                times.append(time.perf_counter() - t0)
        concat_ms[n] = [round(x * 1e3, 3) for x in times]
        t = hip.Table.__new__(hip.Table)
        t.ctx, t.h = ctx, h
        t.nrows, t.ncols = int(hip.lib().ph_table_rows(t.h)), table.num_columns
        assert t.nrows == nrows
        loader._attach_dicts(t)
        res["table_bytes"] = table_bytes(t)
        res["result_types"] = [int(t.col(k).type) for k in range(t.ncols)]
        res["code_columns_identical"] = all(p.dicts[k] == t.dicts[k] for p in parts for k in range(t.ncols) if p.col(k).type == hip.PH_CODE8)
        t.free()
        for p in parts:
            p.free()
    nbytes = res["table_bytes"]
    res["concat_ms"] = {str(n): v for n, v in concat_ms.items()}
    res["concat_gbps"] = {str(n): round(2 * nbytes / statistics.median(v) / 1e6, 1) for n, v in concat_ms.items()}
    if not a.only:
        import torch
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").zero_()
        dst = torch.empty_like(src)

        def copy():
            dst.copy_(src)
            torch.cuda.synchronize()
        d2d = timed(copy, a.warmup, a.runs)
        del src, dst
        res["d2d_ms"] = [round(x * 1e3, 3) for x in d2d]
        res["d2d_gbps"] = round(2 * nbytes / statistics.median(d2d) / 1e9, 1)
        res["concat_over_d2d"] = {str(n): round(statistics.median(v) / 1e3 / statistics.median(d2d), 2) for n, v in concat_ms.items()}
        if len(counts) > 1:
            res["pieces_hi_over_lo"] = round(statistics.median(concat_ms[max(counts)]) / statistics.median(concat_ms[min(counts)]), 3)
        data = parquet_of(table)
        res["file_bytes"] = len(data)

        def whole():
            t = loader.table_from_parquet_device(ctx, data)
            assert t.nrows == nrows
            t.free()
        res["parquet_e2e_ms"] = [round(x * 1e3, 2) for x in timed(whole, a.warmup, a.runs)]
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
