"""Text load path: lineitem .tbl text -> resident table through ph_table_create_csv, against pyarrow.csv + ph_table_create_arrow.

  python scripts/bench_csv_load.py [--gb 1.0] [--warmup 3] [--runs 10] [--arrow-runs 5] [--out FILE] [--device-only]
                                   [--quoting] [--quoted-text]

The text is the SF0.01 lineitem written as dbgen writes it (field order, '|' after every field, a filler comment) and repeated to
about --gb gigabytes: parse throughput does not depend on the key order. Reported (medians over the timed runs, one JSON line):
  csv_e2e_gbps       text bytes / wall time of loader.table_from_csv (upload, kernels, column finishing; the call returns synchronised)
  h2d_gbps           the same bytes through ph_dev_upload alone (pageable -> pinned staging -> device): the bound csv_e2e is read against
  csv_after_upload   share of the end-to-end time that is not the upload (kernels, scans, allocation, finishing), by difference
  arrow_e2e_gbps     pyarrow.csv.read_csv (16 threads) + loader.table_from_arrow_c over the same bytes and columns
--quoting loads the same text with PH_CSV_QUOTES (record starts by quote parity, the bounded field walk); --quoted-text (implies
--quoting) writes the four VARCHAR fields of every record between quotes first. The JSON line names the mode.
The per-kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python scripts/bench_csv_load.py --device-only` run.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plan_amd import hip, loader, tpch, tpchgen  # noqa: E402


def lineitem_tbl(L, quoted=False):
    n = len(L["l_orderkey"])
    fields = [["regular deposits haggle x"] * n for _ in tpch.TBL_COLUMNS["lineitem"]]
    for cname, typ, _scale, dic in tpch.SCHEMA["lineitem"]:
        v = L[cname]
        if typ == hip.PH_CODE8:
            col = np.array(dic)[v].tolist()
            if quoted:
                col = ['"%s"' % x for x in col]
        elif typ == hip.PH_DEC64:
            col = ["%d.%02d" % divmod(int(x), 100) for x in v.tolist()]
        elif typ == hip.PH_DATE:
            col = np.datetime_as_string(v.astype("int64").astype("datetime64[D]")).tolist()
        else:
            col = [str(x) for x in v.tolist()]
        fields[tpch.TBL_FIELDS["lineitem"][cname]] = col
    return "".join("|".join(r) + "|\n" for r in zip(*fields)).encode()


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
    ap.add_argument("--device-only", action="store_true", help="the device path alone (for a profiler run)")
    ap.add_argument("--quoting", action="store_true", help="load with PH_CSV_QUOTES")
    ap.add_argument("--quoted-text", action="store_true", help="the four VARCHAR fields of every record quoted (implies --quoting)")
    a = ap.parse_args()
    quoting = a.quoting or a.quoted_text

    cols = [c for c, _t, _s, _d in tpch.SCHEMA["lineitem"]]
    one = lineitem_tbl(tpchgen.lineitem((1, 100), columns=cols), a.quoted_text)
    reps = max(1, round(a.gb * 1e9 / len(one)))
    text = one * reps
    nbytes, nrows = len(text), one.count(b"\n") * reps
    spec = [(c, tpch.TBL_FIELDS["lineitem"][c], hip.PH_STR if typ == hip.PH_CODE8 else typ, scale) for c, typ, scale, _d in tpch.SCHEMA["lineitem"]]
    ctx = hip.Ctx(0)
    res = {"bench": "csv_load", "mode": "quoted_text" if a.quoted_text else "quoting" if quoting else "default", "text_bytes": nbytes, "rows": nrows, "columns": len(spec), "warmup": a.warmup, "runs": a.runs}

    def device_load():
        t = loader.table_from_csv(ctx, text, spec, quoting=True) if quoting else loader.table_from_csv(ctx, text, spec)
        assert t.nrows == nrows
        t.free()
    csv_s = timed(device_load, a.warmup, a.runs)
    res["csv_e2e_ms"] = [round(s * 1e3, 2) for s in csv_s]
    res["csv_e2e_gbps"] = round(nbytes / statistics.median(csv_s) / 1e9, 3)
    if not a.device_only:
        dev = ctx.alloc(nbytes)

        def upload():
            hip.check(hip.lib().ph_dev_upload(ctx.h, dev, text, hip.i64(nbytes)))   # synchronises before it returns
        h2d_s = timed(upload, a.warmup, a.runs)
        ctx.free(dev)
        res["h2d_ms"] = [round(s * 1e3, 2) for s in h2d_s]
        res["h2d_gbps"] = round(nbytes / statistics.median(h2d_s) / 1e9, 3)
        res["csv_after_upload_share"] = round(1 - statistics.median(h2d_s) / statistics.median(csv_s), 3)

        import pyarrow as pa
        import pyarrow.csv as pacsv
        pa.set_cpu_count(16)
        pa.set_io_thread_count(16)
        names = tpch.TBL_COLUMNS["lineitem"] + ["trailing"]
        pa_type = {hip.PH_I32: pa.int32(), hip.PH_I64: pa.int64(), hip.PH_DATE: pa.date32(), hip.PH_DEC64: pa.decimal128(15, 2), hip.PH_CODE8: pa.string()}
        types = {c: pa_type[typ] for c, typ, _s, _d in tpch.SCHEMA["lineitem"]}

        def arrow_load():
            tbl = pacsv.read_csv(pa.BufferReader(text), read_options=pacsv.ReadOptions(use_threads=True, column_names=names),
                                 parse_options=pacsv.ParseOptions(delimiter="|", quote_char='"' if a.quoted_text else False),
                                 convert_options=pacsv.ConvertOptions(column_types=types, include_columns=cols, strings_can_be_null=False))
            t = loader.table_from_arrow_c(ctx, tbl)
            assert t.nrows == nrows
            t.free()
        arrow_s = timed(arrow_load, 1, a.arrow_runs)
        res["arrow_runs"] = a.arrow_runs
        res["arrow_e2e_ms"] = [round(s * 1e3, 2) for s in arrow_s]
        res["arrow_e2e_gbps"] = round(nbytes / statistics.median(arrow_s) / 1e9, 3)
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
