#!/usr/bin/env python3
"""bench.py — throughput of the hot path on MI355X, one process per GPU.

Headline: a "step" is one pass of the fused Agg <- Scan(filter) pipeline (TPC-H Q1: filter +
4-group hash aggregate, 8 aggregates) over the rank's device-resident lineitem shard, plus — for
N > 1 — the merge of the per-rank partial group rows (a few hundred bytes, all-gathered over RCCL
through the C ABI's ph_comm_allgather, asynchronously behind the next step's scan).
The Q1/Q6 data path needs no collective: lineitem is partitioned by order ranges across ranks.
  --scaling weak   (default) every rank holds an SF`--sf` shard of an SF(sf*N) database
  --scaling strong the SF`--sf` database is split N ways

`python bench.py --gpus N` without a launcher starts the N ranks itself (a torch.distributed.run
child, before anything touches the GPU in this process).

ONE JSON line on rank 0 (driver contract). A plain run sets up, warms up, times --steps steps and
prints the contract's fields (metric, value, unit, higher_is_better, dtype, ms_per_step, ...) and the
workload's config; --dump-outputs DIR also writes what the last timed step computed as
DIR/<name>.npy (float64: the result's groups or rows, column by column, as a caller receives them;
the same arguments give the same generated inputs). --full adds, each measured after the timed steps:
  roofline       dominant kernel of the headline: algorithmic bytes / average launch duration from
                 HIP events on the launch stream; peak_measured = streaming-read ceiling measured in
                 this run (ph_dev_read_reduce); traffic = HBM bytes of the committed PMC passes
  stage_ms       (--query q3 / q9) per-stage times from extra steps with a host sync per stage
  cpu_baseline   the oracle (CPU restatement of the reference path, 1 thread) on a bounded sample
  N = 1: companions q6_single_gpu, q1_sf1, q3_single_gpu, q9_single_gpu, general_forms (every BASELINE.json
         config, each with its own roofline; Q3 / Q9 with their own cpu_baseline), and q3_operator_interface /
         q9_operator_interface: the same two queries through the C++ OperatorExec layer as one resident-plan executor
  N > 1: companions q3_partitioned, q3_partitionwise, q9_partitioned, q9_partitionwise — Q3 / Q9 over an SF`--sf` database split N
         ways (strong scaling, BASELINE.json configs 4 and 5), join sides hash-partitioned by order
         key and exchanged with ph_comm_exchange_columns, small build sides broadcast; probe rows/s
         and exchange bytes against the xGMI peak
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

Q1_BYTES_PER_ROW = 34  # qty 4 + ext/disc/tax 3x8 + flag 1 + status 1 + shipdate 4
Q6_BYTES_PER_ROW = 24
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
XGMI_PEAK_GBS = 7 * 153.0  # per GPU, all 7 links busy (MI355X_MICROARCH.md)


def pmc_traffic_any(q, names):
    """first of several kernel names (a kernel renamed between rounds) that a committed PMC summary knows"""
    for nm in names:
        t = pmc_traffic((q, nm))
        if t is not None:
            return t
    return None


def pmc_traffic(kernel_key):
    """HBM bytes per launch from the committed PMC passes (profiles/r0N_pmc_summary.json, newest
    round first: separate rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE runs of bench.py,
    scripts/pmc_r2.sh; KiB units, FETCH_SIZE x2 on gfx950 per MI355X_MICROARCH.md §HBM). Valid for
    the SF10 one-GPU workload those passes ran; the caller passes None otherwise."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_summary.json")), reverse=True):
        try:
            d = json.load(open(path))
            q, kern = kernel_key
            fetch = [e["avg"] for e in d[f"{q} FETCH_SIZE"] if kern in e["kernel"]][0]
            write = [e["avg"] for e in d.get(f"{q} WRITE_SIZE", []) if kern in e["kernel"]]
            return fetch * 1024 * 2 + (write[0] * 1024 if write else 0)
        except Exception:  # noqa: BLE001 - an older summary without this kernel: try the next
            continue
    return None


def spawn_ranks(args):
    """--gpus N without WORLD_SIZE: start the N ranks as a child torch.distributed.run. Nothing in
    this process has touched torch or HIP yet, and the launcher is a child, not an exec."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run(cmd, env=env)
    sys.exit(r.returncode)


class Harness:
    """per-process state shared by the query benches"""

    def __init__(self, args):
        import torch
        import torch.distributed as dist
        from plan_amd import dist as pdist, hip
        self.args, self.torch, self.dist, self.pdist, self.hip = args, torch, dist, pdist, hip
        self.rank = int(os.environ.get("RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU (torch.cuda.is_available() is False)")
        # Rehearsal knob for a one-GPU box: PH_BENCH_BACKEND=gloo puts every rank on device 0 and
        # carries the exchange protocol over gloo (the real runs: RCCL through the C ABI).
        self.backend = os.environ.get("PH_BENCH_BACKEND", "nccl")
        self.local_rank = local_rank if self.backend == "nccl" else 0
        torch.cuda.set_device(self.local_rank)
        # a non-default torch stream, shared with the library so torch.cuda.Event sees its kernels
        self.stream = torch.cuda.Stream()
        torch.cuda.set_stream(self.stream)
        self.ctx = hip.Ctx(self.local_rank, stream=self.stream.cuda_stream)
        self.comm = None
        if self.world > 1:
            # torch.distributed over gloo is only the host side channel (communicator id, object
            # gathers of the rehearsal); the data path is ph_comm = RCCL through the C ABI
            dist.init_process_group("gloo")
            if self.backend == "nccl":
                self.comm = pdist.init_rccl(self.ctx)

    def barrier(self):
        if self.comm is not None:
            self.comm.wait()
            self.comm.barrier()
        elif self.world > 1:
            self.torch.cuda.synchronize()
            self.dist.barrier()
        self.torch.cuda.synchronize()

    def allreduce(self, vals, op):
        if self.world == 1:
            return list(vals)
        if self.comm is not None:
            return self.comm.allreduce(vals, op)
        t = self.torch.tensor(vals, dtype=self.torch.int64)
        self.dist.all_reduce(t, op={"sum": self.dist.ReduceOp.SUM, "max": self.dist.ReduceOp.MAX}[op])
        return [int(x) for x in t.tolist()]

    def max_elapsed(self, seconds):
        return self.allreduce([int(seconds * 1e9)], "max")[0] / 1e9

    def events_ms(self, fn, reps):
        """average / min duration of fn() from HIP events on the launch stream"""
        T = self.torch
        ev = [(T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record(self.stream)
            fn()
            b.record(self.stream)
        T.cuda.synchronize()
        d = sorted(a.elapsed_time(b) for a, b in ev)
        return sum(d) / len(d), d[0]

    def peak_measured(self):
        """streaming-read ceiling: read-only reduce over 2 GiB (>> the 256 MiB Infinity Cache)"""
        nbytes = 2 << 30
        buf = self.ctx.alloc(nbytes)
        out = self.ctx.alloc(8 * 4096)
        self.hip.check(self.hip.lib().ph_dev_memset(self.ctx.h, buf, 1, self.hip.i64(nbytes)))
        best = 0.0
        for grid in (256, 512, 1024):
            self.hip.read_reduce(self.ctx, buf, nbytes, out, grid)
            avg, _ = self.events_ms(lambda: self.hip.read_reduce(self.ctx, buf, nbytes, out, grid), 10)
            best = max(best, nbytes / (avg * 1e-3) / 1e9)
        self.ctx.free(buf)
        self.ctx.free(out)
        return best

    def close(self):
        if self.comm is not None:
            self.comm.close()
        self.ctx.close()
        if self.world > 1:
            self.dist.destroy_process_group()


def shard_orders(h, sf, scaling):
    """(sf_total, first order, number of orders) of this rank's shard"""
    from plan_amd import tpchgen
    if scaling == "weak":
        n = tpchgen.orders_count((sf, 1))
        return (sf * h.world, 1), h.rank * n, n
    n = tpchgen.orders_count((sf, 1))
    a, b = h.rank * n // h.world, (h.rank + 1) * n // h.world
    return (sf, 1), a, b - a


def roofline(achieved, **extra):
    d = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS}
    d.update(extra)
    return d


# ---------------------------------------------------------------------------------- outputs (--dump-outputs)

def agg_outputs(r):
    """A fused scan plan's result (ScanPlan.fetch / fetch_merged) as float64 arrays, groups in key order:
    keys (codes; none without GROUP BY), sum (every aggregate's exact sum as its decimal value), count (rows per aggregate)."""
    import numpy as np
    keys, na = r["keys"], len(r["scale"])
    order = np.lexsort(keys.T[::-1]) if keys.shape[1] else np.arange(r["ngroups"])
    sums = np.array([[v / 10 ** sc for v, sc in zip(row, r["scale"])] for row in r["sum"]], dtype=np.float64).reshape(-1, na)
    counts = np.array(r["count"], dtype=np.float64).reshape(-1, na)
    out = {"sum": sums[order], "count": counts[order]}
    if keys.shape[1]:
        out["keys"] = keys[order].astype(np.float64)
    return out


def q3_outputs(top):
    """Q3's top-10 rows (revenue desc, o_orderdate), column by column; revenue as its decimal value"""
    import numpy as np
    return {"l_orderkey": np.array([t[0] for t in top], dtype=np.float64),
            "revenue": np.array([t[1] / 10 ** 4 for t in top], dtype=np.float64),
            "o_orderdate": np.array([t[2] for t in top], dtype=np.float64),
            "o_shippriority": np.array([t[3] for t in top], dtype=np.float64)}


def q9_outputs(rows):
    """Q9's groups ordered by (nation key, year); sum_profit as its decimal value"""
    import numpy as np
    rows = sorted(rows, key=lambda x: (x[0], x[1]))
    return {"nationkey": np.array([x[0] for x in rows], dtype=np.float64),
            "o_year": np.array([x[1] for x in rows], dtype=np.float64),
            "sum_profit": np.array([x[2] / 10 ** 4 for x in rows], dtype=np.float64)}


def write_outputs(path, outputs):
    """DIR/<name>.npy per array (the results are a few hundred values: far below the 64 MB bound)"""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name, arr in outputs.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(arr, dtype=np.float64))


# ---------------------------------------------------------------------------------- Q1 / Q6

def bench_scan(h, query, sf, steps, warmup, scaling, L=None, table=None, with_exchange=True, full=True, outputs=None):
    """fused scan plan over this rank's lineitem shard; returns (line dict, L, table). full=False leaves out the
    roofline (extra event-timed launches); outputs (a dict) receives the last timed step's result arrays."""
    import numpy as np
    from plan_amd import queries, tpchgen
    ctx, hip = h.ctx, h.hip
    gen_s = load_s = 0.0
    if table is None:
        sf_total, first, n_ord = shard_orders(h, sf, scaling)
        t0 = time.time()
        L = tpchgen.lineitem(sf_total, first, n_ord, columns=["l_quantity", "l_extendedprice", "l_discount", "l_tax",
                                                               "l_returnflag", "l_linestatus", "l_shipdate"])
        gen_s = time.time() - t0
        t0 = time.time()
        table = queries.lineitem_table(ctx, L)
        load_s = time.time() - t0
    nrows = table.nrows
    make = (lambda: queries.q1_plan(ctx, table)) if query == "q1" else (lambda: queries.q6_plan(ctx, table))
    bytes_per_row = Q1_BYTES_PER_ROW if query == "q1" else Q6_BYTES_PER_ROW
    exchange = with_exchange and h.world > 1
    # N > 1: two plans (two partial-result buffers) alternate; the all-gather of step i runs on the
    # communicator's stream and overlaps the scan of step i+1, which writes the OTHER buffer; a
    # buffer's collective is waited for (stream-side) before its plan runs again.
    plans = [make()] + ([make()] if exchange else [])
    gath, nwords = [], 0
    if exchange:
        for pl in plans:
            ptr, nwords = pl.partials_dev()
            gath.append((hip.vp(ptr), ctx.alloc(h.world * nwords * 8)))
    state = {"i": 0}

    def step():
        b = state["i"] % len(plans)
        state["i"] += 1
        if exchange and h.comm is not None:
            h.comm.wait(keep=1)   # the collective that read THIS buffer (two steps ago) is done; the last one may still run
        plans[b].run()
        if exchange:
            if h.comm is not None:
                h.comm.allgather(gath[b][0], gath[b][1], nwords * 8, async_=True)
            else:  # gloo rehearsal: through host memory
                mine = ctx.download(gath[b][0], np.uint64, nwords)
                state["host"] = np.concatenate(h.pdist._gather_objects(mine))

    def merged_result():
        if not exchange:
            return plans[0].fetch()
        last = (state["i"] - 1) % len(plans)
        if h.comm is not None:
            h.comm.wait()
            words = ctx.download(gath[last][1], np.uint64, h.world * nwords)
        else:
            words = state["host"]
        return plans[last].fetch_merged(words, h.world)

    for _ in range(warmup):
        step()
    result = merged_result()
    h.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    h.barrier()
    elapsed = h.max_elapsed(time.perf_counter() - t0)
    result = merged_result()
    if outputs is not None:
        outputs.update(agg_outputs(result))
    total_rows = h.allreduce([nrows], "sum")[0] if with_exchange else nrows
    line = {
        "metric": "rows/sec through hash-agg (Q1)" if query == "q1" else "rows/sec through filter+SUM (Q6)",
        "value": total_rows * steps / elapsed, "unit": "rows/s", "n_gpus": h.world if with_exchange else 1,
        "steps": steps, "warmup": warmup, "ms_per_step": elapsed / steps * 1e3, "higher_is_better": True,
        "scaling": scaling, "vs_baseline": None, "dtype": "int64", "data": "synthetic",
        "config": {
            "workload": f"TPC-H {query.upper()} fused filter+hash-aggregate over lineitem, {nrows} rows on rank 0, "
                        f"{total_rows} in total ({'SF%d per GPU' % sf if scaling == 'weak' else 'SF%d split %d ways' % (sf, h.world)}), "
                        "table resident in HBM",
            "rows_per_gpu": nrows, "kernel_family": plans[0].kind, "groups": result["ngroups"],
            "rows_aggregated": sum(c[-1] for c in result["count"]) if query == "q1" else result["count"][0][0] if result["ngroups"] else 0,
            "parallelism": (f"row-range shards x{h.world}; per step the raw partial group rows ({nwords * 8} B) are "
                            f"all-gathered with ph_comm_allgather ({'RCCL' if h.comm is not None else 'gloo rehearsal'}) "
                            "asynchronously behind the next step's scan") if exchange else "single GPU",
            "generate_s": round(gen_s, 2), "pcie_load_s": round(load_s, 2),
        },
    }
    if full:
        # roofline: per-launch duration of one ph_scan_plan_run (scan kernel + the 1-wave merge kernel)
        avg_ms, min_ms = h.events_ms(plans[0].run, steps)
        achieved = nrows * bytes_per_row / (avg_ms * 1e-3) / 1e9
        kern = "lowcard_chain_kernel" if query == "q1" else "filter_sumprod_kernel"
        traffic = pmc_traffic((query, kern)) if (h.world == 1 and nrows == 59986052) else None
        line["roofline"] = roofline(achieved, traffic=traffic, kernel=kern, avg_launch_ms=avg_ms, min_launch_ms=min_ms,
                                    algorithmic_bytes_per_launch=nrows * bytes_per_row)
    for pl in plans:
        pl.free()
    for _, g in gath:
        ctx.free(g)
    return line, L, table


# ---------------------------------------------------------------------------------- Q3

def bench_q3(h, sf, steps, warmup, scaling, partitionwise=False, full=True, outputs=None):
    """Q3: customer |x| orders |x| lineitem hash joins + 3-column group-by from the operator-granular
    kernels; N > 1: join sides hash-partitioned by order key and exchanged (plan_amd/pipelines.py).
    A step = one whole Q3, tables resident, top-10 rows on the host at the end. full=False leaves out
    the stage timings and the roofline (extra steps and launches after the timed region)."""
    from plan_amd import pipelines, tpchgen
    T = h.torch
    sf_total, first, n_ord = shard_orders(h, sf, scaling)
    tot_ord = tpchgen.orders_count(sf_total)
    tot_cust = tot_ord // 10
    c0, c1 = h.rank * tot_cust // h.world, (h.rank + 1) * tot_cust // h.world
    L = tpchgen.lineitem(sf_total, first, n_ord, columns=["l_orderkey", "l_extendedprice", "l_discount", "l_shipdate"])
    Od = tpchgen.orders(sf_total, first, n_ord, columns=["o_orderkey", "o_custkey", "o_orderdate", "o_shippriority"])
    C = tpchgen.customer(sf_total, c0, c1 - c0)
    nrows, n_o, n_c = len(L["l_orderkey"]), len(Od["o_orderkey"]), len(C["c_custkey"])
    pipe = pipelines.Q3Pipeline(h.ctx, L, Od, C)
    # N > 1: the hash-partitioned exchange plan (BASELINE.json config 4) unless the caller asks for the
    # partition-wise join that the shards' co-partitioning by order key allows (reported beside it)
    pipe.allow_partitionwise = partitionwise
    pw = h.world > 1 and partitionwise and pipe.copartitioned
    pipe.time_stages = False   # the measured steps run without a host sync per stage
    for _ in range(warmup):
        r = pipe.run()
    h.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        r = pipe.run()
    h.barrier()
    elapsed = h.max_elapsed(time.perf_counter() - t0)
    if outputs is not None:
        outputs.update(q3_outputs(r["top"]))
    total_rows = h.allreduce([nrows], "sum")[0]
    ms_step = elapsed / steps * 1e3
    line = {
        "metric": "rows/sec through hash-join probe + hash-agg (Q3)",
        "value": total_rows * steps / elapsed, "unit": "rows/s", "n_gpus": h.world, "steps": steps, "warmup": warmup,
        "ms_per_step": ms_step, "higher_is_better": True, "scaling": scaling, "vs_baseline": None, "dtype": "int64",
        "data": "synthetic",
        "config": {
            "workload": f"TPC-H Q3 over customer/orders/lineitem, {nrows} lineitem rows on rank 0, {total_rows} in total "
                        f"({'SF%d per GPU' % sf if scaling == 'weak' else 'SF%d split %d ways' % (sf, h.world)}), tables resident in HBM",
            "join_rows_rank0": r["join_rows"],
            "parallelism": ("partition-wise join: the ranks' order-key ranges are disjoint and hold their own lineitem rows (statistic "
                            "all-gathered at load), so only the customer keys are broadcast (ph_comm_allgather_rows) and the top-10 "
                            f"candidates merged; x{h.world} ({'RCCL' if h.comm is not None else 'gloo rehearsal'})") if pw else
                           (f"customer keys broadcast (ph_comm_allgather_rows), orders and lineitem rows hash-partitioned by order key "
                            f"x{h.world} (ph_partition_dev) and exchanged with ph_comm_exchange_columns "
                            f"({'RCCL' if h.comm is not None else 'gloo rehearsal'})") if h.world > 1 else "single GPU",
            "top1": list(r["top"][0]) if r["top"] else None,
        },
    }
    if not full:
        pipe.free()
        return line
    # stage times for the report: a few extra steps, outside the timed region, with a sync per stage
    pipe.time_stages = True
    ev = (T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True))
    pipe.probe_events = ev
    probe_dev_ms, agg_t, stage_steps = 0.0, {}, min(steps, 10)
    for _ in range(stage_steps):
        r = pipe.run()
        for k, v in r["timings"].items():
            agg_t[k] = agg_t.get(k, 0) + v
        if "lineitem_filter_probe" in r["timings"]:
            T.cuda.synchronize()
            probe_dev_ms += ev[0].elapsed_time(ev[1])
    h.barrier()
    probe_rows = agg_t["probe_rows"] / stage_steps
    fused = "lineitem_filter_probe" in agg_t
    probe_ms = agg_t["lineitem_filter_probe" if fused else "lineitem_probe"] / stage_steps * 1e3
    host_probe_ms = probe_ms
    if fused and probe_dev_ms > 0:
        probe_ms = probe_dev_ms / stage_steps   # HIP events on the launch stream: the stage's kernels only
    pairs = r["join_rows"]
    kept = pipe.lineitem_filter_rows()
    # probe-stage algorithmic bytes, counted once (BASELINE.md's Q3 row): fused Filter -> probe reads
    # every lineitem row's l_shipdate (4 B) and 16 B per row the filter keeps (selection entry 4 + key
    # 8 + bucket head 4), plus per output pair next 4 + build key 8 + the pair 8 + its selection
    # entry 4. Implementation passes (candidate slices, the emit kernel's second walk) are NOT counted.
    probe_bytes = (nrows * 4 + kept * 16 + pairs * 24) if fused else (probe_rows * 16 + pairs * 24)
    # whole query: inputs read once + 16 B per build row written + 16 B per probe row
    # read + 32 B per join-output row for the group table
    build_rows = r.get("build_rows", 0)
    whole_bytes = n_c * 5 + n_o * 20 + nrows * 28 + build_rows * 16 + (kept + pipe.orders_filter_rows()) * 16 + pairs * 32
    sent = agg_t.get("exchange_bytes_sent", 0) / stage_steps
    exch_ms = agg_t.get("lineitem_exchange", 0) / stage_steps * 1e3
    line["config"].update({
        "groups_rank0": r["ngroups"], "join_rows_rank0": pairs,
        "stage_ms": {kk: round(v / stage_steps * 1e3, 3) for kk, v in agg_t.items() if kk not in ("probe_rows", "exchange_bytes_sent")},
        "stage_ms_note": f"{stage_steps} extra steps after the timed region, one host sync per stage (the timed steps have none)",
        "probe_rows_per_s": probe_rows / (probe_ms * 1e-3),
    })
    line["roofline"] = roofline(probe_bytes / (probe_ms * 1e-3) / 1e9,
                                traffic=pmc_traffic_any("q3", ("direct_cand_vec_kernel<8", "join_cand_vec_kernel<8", "join_cand_fast_kernel<8")) if (h.world == 1 and nrows == 59986052) else None,
                                traffic_note="PMC traffic of the lineitem candidate kernel (direct_cand_vec_kernel<8,1>: l_shipdate + l_orderkey streamed, "
                                             "the occupancy bitmap of the gated orders table, its slots only for matching rows; ~138 of ~155 us); "
                                             "traffic_stage_kernels has the stage's other kernel",
                                traffic_stage_kernels=({k: pmc_traffic(("q3", k)) for k in ("direct_emit_kernel",)}
                                                       if (h.world == 1 and nrows == 59986052) else None),
                                kernel="direct_cand_vec_kernel+scan+direct_emit_kernel (lineitem Filter+probe stage against the gated orders table)"
                                       if (h.world == 1 or pw) else "join_cand_vec_kernel+join_chain_fast_kernel+scan+join_emit_kernel (lineitem Filter+probe stage)",
                                avg_launch_ms=probe_ms, algorithmic_bytes_per_launch=probe_bytes,
                                timing="HIP events on the launch stream around the stage" if fused and probe_dev_ms > 0 else "host clock around the stage",
                                host_timed_stage_ms=host_probe_ms,
                                whole_query={"algorithmic_bytes": whole_bytes, "achieved": whole_bytes / (ms_step * 1e-3) / 1e9,
                                             "frac": whole_bytes / (ms_step * 1e-3) / 1e9 / HBM_PEAK_GBS})
    if h.world > 1:
        line["exchange"] = {"bytes_sent_rank0_per_step": sent, "lineitem_exchange_ms": exch_ms,
                            "achieved_GBps": sent / (exch_ms * 1e-3) / 1e9 if exch_ms > 0 else None,
                            "xgmi_peak_GBps": XGMI_PEAK_GBS, "note": "lineitem side of the order-key stage: 24 B per row sent to other ranks"}
    pipe.free()
    return line


# ---------------------------------------------------------------------------------- Q9

def bench_q9(h, sf, steps, warmup, scaling="weak", partitionwise=False, full=True, outputs=None):
    """Q9: LIKE + four hash joins (one composite) + profit expression + 175-group aggregate
    (plan_amd/pipelines.py Q9Pipeline). A step = one whole Q9. N > 1: every table sharded by row ranges,
    the small build sides broadcast, lineitem x orders hash-partitioned by order key (two all-to-alls).
    full=False leaves out the stage timings and the roofline (extra steps and launches after the timed region)."""
    from plan_amd import pipelines, tpchgen
    sf_total, first, n_ord = shard_orders(h, sf, scaling)
    L = tpchgen.lineitem(sf_total, first, n_ord, columns=["l_orderkey", "l_partkey", "l_suppkey", "l_quantity", "l_extendedprice", "l_discount"])
    Od = tpchgen.orders(sf_total, first, n_ord, columns=["o_orderkey", "o_orderdate"])
    tot_p = int(tpchgen.lib().tpchgen_part_count(tpchgen._i64(sf_total[0]), tpchgen._i64(sf_total[1])))
    tot_s = int(tpchgen.lib().tpchgen_supplier_count(tpchgen._i64(sf_total[0]), tpchgen._i64(sf_total[1])))
    p0, p1 = h.rank * tot_p // h.world, (h.rank + 1) * tot_p // h.world
    s0, s1 = h.rank * tot_s // h.world, (h.rank + 1) * tot_s // h.world
    P, PS, S = tpchgen.part(sf_total, p0, p1 - p0), tpchgen.partsupp(sf_total, p0, p1 - p0), tpchgen.supplier(sf_total, s0, s1 - s0)
    nrows = len(L["l_orderkey"])
    pipe = pipelines.Q9Pipeline(h.ctx, L, Od, P, PS, S)
    pipe.allow_partitionwise = partitionwise   # N > 1: the order-key stage exchanged (BASELINE.json config 5) or rank-local
    pw = h.world > 1 and partitionwise and pipe.copartitioned
    pipe.time_stages = False
    for _ in range(warmup):
        r = pipe.run()
    h.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        r = pipe.run()
    h.barrier()
    elapsed = h.max_elapsed(time.perf_counter() - t0)
    if outputs is not None:
        outputs.update(q9_outputs(r["rows"]))
    total_rows = h.allreduce([nrows], "sum")[0]
    ms_step = elapsed / steps * 1e3
    line = {
        "metric": "rows/sec through 4 hash joins + hash-agg (Q9)", "value": total_rows * steps / elapsed, "unit": "rows/s",
        "n_gpus": h.world, "steps": steps, "warmup": warmup, "ms_per_step": ms_step, "higher_is_better": True, "scaling": scaling,
        "dtype": "int64",
        "config": {"workload": f"TPC-H Q9, {nrows} lineitem rows on rank 0, {total_rows} in total "
                               f"({'SF%d per GPU' % sf if scaling == 'weak' else 'SF%d split %d ways' % (sf, h.world)}), tables resident in HBM",
                   "groups": r["ngroups"], "join_rows_rank0": r["join_rows"],
                   "parallelism": ("pink part keys, their partsupp rows and supplier broadcast (ph_comm_allgather_rows); lineitem x orders "
                                   "partition-wise (the shards are co-partitioned by order key: statistic all-gathered at load), the 175 partial "
                                   f"groups merged; x{h.world} ({'RCCL' if h.comm is not None else 'gloo rehearsal'})") if pw else
                                  ("pink part keys, their partsupp rows and supplier broadcast (ph_comm_allgather_rows); the intermediate and orders "
                                   f"hash-partitioned by order key x{h.world} and exchanged with ph_comm_exchange_columns "
                                   f"({'RCCL' if h.comm is not None else 'gloo rehearsal'})") if h.world > 1 else "single GPU"},
    }
    if not full:
        pipe.free()
        return line
    pipe.time_stages = True
    agg_t, stage_steps = {}, min(steps, 10)
    for _ in range(stage_steps):
        r = pipe.run()
        for k, v in r["timings"].items():
            agg_t[k] = agg_t.get(k, 0) + v
    line["config"].update({
        "exchange_bytes_sent_rank0_per_step": (agg_t.get("exchange_bytes_sent", 0) / stage_steps) if h.world > 1 else 0,
        "stage_ms": {kk: round(v / stage_steps * 1e3, 3) for kk, v in agg_t.items() if kk != "exchange_bytes_sent"},
        "stage_ms_note": f"{stage_steps} extra steps after the timed region, one host sync per stage"})
    # algorithmic bytes, SURVEY §8(d)'s accounting over the six inputs, each read once:
    # lineitem (partkey 4 + suppkey 4 + orderkey 8 + ext 8 + disc 8 + qty 4 = 36 B), part (key 4 +
    # name offsets 4 + name bytes), partsupp (4+4+8), supplier (4+4), orders (8+4), nation negligible
    inputs = (nrows * 36 + len(P["p_partkey"]) * 8 + len(P["p_name_bytes"]) + len(PS["ps_partkey"]) * 16 +
              len(S["s_suppkey"]) * 8 + len(Od["o_orderkey"]) * 12)
    # the dominant kernel, timed live with HIP events on the launch stream over the same row ids: the late
    # materialisation of five lineitem columns at the rows that survive the part join (ph_gather_multi)
    pipe.keep_gather_ids = True
    pipe.time_stages = False
    pipe.run()
    pipe.keep_gather_ids = False
    ids, n1 = pipe.kept_gather_ids
    gcols = [pipe.l_supp, pipe.l_key, pipe.l_ext, pipe.l_disc, pipe.l_qty]
    colocated = pipe.l_tab.colocated([0, 1, 2, 3, 4])
    T = h.torch
    ev = [T.cuda.Event(enable_timing=True) for _ in range(2)]
    reps = 20
    for w in range(2):
        ev[0].record()
        for _ in range(reps):
            for o in h.hip.gather_multi(h.ctx, gcols, ids, n1):
                h.ctx.free(o)
        ev[1].record()
        T.cuda.synchronize()
    gm_ms = ev[0].elapsed_time(ev[1]) / reps
    h.ctx.free(ids)
    gm_bytes = n1 * (4 + 2 * (4 + 8 + 8 + 8 + 4))   # row id + the five values read and written once
    line["roofline"] = roofline(gm_bytes / (gm_ms * 1e-3) / 1e9,
                                traffic=pmc_traffic(("q9", "gather_group_kernel" if colocated else "gather_multi_kernel")) if (h.world == 1 and nrows == 59986052) else None,
                                kernel=("gather_group_kernel" if colocated else "gather_multi_kernel") +
                                       " (the late materialisation: five lineitem columns at the ~5 % of rows that survive the part join" +
                                       ("; read from their co-located copy, ph_table_colocate: 32 bytes per row side by side)" if colocated else ")"),
                                avg_launch_ms=gm_ms, algorithmic_bytes_per_launch=gm_bytes,
                                timing="HIP events on the launch stream around 20 launches over the query's own row ids",
                                note=("one sector per surviving row id out of the co-located copy; out of the five column arrays every 4- or 8-byte value "
                                      "cost a line of its own (rounds 1-2: 1.27 GB of traffic, 245 us)") if colocated else
                                     ("every gathered 4- or 8-byte value costs one 128-byte line: traffic = the distinct lines the row ids touch "
                                      "(83 % of a 4-byte column's lines at 5.4 % row density)"),
                                whole_query={"algorithmic_bytes": inputs, "achieved": inputs / (ms_step * 1e-3) / 1e9,
                                             "frac": inputs / (ms_step * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                             "timing": "host clock around the timed steps (one query = ~38 launches)"})
    pipe.free()
    return line


# ---------------------------------------------------------------------------------- general operator forms

def bench_general_forms(h, sf):
    """The operator-granular forms a plan gets when NO statistic or hint applies ("far below roofline"): the hash
    aggregate at 65 536 groups over 32 M rows, and ph_join_build WITHOUT a key range over 15 M build keys + a 60 M-row inner
    probe — once with TPC-H order keys (dense in their range: the library reads the range off the column and takes the direct
    table) and once with random 62-bit keys probed in random order (the radix-partitioned form). Wall time per call around a
    stream synchronisation, best of 3 (scripts/bench_ops.py, scripts/join_auto_probe.py)."""
    import numpy as np
    from plan_amd import tpchgen
    hip, ctx = h.hip, h.ctx
    rng = np.random.default_rng(0)

    def best(f, reps=3):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); f(); ctx.sync(); ts.append(time.perf_counter() - t0)
        return min(ts)
    out = {}
    n = 32_000_000
    vals = hip.DevColumn(ctx, hip.PH_I64, rng.integers(0, 10**6, n).astype(np.int64))
    keys = hip.DevColumn(ctx, hip.PH_I64, rng.integers(0, 65536, n).astype(np.int64))

    def agg_run():
        agg = hip.Agg(ctx, [hip.PH_I64], [(hip.PH_A_SUM, 0), (hip.PH_A_COUNT_STAR, -1)], 65536)
        agg.sink([keys], [vals], None, n)
        agg.group_count()
        agg.free()
    agg_run()
    t = best(agg_run)
    out["agg_sink_65k_groups"] = {"rows": n, "groups": 65536, "ms": t * 1e3, "rows_per_s": n / t,
                                  "algorithmic_GBps": n * 16 / t / 1e9, "frac_of_hbm_peak": n * 16 / t / 1e9 / HBM_PEAK_GBS,
                                  "form": "bulk build, second form: count + LDS-staged scatter + sliced LDS tables + merge (4 passes over the rows' 16 B)"}
    keys.free()
    card4 = 4_000_000
    keys = hip.DevColumn(ctx, hip.PH_I64, rng.integers(0, card4, n).astype(np.int64))

    def agg_run4():
        agg = hip.Agg(ctx, [hip.PH_I64], [(hip.PH_A_SUM, 0), (hip.PH_A_COUNT_STAR, -1)], card4)
        agg.sink([keys], [vals], None, n)
        agg.group_count()
        agg.free()
    agg_run4()
    t = best(agg_run4)
    out["agg_sink_4m_groups"] = {"rows": n, "groups": card4, "ms": t * 1e3, "rows_per_s": n / t, "algorithmic_GBps": n * 16 / t / 1e9,
                                 "form": "bulk build, second form with two partition levels (64 x 128 bins), one workgroup per bin builds straight into the table"}
    vals.free(); keys.free()
    L = tpchgen.lineitem((sf, 1), columns=["l_orderkey"])
    O = tpchgen.orders((sf, 1), columns=["o_orderkey"])
    nl, no = len(L["l_orderkey"]), len(O["o_orderkey"])
    sparse = rng.integers(0, 2**62, no).astype(np.int64)
    cases = (("order_keys", O["o_orderkey"], L["l_orderkey"]), ("random_62bit_keys", sparse, sparse[rng.integers(0, no, nl)]))
    del L, O
    for name, bk, pk in cases:
        b, p = hip.DevColumn(ctx, hip.PH_I64, bk), hip.DevColumn(ctx, hip.PH_I64, pk)
        hip.Join(ctx, [b], None, no).free()
        tb = best(lambda: hip.Join(ctx, [b], None, no).free())
        j = hip.Join(ctx, [b], None, no)

        def probe():
            m, x, y = j.probe_inner([p], None, nl, nl)
            ctx.free(x); ctx.free(y)
            return m
        probe()
        tp = best(probe)
        out["join_unhinted_" + name] = {"build_rows": no, "probe_rows": nl, "table": j.kind, "build_ms": tb * 1e3, "probe_ms": tp * 1e3,
                                        "total_ms": (tb + tp) * 1e3, "probe_rows_per_s": nl / tp,
                                        "algorithmic_GBps": (no * 8 + nl * 8 + nl * 8) / (tb + tp) / 1e9}
        j.free(); b.free(); p.free()
    return out


# ---------------------------------------------------------------------------------- operator interface

def bench_operator_interface(h, sf, steps, warmup):
    """Q3 and Q9 behind the reference's OperatorExec interface: the C++ host layer (plan_amd/csrc/host, what the Go
    shim is written after) builds, for every step, the executor tree limitExecutor <- gpuOrderExecutor <-
    gpuResidentPlanExecutor over the resident database, pulls it like execOps (executor.go:151-188) and closes it.
    The whole Agg <- Join* <- Scan subtree is ONE executor whose plan (ph_plan) the library lowers from the tables'
    statistics. A step = one whole query, result text included; timed by the host layer like Run's
    "Query N took" (executor_bench.go:126-137)."""
    import ctypes
    lib = ctypes.CDLL(os.path.join(ROOT, "plan_amd", "libplantpch.so"))
    lib.planhost_last_error.restype = ctypes.c_char_p
    lib.planhost_tpch_rows.restype = ctypes.c_int64
    db = ctypes.c_void_p()
    t0 = time.time()
    # a context of its own (ph_ctx_create: the library's own non-blocking stream), as the shim gives every executor one and as
    # host_tester runs — not the torch stream the Python pipelines are timed on (Q3 measured ~35 us slower per query on that one)
    from plan_amd import hip as _hip
    octx = _hip.Ctx(h.local_rank)
    if lib.planhost_tpch_load(octx.h, ctypes.c_int64(sf), ctypes.c_int64(1), ctypes.byref(db)) != 0:
        raise RuntimeError(lib.planhost_last_error().decode())
    load_s = time.time() - t0
    out = {}

    def parity(q, text):
        """The result text of this run against the oracle's text for the same generator data: committed fixtures (tests/golden/sf10/oracle_q*.txt,
        made by scripts/oracle_sf10_texts.py and re-derived live by tests/test_gpu_sf10_parity.py) at SF10, the reference's own result files
        (tests/golden/plan_q*.txt = cases/tpch/1g/plan) at SF1. A timing without a checked result says "unchecked"."""
        path = {10: os.path.join(ROOT, "tests", "golden", "sf10", f"oracle_q{q}.txt"), 1: os.path.join(ROOT, "tests", "golden", f"plan_q{q}.txt")}.get(sf)
        if not path or not os.path.exists(path):
            return "unchecked (no fixture at this scale factor)"
        return "ok: byte-identical to " + os.path.relpath(path, ROOT) if open(path).read() == text else "MISMATCH against " + os.path.relpath(path, ROOT)

    try:
        nl = int(lib.planhost_tpch_rows(db, b"lineitem"))
        for q in (3, 9):
            avg, mn = ctypes.c_double(), ctypes.c_double()
            text, explain = ctypes.create_string_buffer(1 << 16), ctypes.create_string_buffer(1 << 14)
            if lib.planhost_tpch_run(db, ctypes.c_int32(q), ctypes.c_int32(steps), ctypes.c_int32(warmup), ctypes.byref(avg), ctypes.byref(mn),
                                     text, ctypes.c_int64(len(text)), explain, ctypes.c_int64(len(explain))) != 0:
                out[f"q{q}_operator_interface"] = {"error": lib.planhost_last_error().decode()}
                continue
            rows = text.value.decode().split("\n")
            out[f"q{q}_operator_interface"] = {
                "metric": f"rows/sec through Q{q} behind the OperatorExec interface (C++ host layer, one resident-plan executor)",
                "value": nl / (avg.value * 1e-3), "unit": "rows/s", "n_gpus": 1, "ms_per_step": avg.value, "min_ms": mn.value, "steps": steps, "warmup": warmup,
                "parity": parity(q, text.value.decode()),
                "config": {"workload": f"TPC-H Q{q} at SF{sf}: limitExecutor <- gpuOrderExecutor <- gpuResidentPlanExecutor(ph_plan) built, pulled and closed per step; "
                                       f"{nl} lineitem rows, all eight tables resident (generated + loaded by the host layer in {load_s:.1f} s)",
                           "result_rows": len([r for r in rows[1:] if r]), "first_row": rows[1] if len(rows) > 1 else None,
                           "forms_chosen_by_the_library": [l.strip() for l in explain.value.decode().split("\n") if l.startswith(("join", "agg"))]},
            }
        # every other query whose reference golden the host layer reproduces (tests/test_host_layer.py): whole-query wall time behind the
        # operator interface at this scale factor, few steps (a record of where each plan stands, not a tuned number)
        others = {}
        for q in (1, 2, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22):
            avg, mn = ctypes.c_double(), ctypes.c_double()
            text, explain = ctypes.create_string_buffer(1 << 22), ctypes.create_string_buffer(1 << 14)
            if lib.planhost_tpch_run(db, ctypes.c_int32(q), ctypes.c_int32(3), ctypes.c_int32(2), ctypes.byref(avg), ctypes.byref(mn),
                                     text, ctypes.c_int64(len(text)), explain, ctypes.c_int64(len(explain))) != 0:
                others[f"q{q}"] = {"error": lib.planhost_last_error().decode()}
                continue
            others[f"q{q}"] = {"ms": round(avg.value, 3), "min_ms": round(mn.value, 3), "result_rows": len([r for r in text.value.decode().split("\n")[1:] if r]),
                               "parity": parity(q, text.value.decode())}
            if q in (1, 6):
                # the fused scans behind the operator interface against the same roofline as the headline: SURVEY §8(d)'s algorithmic bytes per
                # row (Q1 34 B, Q6 24 B) x the table's rows / the WHOLE query's wall time (executor built, pulled, text made, closed)
                per_row = 34 if q == 1 else 24
                gbps = per_row * nl / (avg.value * 1e-3) / 1e9
                others[f"q{q}"]["roofline"] = {"bound": "hbm", "achieved": gbps, "peak": 8000.0, "unit": "GB/s", "frac": gbps / 8000.0,
                                               "algorithmic_bytes_per_query": per_row * nl, "over": "whole-query wall time behind OperatorExec, host work included"}
        out["tpch_operator_interface"] = {"workload": f"TPC-H SF{sf}, the 20 other queries with a reference golden (all 22 are reproduced), through the C++ OperatorExec layer (3 steps behind 2 warm-up runs each)",
                                          "queries": others}
    finally:
        lib.planhost_tpch_free(db)
        octx.close()
    return out


def bench_operator_interface_ranks(h, sf, steps, warmup):
    """Q3 and Q9 behind the OperatorExec interface over ALL ranks: every rank loads its SHARD of the SF`sf` database through
    the C++ host layer (planhost_tpch_load_shard: orders / lineitem by order ranges, the other tables by row ranges, NATION / REGION whole), builds
    the same executor tree per step and announces the ranks' communicator (gpuResidentPlanExecutor::SetComm -> ph_plan_set_comm); the library
    inserts the exchanges (co-location by key ranges, broadcast of small build sides, hash-partitioned all-to-all over RCCL, merge of partial
    states) and every rank's executor emits the complete result. Strong scaling: the SF`sf` database split N ways. RCCL only (the one-GPU
    rehearsal's gloo transport lives above the ABI; the in-process transport of the 2-rank tests needs the ranks in one process)."""
    import ctypes
    if h.comm is None:
        return {"skipped": "needs the RCCL communicator (PH_BENCH_BACKEND=gloo rehearsal: the in-library split is covered by tests/test_gpu_multirank_plan.py "
                           "and host_tester ranks, over the in-process transport)"}
    lib = ctypes.CDLL(os.path.join(ROOT, "plan_amd", "libplantpch.so"))
    lib.planhost_last_error.restype = ctypes.c_char_p
    lib.planhost_tpch_rows.restype = ctypes.c_int64
    db = ctypes.c_void_p()
    if lib.planhost_tpch_load_shard(h.ctx.h, ctypes.c_int64(sf), ctypes.c_int64(1), ctypes.c_int32(h.rank), ctypes.c_int32(h.world), ctypes.byref(db)) != 0:
        raise RuntimeError(lib.planhost_last_error().decode())
    out = {}
    try:
        nl = h.allreduce([int(lib.planhost_tpch_rows(db, b"lineitem"))], "sum")[0]
        for q in (3, 9):
            avg, mn = ctypes.c_double(), ctypes.c_double()
            text, explain = ctypes.create_string_buffer(1 << 16), ctypes.create_string_buffer(1 << 14)
            rc = lib.planhost_tpch_run_comm(db, h.comm.h, ctypes.c_int32(q), ctypes.c_int32(steps), ctypes.c_int32(warmup), ctypes.byref(avg), ctypes.byref(mn),
                                            text, ctypes.c_int64(len(text)), explain, ctypes.c_int64(len(explain)))
            bad = h.allreduce([1 if rc != 0 else 0], "max")[0]
            if bad:
                out[f"q{q}"] = {"error": lib.planhost_last_error().decode() if rc != 0 else "another rank failed"}
                continue
            ms = h.allreduce([int(avg.value * 1e6)], "max")[0] / 1e6     # the slowest rank's average: every step ends in collectives
            rows = text.value.decode().split("\n")
            path = os.path.join(ROOT, "tests", "golden", "sf10", f"oracle_q{q}.txt") if sf == 10 else os.path.join(ROOT, "tests", "golden", f"plan_q{q}.txt") if sf == 1 else None
            parity = "unchecked (no fixture at this scale factor)" if not path or not os.path.exists(path) else \
                ("ok: byte-identical to " + os.path.relpath(path, ROOT) if open(path).read() == text.value.decode() else "MISMATCH against " + os.path.relpath(path, ROOT))
            out[f"q{q}"] = {"metric": f"rows/sec through Q{q} behind the OperatorExec interface over {h.world} ranks (ph_plan_set_comm)", "value": nl / (ms * 1e-3),
                            "unit": "rows/s", "n_gpus": h.world, "ms_per_step": ms, "steps": steps, "warmup": warmup, "scaling": "strong", "parity": parity,
                            "config": {"workload": f"TPC-H Q{q} at SF{sf} split over {h.world} ranks, {nl} lineitem rows in all", "result_rows": len([r for r in rows[1:] if r]),
                                       "forms_chosen_by_the_library": [l.strip() for l in explain.value.decode().split("\n") if l.strip().startswith(("join", "agg", "exchange", "broadcast"))]}}
    finally:
        lib.planhost_tpch_free(db)
    return out


# ---------------------------------------------------------------------------------- CPU baselines

def cpu_baselines(L, max_rows):
    """the oracle (CPU restatement of the reference path) on the GPU box's host cores"""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as O
    import tpch_data
    from plan_amd import queries, tpchgen
    out = {}
    n = len(L["l_shipdate"])
    m = min(n, max_rows)
    sample = {k: v[:m] for k, v in L.items()}
    t0 = time.perf_counter()
    O.q1(sample, queries.q1_shipdate_cutoff())
    dt = time.perf_counter() - t0
    ncpu = os.cpu_count()
    out["q1"] = {"value": m / dt, "unit": "rows/s", "cores": 1, "kind": "port",
                 "sample": f"first {m} rows of the same lineitem shard, oracle q1 pipeline (chunked 2048-row CPU restatement of the "
                           f"reference path, single thread like the reference), {dt:.1f} s, host has {ncpu} logical CPUs"}
    # all cores, NOT reference-faithful (the reference runs one goroutine): the same pipeline on
    # disjoint row slices from a thread pool (the oracle calls release the GIL)
    from concurrent.futures import ThreadPoolExecutor
    k = max(1, min(64, ncpu or 1))
    per = min(n // k, 2_000_000)
    if per >= 4096:
        slices = [{c: v[i * per:(i + 1) * per] for c, v in L.items()} for i in range(k)]
        t0 = time.perf_counter()
        with ThreadPoolExecutor(k) as ex:
            list(ex.map(lambda s: O.q1(s, queries.q1_shipdate_cutoff()), slices))
        dt2 = time.perf_counter() - t0
        out["q1_all_cores"] = {"value": k * per / dt2, "unit": "rows/s", "cores": k, "kind": "port",
                               "sample": f"{k} threads x {per} rows, {dt2:.1f} s — not reference-faithful (the reference is single-threaded)"}
    t0 = time.perf_counter()
    O.q6(sample, *queries.q6_constants())
    dt = time.perf_counter() - t0
    out["q6"] = {"value": m / dt, "unit": "rows/s", "cores": 1, "kind": "port", "sample": f"first {m} rows, oracle q6 pipeline, {dt:.1f} s"}
    t1 = tpch_data.load(1, 1, q9=True)
    t0 = time.perf_counter()
    O.q3(t1, "HOUSEHOLD", tpchgen.days(1995, 3, 29))
    dt = time.perf_counter() - t0
    nl = len(t1["lineitem"]["l_orderkey"])
    out["q3"] = {"value": nl / dt, "unit": "rows/s", "cores": 1, "kind": "port",
                 "sample": f"oracle q3 pipeline at SF1 ({nl} lineitem rows; the SF10 run would take ~10x), {dt:.1f} s"}
    t0 = time.perf_counter()
    O.q9(t1, "%pink%")
    dt = time.perf_counter() - t0
    out["q9"] = {"value": nl / dt, "unit": "rows/s", "cores": 1, "kind": "port",
                 "sample": f"oracle q9 pipeline at SF1 ({nl} lineitem rows, LIKE + five chained joins + 175 groups, 2048-row chunks), {dt:.1f} s"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sf", type=int, default=10, help="scale factor (per GPU for weak scaling, total for strong)")
    ap.add_argument("--query", default="q1", choices=["q1", "q6", "q3", "q9"])
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-companions", action="store_true", help="headline query only")
    ap.add_argument("--cpu-rows", type=int, default=16_000_000)
    ap.add_argument("--companion-timeout", type=float, default=240.0)
    ap.add_argument("--full", action="store_true",
                    help="also the rooflines, the measured read ceiling, the CPU baselines and the companion benches")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed as DIR/<name>.npy (float64)")
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        spawn_ranks(args)   # does not return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"WORLD_SIZE={world} but --gpus {args.gpus}")

    h = Harness(args)
    rank0 = h.rank == 0
    comp_steps, comp_warm = min(args.steps, 30), min(args.warmup, 5)
    outputs = {} if args.dump_outputs else None
    if args.query in ("q1", "q6"):
        out, L, table = bench_scan(h, args.query, args.sf, args.steps, args.warmup, args.scaling, full=args.full, outputs=outputs)
    elif args.query == "q3":
        out, L, table = bench_q3(h, args.sf, args.steps, args.warmup, args.scaling, full=args.full, outputs=outputs), None, None
    else:
        if world != 1:
            raise SystemExit("--query q9 is a one-GPU bench")
        out, L, table = bench_q9(h, args.sf, args.steps, args.warmup, args.scaling, full=args.full, outputs=outputs), None, None
    if outputs is not None and rank0:
        write_outputs(args.dump_outputs, outputs)
    if args.full:
        out["roofline"]["peak_measured"] = h.peak_measured()
        out["roofline"]["frac_of_measured"] = out["roofline"]["achieved"] / out["roofline"]["peak_measured"]
    out["config"]["rccl_ranks"] = h.comm.n if h.comm is not None else (1 if world == 1 else f"gloo rehearsal x{world}")

    # ---- companions: never fatal for the headline, and bounded in time (a wedged collective on
    # one rank must not cost the line): a watchdog prints what is there and ends every rank
    done = threading.Event()

    def watchdog():
        if not done.wait(args.companion_timeout):
            if rank0:
                out.setdefault("companion_error", f"companions exceeded {args.companion_timeout:.0f} s; stopped")
                print(json.dumps(out), flush=True)
            os._exit(3)   # a wedged collective or a hung kernel is a FAILED run: what was measured is printed, the exit code says so

    companions = args.full and args.query == "q1" and not args.no_companions
    if companions:
        threading.Thread(target=watchdog, daemon=True).start()

    def attempt(name, fn):
        try:
            out[name] = fn()
        except Exception as e:  # noqa: BLE001 - reported, never fatal for the headline
            out[name] = {"error": f"{type(e).__name__}: {e}"}

    def brief(line):
        return {k: line[k] for k in ("metric", "value", "unit", "n_gpus", "ms_per_step", "steps", "scaling", "config", "roofline", "exchange") if k in line}

    if companions and world == 1:
        attempt("q6_single_gpu", lambda: brief(bench_scan(h, "q6", args.sf, comp_steps, comp_warm, "weak", L=L, table=table)[0]))
        if not args.no_cpu_baseline:
            cb = cpu_baselines(L, args.cpu_rows)
            out["cpu_baseline"] = cb["q1"]
            if "q1_all_cores" in cb:
                out["cpu_baseline_all_cores"] = cb["q1_all_cores"]
        table.free()
        del L
        attempt("q1_sf1", lambda: brief(bench_scan(h, "q1", 1, max(args.steps, 100), comp_warm, "weak")[0]))
        # the join queries take ~0.5-1 ms a step: 50 steps behind 8 warm-up steps (memory pool and clocks settled),
        # like their stand-alone runs
        attempt("q3_single_gpu", lambda: brief(bench_q3(h, args.sf, max(comp_steps, 50), max(comp_warm, 8), "weak")))
        attempt("q9_single_gpu", lambda: brief(bench_q9(h, args.sf, max(comp_steps, 50), max(comp_warm, 8))))
        try:   # the same two queries behind the operator interface (C++ host layer -> ph_plan)
            out.update(bench_operator_interface(h, args.sf, max(comp_steps, 50), max(comp_warm, 8)))
        except Exception as e:  # noqa: BLE001 - reported, never fatal for the headline
            out["q3_operator_interface"] = out["q9_operator_interface"] = {"error": f"{type(e).__name__}: {e}"}
        attempt("general_forms", lambda: bench_general_forms(h, args.sf))
        if not args.no_cpu_baseline:
            if "error" not in out["q6_single_gpu"]:
                out["q6_single_gpu"]["cpu_baseline"] = cb["q6"]
            if "error" not in out["q3_single_gpu"]:
                out["q3_single_gpu"]["cpu_baseline"] = cb["q3"]
            if "error" not in out["q9_single_gpu"]:
                out["q9_single_gpu"]["cpu_baseline"] = cb["q9"]
    elif companions:
        table.free()
        del L
        # BASELINE.json config 4: Q3 at SF`--sf`, hash-partitioned across the N GPUs (strong scaling)
        attempt("q3_partitioned", lambda: brief(bench_q3(h, args.sf, comp_steps, comp_warm, "strong")))
        # the same database and query as a partition-wise join (the shards are co-partitioned by order key)
        attempt("q3_partitionwise", lambda: brief(bench_q3(h, args.sf, comp_steps, comp_warm, "strong", partitionwise=True)))
        # BASELINE.json config 5: Q9 at SF`--sf`, multi-stage partitioned build/probe across the N GPUs
        attempt("q9_partitioned", lambda: brief(bench_q9(h, args.sf, comp_steps, comp_warm, "strong")))
        attempt("q9_partitionwise", lambda: brief(bench_q9(h, args.sf, comp_steps, comp_warm, "strong", partitionwise=True)))
        # the same two queries with the split INSIDE the boundary: the C++ OperatorExec layer over every rank's shard, ph_plan_set_comm
        attempt("operator_interface_over_ranks", lambda: bench_operator_interface_ranks(h, args.sf, min(comp_steps, 20), min(comp_warm, 3)))
    elif args.full and rank0 and world == 1 and not args.no_cpu_baseline and L is not None:
        cb = cpu_baselines(L, args.cpu_rows)
        out["cpu_baseline"] = cb[args.query]
    done.set()
    if rank0:
        print(json.dumps(out), flush=True)
    try:
        h.barrier()
        h.close()
    except Exception:  # noqa: BLE001 - the line is out; teardown problems are not results
        pass


if __name__ == "__main__":
    main()
