"""ph_sort_rows timing: python scripts/bench_sort.py"""
import os, re, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from plan_amd import hip, tpchgen
ctx = hip.Ctx(0)
rng = np.random.default_rng(1)


def best_of(keys, desc, n, reps=4):
    out = hip.sort_rows(ctx, keys, desc, None, n)   # warm-up
    ctx.sync(); ctx.free(out)
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter(); out = hip.sort_rows(ctx, keys, desc, None, n); ctx.sync(); best = min(best, time.perf_counter() - t0); ctx.free(out)
    return best


for n in (113_000, 10_000_000):
    rev = hip.DevColumn(ctx, hip.PH_DEC64, rng.integers(0, 5 * 10**9, n).astype(np.int64), 4)
    date = hip.DevColumn(ctx, hip.PH_DATE, rng.integers(8000, 10500, n).astype(np.int32))
    for keys, desc, label in (([rev, date], [True, False], "revenue desc, date"), ([date], [False], "date")):
        best = 1e9
        for _ in range(4):
            t0 = time.perf_counter(); out = hip.sort_rows(ctx, keys, desc, None, n); ctx.sync(); best = min(best, time.perf_counter() - t0); ctx.free(out)
        print(f"sort {n} rows by ({label}): {best*1e3:.3f} ms  {n/best/1e9:.2f} G rows/s")
    rev.free(); date.free()

# VARCHAR keys (PH_STR)
O = tpchgen.orders((10, 1), columns=["o_comment"])
n = len(O["o_comment_off"]) - 1
com = hip.DevColumn(ctx, hip.PH_STR, O["o_comment_off"], aux=O["o_comment_bytes"])
best = best_of([com], [True], n)
print(f"sort {n} rows by (o_comment desc) SF10: {best*1e3:.3f} ms  {n/best/1e9:.2f} G rows/s")
com.free(); del O

n = 1_500_000
names = [b"Customer#%09d" % v for v in rng.permutation(n) + 1]
col = hip.str_column(ctx, names)
best = best_of([col], [False], n)
print(f"sort {n} rows by (c_name 'Customer#%09d', shuffled): {best*1e3:.3f} ms  {n/best/1e9:.2f} G rows/s")
col.free(); del names

C = tpchgen.customer((10, 1), text=True)
n = len(C["c_custkey"])
com = hip.DevColumn(ctx, hip.PH_STR, C["c_comment_off"], aux=C["c_comment_bytes"])
key = hip.DevColumn(ctx, hip.PH_I32, C["c_custkey"].astype(np.int32))
best = best_of([com, key], [False, True], n)
print(f"sort {n} rows by (c_comment, c_custkey desc) SF10: {best*1e3:.3f} ms  {n/best/1e9:.2f} G rows/s")
com.free(); key.free()
ctx.close()

# the operator interface: gpuOrderExecutor over SF1 customer (150 000 rows: the device sort), VARCHAR keys as PH_STR vs ranked on the host
tester = os.path.join(ROOT, "plan_amd", "host_tester")
for label, extra in (("PH_STR keys", {}), ("PH_ORDER_HOST_RANKS=1", {"PH_ORDER_HOST_RANKS": "1"})):
    times = []
    for _ in range(3):
        r = subprocess.run([tester, "order_text", "1", "1"], capture_output=True, text=True, check=True, timeout=600,
                           env=dict(os.environ, PH_HOST_TIMING="1", **extra))
        times += [float(x) for x in re.findall(r"order: sortAll ([0-9.]+) us", r.stderr)]
    print(f"host_tester order_text 1 1, {label}: sortAll {min(times)/1e3:.2f} ms (best of {len(times)}, incl. the child's Execute)")
