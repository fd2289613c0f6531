"""Does the bins body of the packed Q1 scan gain from more workgroups a CU? (DESIGN.md §4.1 "The halving fold and the residency probe")
A lineitem_like table of SF10's size (59 986 052 rows, lineitem's field widths) with its packed scan group, the Q1-shaped plan
event-timed at PH_SCAN_GRID = 512, 768, 1024, 1280 (two to five workgroups a CU on 256 CUs): 30 runs a grid, the grids alternating, four
rounds; min / mean / max per grid over all rounds.
With the library as it is a workgroup's LDS (61.3 KiB at six slots) admits two workgroups a CU, so a larger grid only queues; the probe
measures residency on a build whose workgroups are smaller (profiles/README.md has the one it was run on).

  python scripts/hist_residency_probe.py [--dicts 3x2] [--rows N] > profiles/hist_residency_probe.txt

--dicts AxB: the sizes of the two group dictionaries; the rows are dealt to the A x B slots in equal shares. The bins body runs only in
lineitem's bit layout, whose slot field has three bits, and with at most six slots: five or six. With fewer (2x1, say) the slot field is narrower, the
layout another, and the plan runs the columns body: the script says so and stops."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch

from plan_amd import hip
from test_gpu_narrow_scan import D, E, K0, K1, P, Q, T, lc_data, lc_plan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dicts", default="3x2")
    ap.add_argument("--rows", type=int, default=59_986_052)
    ap.add_argument("--grids", default="512,768,1024,1280", help="the first is the base of the go / no-go line")
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=4)
    a = ap.parse_args()
    nk0, nk1 = (int(x) for x in a.dicts.split("x"))
    GRIDS = tuple(int(g) for g in a.grids.split(","))
    n = a.rows
    c = lc_data(n, 1, 8036, 10561, q=(1, 50), e=(90100, 10494950), d=(0, 10), t=(0, 8))
    slot = np.arange(n) % (nk0 * nk1)     # equal shares, interleaved
    c["k0"], c["k1"] = (slot // nk1).astype(np.uint8), (slot % nk1).astype(np.uint8)

    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = hip.Ctx(0, stream=stream.cuda_stream)
    t = hip.Table(ctx, [(hip.PH_I32, c["q"]), (hip.PH_DEC64, c["e"], 2), (hip.PH_DEC64, c["d"], 2), (hip.PH_DEC64, c["t"], 2),
                        (hip.PH_CODE8, c["k0"], 0, None, [chr(97 + i) for i in range(nk0)]),
                        (hip.PH_CODE8, c["k1"], 0, None, [chr(120 + i) for i in range(nk1)]), (hip.PH_DATE, c["p"])], n)
    t.pack_scan_group([P, Q, E, D, T, K0, K1])
    pl = lc_plan(ctx, t, 8036, 10471, hip.PH_DATE)     # as Q1: nearly every row passes
    pl.run()
    pl.fetch()
    print(f"rows {n}, dictionaries {nk0} x {nk1}, variant {pl.variant}, row body {pl.row_body}, {pl.bytes_per_row} bytes a row")
    if pl.row_body != "bins":
        print("the plan does not run the bins body on this table: nothing to measure")
        return 1

    times = {g: [] for g in GRIDS}
    for rnd in range(a.rounds):
        for g in GRIDS:
            os.environ["PH_SCAN_GRID"] = str(g)
            pl.run()
            pl.fetch()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.runs)]
            for s, e in ev:
                s.record(stream)
                pl.run()
                e.record(stream)
            torch.cuda.synchronize()
            pl.fetch()
            ms = [s.elapsed_time(e) for s, e in ev]
            times[g] += ms
            print(f"round {rnd} grid {g}: min {min(ms) * 1e3:.1f} mean {sum(ms) / len(ms) * 1e3:.1f} max {max(ms) * 1e3:.1f} us")
    for g in GRIDS:
        ms = times[g]
        print(f"grid {g} ({g / 256:g} workgroups a CU on 256 CUs): {len(ms)} runs, min {min(ms) * 1e3:.1f} mean {sum(ms) / len(ms) * 1e3:.1f} "
              f"max {max(ms) * 1e3:.1f} us")
    base = times[GRIDS[0]]
    best = min(GRIDS[1:], key=lambda g: max(times[g]))
    need = 3 * (max(base) - min(base))
    gain = min(base) - max(times[best])
    print(f"best of the others by its slowest run: {best}; every run faster than every run at {GRIDS[0]} by {gain * 1e3:.1f} us, "
          f"three times the spread at {GRIDS[0]} is {need * 1e3:.1f} us: {'go' if gain > need else 'no-go'}")
    pl.free()
    t.free()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
