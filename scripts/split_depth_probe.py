"""How many tiles of loads should the split bins scan keep ahead of the tile in work? (DESIGN.md §4.1 "A ring of tile buffers")
A lineitem_like table of SF10's size (59 986 052 rows, lineitem's field widths) with its scan group in the split form, the Q1-shaped
plan event-timed at PH_SCAN_DEPTH = 2, 3, 4 (the register tile buffers of lowcard_chain_kernel_split<true>; depth - 1 tiles of loads
are ahead) x PH_SCAN_GRID = 512, 256: 30 runs a setting, the settings taken in turn, four rounds in one sitting; min / mean / max per
setting and round, then over all rounds. Every run is the scan kernel and the merge launch, as in a step of bench.py.

  python scripts/split_depth_probe.py [--rows N] > profiles/split_depth_probe.txt

The default depth is the one with the lowest mean at grid 512 if its mean is below depth 2's in every round; otherwise it stays 2. The
grid 256 column is a record: the default grid is not this probe's to change.

The probe said no (profiles/split_depth_probe.txt: 74.7 / 76.3 / 78.1 us at depths 2 / 3 / 4), so the rings and PH_SCAN_DEPTH are not
in the library: it was run on a measurement build that had them (DESIGN.md §4.1 describes it), and on the committed library, which
does not read PH_SCAN_DEPTH, every depth runs the same two-buffer loop."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch

from plan_amd import hip
from test_gpu_narrow_scan import D, E, K0, K1, P, Q, T, lc_data, lc_plan, lc_result

SPLIT56 = 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=59_986_052)
    ap.add_argument("--depths", default="2,3,4", help="the first is the base the others are compared with")
    ap.add_argument("--grids", default="512,256", help="the first is the grid the choice is made at")
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=4)
    a = ap.parse_args()
    DEPTHS = tuple(int(d) for d in a.depths.split(","))
    GRIDS = tuple(int(g) for g in a.grids.split(","))
    n = a.rows
    c = lc_data(n, 1, 8036, 10561, q=(1, 50), e=(90100, 10494950), d=(0, 10), t=(0, 8))
    slot = np.arange(n) % 6     # equal shares, interleaved
    c["k0"], c["k1"] = (slot // 2).astype(np.uint8), (slot % 2).astype(np.uint8)

    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = hip.Ctx(0, stream=stream.cuda_stream)
    t = hip.Table(ctx, [(hip.PH_I32, c["q"]), (hip.PH_DEC64, c["e"], 2), (hip.PH_DEC64, c["d"], 2), (hip.PH_DEC64, c["t"], 2),
                        (hip.PH_CODE8, c["k0"], 0, None, ["a", "b", "c"]), (hip.PH_CODE8, c["k1"], 0, None, ["x", "y"]), (hip.PH_DATE, c["p"])], n)
    t.pack_scan_group_ex([P, Q, E, D, T, K0, K1], SPLIT56)
    pl = lc_plan(ctx, t, 8036, 10471, hip.PH_DATE)     # as Q1: nearly every row passes
    pl.run()
    want = lc_result(pl.fetch())
    print(f"rows {n}, variant {pl.variant}, row body {pl.row_body}, {pl.bytes_per_row} bytes a row")
    if pl.variant != "split56" or pl.row_body != "bins":
        print("the plan does not run the bins body over a split group on this table: nothing to measure")
        return 1

    settings = [(d, g) for d in DEPTHS for g in GRIDS]
    times = {s: [] for s in settings}
    means = {s: [] for s in settings}
    for rnd in range(a.rounds):
        for d, g in settings:
            os.environ["PH_SCAN_DEPTH"], os.environ["PH_SCAN_GRID"] = str(d), str(g)
            pl.run()
            assert lc_result(pl.fetch()) == want, (d, g)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.runs)]
            for s, e in ev:
                s.record(stream)
                pl.run()
                e.record(stream)
            torch.cuda.synchronize()
            pl.fetch()
            ms = [s.elapsed_time(e) for s, e in ev]
            times[(d, g)] += ms
            means[(d, g)].append(sum(ms) / len(ms))
            print(f"round {rnd} depth {d} grid {g}: min {min(ms) * 1e3:.1f} mean {sum(ms) / len(ms) * 1e3:.1f} max {max(ms) * 1e3:.1f} us")
    for d, g in settings:
        ms = times[(d, g)]
        print(f"depth {d} grid {g}: {len(ms)} runs, min {min(ms) * 1e3:.1f} mean {sum(ms) / len(ms) * 1e3:.1f} max {max(ms) * 1e3:.1f} us")
    g0, base = GRIDS[0], DEPTHS[0]
    best = min(DEPTHS, key=lambda d: sum(times[(d, g0)]) / len(times[(d, g0)]))
    every = best != base and all(m < b for m, b in zip(means[(best, g0)], means[(base, g0)]))
    print(f"lowest mean at grid {g0}: depth {best}; its mean below depth {base}'s in every round: {'yes' if every else 'no'}; "
          f"the default depth: {best if every else base}")
    pl.free()
    t.free()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
