"""GPU tests of the tile loop of the bins body over a split scan group (lowcard_chain_kernel_group<SplitLoad, BinsBody>) by the number of tiles a
workgroup works through: the two-buffer loop loads one tile ahead, leaves after either of its two unrolled halves, and the tile it
loads beyond the range is the substitute (the range's first tile). The cases were written for a ring of three and four tile buffers,
which was measured slower and is not in the library (DESIGN.md §4.1 "A ring of tile buffers: measured, not shipped"); they pin the loop
that ships at the shapes where a deeper loop would have differed. Every comparison is equality of integers, first rows included: against
the numpy / Python-integer restatement and against the same plan under PH_SCAN_HIST=0, the columns body.
Tables and plans come from test_gpu_narrow_scan's, test_gpu_hist_scan's and test_gpu_split_scan's helpers."""
import numpy as np
import pytest

from plan_amd import hip
from test_gpu_narrow_scan import lc_plan, lc_result, lc_want
from test_gpu_hist_scan import plan_signed, want_signed
from test_gpu_split_scan import P_HI, P_LO, TILE, fields, slot_table, split_table

pytestmark = pytest.mark.gpu

GRIDS = (None, "1", "2", "3")     # None: the plan's own grid
SWITCHES = ("PH_SCAN_GRID", "PH_SCAN_HIST", "PH_SCAN_SPLIT", "PH_SCAN_PACK_MIN_BYTES")


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PH_SCAN_SPLIT_MIN_BYTES", "0")


def run_ranges(pl, ranges, body):
    out = []
    for b, e in ranges:
        pl.run(b, e)
        assert pl.variant == "split56" and pl.bytes_per_row == 7 and pl.row_body == body, (b, e)
        out.append(lc_result(pl.fetch()))
    return out


def check_grids(pl, monkeypatch, ranges, want, grids=GRIDS):
    """every range at every grid: equal to `want` and, in the result's own order, to the columns body's"""
    for grid in grids:
        if grid is None:
            monkeypatch.delenv("PH_SCAN_GRID", raising=False)
        else:
            monkeypatch.setenv("PH_SCAN_GRID", grid)
        got = run_ranges(pl, ranges, "bins")
        monkeypatch.setenv("PH_SCAN_HIST", "0")
        ref = run_ranges(pl, ranges, "columns")
        monkeypatch.delenv("PH_SCAN_HIST")
        for (b, e), g, r, w in zip(ranges, got, ref, want):
            assert sorted(g) == w, (grid, b, e)
            assert g == r, (grid, b, e)
    monkeypatch.delenv("PH_SCAN_GRID", raising=False)


# ---------------------------------------------------------------- one to eight tiles per workgroup

@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7])
def test_tile_counts(ctx, monkeypatch, k):
    """k 4096 - 1, k 4096 and k 4096 + 1 rows at grids 1, 2, 3 and the plan's own: a workgroup works through 1 to 8 tiles, in equal
    and unequal shares, an odd and an even number of them. With k 4096 rows the tile loaded beyond the last is the substitute; with
    one row more the last tile holds one row."""
    for n in (k * TILE - 1, k * TILE, k * TILE + 1):
        c = fields(n, 700 + n % 97 + k)
        t = split_table(ctx, c)
        lo, hi = P_LO + 200, P_HI - 200
        pl = lc_plan(ctx, t, lo, hi, c["ptype"])
        ranges = [(0, n)]
        check_grids(pl, monkeypatch, ranges, [lc_want(c, lo, hi, b, e) for b, e in ranges])
        pl.free()
        t.free()


# ---------------------------------------------------------------- masked first and last tiles, both in one, the empty range

@pytest.mark.parametrize("n", [5 * TILE - 1, 7 * TILE], ids=["five_tiles", "seven_tiles"])
def test_range_cuts_on_five_and_seven_tiles(ctx, monkeypatch, n):
    c = fields(n, 800 + n % 89)
    t = split_table(ctx, c)
    lo, hi = P_LO + 200, P_HI - 200
    pl = lc_plan(ctx, t, lo, hi, c["ptype"])
    mid = 3 * TILE + 1234
    ranges = [(b, e) for b in (0, 1, TILE - 1, TILE, TILE + 1) for e in (n, n - 1, mid, b)]
    want = [lc_want(c, lo, hi, b, e) for b, e in ranges]
    assert all(w == [] for (b, e), w in zip(ranges, want) if b == e) and want[0] != []
    check_grids(pl, monkeypatch, ranges, want, grids=(None, "1", "2"))
    # both masks in one tile: a range inside the last tile, and two inside the first and the second
    inside = [(n - TILE // 2, n - 3), (5, TILE - 5), (TILE + 7, TILE + 8)]
    check_grids(pl, monkeypatch, inside, [lc_want(c, lo, hi, b, e) for b, e in inside], grids=(None, "1"))
    pl.free()
    t.free()


# ---------------------------------------------------------------- one failing row, one passing row per tile

@pytest.mark.parametrize("passing", [False, True], ids=["one_failing_row_a_tile", "one_passing_row_a_tile"])
def test_one_row_per_tile(ctx, monkeypatch, passing):
    """seven tiles; tile i's special row is row 601 i + 3 of it (another wave, lane and quad row each time): the only row that fails,
    or the only one that passes"""
    n = 7 * TILE
    c = fields(n, 900 + passing)
    lo, hi = P_LO + 1000, P_LO + 3000
    special = np.array([i * TILE + 601 * i + 3 for i in range(7)])
    body = np.arange(n) >= 2    # rows 0 and 1 pin the columns' ranges: P_LO and P_HI, both outside [lo, hi]
    c["p"][body] = (lo + np.arange(n) % 2001)[body] if not passing else (P_LO + np.arange(n) % 1000)[body]
    c["p"][special] = hi + 1 if not passing else lo + 7
    t = split_table(ctx, c)
    pl = lc_plan(ctx, t, lo, hi, c["ptype"])
    ranges = [(0, n), (3, n - 3)]
    want = [lc_want(c, lo, hi, b, e) for b, e in ranges]
    assert sum(g[3] for g in want[0]) == (7 if passing else n - 2 - 7)
    check_grids(pl, monkeypatch, ranges, want)
    pl.free()
    t.free()


# ---------------------------------------------------------------- six slots, factors of both signs

@pytest.mark.parametrize("s2", [1, -1], ids=["f2_100_plus_t", "f2_100_minus_t"])
def test_six_slots_signed_factors_on_five_tiles(ctx, monkeypatch, s2):
    n = 5 * TILE + 9
    c = fields(n, 950 + s2, d=(93, 108), t=(93, 108))
    lo, hi = P_LO + 300, P_HI - 300
    c["p"][4 * 501 + 3] = hi
    t = slot_table(ctx, c, 6)
    pl = plan_signed(ctx, t, lo, hi, c["ptype"], s2)
    ranges = [(0, n), (3, n - 3), (TILE - 1, 4 * TILE + 1)]
    want = [want_signed(c, lo, hi, b, e, s2, nk1=1) for b, e in ranges]
    assert len(want[0]) == 6
    check_grids(pl, monkeypatch, ranges, want, grids=(None, "1", "2"))
    pl.free()
    t.free()
