"""GPU tests of the halving fold of the bins row body (lch_fold in scan_kernels.hip, DESIGN.md §4.1 "The halving fold and the residency
probe"): a slot the fold pads with identities, long shares of one bin in one workgroup, many workgroups, and four waves adding to one
bin. Every comparison is equality of integers, against numpy / Python integers and against the same plan under PH_SCAN_HIST=0 (the
columns body). Tables, plans and references come from test_gpu_hist_scan's, test_gpu_packed_scan's and test_gpu_narrow_scan's helpers
(want_signed with s2 = 1 is lc_want, vectorised). tests/test_hist_fold_halving.py pins the exchange schedule without a GPU."""
import numpy as np
import pytest

from plan_amd import hip
from test_gpu_hist_scan import TILE, both_bodies, spread_slots, want_signed
from test_gpu_narrow_scan import lc_plan, lc_table
from test_gpu_packed_scan import COLS, lineitem_like

pytestmark = pytest.mark.gpu

P_LO, P_HI = 8036, 8036 + 4095
E_MAX, Q_MAX = 2 ** 24 - 1, 63


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in ("PH_SCAN_GRID", "PH_SCAN_PACK_MIN_BYTES", "PH_SCAN_HIST"):
        monkeypatch.delenv(k, raising=False)


# ---------------------------------------------------------------- five slots: the sixth is the fold's padding

def test_five_slots_pad_the_fold(ctx, monkeypatch):
    """5 x 1 dictionaries: lineitem's bit layout (a slot field of three bits) with nslots = 5, so words 30..35 and the sixth minimum of the
    fold are identities that no lane may store; three tiles and a few rows, one workgroup and several"""
    n = 3 * TILE + 41
    c = lineitem_like(n, seed=31)
    c["k0"] = (np.random.default_rng(32).integers(0, 5, n)).astype(np.uint8)
    c["k1"] = np.zeros(n, np.uint8)
    t = hip.Table(ctx, [(hip.PH_I32, c["q"]), (hip.PH_DEC64, c["e"], 2), (hip.PH_DEC64, c["d"], 2), (hip.PH_DEC64, c["t"], 2),
                        (hip.PH_CODE8, c["k0"], 0, None, list("abcde")), (hip.PH_CODE8, c["k1"], 0, None, ["x"]), (hip.PH_DATE, c["p"])], n)
    t.pack_scan_group(COLS)
    pl = lc_plan(ctx, t, 8500, 10000, c["ptype"])
    ranges = [(0, n), (3, n - 3), (TILE, 2 * TILE)]
    for grid in (None, "1"):
        if grid is not None:
            monkeypatch.setenv("PH_SCAN_GRID", grid)
        got = both_bodies(pl, monkeypatch, ranges)
        for (b, e), g in zip(ranges, got):
            assert len(g) == 5 and sorted(g) == want_signed(c, 8500, 10000, b, e, 1, nk1=1), (grid, b, e)
    pl.free()
    t.free()


# ---------------------------------------------------------------- one bin

def one_bin_table(n, pin):
    """every row in bin (slot 5, d = t = 15) with p, q and e at their maximum codes, but row `pin`: the only row of slot 0, minimum codes"""
    c = dict(p=np.full(n, P_HI, np.int32), q=np.full(n, Q_MAX, np.int32), e=np.full(n, E_MAX, np.int64), d=np.full(n, 15, np.int64),
             t=np.full(n, 15, np.int64), k0=np.full(n, 2, np.uint8), k1=np.full(n, 1, np.uint8), ptype=hip.PH_DATE)
    c["p"][pin], c["q"][pin], c["e"][pin], c["d"][pin], c["t"][pin], c["k0"][pin], c["k1"][pin] = P_LO, 0, 0, 0, 0, 0, 0
    return c


def one_bin_range_want(pin, b, e):
    """the groups over rows [b, e) in closed form and Python integers (test_gpu_hist_scan.one_bin_want for any range)"""
    inside = b <= pin < e
    m = e - b - inside
    first = b if pin != b else b + 1
    out = [(first, (2, 1), [Q_MAX * m, E_MAX * m, E_MAX * 85 * m, E_MAX * 85 * 115 * m, 15 * m], m)] if m > 0 else []
    if inside:
        out.append((pin, (0, 0), [0, 0, 0, 0, 0], 1))
    return sorted(out)


def test_long_shares_of_one_bin_in_one_workgroup(ctx, monkeypatch):
    """PH_SCAN_GRID=1 over up to 511 tiles of one bin: one lane of each wave holds all of a slot's rows, every other lane zeros, and
    slot 0's single row sits in one lane of one wave; the last range starts inside tile 3"""
    n = 512 * TILE
    pin = 255 * TILE - 1
    c = one_bin_table(n, pin)
    t = lc_table(ctx, c)
    t.pack_scan_group(COLS)
    pl = lc_plan(ctx, t, P_LO, P_HI, c["ptype"])
    monkeypatch.setenv("PH_SCAN_GRID", "1")
    ranges = [(0, k * TILE) for k in (254, 255, 256, 511)] + [(0, 255 * TILE + 1), (3 * TILE + 7, 3 * TILE + 7 + 256 * TILE)]
    got = both_bodies(pl, monkeypatch, ranges)
    for (b, e), g in zip(ranges, got):
        assert sorted(g) == one_bin_range_want(pin, b, e), (b, e)
    pl.free()
    t.free()


def test_four_waves_add_to_one_bin(ctx, monkeypatch):
    """one tile whose 4096 rows all lie in one bin, at grid 1 and at the default grid"""
    n = TILE
    c = one_bin_table(n + 1, n)      # the pinning row behind the tile
    t = lc_table(ctx, c)
    t.pack_scan_group(COLS)
    pl = lc_plan(ctx, t, P_LO, P_HI, c["ptype"])
    ranges = [(0, n), (0, n + 1)]
    for grid in ("1", None):
        if grid is not None:
            monkeypatch.setenv("PH_SCAN_GRID", grid)
        else:
            monkeypatch.delenv("PH_SCAN_GRID")
        got = both_bodies(pl, monkeypatch, ranges)
        for (b, e), g in zip(ranges, got):
            assert sorted(g) == one_bin_range_want(n, b, e), (grid, b, e)
    pl.free()
    t.free()


# ---------------------------------------------------------------- many workgroups

def test_many_workgroups_and_grids(ctx, monkeypatch):
    """1300 random tiles, six slots: the default grid (two or three tiles a workgroup) and PH_SCAN_GRID = 768 and 1280 (two tiles for some
    workgroups, one for the others)"""
    n = 1300 * TILE - 11
    c = spread_slots(lineitem_like(n, seed=22))
    lo, hi = 8500, 10300
    t = lc_table(ctx, c)
    t.pack_scan_group(COLS)
    pl = lc_plan(ctx, t, lo, hi, c["ptype"])
    ranges = [(0, n), (7, n - 4097)]
    want = [want_signed(c, lo, hi, b, e, 1) for b, e in ranges]
    assert len(want[0]) == 6
    for grid in (None, "768", "1280"):
        if grid is not None:
            monkeypatch.setenv("PH_SCAN_GRID", grid)
        got = both_bodies(pl, monkeypatch, ranges)
        assert [sorted(g) for g in got] == want, grid
    pl.free()
    t.free()
