"""GPU parity of the fused Q1-shaped scan over a packed scan group (ph_table_pack_scan_group): one 64-bit word a
row instead of seven arrays. Every comparison is equality: against a numpy restatement and against the same plan's result
before the group existed (the lean kernel over the narrowed copies). Tables and plans come from test_gpu_narrow_scan's helpers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from plan_amd import hip, tpchgen  # noqa: E402
from test_gpu_narrow_scan import D, E, K0, K1, P, Q, T, lc_data, lc_plan, lc_result, lc_table, lc_want  # noqa: E402

pytestmark = pytest.mark.gpu

COLS = [P, Q, E, D, T, K0, K1]   # the group's columns by role: predicate, q, e, d, t, the two group columns
N = 5 * 4096 + 7
D0 = tpchgen.days(1994, 1, 1)


def padded(n):
    return -(-n // 8192) * 8192


def slots(c):
    """six slots: k0 = 2 only where a test puts it — (2, 1) at a single row, (2, 0) only in the last partial tile"""
    n = len(c["p"])
    rng = np.random.default_rng(n)
    c["k0"] = rng.integers(0, 2, n).astype(np.uint8)
    c["k0"][0], c["k1"][0] = 0, 0               # slot 0 ...
    c["k0"][777], c["k1"][777] = 2, 1           # ... and the last slot, used by this row alone
    c["k0"][n - 3], c["k1"][n - 3] = 2, 0       # used only in the last partial tile
    return c


def lineitem_like(n=N, seed=1):
    """lineitem's value ranges: the layout the kernel has a compile-time instance for (12, 6, 24, 4, 4, 3 bits)"""
    return slots(lc_data(n, seed, 8036, 10561, q=(1, 50), e=(90100, 10494950), d=(0, 10), t=(0, 8)))


def full_fields(n=N, seed=2):
    """every field's span all ones (rows 0 and 1 hold code 0 and the maximum of every column: lc_data), factors 100 - d and
    100 + t of both signs, negative e: 12 + 6 + 24 + 8 + 8 + 3 = 61 bits, the layout read at run time"""
    return slots(lc_data(n, seed, D0, D0 + 4095, q=(-13, 50), e=(-(2 ** 23), 2 ** 23 - 1), d=(0, 255), t=(-200, 55)))


def intervals_of(c):
    lo, hi = int(c["p"].min()), int(c["p"].max())
    mid = (lo + hi) // 2
    return [(lo, hi), (lo + 100, mid), (mid, mid - 1), (hi + 1, hi + 50), (lo, lo), (hi, hi)]   # third and fourth: empty code intervals


def boundary_ranges(n):
    """row ranges that start and end one row before, at and after the boundaries of a lane's 2 rows, a load's 128, a wave's 1024 and
    a tile's 4096 (most starts are no multiple of 16)"""
    edges = sorted({b + k * m for m in (2, 128, 1024, 4096) for k in (1, 3) for b in (-1, 0, 1) if 0 <= b + k * m <= n})
    r = [(b, n) for b in edges] + [(0, e) for e in edges] + [(b, 2 * 4096 + e) for b, e in zip(edges, edges) if 2 * 4096 + e <= n]
    r += [(m - 1, m + 1) for m in (2, 128, 1024, 4096)] + [(m, m + 1) for m in (2, 128, 1024, 4096)] + [(0, n), (5, 5), (n - 1, n), (5 * 4096, n), (5 * 4096 + 1, n - 1)]
    return r


def run_ranges(pl, ranges):
    out = []
    for b, e in ranges:
        pl.run(b, e)
        out.append(lc_result(pl.fetch()))
    return out


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in ("PH_SCAN_GRID", "PH_SCAN_PACK_MIN_BYTES"):
        monkeypatch.delenv(k, raising=False)


# ---------------------------------------------------------------- the group asked for by name

@pytest.mark.parametrize("make", [lineitem_like, full_fields], ids=["lineitem_layout", "full_fields"])
def test_group_by_name_ranges_slots_and_grids(ctx, monkeypatch, make):
    c = make()
    n = len(c["p"])
    ranges = boundary_ranges(n)
    t = lc_table(ctx, c)
    plans, before, want = [], [], []
    for lo, hi in intervals_of(c):
        pl = lc_plan(ctx, t, lo, hi, c["ptype"])
        assert pl.kind == "lowcard_chain" and pl.variant == "narrow32_lean" and pl.bytes_per_row == 11
        plans.append(pl)
        before.append(run_ranges(pl, ranges))
        want.append([lc_want(c, lo, hi, b, e) for b, e in ranges])
        assert pl.variant == "narrow32_lean" and pl.bytes_per_row == 11   # no group yet, none triggered on this small table
        for got, w in zip(before[-1], want[-1]):
            assert sorted(got) == w
    # six slots were used, one by a single row, one only in the last partial tile; the empty intervals gave nothing
    full = dict((g[1], g) for g in before[0][ranges.index((0, n))])
    assert len(full) == 6 and full[(2, 1)][3] == 1 and full[(2, 1)][0] == 777 and full[(2, 0)][0] == n - 3
    assert all(r == [] for r in before[2]) and all(r == [] for r in before[3])
    assert t.scan_group_bytes() == 0
    t.pack_scan_group(COLS)
    assert t.scan_group_bytes() == padded(n) * 8
    narrow = t.narrow_bytes()
    t.pack_scan_group(COLS)   # found, not built again
    assert t.scan_group_bytes() == padded(n) * 8 and t.narrow_bytes() == narrow == padded(n) * 9
    for grid in (None, "1", "2"):
        if grid is not None:
            monkeypatch.setenv("PH_SCAN_GRID", grid)
        for pl, b4 in zip(plans, before):
            got = run_ranges(pl, ranges)
            assert pl.variant == "packed64" and pl.bytes_per_row == 8
            assert got == b4   # the same groups, in the same order, with the same first row ids, sums and counts
    for pl in plans:
        pl.free()
    t.free()


@pytest.mark.parametrize("n,ranges", [(3 * 8192 - 5, [(48, None), (16, -1), (4097 + 32, None), (0, None)]),   # the last tile reaches past the padding
                                      (8192, [(0, None), (16, None), (1, -1), (4090, None)])],                   # no padding at all
                         ids=["last_tile_past_padding", "rows_fill_the_padding"])
def test_last_tile_and_padding(ctx, n, ranges):
    c = full_fields(n, seed=3)
    ranges = [(b, n if e is None else n + e) for b, e in ranges]
    t = lc_table(ctx, c)
    lo, hi = D0 + 5, D0 + 4000
    pl = lc_plan(ctx, t, lo, hi, c["ptype"])
    before = run_ranges(pl, ranges)
    assert pl.variant == "narrow32_lean"
    t.pack_scan_group(COLS)
    got = run_ranges(pl, ranges)
    assert pl.variant == "packed64" and pl.bytes_per_row == 8
    assert got == before
    for (b, e), g in zip(ranges, got):
        assert sorted(g) == lc_want(c, lo, hi, b, e)
    pl.free()
    t.free()


# ---------------------------------------------------------------- the automatic path

def auto_runs(ctx, c, runs=3):
    """one plan over a fresh table, `runs` full scans: [(variant, bytes per row, result, scan_group_bytes) after each run]"""
    t = lc_table(ctx, c)
    pl = lc_plan(ctx, t, D0 + 10, D0 + 3000, c["ptype"])
    out = []
    for _ in range(runs):
        pl.run()
        out.append([pl.variant, pl.bytes_per_row, lc_result(pl.fetch()), t.scan_group_bytes()])
    pl.free()
    t.free()
    return out


def test_second_full_scan_builds_and_binds(ctx, monkeypatch):
    monkeypatch.setenv("PH_SCAN_PACK_MIN_BYTES", "0")
    c = full_fields()
    n = len(c["p"])
    t = lc_table(ctx, c)
    lo, hi = D0 + 10, D0 + 3000
    pl = lc_plan(ctx, t, lo, hi, c["ptype"])
    pl.run()
    r1 = lc_result(pl.fetch())
    assert pl.variant == "narrow32_lean" and pl.bytes_per_row == 11 and t.scan_group_bytes() == 0
    pl.run()
    r2 = lc_result(pl.fetch())
    assert pl.variant == "packed64" and pl.bytes_per_row == 8 and t.scan_group_bytes() == padded(n) * 8
    assert r1 == r2 and sorted(r1) == lc_want(c, lo, hi, 0, n)
    # a second plan over the same table binds the same group at its first run
    p2 = lc_plan(ctx, t, lo + 7, hi - 7, c["ptype"])
    assert p2.variant == "narrow32_lean" and p2.bytes_per_row == 11
    p2.run(3, n - 2)
    assert p2.variant == "packed64" and p2.bytes_per_row == 8
    assert sorted(lc_result(p2.fetch())) == lc_want(c, lo + 7, hi - 7, 3, n - 2)
    assert t.scan_group_bytes() == padded(n) * 8
    pl.free()
    p2.free()
    t.free()


def test_two_half_scans_count_as_one(ctx, monkeypatch):
    """the trigger counts rows: the group is built by the run that takes the count to twice the table's rows"""
    monkeypatch.setenv("PH_SCAN_PACK_MIN_BYTES", "0")
    c = full_fields()
    n = len(c["p"])
    t = lc_table(ctx, c)
    pl = lc_plan(ctx, t, D0, D0 + 4095, c["ptype"])
    for b, e in [(0, n // 2), (n // 2, n), (0, n - 1)]:
        pl.run(b, e)
        assert pl.variant == "narrow32_lean" and t.scan_group_bytes() == 0
    pl.run(0, 1)
    assert pl.variant == "packed64" and t.scan_group_bytes() == padded(n) * 8
    assert sorted(lc_result(pl.fetch())) == lc_want(c, D0, D0 + 4095, 0, 1)
    pl.free()
    t.free()


def test_budget_zero_never_builds(ctx, monkeypatch):
    monkeypatch.setenv("PH_SCAN_PACK_MIN_BYTES", "0")
    c = full_fields()
    t = lc_table(ctx, c)
    t.set_colocate_budget(0)
    pl = lc_plan(ctx, t, D0 + 10, D0 + 3000, c["ptype"])
    res = []
    for _ in range(3):
        pl.run()
        res.append(lc_result(pl.fetch()))
        assert pl.variant == "narrow32_lean" and pl.bytes_per_row == 11 and t.scan_group_bytes() == 0
    assert res[0] == res[1] == res[2]
    t.pack_scan_group(COLS)   # by name: the host's decision, not limited by the budget
    pl.run()
    assert pl.variant == "packed64" and lc_result(pl.fetch()) == res[0]
    pl.free()
    t.free()


def test_without_the_override_never_built_on_a_small_table(ctx):
    runs = auto_runs(ctx, full_fields())
    assert [r[:2] + r[3:] for r in runs] == [["narrow32_lean", 11, 0]] * 3
    assert runs[0][2] == runs[1][2] == runs[2][2]


def test_switched_off_in_a_child_process(ctx, monkeypatch):
    """PH_SCAN_PACK=0 (read once per process): no automatic build, and a group built by name is not bound"""
    monkeypatch.setenv("PH_SCAN_PACK_MIN_BYTES", "0")
    here = auto_runs(ctx, full_fields())
    assert [r[0] for r in here] == ["narrow32_lean", "packed64", "packed64"]
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"packed_child_{os.getpid()}.json")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, PH_SCAN_PACK="0", PH_SCAN_PACK_MIN_BYTES="0"), check=True, timeout=300)
    with open(out) as f:
        child = json.load(f)
    os.remove(out)
    assert [r[:2] + r[3:] for r in child["auto"]] == [["narrow32_lean", 11, 0]] * 3
    assert child["by_name"][0] == "narrow32_lean" and child["by_name"][1] == 11 and child["by_name"][3] > 0
    want = json.loads(json.dumps(here[0][2]))
    assert all(r[2] == want for r in child["auto"]) and child["by_name"][2] == want


def test_ineligible_sets(ctx, monkeypatch):
    monkeypatch.setenv("PH_SCAN_PACK_MIN_BYTES", "0")
    cases = {
        # e over 2^32 values: no narrowed copy, the plan reads the wide columns
        "no_narrowed_copy": (lc_data(N, 4, D0, D0 + 100, e=(-(2 ** 31), 2 ** 31)), "wide", 34),
        # a one-byte predicate column: narrowed, but not the lean instance's width tuple
        "other_width_tuple": (lc_data(N, 5, D0, D0 + 255), None, 10),
    }
    for name, (c, variant, bpr) in cases.items():
        t = lc_table(ctx, c)
        with pytest.raises(hip.PlanHipError) as ei:
            t.pack_scan_group(COLS)
        assert ei.value.code == hip.PH_EUNSUPPORTED and "narrowed copy" in str(ei.value), name
        pl = lc_plan(ctx, t, D0 + 10, D0 + 90, c["ptype"])
        variant = variant or pl.variant
        assert variant not in ("narrow32_lean", "packed64")
        res = []
        for _ in range(3):
            pl.run()
            res.append(lc_result(pl.fetch()))
            assert pl.variant == variant and pl.bytes_per_row == bpr and t.scan_group_bytes() == 0, name
        assert res[0] == res[1] == res[2] and sorted(res[0]) == lc_want(c, D0 + 10, D0 + 90, 0, N), name
        pl.free()
        t.free()
    # a NULL-able column, a column named twice, a wrong count
    c = full_fields()
    valid = np.full((N + 7) // 8, 0xFF, np.uint8)
    valid[1] = 0xFD
    t = hip.Table(ctx, [(hip.PH_I32, c["q"], 0, valid), (hip.PH_DEC64, c["e"], 2), (hip.PH_DEC64, c["d"], 2), (hip.PH_DEC64, c["t"], 2),
                        (hip.PH_CODE8, c["k0"], 0, None, ["a", "b", "c"]), (hip.PH_CODE8, c["k1"], 0, None, ["x", "y"]), (hip.PH_DATE, c["p"])], N)
    for cols, code in ((COLS, hip.PH_EUNSUPPORTED), ([P, Q, E, D, D, K0, K1], hip.PH_EUNSUPPORTED), (COLS[:6], hip.PH_EINVAL)):
        with pytest.raises(hip.PlanHipError) as ei:
            t.pack_scan_group(cols)
        assert ei.value.code == code
    assert t.scan_group_bytes() == 0
    t.free()


if __name__ == "__main__":   # test_switched_off_in_a_child_process: the same runs under PH_SCAN_PACK=0
    _ctx = hip.Ctx(0)
    _c = full_fields()
    _res = {"auto": auto_runs(_ctx, _c)}
    _t = lc_table(_ctx, _c)
    _t.pack_scan_group(COLS)
    _pl = lc_plan(_ctx, _t, D0 + 10, D0 + 3000, _c["ptype"])
    _pl.run()
    _res["by_name"] = [_pl.variant, _pl.bytes_per_row, lc_result(_pl.fetch()), _t.scan_group_bytes()]
    _pl.free()
    _t.free()
    _ctx.close()
    with open(sys.argv[1], "w") as _f:
        json.dump(_res, _f)
