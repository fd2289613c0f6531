"""GPU tests of the fused Q1-shaped scan over a scan group in the split form (ph_table_pack_scan_group_ex, "split56", DESIGN.md §3 and
§4.1): 7 bytes a row in blocks of 1024 rows instead of one 64-bit word a row. Every comparison is equality of integers: against a
numpy / Python-integer restatement and against the same plan's results under PH_SCAN_SPLIT=0 (read at every run: the group is not bound
and the plan reads the narrowed copies). Tables have lineitem's field widths (12, 6, 24, 4, 4 bits and 3 for the slot): the split form
exists for that layout only. A column's width comes from its minimum and maximum, so such a table has at least two rows; the one-row case
is one-row ranges of such tables, and a one-row table is checked to be refused the split form.
Tables and plans come from test_gpu_narrow_scan's, test_gpu_packed_scan's and test_gpu_hist_scan's helpers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from plan_amd import hip  # noqa: E402
from test_gpu_narrow_scan import lc_data, lc_plan, lc_result, lc_table, lc_want  # noqa: E402
from test_gpu_packed_scan import COLS, D0, full_fields, padded  # noqa: E402
from test_gpu_hist_scan import plan_signed, want_signed  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 4096
WORD64, SPLIT56 = 0, 1
P_LO, P_HI = D0, D0 + 4095
SWITCHES = ("PH_SCAN_GRID", "PH_SCAN_PACK_MIN_BYTES", "PH_SCAN_SPLIT_MIN_BYTES", "PH_SCAN_SPLIT", "PH_SCAN_HIST")


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def fields(n, seed, d=(0, 15), t=(0, 15)):
    """every field's span all ones — 12, 6, 24, 4, 4 bits, lineitem's layout; rows 0 and 1 hold code 0 and the maximum of every field
    (lc_data); six slots, anywhere"""
    return lc_data(n, seed, P_LO, P_HI, q=(-13, 50), e=(-(2 ** 23), 2 ** 23 - 1), d=d, t=t)


def split_table(ctx, c):
    t = lc_table(ctx, c)
    t.pack_scan_group_ex(COLS, SPLIT56)
    assert t.scan_group_bytes() == padded(len(c["p"])) * 7
    return t


def run_ranges(pl, ranges):
    out = []
    for b, e in ranges:
        pl.run(b, e)
        out.append(lc_result(pl.fetch()))
    return out


def check_split(pl, monkeypatch, ranges, want, body="bins", grids=(None, "1", "2")):
    """pl is a fresh plan over a table that holds a split group. Under PH_SCAN_SPLIT=0 it reads the narrowed copies; then it binds the
    group: the same results at every grid, under the default row body and under PH_SCAN_HIST=0; all equal to `want`. Returns the results."""
    monkeypatch.setenv("PH_SCAN_SPLIT", "0")
    ref = run_ranges(pl, ranges)
    assert pl.variant == "narrow32_lean" and pl.bytes_per_row == 11
    monkeypatch.delenv("PH_SCAN_SPLIT")
    for (b, e), r, w in zip(ranges, ref, want):
        assert sorted(r) == w, (b, e)
    for grid in grids:
        if grid is not None:
            monkeypatch.setenv("PH_SCAN_GRID", grid)
        for (b, e), r in zip(ranges, ref):
            pl.run(b, e)
            assert pl.variant == "split56" and pl.bytes_per_row == 7 and pl.row_body == body, (grid, b, e)
            assert lc_result(pl.fetch()) == r, (grid, b, e)
    monkeypatch.delenv("PH_SCAN_GRID", raising=False)
    monkeypatch.setenv("PH_SCAN_HIST", "0")
    for (b, e), r in zip(ranges, ref):
        assert pl.row_body == "columns"
        pl.run(b, e)
        assert pl.variant == "split56" and lc_result(pl.fetch()) == r, ("columns", b, e)
    monkeypatch.delenv("PH_SCAN_HIST")
    return ref


def cut_ranges(n):
    """row ranges that start and end one row before, at and after the boundaries of a quad's 4 rows, a load's 256, a block's 1024 and a
    tile's 4096: most starts are no multiple of 4, and none but 4096 and 12288 of 4096"""
    edges = sorted({b + k * m for m in (4, 256, 1024, TILE) for k in (1, 3) for b in (-1, 0, 1) if 0 <= b + k * m <= n})
    r = [(b, n) for b in edges] + [(0, e) for e in edges] + [(b, e) for b, e in zip(edges, edges[3:])]
    r += [(m - 1, m + 1) for m in (4, 256, 1024, TILE) if m + 1 <= n] + [(m, m + 1) for m in (4, 256, 1024, TILE) if m + 1 <= n]
    r += [(0, n), (0, 1), (n - 1, n), (n, n), (0, 0), (min(5, n), min(5, n))]
    return sorted(set(r))


# ---------------------------------------------------------------- sizes, range cuts, grids

@pytest.mark.parametrize("n", [2, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 12289])
def test_sizes_ranges_and_grids(ctx, monkeypatch, n):
    c = fields(n, 100 + n)
    ranges = cut_ranges(n)
    if n == 12289:
        assert any(b % 4 and b % TILE for b, _ in ranges) and (TILE + 1, n) in ranges and (3 * TILE - 1, n) in ranges
    t = split_table(ctx, c)
    lo, hi = P_LO + 200, P_HI - 200
    pl = lc_plan(ctx, t, lo, hi, c["ptype"])
    assert pl.kind == "lowcard_chain"
    check_split(pl, monkeypatch, ranges, [lc_want(c, lo, hi, b, e) for b, e in ranges])
    pl.free()
    # every row passing, so that rows 0 and 1 (all codes 0, all codes at their maximum) count
    pl = lc_plan(ctx, t, P_LO, P_HI, c["ptype"])
    some = [(0, n), (0, 1), (1, 2), (1, n), (n - 1, n)]
    check_split(pl, monkeypatch, some, [lc_want(c, P_LO, P_HI, b, e) for b, e in some], grids=(None,))
    pl.free()
    t.free()


def test_a_one_row_table_has_another_layout(ctx):
    """one row: every field is one bit wide, which is not lineitem's layout, so the split form is refused and the 64-bit form serves"""
    c = dict(p=np.array([P_LO + 7], np.int32), q=np.array([5], np.int32), e=np.array([12345], np.int64), d=np.array([3], np.int64),
             t=np.array([2], np.int64), k0=np.array([2], np.uint8), k1=np.array([1], np.uint8), ptype=hip.PH_DATE)
    t = lc_table(ctx, c)
    with pytest.raises(hip.PlanHipError) as ei:
        t.pack_scan_group_ex(COLS, SPLIT56)
    assert ei.value.code == hip.PH_EUNSUPPORTED and t.scan_group_bytes() == 0
    t.free()


# ---------------------------------------------------------------- field extremes, row by row of a quad

def test_field_extremes_in_each_row_of_a_quad(ctx, monkeypatch):
    """code 0 of every field with slot 0, and the maximum of every field with the last slot, in each of a quad's four rows in turn, in
    quads of different loads, lanes, blocks and tiles; everything else strictly inside, so the two one-value predicates select exactly
    those rows. Row 3 of a quad carries slot = max and shipdate = max in its three top bytes."""
    n = 2 * TILE + 77
    c = fields(n, 21)
    inside = np.arange(n) >= 2
    c["p"][inside] = np.clip(c["p"][inside], P_LO + 1, P_HI - 1)
    quads = [8, 256 + 4 * 63, 1024 + 2 * 256 + 16, 3 * 1024 + 3 * 256 + 252, TILE + 4, TILE + 1024 + 256, TILE + 2048 + 768 + 128, 2 * TILE + 72]
    zero_rows, max_rows = [], []
    for i, qb in enumerate(quads):
        r = qb + i % 4                      # the quad's row i % 4
        rows, (p, q, e, d, tt, k0, k1) = (zero_rows, (P_LO, -13, -(2 ** 23), 0, 0, 0, 0)) if i < 4 else (max_rows, (P_HI, 50, 2 ** 23 - 1, 15, 15, 2, 1))
        c["p"][r], c["q"][r], c["e"][r], c["d"][r], c["t"][r], c["k0"][r], c["k1"][r] = p, q, e, d, tt, k0, k1
        rows.append(r)
    assert sorted(r % 4 for r in zero_rows) == sorted(r % 4 for r in max_rows) == [0, 1, 2, 3]
    t = split_table(ctx, c)
    ranges = [(0, n), (2, n)] + [(r, r + 1) for r in zero_rows + max_rows] + [(r - 3, min(n, r + 4)) for r in zero_rows + max_rows]
    for lo, hi in [(P_LO, P_HI), (P_HI, P_HI), (P_LO, P_LO), (P_LO + 1, P_HI - 1)]:
        pl = lc_plan(ctx, t, lo, hi, c["ptype"])
        got = check_split(pl, monkeypatch, ranges, [lc_want(c, lo, hi, b, e) for b, e in ranges], grids=(None, "1"))
        if lo == hi:   # from row 2 on only the special rows pass: one group, with the first of them as its first row
            rows = max_rows if lo == P_HI else zero_rows
            g = got[ranges.index((2, n))]
            assert len(g) == 1 and g[0][0] == rows[0] and g[0][3] == 4 and g[0][1] == ((2, 1) if lo == P_HI else (0, 0))
        pl.free()
    t.free()


# ---------------------------------------------------------------- first rows, failing rows, empty tiles and ranges

def test_first_rows_failing_rows_and_empty_tiles(ctx, monkeypatch):
    """tile 0: no row passes; tile 1: one row passes; tile 2: random. Slot (2, 1)'s only passing row is row 3 of a quad (the first-row
    minimum is taken of the rebuilt row's id); slot (2, 0)'s only row is the last of the range; empty ranges give nothing."""
    n = 3 * TILE + 5
    c = fields(n, 22)
    lo, hi = P_LO + 1000, P_LO + 3000
    c["p"][2:2 * TILE] = P_LO + (np.arange(2, 2 * TILE) % 900)     # below lo
    c["p"][TILE + 1234] = P_LO + 2000
    c["k0"][c["k0"] == 2] = 1                                      # slots (2, *) only where put below
    r3 = 2 * TILE + 1024 + 256 + 4 * 17 + 3                        # row 3 of a quad
    c["k0"][r3], c["k1"][r3], c["p"][r3] = 2, 1, hi
    c["k0"][r3 - 4], c["k1"][r3 - 4], c["p"][r3 - 4] = 2, 1, hi + 1   # the same slot earlier, failing
    c["k0"][n - 1], c["k1"][n - 1], c["p"][n - 1] = 2, 0, lo
    t = split_table(ctx, c)
    pl = lc_plan(ctx, t, lo, hi, c["ptype"])
    ranges = [(0, TILE), (0, 2 * TILE), (TILE, 2 * TILE), (TILE + 1234, TILE + 1235), (TILE + 1235, 2 * TILE), (7, 7), (n, n), (0, 0), (TILE, TILE),
              (0, n), (2 * TILE, n), (n - 1, n), (0, n - 1), (r3, r3 + 1), (r3 - 3, r3 + 1), (r3 + 1, n), (5, n - 1)]
    got = check_split(pl, monkeypatch, ranges, [lc_want(c, lo, hi, b, e) for b, e in ranges])
    by = dict(zip(ranges, got))
    assert by[(0, TILE)] == [] and by[(7, 7)] == [] and by[(n, n)] == [] and by[(TILE + 1235, 2 * TILE)] == [] and by[(TILE, TILE)] == []
    assert len(by[(TILE, 2 * TILE)]) == 1 and by[(TILE, 2 * TILE)][0][0] == TILE + 1234 and by[(TILE, 2 * TILE)][0][3] == 1
    g21 = [g for g in by[(0, n)] if g[1] == (2, 1)]
    assert len(g21) == 1 and g21[0][0] == r3 and g21[0][3] == 1
    g20 = [g for g in by[(0, n)] if g[1] == (2, 0)]
    assert len(g20) == 1 and g20[0][0] == n - 1 and g20[0][3] == 1 and not [g for g in by[(0, n - 1)] if g[1] == (2, 0)]
    pl.free()
    t.free()


# ---------------------------------------------------------------- the instances

def slot_table(ctx, c, nslots):
    """nslots x 1 dictionaries: k0 = row % nslots, but the last slot only at row 3 of a quad"""
    n = len(c["p"])
    c["k0"] = (np.arange(n) % (nslots - 1)).astype(np.uint8)
    c["k0"][4 * 501 + 3] = nslots - 1
    c["k1"] = np.zeros(n, np.uint8)
    t = hip.Table(ctx, [(hip.PH_I32, c["q"]), (hip.PH_DEC64, c["e"], 2), (hip.PH_DEC64, c["d"], 2), (hip.PH_DEC64, c["t"], 2),
                        (hip.PH_CODE8, c["k0"], 0, None, list("abcdefgh")[:nslots]), (hip.PH_CODE8, c["k1"], 0, None, ["x"]), (hip.PH_DATE, c["p"])], n)
    t.pack_scan_group_ex(COLS, SPLIT56)
    return t


@pytest.mark.parametrize("nslots,s2", [(5, 1), (5, -1), (6, 1), (6, -1), (7, 1)], ids=["five_plus", "five_minus", "six_plus", "six_minus", "seven"])
def test_five_six_and_seven_slots_signed_factors(ctx, monkeypatch, nslots, s2):
    """d and t around 100: f1 = 100 - d runs from 7 to -8 and, with s2 = -1, f2 = 100 - t crosses zero too; e of both signs. Five and six
    slots run the bins body, seven the columns."""
    n = 2 * TILE + 9
    c = fields(n, 30 + nslots, d=(93, 108), t=(93, 108))
    lo, hi = P_LO + 300, P_HI - 300
    c["p"][4 * 501 + 3] = hi
    t = slot_table(ctx, c, nslots)
    pl = plan_signed(ctx, t, lo, hi, c["ptype"], s2)
    ranges = [(0, n), (3, n - 3), (4 * 501 + 3, 4 * 501 + 4), (TILE - 1, TILE + 1)]
    want = [want_signed(c, lo, hi, b, e, s2, nk1=1) for b, e in ranges]
    assert len(want[0]) == nslots and want[0][-1][0] == 4 * 501 + 3
    check_split(pl, monkeypatch, ranges, want, body="bins" if nslots <= 6 else "columns", grids=(None, "2"))
    pl.free()
    t.free()


@pytest.fixture(scope="module")
def one_bin():
    """1024 tiles, every row in bin (slot 5, d = t = 15) with p, q and e at their maximum codes, but the one row that pins the columns'
    minima: the last row of tile 1022 (row 3 of a quad), so that both lengths below have it in their last tile or the one before"""
    n = 1024 * TILE
    c = dict(p=np.full(n, 8036 + 4095, np.int32), q=np.full(n, 63, np.int32), e=np.full(n, 2 ** 24 - 1, np.int64), d=np.full(n, 15, np.int64),
             t=np.full(n, 15, np.int64), k0=np.full(n, 2, np.uint8), k1=np.full(n, 1, np.uint8), ptype=hip.PH_DATE)
    r = 1023 * TILE - 1
    c["p"][r], c["q"][r], c["e"][r], c["d"][r], c["t"][r], c["k0"][r], c["k1"][r] = 8036, 0, 0, 0, 0, 0, 0
    return c


def one_bin_want(n):
    """the two groups over rows [0, n), n beyond the pinning row, in closed form and Python integers"""
    m = n - 1
    big = (0, (2, 1), [63 * m, (2 ** 24 - 1) * m, (2 ** 24 - 1) * 85 * m, (2 ** 24 - 1) * 85 * 115 * m, 15 * m], m)
    return sorted([big, (1023 * TILE - 1, (0, 0), [0, 0, 0, 0, 0], 1)])


@pytest.mark.parametrize("tiles", [1023, 1024], ids=["at_the_bound", "one_tile_beyond"])
def test_one_bin_1023_tiles_in_one_workgroup_and_one_more(ctx, monkeypatch, one_bin, tiles):
    """PH_SCAN_GRID=1 over 1023 tiles: the bound of the bins' packed count and sum exactly, every row on one bin. One tile more: the run
    raises its grid or takes the columns; either way the same integers."""
    n = tiles * TILE
    c = {k: (v[:n] if k != "ptype" else v) for k, v in one_bin.items()}
    t = split_table(ctx, c)
    pl = lc_plan(ctx, t, 8036, 8036 + 4095, c["ptype"])
    monkeypatch.setenv("PH_SCAN_GRID", "1")
    pl.run(0, n)
    assert pl.variant == "split56" and pl.bytes_per_row == 7 and (pl.row_body == "bins" if tiles == 1023 else pl.row_body in ("bins", "columns"))
    got = lc_result(pl.fetch())
    assert sorted(got) == one_bin_want(n)
    monkeypatch.setenv("PH_SCAN_HIST", "0")
    pl.run(0, n)
    assert pl.row_body == "columns" and lc_result(pl.fetch()) == got
    pl.free()
    t.free()


# ---------------------------------------------------------------- the automatic path and the explicit forms

N_AUTO = 2 * TILE + 77


def auto_runs(ctx, c, runs=3, budget=None):
    """one plan over a fresh table, `runs` full scans: [(variant, bytes per row, result, scan_group_bytes) after each run]"""
    t = lc_table(ctx, c)
    if budget is not None:
        t.set_colocate_budget(budget)
    pl = lc_plan(ctx, t, P_LO + 10, P_LO + 3000, c["ptype"])
    out = []
    for _ in range(runs):
        pl.run()
        out.append([pl.variant, pl.bytes_per_row, lc_result(pl.fetch()), t.scan_group_bytes()])
    pl.free()
    t.free()
    return out


def test_second_full_scan_builds_and_binds_the_split_form(ctx, monkeypatch):
    monkeypatch.setenv("PH_SCAN_PACK_MIN_BYTES", "0")
    monkeypatch.setenv("PH_SCAN_SPLIT_MIN_BYTES", "0")
    c = fields(N_AUTO, 40)
    n = N_AUTO
    t = lc_table(ctx, c)
    lo, hi = P_LO + 10, P_LO + 3000
    pl = lc_plan(ctx, t, lo, hi, c["ptype"])
    pl.run()
    r1 = lc_result(pl.fetch())
    assert pl.variant == "narrow32_lean" and pl.bytes_per_row == 11 and t.scan_group_bytes() == 0
    pl.run()
    r2 = lc_result(pl.fetch())
    assert pl.variant == "split56" and pl.bytes_per_row == 7 and pl.row_body == "bins" and t.scan_group_bytes() == padded(n) * 7
    assert r1 == r2 and sorted(r1) == lc_want(c, lo, hi, 0, n)
    p2 = lc_plan(ctx, t, lo + 7, hi - 7, c["ptype"])   # a second plan binds the same group at its first run
    assert p2.variant == "narrow32_lean" and p2.bytes_per_row == 11
    p2.run(3, n - 2)
    assert p2.variant == "split56" and p2.bytes_per_row == 7
    assert sorted(lc_result(p2.fetch())) == lc_want(c, lo + 7, hi - 7, 3, n - 2)
    assert t.scan_group_bytes() == padded(n) * 7
    # the set has its group: the 64-bit form by name is refused, the split form is found
    with pytest.raises(hip.PlanHipError) as ei:
        t.pack_scan_group(COLS)
    assert ei.value.code == hip.PH_EUNSUPPORTED and "other form" in str(ei.value)
    with pytest.raises(hip.PlanHipError) as ei:
        t.pack_scan_group_ex(COLS, WORD64)
    assert ei.value.code == hip.PH_EUNSUPPORTED
    t.pack_scan_group_ex(COLS, SPLIT56)
    assert t.scan_group_bytes() == padded(n) * 7
    pl.free()
    p2.free()
    t.free()


def test_without_the_size_override_a_small_table_gets_the_word(ctx, monkeypatch):
    monkeypatch.setenv("PH_SCAN_PACK_MIN_BYTES", "0")
    c = fields(N_AUTO, 40)
    monkeypatch.setenv("PH_SCAN_SPLIT_MIN_BYTES", "0")
    split = auto_runs(ctx, c)
    monkeypatch.delenv("PH_SCAN_SPLIT_MIN_BYTES")
    word = auto_runs(ctx, c)
    assert [r[:2] + r[3:] for r in split] == [["narrow32_lean", 11, 0], ["split56", 7, padded(N_AUTO) * 7], ["split56", 7, padded(N_AUTO) * 7]]
    assert [r[:2] + r[3:] for r in word] == [["narrow32_lean", 11, 0], ["packed64", 8, padded(N_AUTO) * 8], ["packed64", 8, padded(N_AUTO) * 8]]
    assert all(r[2] == split[0][2] for r in split + word)
    # one byte below the 64-bit group's size still splits, its size itself does not
    monkeypatch.setenv("PH_SCAN_SPLIT_MIN_BYTES", str(padded(N_AUTO) * 8 - 1))
    assert auto_runs(ctx, c, 2)[1][0] == "split56"
    monkeypatch.setenv("PH_SCAN_SPLIT_MIN_BYTES", str(padded(N_AUTO) * 8))
    assert auto_runs(ctx, c, 2)[1][0] == "packed64"


def test_no_split_group_when_switched_off_out_of_budget_or_another_layout(ctx, monkeypatch):
    monkeypatch.setenv("PH_SCAN_PACK_MIN_BYTES", "0")
    monkeypatch.setenv("PH_SCAN_SPLIT_MIN_BYTES", "0")
    c = fields(N_AUTO, 41)
    here = auto_runs(ctx, c)
    assert [r[0] for r in here] == ["narrow32_lean", "split56", "split56"]
    # PH_SCAN_SPLIT=0: the automatic group is the 64-bit word, and the split form by name is refused
    monkeypatch.setenv("PH_SCAN_SPLIT", "0")
    off = auto_runs(ctx, c)
    assert [r[:2] + r[3:] for r in off] == [["narrow32_lean", 11, 0], ["packed64", 8, padded(N_AUTO) * 8], ["packed64", 8, padded(N_AUTO) * 8]]
    t = lc_table(ctx, c)
    with pytest.raises(hip.PlanHipError) as ei:
        t.pack_scan_group_ex(COLS, SPLIT56)
    assert ei.value.code == hip.PH_EUNSUPPORTED and t.scan_group_bytes() == 0
    t.free()
    monkeypatch.delenv("PH_SCAN_SPLIT")
    # budget 0: nothing is built
    none = auto_runs(ctx, c, budget=0)
    assert [r[:2] + r[3:] for r in none] == [["narrow32_lean", 11, 0]] * 3
    assert all(r[2] == here[0][2] for r in off + none)
    # another layout (8-bit d and t): the 64-bit word, and the split form by name is refused
    o = full_fields(N_AUTO, 42)
    t = lc_table(ctx, o)
    with pytest.raises(hip.PlanHipError) as ei:
        t.pack_scan_group_ex(COLS, SPLIT56)
    assert ei.value.code == hip.PH_EUNSUPPORTED and "lineitem" in str(ei.value) and t.scan_group_bytes() == 0
    pl = lc_plan(ctx, t, P_LO + 10, P_LO + 3000, o["ptype"])
    res = []
    for _ in range(3):
        pl.run()
        res.append([pl.variant, pl.bytes_per_row, lc_result(pl.fetch())])
    assert [r[:2] for r in res] == [["narrow32_lean", 11], ["packed64", 8], ["packed64", 8]] and t.scan_group_bytes() == padded(N_AUTO) * 8
    assert res[0][2] == res[1][2] == res[2][2] and sorted(res[0][2]) == lc_want(o, P_LO + 10, P_LO + 3000, 0, N_AUTO)
    with pytest.raises(hip.PlanHipError) as ei:   # the word exists: the other form is refused
        t.pack_scan_group_ex(COLS, SPLIT56)
    assert ei.value.code == hip.PH_EUNSUPPORTED
    pl.free()
    t.free()
    # a bad form
    t = lc_table(ctx, c)
    with pytest.raises(hip.PlanHipError) as ei:
        t.pack_scan_group_ex(COLS, 2)
    assert ei.value.code == hip.PH_EINVAL
    t.free()


def test_pack_switched_off_in_a_child_process(ctx, monkeypatch):
    """PH_SCAN_PACK=0 (read once per process): no automatic build, and a split group built by name is not bound"""
    monkeypatch.setenv("PH_SCAN_PACK_MIN_BYTES", "0")
    monkeypatch.setenv("PH_SCAN_SPLIT_MIN_BYTES", "0")
    here = auto_runs(ctx, fields(N_AUTO, 43))
    assert [r[0] for r in here] == ["narrow32_lean", "split56", "split56"]
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"split_child_{os.getpid()}.json")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, PH_SCAN_PACK="0"), check=True, timeout=300)
    with open(out) as f:
        child = json.load(f)
    os.remove(out)
    assert [r[:2] + r[3:] for r in child["auto"]] == [["narrow32_lean", 11, 0]] * 3
    assert child["by_name"][:2] == ["narrow32_lean", 11] and child["by_name"][3] == padded(N_AUTO) * 7
    want = json.loads(json.dumps(here[0][2]))
    assert all(r[2] == want for r in child["auto"]) and child["by_name"][2] == want


if __name__ == "__main__":   # test_pack_switched_off_in_a_child_process: the same runs under PH_SCAN_PACK=0
    _ctx = hip.Ctx(0)
    _c = fields(N_AUTO, 43)
    _res = {"auto": auto_runs(_ctx, _c)}
    _t = lc_table(_ctx, _c)
    _t.pack_scan_group_ex(COLS, SPLIT56)
    _pl = lc_plan(_ctx, _t, P_LO + 10, P_LO + 3000, _c["ptype"])
    _pl.run()
    _res["by_name"] = [_pl.variant, _pl.bytes_per_row, lc_result(_pl.fetch()), _t.scan_group_bytes()]
    _pl.free()
    _t.free()
    _ctx.close()
    with open(sys.argv[1], "w") as _f:
        json.dump(_res, _f)
