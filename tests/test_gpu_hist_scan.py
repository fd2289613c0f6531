"""GPU tests of the bins row body of the packed Q1-shaped scan (BinsBody of lowcard_chain_kernel_group, ph_scan_plan_row_body == "bins"):
prices binned by (slot, tax, discount), products folded once per workgroup. Every comparison is equality of integers, against a numpy /
Python-integer restatement and against the same plan's result under PH_SCAN_HIST=0 (the columns body; the switch is read at every run).
Tables and plans come from test_gpu_narrow_scan's and test_gpu_packed_scan's helpers."""
import numpy as np
import pytest

from plan_amd import hip
from test_gpu_narrow_scan import D, E, K0, K1, P, Q, T, exact_sum, lc_data, lc_plan, lc_result, lc_table, lc_want
from test_gpu_packed_scan import COLS, D0, full_fields, lineitem_like

pytestmark = pytest.mark.gpu

TILE = 4096


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in ("PH_SCAN_GRID", "PH_SCAN_PACK_MIN_BYTES", "PH_SCAN_HIST"):
        monkeypatch.delenv(k, raising=False)


def plan_signed(ctx, t, lo, hi, ptype, s2):
    """lc_plan with the second factor (1 + s2 t): s2 = -1 gives a negative B2"""
    e, d, tt = hip.X_COL(E), hip.X_COL(D), hip.X_COL(T)
    one = hip.X_CONST(1, 0)
    dp = [e, one, d, hip.X_SUB, hip.X_MUL]
    aggs = [hip.aggexpr(hip.PH_A_SUM, [hip.X_COL(Q)]), hip.aggexpr(hip.PH_A_SUM, [e]), hip.aggexpr(hip.PH_A_SUM, dp),
            hip.aggexpr(hip.PH_A_SUM, dp + [one, tt, hip.X_ADD if s2 > 0 else hip.X_SUB, hip.X_MUL]), hip.aggexpr(hip.PH_A_AVG, [d]),
            hip.aggexpr(hip.PH_A_COUNT_STAR)]
    preds = [hip.pred(P, hip.PH_GE, hip.const(ptype, i=lo)), hip.pred(P, hip.PH_LE, hip.const(ptype, i=hi))]
    return hip.ScanPlan(ctx, t, preds, [K0, K1], aggs)


def want_signed(c, lo, hi, b, e_, s2, nk1=2):
    """lc_want with the second factor 100 + s2 t, in Python integers"""
    sl = slice(b, e_)
    p, q, e, d, t = (np.asarray(c[k][sl]).astype(np.int64) for k in ("p", "q", "e", "d", "t"))
    m = (p >= lo) & (p <= hi)
    slot = c["k0"][sl].astype(np.int64) * nk1 + c["k1"][sl].astype(np.int64)
    out = []
    for s in sorted(set(slot[m].tolist())):
        g = m & (slot == s)
        dp = e[g] * (100 - d[g])
        out.append((int(np.flatnonzero(g)[0]) + b, (s // nk1, s % nk1),
                    [exact_sum(q[g]), exact_sum(e[g]), exact_sum(dp), exact_sum(dp * (100 + s2 * t[g])), exact_sum(d[g])], int(g.sum())))
    return sorted(out)


def both_bodies(pl, monkeypatch, ranges, bins=True):
    """every range under the default and under PH_SCAN_HIST=0: the results of the former, after asserting which body ran and that both agree"""
    got = []
    for b, e in ranges:
        pl.run(b, e)
        assert pl.variant == "packed64" and pl.row_body == ("bins" if bins else "columns"), (b, e)
        got.append(lc_result(pl.fetch()))
    monkeypatch.setenv("PH_SCAN_HIST", "0")
    for (b, e), g in zip(ranges, got):
        assert pl.row_body == "columns"
        pl.run(b, e)
        assert lc_result(pl.fetch()) == g, (b, e)
    monkeypatch.delenv("PH_SCAN_HIST")
    return got


def cut_ranges(n):
    """row ranges that start and end one row before, at and after the boundaries of a lane's 2 rows, a load's 128, a wave's 1024 and the
    4096-row tile"""
    edges = sorted({b + k * m for m in (2, 128, 1024, TILE) for k in (1, 3) for b in (-1, 0, 1) if 0 <= b + k * m <= n})
    r = [(b, n) for b in edges] + [(0, e) for e in edges] + [(b, 2 * TILE + e) for b, e in zip(edges, edges) if 2 * TILE + e <= n]
    r += [(m - 1, m + 1) for m in (2, 128, 1024, TILE)] + [(m, m + 1) for m in (2, 128, 1024, TILE)]
    return r + [(0, n), (5, 5), (n - 1, n), (3 * TILE, n), (3 * TILE + 1, n - 1)]


def spread_slots(c):
    """all six slots, everywhere"""
    rng = np.random.default_rng(len(c["p"]) + 1)
    c["k0"] = rng.integers(0, 3, len(c["p"])).astype(np.uint8)
    c["k1"] = rng.integers(0, 2, len(c["p"])).astype(np.uint8)
    return c


# ---------------------------------------------------------------- range cuts

@pytest.mark.parametrize("s2", [1, -1], ids=["f2_100_plus_t", "f2_100_minus_t"])
def test_range_cuts_grids_and_signed_factors(ctx, monkeypatch, s2):
    """3 tiles + 5 rows, six slots, d and t around 100: f1 = 100 - d runs from 7 to -8 (B1c = -1 < 0, crossing zero) and f2 = 100 + t is
    positive or, with s2 = -1, 100 - t crosses zero too (B2c < 0); e of both signs"""
    n = 3 * TILE + 5
    c = spread_slots(lc_data(n, 11, 8036, 10561, q=(-20, 40), e=(-(2 ** 23) + 5, 2 ** 23), d=(93, 108), t=(93, 108)))
    ranges = cut_ranges(n)
    t = lc_table(ctx, c)
    t.pack_scan_group(COLS)
    lo, hi = 8036 + 300, 10561 - 300
    pl = plan_signed(ctx, t, lo, hi, c["ptype"], s2)
    assert pl.kind == "lowcard_chain"
    want = [want_signed(c, lo, hi, b, e, s2) for b, e in ranges]
    assert len(want[ranges.index((0, n))]) == 6
    for grid in (None, "1", "2"):
        if grid is not None:
            monkeypatch.setenv("PH_SCAN_GRID", grid)
        got = both_bodies(pl, monkeypatch, ranges)
        assert [sorted(g) for g in got] == want, grid
    pl.free()
    t.free()


# ---------------------------------------------------------------- field extremes

def test_field_extremes_first_and_last_bins(ctx, monkeypatch):
    """every field's span all ones (12, 6, 24, 4, 4 bits): row 0 holds code 0 of every field in slot 0 (the table's first bin), row 1 the
    maximum of every field in slot 5 (d = t = 15, the table's last bin); slot 2 sees only d = t = 15 with e at both ends, slot 3 only
    d = t = 0"""
    n = 2 * TILE + 77
    c = spread_slots(lc_data(n, 12, D0, D0 + 4095, q=(-13, 50), e=(-(2 ** 23), 2 ** 23 - 1), d=(0, 15), t=(0, 15)))
    c["k0"][0], c["k1"][0] = 0, 0
    c["k0"][1], c["k1"][1] = 2, 1
    s2 = (c["k0"] == 1) & (c["k1"] == 0)
    s3 = (c["k0"] == 1) & (c["k1"] == 1)
    c["d"][s2], c["t"][s2] = 15, 15
    c["e"][s2] = np.where(np.arange(n)[s2] % 2 == 0, 2 ** 23 - 1, -(2 ** 23))
    c["d"][s3], c["t"][s3] = 0, 0
    t = lc_table(ctx, c)
    t.pack_scan_group(COLS)
    for lo, hi in [(D0, D0 + 4095), (D0 + 4095, D0 + 4095), (D0, D0), (D0 + 1, D0 + 4094)]:
        pl = lc_plan(ctx, t, lo, hi, c["ptype"])
        ranges = [(0, n), (0, 2), (1, 2), (1, n), (2, n)]
        got = both_bodies(pl, monkeypatch, ranges)
        for (b, e), g in zip(ranges, got):
            assert sorted(g) == lc_want(c, lo, hi, b, e), (lo, hi, b, e)
        pl.free()
    t.free()


# ---------------------------------------------------------------- all rows in one bin, at the bound

@pytest.fixture(scope="module")
def one_bin():
    """1024 tiles, every row in bin (slot 5, d = t = 15) with p, q and e at their maximum codes, but the one row that pins the columns'
    minima: the last row of tile 1022, so that both lengths below have it in their last tile or the one before"""
    n = 1024 * TILE
    c = dict(p=np.full(n, 8036 + 4095, np.int32), q=np.full(n, 63, np.int32), e=np.full(n, 2 ** 24 - 1, np.int64), d=np.full(n, 15, np.int64),
             t=np.full(n, 15, np.int64), k0=np.full(n, 2, np.uint8), k1=np.full(n, 1, np.uint8), ptype=hip.PH_DATE)
    r = 1023 * TILE - 1
    c["p"][r], c["q"][r], c["e"][r], c["d"][r], c["t"][r], c["k0"][r], c["k1"][r] = 8036, 0, 0, 0, 0, 0, 0
    return c


def one_bin_want(c, n):
    """the two groups over rows [0, n), n beyond the pinning row, in closed form and Python integers"""
    m = n - 1
    big = (0, (2, 1), [63 * m, (2 ** 24 - 1) * m, (2 ** 24 - 1) * 85 * m, (2 ** 24 - 1) * 85 * 115 * m, 15 * m], m)
    return sorted([big, (1023 * TILE - 1, (0, 0), [0, 0, 0, 0, 0], 1)])


def test_one_bin_1023_tiles_in_one_workgroup(ctx, monkeypatch, one_bin):
    """PH_SCAN_GRID=1 over 1023 tiles: the bound of the bins' packed count and sum exactly, every lane of every row on one bin"""
    n = 1023 * TILE
    c = {k: (v[:n] if k != "ptype" else v) for k, v in one_bin.items()}
    t = lc_table(ctx, c)
    t.pack_scan_group(COLS)
    pl = lc_plan(ctx, t, 8036, 8036 + 4095, c["ptype"])
    monkeypatch.setenv("PH_SCAN_GRID", "1")
    got = both_bodies(pl, monkeypatch, [(0, n)])
    assert sorted(got[0]) == one_bin_want(c, n)
    pl.free()
    t.free()


def test_one_bin_one_tile_beyond_the_bound(ctx, monkeypatch, one_bin):
    """1024 tiles under PH_SCAN_GRID=1: more than a workgroup of the bins body may fold, so the run raises its grid or takes the columns;
    either way the result is the same"""
    c = one_bin
    n = len(c["p"])
    t = lc_table(ctx, c)
    t.pack_scan_group(COLS)
    pl = lc_plan(ctx, t, 8036, 8036 + 4095, c["ptype"])
    monkeypatch.setenv("PH_SCAN_GRID", "1")
    pl.run(0, n)
    assert pl.variant == "packed64" and pl.row_body in ("bins", "columns")
    got = lc_result(pl.fetch())
    assert sorted(got) == one_bin_want(c, n)
    monkeypatch.setenv("PH_SCAN_HIST", "0")
    pl.run(0, n)
    assert pl.row_body == "columns" and lc_result(pl.fetch()) == got
    pl.free()
    t.free()


# ---------------------------------------------------------------- failing and out-of-range rows

def test_failing_rows_empty_tiles_and_first_rows(ctx, monkeypatch):
    """tile 0: no row passes; tile 1: one row passes; tile 2: random; the last row of the table is the only passing row of slot (2, 1)"""
    n = 3 * TILE + 5
    c = lineitem_like(n, seed=13)
    lo, hi = 9000, 10000
    c["p"][:2 * TILE] = 8036 + (np.arange(2 * TILE) % 900)     # below lo (row 0 keeps the minimum)
    c["p"][1] = 10561                                         # the maximum, above hi
    c["p"][TILE + 1234] = 9500
    c["k0"][c["k0"] == 2] = 1                                  # slots (2, *) only where put below
    c["k0"][n - 1], c["k1"][n - 1], c["p"][n - 1] = 2, 1, 9999
    c["k0"][n - 2], c["k1"][n - 2], c["p"][n - 2] = 2, 0, 10001   # fails
    t = lc_table(ctx, c)
    t.pack_scan_group(COLS)
    pl = lc_plan(ctx, t, lo, hi, c["ptype"])
    ranges = [(0, TILE), (0, 2 * TILE), (TILE, 2 * TILE), (TILE + 1234, TILE + 1235), (TILE + 1235, 2 * TILE), (7, 7), (n, n), (0, 0),
              (0, n), (2 * TILE, n), (n - 1, n), (n - 2, n - 1), (0, n - 1)]
    for grid in (None, "1"):
        if grid is not None:
            monkeypatch.setenv("PH_SCAN_GRID", grid)
        got = both_bodies(pl, monkeypatch, ranges)
        for (b, e), g in zip(ranges, got):
            assert sorted(g) == lc_want(c, lo, hi, b, e), (b, e)
        by = dict(zip(ranges, got))
        assert by[(0, TILE)] == [] and by[(7, 7)] == [] and by[(n, n)] == [] and by[(TILE + 1235, 2 * TILE)] == []
        assert len(by[(TILE, 2 * TILE)]) == 1 and by[(TILE, 2 * TILE)][0][0] == TILE + 1234 and by[(TILE, 2 * TILE)][0][3] == 1
        last = [g for g in by[(0, n)] if g[1] == (2, 1)]
        assert len(last) == 1 and last[0][0] == n - 1 and last[0][3] == 1
        assert not [g for g in by[(0, n)] if g[1] == (2, 0)] and not [g for g in by[(0, n - 1)] if g[1][0] == 2]
    pl.free()
    t.free()


# ---------------------------------------------------------------- ineligible plans

def test_seven_slots_run_the_columns(ctx, monkeypatch):
    """seven slots (7 x 1 dictionaries) in lineitem's bit layout: more than the bins' tables hold"""
    n = 2 * TILE + 9
    c = lineitem_like(n, seed=14)
    c["k0"] = (np.arange(n) % 7).astype(np.uint8)
    c["k1"] = np.zeros(n, np.uint8)
    t = hip.Table(ctx, [(hip.PH_I32, c["q"]), (hip.PH_DEC64, c["e"], 2), (hip.PH_DEC64, c["d"], 2), (hip.PH_DEC64, c["t"], 2),
                        (hip.PH_CODE8, c["k0"], 0, None, list("abcdefg")), (hip.PH_CODE8, c["k1"], 0, None, ["x"]), (hip.PH_DATE, c["p"])], n)
    t.pack_scan_group(COLS)
    pl = lc_plan(ctx, t, 8500, 10000, c["ptype"])
    ranges = [(0, n), (3, n - 3)]
    got = both_bodies(pl, monkeypatch, ranges, bins=False)
    for (b, e), g in zip(ranges, got):
        assert len(g) == 7 and sorted(g) == want_signed(c, 8500, 10000, b, e, 1, nk1=1)
    pl.free()
    t.free()


def test_another_layout_runs_the_columns(ctx, monkeypatch):
    """8-bit d and t: not lineitem's layout, so (slot, t, d) are not the 11 bits the bins are named by"""
    c = full_fields()
    n = len(c["p"])
    t = lc_table(ctx, c)
    t.pack_scan_group(COLS)
    pl = lc_plan(ctx, t, D0 + 10, D0 + 3000, c["ptype"])
    got = both_bodies(pl, monkeypatch, [(0, n), (17, n - 1)], bins=False)
    assert sorted(got[0]) == lc_want(c, D0 + 10, D0 + 3000, 0, n) and sorted(got[1]) == lc_want(c, D0 + 10, D0 + 3000, 17, n - 1)
    pl.free()
    t.free()


def test_row_body_before_a_group_is_bound(ctx):
    c = lineitem_like()
    t = lc_table(ctx, c)
    pl = lc_plan(ctx, t, 8500, 10000, c["ptype"])
    pl.run()
    assert pl.variant == "narrow32_lean" and pl.row_body == "columns"
    t.pack_scan_group(COLS)
    pl.run()
    assert pl.variant == "packed64" and pl.row_body == "bins"
    assert sorted(lc_result(pl.fetch())) == lc_want(c, 8500, 10000, 0, len(c["p"]))
    pl.free()
    t.free()
