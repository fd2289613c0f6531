"""GPU tests of the lean instance of the narrow lowcard_chain scan (ph_scan_plan_variant == "narrow32_lean"): factors folded
into the code domain, slot addresses in 32 bits, interior tiles without the row-range test, register buffers that swap roles; and of
ph_scan_plan_run over any row_begin for both narrow scans (filter_sumprod keeps its fixed-width instance, "narrow32"). Every case is checked against Python integers / numpy exact sums (the helpers of test_gpu_narrow_scan.py), asserts the variant the
plan took, and is compared bit for bit with the same case run in a child process under PH_SCAN_LEAN=0 (the kernels from before the lean
instances; the switch is read once per process).

The multiplies themselves are not narrowed to 24 bits: on gfx950 v_mul_lo_u32 issues at the rate of v_mul_u32_u24 (profiles/
int_issue_gfx950.txt), so there is no 24-bit product form and no operand-range proof to bind here. What selects the lean instance is
FORM_NARROW32 (|e|, |f1|, |f2|, |e f1| < 2^31, bound on both sides below), the code widths of TPC-H lineitem, and |B| < 2^23 of the factors
(reached from both sides through the scale of the literal in `1 - d`)."""
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
from test_gpu_narrow_scan import E, D, K0, K1, P, Q, T, exact_sum, lc_plan, lc_result, lc_table, lc_want  # noqa: E402,F401

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
TILE = 4096
N = 5 * TILE + 7
D0 = tpchgen.days(1994, 1, 1)
LONE_SLOT, LONE_ROW = (2, 1), 5000      # a slot used by a single row
LAST_SLOT = (2, 0)                      # a slot used only in the last, partial tile
SLOT_11_SHIFT = 1200                    # rows of slot (1, 1) have their dates shifted: one interval passes that slot alone


def ranges(n):
    """the row ranges of the issue: tile-aligned, off by one on either side of a tile and of a lane's 16 rows, empty, one row, inside one lane"""
    return [(0, n), (1, n), (15, n - 1), (16, TILE), (17, TILE + 1), (TILE - 1, TILE + 1), (TILE, 2 * TILE), (TILE + 5, 3 * TILE + 9),
            (8, 8), (TILE + 1, TILE + 2), (TILE + 18, TILE + 27)]


def tile_columns(n=N, seed=3):
    """the code widths of TPC-H Q1 (p 2, q 1, e 4, d 1, t 1), all six slots in use; every column's min and max pinned in rows 0 and 1"""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    k0 = rng.integers(0, 2, n).astype(np.uint8)
    k1 = rng.integers(0, 2, n).astype(np.uint8)
    k0[LONE_ROW], k1[LONE_ROW] = LONE_SLOT
    k0[[n - 3, n - 1]], k1[[n - 3, n - 1]] = LAST_SLOT
    p = D0 + (i & 1) * 600 + i % 7 + SLOT_11_SHIFT * ((k0 == 1) & (k1 == 1))

    def col(lo, hi):
        v = rng.integers(lo, hi, n, endpoint=True, dtype=np.int64)
        v[0], v[1] = lo, hi
        return v

    return dict(p=p.astype(np.int32), q=col(1, 50).astype(np.int32), e=col(90_000, 10_500_000), d=col(0, 10), t=col(0, 8), k0=k0, k1=k1,
                ptype=hip.PH_DATE)


# every row, no row (an interval below the column: the code range is empty), alternate rows (even rows outside slot (1, 1)), one slot
INTERVALS = [(I32_MIN, I32_MAX), (D0 - 10, D0 - 1), (D0, D0 + 100), (D0 + SLOT_11_SHIFT, D0 + 3000)]


def run_lowcard(ctx, c, intervals, row_ranges, grids=("2", None)):
    """[variant, [[grid, lo, hi, b, e, groups]...]]: every (grid, interval, range) of one table, each checked against numpy"""
    t = lc_table(ctx, c)
    out, variant = [], None
    for lo, hi in intervals:
        pl = lc_plan(ctx, t, lo, hi, c["ptype"])
        assert pl.kind == "lowcard_chain"
        variant = pl.variant
        for grid in grids:   # PH_SCAN_GRID is read at every run: 2 workgroups loop over several tiles, the default grid has one tile each
            if grid is None:
                os.environ.pop("PH_SCAN_GRID", None)
            else:
                os.environ["PH_SCAN_GRID"] = grid
            for b, e_ in row_ranges:
                pl.run(b, e_)
                got = lc_result(pl.fetch())
                want = lc_want(c, lo, hi, b, e_)
                assert [g[1:] for g in got] == [(w[1], w[2], w[3]) for w in want], (grid, lo, hi, b, e_)
                assert [g[0] for g in got] == [w[0] for w in want], (grid, lo, hi, b, e_)
                out.append([grid, lo, hi, b, e_, got])
        os.environ.pop("PH_SCAN_GRID", None)
        pl.free()
    t.free()
    return [variant, out]


# ---------------------------------------------------------------- filter_sumprod over the same table (Q6's widths: p 2, q 1, d 1, e 4)
def fs_plan(ctx, t, lo, hi, every_d=False):
    dlo, dhi = (-1e30, 1e30) if every_d else (0.015, 0.085)
    preds = [hip.pred(P, hip.PH_GE, hip.const(hip.PH_DATE, i=lo)), hip.pred(P, hip.PH_LE, hip.const(hip.PH_DATE, i=hi)),
             hip.pred(D, hip.PH_GE, hip.const(hip.PH_F32, f=dlo)), hip.pred(D, hip.PH_LE, hip.const(hip.PH_F32, f=dhi)),
             hip.pred(Q, hip.PH_LT, hip.const(hip.PH_I32, i=40))]
    aggs = [hip.aggexpr(hip.PH_A_SUM, [hip.X_COL(E), hip.X_COL(D), hip.X_MUL]), hip.aggexpr(hip.PH_A_COUNT_STAR)]
    return hip.ScanPlan(ctx, t, preds, [], aggs)


def fs_want(c, lo, hi, b, e_, every_d=False):
    sl = slice(b, e_)
    p, q, e, d = (np.asarray(c[k][sl]).astype(np.int64) for k in ("p", "q", "e", "d"))
    m = (p >= lo) & (p <= hi) & (q < 40)
    if not every_d:
        m &= (d >= 2) & (d <= 8)
    return [sum(int(x) * int(y) for x, y in zip(e[m], d[m])), int(m.sum())]


def run_fs(ctx, c, intervals, row_ranges, grids=("2", None), every_d=False):
    t = lc_table(ctx, c)
    out, variant = [], None
    for lo, hi in intervals:
        pl = fs_plan(ctx, t, lo, hi, every_d)
        assert pl.kind == "filter_sumprod"
        variant = pl.variant
        for grid in grids:
            if grid is None:
                os.environ.pop("PH_SCAN_GRID", None)
            else:
                os.environ["PH_SCAN_GRID"] = grid
            for b, e_ in row_ranges:
                pl.run(b, e_)
                r = pl.fetch()
                got = [int(r["sum"][0][0]), int(r["count"][0][1])] if r["ngroups"] else [0, 0]
                assert got == fs_want(c, lo, hi, b, e_, every_d), (grid, lo, hi, b, e_)
                out.append([grid, lo, hi, b, e_, got])
        os.environ.pop("PH_SCAN_GRID", None)
        pl.free()
    t.free()
    return [variant, out]


# ---------------------------------------------------------------- what admits the lean instance, both sides
def form_columns(n=TILE, seed=5, e=(90_000, 10_500_000), d=(0, 10), t=(0, 8), q=(1, 50)):
    """2^12 rows; every column's min in row 0, its max in row 1, and the row of the largest |e f1| (max |e| with min d) in row 2"""
    rng = np.random.default_rng(seed)

    def col(lo, hi):
        v = rng.integers(lo, hi, n, endpoint=True, dtype=np.int64)
        v[0], v[1] = lo, hi
        return v

    c = dict(p=(D0 + np.arange(n) % 300).astype(np.int32), q=col(*q).astype(np.int32), e=col(*e), d=col(*d), t=col(*t),
             k0=rng.integers(0, 3, n).astype(np.uint8), k1=rng.integers(0, 2, n).astype(np.uint8), ptype=hip.PH_DATE)
    c["e"][2] = e[1] if abs(e[1]) >= abs(e[0]) else e[0]
    c["d"][2] = d[0]
    return c


E_EDGE = (2 ** 31 - 1) // 355   # the largest e with e (100 - d) <= 2^31 - 1 at d = -255


def form_cases():
    """(name, columns, variant expected by default). The bounds are data properties, checked here on the CPU before any launch."""
    cases = []
    c = form_columns(e=(E_EDGE - 70_000, E_EDGE), d=(-255, 0))
    assert int(c["e"].max()) * (100 - int(c["d"].min())) <= I32_MAX
    cases.append(("ef1_at_2_31_below", c, "narrow32_lean"))
    c = form_columns(e=(E_EDGE - 70_000, E_EDGE + 1), d=(-255, 0))
    assert int(c["e"].max()) * (100 - int(c["d"].min())) > I32_MAX
    cases.append(("ef1_at_2_31_above", c, "narrow64"))
    # 46 341 x 46 340, the edge of the existing 32-bit proof: f1 = 46 340 needs a two-byte discount range (the run-time-width instance)
    c = form_columns(e=(-30_000, 46_341), d=(100 - 46_340, 100 - 46_340 + 300))
    assert 46_341 * 46_340 <= I32_MAX < 46_341 * 46_341
    cases.append(("ef1_46341_46340", c, "narrow_rt"))
    c = form_columns(e=(-30_000, 46_341), d=(100 - 46_341, 100 - 46_341 + 300))
    cases.append(("ef1_46341_46341", c, "narrow64"))
    # e, f1 = 100 - d and f2 = 100 + t of both signs: sign extension of the 32-bit product, signed multiply-adds on the codes
    c = form_columns(e=(-5_000_000, 5_000_000), d=(-55, 200), t=(-200, 55), q=(-100, 100))
    cases.append(("both_signs", c, "narrow32_lean"))
    # a discount column whose codes need four bytes, maximum code >= 2^24: not the fixed widths
    c = form_columns(e=(-40, 100), d=(-(2 ** 24) - 5, 10))
    assert int(c["d"].max() - c["d"].min()) >= 2 ** 24
    cases.append(("d_codes_4_bytes", c, "narrow_rt"))
    # four-byte codes of 2^31 and above: base + code is an addition modulo 2^32 (f1 in [-1, 1] keeps |e f1| < 2^31)
    c = form_columns(e=(-(2 ** 30) - 1, 2 ** 30), d=(99, 101))
    assert int(c["e"].max() - c["e"].min()) >= 2 ** 31
    cases.append(("e_codes_from_2_31", c, "narrow32_lean"))
    # one-byte extendedprice: not the fixed widths
    cases.append(("e_codes_1_byte", form_columns(e=(1000, 1255)), "narrow_rt"))
    return cases


def fs_form_cases():
    """the same ladder for a b of filter_sumprod (a = e, b = d; every discount passes): (name, columns, variant expected by default)"""
    cases = []
    for name, e, want in (("a_at_2_31_below", (2 ** 31 - 70_001, 2 ** 31 - 1), "narrow32_lean"), ("a_at_2_31_above", (2 ** 31 - 70_000, 2 ** 31), "narrow64"),
                          ("a_at_minus_2_31_below", (-(2 ** 31) + 1, -(2 ** 31) + 70_001), "narrow32_lean"),
                          ("a_at_minus_2_31_above", (-(2 ** 31), -(2 ** 31) + 70_000), "narrow64")):
        c = form_columns(e=e, d=(-128, 127))
        assert (max(abs(int(c["e"].min())), abs(int(c["e"].max()))) <= I32_MAX) == (want == "narrow32_lean")
        cases.append((name, c, want))
    # a and b of both signs: negative bases, the signed add on the code, the sign-extending 32 x 32 -> 64 multiply
    cases.append(("both_signs", form_columns(e=(-5_000_000, 5_000_000), d=(-55, 200)), "narrow32_lean"))
    c = form_columns(e=(-(2 ** 30) - 1, 2 ** 30), d=(-128, 127))
    assert int(c["e"].max() - c["e"].min()) >= 2 ** 31
    cases.append(("a_codes_from_2_31", c, "narrow32_lean"))
    # b beyond 32 bits: 64-bit products; two-byte discount codes: not the fixed widths
    cases.append(("b_wide", form_columns(e=(0, 70_000), d=(2 ** 31, 2 ** 31 + 200)), "narrow64"))
    cases.append(("b_codes_2_bytes", form_columns(e=(-70_000, 70_000), d=(-300, 300)), "narrow_rt"))
    return cases


# |B| < 2^23 of a factor (the only condition the lean instance adds): `1 - d` with the literal at scale 8 against a discount at scale 2
# gives B = -10^6, at scale 9 B = -10^7 >= 2^23. |e f1| < 2^31 with four-byte e then leaves room for no discount but the one with f1 = 0.
def scaled_plan(ctx, t, scale):
    e, d, tt = hip.X_COL(E), hip.X_COL(D), hip.X_COL(T)
    one = hip.X_CONST(10 ** (scale - 2) * 100, scale)
    dp = [e, one, d, hip.X_SUB, hip.X_MUL]
    aggs = [hip.aggexpr(hip.PH_A_SUM, [hip.X_COL(Q)]), hip.aggexpr(hip.PH_A_SUM, [e]), hip.aggexpr(hip.PH_A_SUM, dp),
            hip.aggexpr(hip.PH_A_SUM, dp + [hip.X_CONST(1, 0), tt, hip.X_ADD, hip.X_MUL]), hip.aggexpr(hip.PH_A_AVG, [d]), hip.aggexpr(hip.PH_A_COUNT_STAR)]
    preds = [hip.pred(P, hip.PH_GE, hip.const(hip.PH_DATE, i=I32_MIN)), hip.pred(P, hip.PH_LE, hip.const(hip.PH_DATE, i=I32_MAX))]
    return hip.ScanPlan(ctx, t, preds, [K0, K1], aggs)


def run_scaled(ctx):
    c = form_columns(d=(100, 100))
    n = len(c["p"])
    t = lc_table(ctx, c)
    out = {}
    for scale in (8, 9):
        pl = scaled_plan(ctx, t, scale)
        assert pl.kind == "lowcard_chain"
        pl.run(0, n)
        got = lc_result(pl.fetch())
        want = lc_want(c, I32_MIN, I32_MAX, 0, n)   # e (1 - d) = 0 at every scale of the literal
        assert [g[1:] for g in got] == [(w[1], w[2], w[3]) for w in want] and all(w[2][2] == 0 for w in want)
        out[str(scale)] = [pl.variant, got]
        pl.free()
    t.free()
    return out


# ---------------------------------------------------------------- bases as far from zero as the lean instance admits, across ranks
def code_sum_cases():
    """bases as far from zero as FORM_NARROW32 and the fixed widths admit (|e| < 2^31 with 4-byte codes; |e f1| < 2^31 then bounds f1)"""
    n = 3 * TILE + 11
    return [("neg_bases", form_columns(n, 7, e=(-(2 ** 31) + 1, -(2 ** 31) + 70_001), d=(99, 101), t=(-108, 100), q=(-(2 ** 31), -(2 ** 31) + 255))),
            ("pos_bases", form_columns(n, 8, e=(2 ** 31 - 70_001, 2 ** 31 - 1), d=(99, 101), t=(-100, 155), q=(2 ** 31 - 256, 2 ** 31 - 1))),
            ("neg_d_base", form_columns(n, 9, e=(-35_000, 36_000), d=(-30_000, -29_745), t=(0, 8), q=(-3, 252)))]


def run_code_sums(ctx):
    out = {}
    for name, c in code_sum_cases():
        n = len(c["p"])
        res = run_lowcard(ctx, c, [(I32_MIN, I32_MAX), (D0 + 10, D0 + 200)], [(0, n), (5, n - 2), (TILE - 3, 2 * TILE + 1)])
        # three row ranges as three ranks through the 128-bit merge of the raw partial words
        t = lc_table(ctx, c)
        pl = lc_plan(ctx, t, I32_MIN, I32_MAX, c["ptype"])
        cuts, words = [0, TILE + 3, 2 * TILE + 5, n], []
        for b, e_ in zip(cuts[:-1], cuts[1:]):
            pl.run(b, e_)
            ptr, nw = pl.partials_dev()
            words.append(ctx.download(hip.vp(ptr), np.uint64, nw))
        merged = lc_result(pl.fetch_merged(np.concatenate(words), 3))
        want = lc_want(c, I32_MIN, I32_MAX, 0, n)
        # first rows of a merged result carry the rank in their upper bits: groups compare by key here
        assert sorted(g[1:] for g in merged) == sorted((w[1], w[2], w[3]) for w in want), name
        pl.free()
        t.free()
        out[name] = res + [sorted(g[1:] for g in merged)]
    return out


def run_all(ctx):
    c = tile_columns()
    out = {"tiles_lc": run_lowcard(ctx, c, INTERVALS, ranges(N)), "tiles_fs": run_fs(ctx, c, INTERVALS, ranges(N))}
    for name, cols, _ in form_cases():
        n = len(cols["p"])
        out["form_" + name] = run_lowcard(ctx, cols, [(I32_MIN, I32_MAX)], [(0, n), (3, n - 1)])
    for name, cols, _ in fs_form_cases():
        n = len(cols["p"])
        out["fsform_" + name] = run_fs(ctx, cols, [(I32_MIN, I32_MAX)], [(0, n), (3, n - 1)], every_d=True)
    out["scaled"] = run_scaled(ctx)
    out["code_sums"] = run_code_sums(ctx)
    return out


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lean(ctx):
    return json.loads(json.dumps(run_all(ctx)))


@pytest.fixture(scope="module")
def parent():
    """PH_SCAN_LEAN=0: every case of this file in a fresh child process (the switch is read once per process)"""
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"lean_child_{os.getpid()}.json")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, PH_SCAN_LEAN="0"), check=True, timeout=600)
    with open(out) as f:
        res = json.load(f)
    os.remove(out)
    return res


def test_tile_paths_lowcard_chain(lean, parent):
    """interior and masked tiles in one launch (grid 2), one tile per workgroup (default grid); sums, counts and first row ids"""
    assert lean["tiles_lc"][0] == "narrow32_lean" and parent["tiles_lc"][0] == "narrow32"
    assert lean["tiles_lc"][1] == parent["tiles_lc"][1]
    everything = [r for r in lean["tiles_lc"][1] if r[1] == I32_MIN and r[3:5] == [0, N]]
    assert all(len(r[5]) == 6 for r in everything)   # all six slots in use
    assert all([g for g in r[5] if tuple(g[1]) == LONE_SLOT][0][3] == 1 for r in everything)
    assert all([g for g in r[5] if tuple(g[1]) == LAST_SLOT][0][0] == N - 3 for r in everything)


def test_tile_paths_filter_sumprod(lean, parent):
    assert lean["tiles_fs"][0] == "narrow32" and parent["tiles_fs"][0] == "narrow32"   # filter_sumprod has no lean instance
    assert lean["tiles_fs"][1] == parent["tiles_fs"][1]
    assert any(r[5][1] > 0 for r in lean["tiles_fs"][1])


@pytest.mark.parametrize("name,want", [(n, v) for n, _, v in form_cases()])
def test_lean_admission_both_sides(lean, parent, name, want):
    got, old = lean["form_" + name], parent["form_" + name]
    assert got[0] == want
    assert old[0] == ("narrow32" if want == "narrow32_lean" else want)
    assert got[1] == old[1]


@pytest.mark.parametrize("name,want", [(n, v) for n, _, v in fs_form_cases()])
def test_lean_admission_filter_sumprod(lean, parent, name, want):
    got, old = lean["fsform_" + name], parent["fsform_" + name]
    want = "narrow32" if want == "narrow32_lean" else want   # filter_sumprod has no lean instance: the fixed-width one on both sides
    assert got[0] == want and old[0] == want
    assert got[1] == old[1] and any(r[5][1] > 0 for r in got[1])


def test_factor_multiplier_bound(lean, parent):
    assert [lean["scaled"][s][0] for s in ("8", "9")] == ["narrow32_lean", "narrow32"]
    assert [parent["scaled"][s][0] for s in ("8", "9")] == ["narrow32", "narrow32"]
    assert lean["scaled"]["8"][1] == parent["scaled"]["8"][1] and lean["scaled"]["9"][1] == parent["scaled"]["9"][1]


def test_code_sums_with_large_bases(lean, parent):
    for name, _ in code_sum_cases():
        assert lean["code_sums"][name][0] == "narrow32_lean" and parent["code_sums"][name][0] == "narrow32", name
        assert lean["code_sums"][name][1:] == parent["code_sums"][name][1:], name


if __name__ == "__main__":   # the parent fixture's child: every case under another environment
    _ctx = hip.Ctx(0)
    _res = run_all(_ctx)
    _ctx.close()
    with open(sys.argv[1], "w") as _f:
        json.dump(_res, _f)
