"""GPU tests of the merge launch of the fused scans (merge_partials_kernel, merge_partials_ops_kernel): a lane loads its words of the
workgroups' partials in batches of B = 8, all of a batch before the first add, and a word beyond the last workgroup contributes the
identity (DESIGN.md §4.1 "The merge issues a lane's loads together"). The number of workgroups is PH_SCAN_GRID, on both sides of one
lane's word (64), of one batch (64 B) and of two (128 B); the plans run the wide kernels (an int32 predicate column over the whole
int32 range has no narrowed copy), whose tiles are 1024 rows, so 64 * 2 B + 1 tiles are 1 049 600 rows.
The values make the merge carry: workgroup w works through tiles w, w + grid, ..., and every row of those tiles lies in one slot with
e of one sign, sized so that the workgroup's sum of e (1 - d)(1 + t) is near +-3e18, as large as the overflow proof admits (|row| x rows
per workgroup < 4e18). A slot's workgroups are two of one sign to one of the other, so the 128-bit total carries into the high word
(or borrows from it) once there are enough of them. Sums, counts and first rows are compared by equality with Python integers."""
import numpy as np
import pytest

from plan_amd import hip
from test_gpu_narrow_scan import D, E, I32_MAX, I32_MIN, K0, K1, P, Q, T, exact_sum, lc_plan, lc_result, lc_table, lc_want

pytestmark = pytest.mark.gpu

B = 8                                   # MERGE_BATCH: loads per lane and batch
WIDE_TILE = 1024
TILES = 64 * 2 * B + 1
N = TILES * WIDE_TILE
GRIDS = [1, 2, 63, 64, 65, 64 * B - 1, 64 * B, 64 * B + 1, 128 * B + 1]
P_LO, P_HI = 0, 1000


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    for k in ("PH_SCAN_GRID", "PH_SCAN_JIT", "PH_SCAN_TAIL"):
        monkeypatch.delenv(k, raising=False)


def columns(grid):
    """the table for a run at `grid` workgroups (see the module's docstring); rows 0 and 1 hold the int32 extremes of p and fail"""
    tiles_per_wg = (TILES + grid - 1) // grid
    m = int(3e18) // (10_000 * tiles_per_wg * WIDE_TILE)      # |e|: f1 = f2 = 100 at d = t = 0
    assert m * 10_000 * tiles_per_wg * WIDE_TILE < 4e18      # within the proof
    wg = (np.arange(N) // WIDE_TILE) % grid
    slot = np.minimum(5, wg * 6 // grid)
    minus = (wg % 3 == 2) ^ (slot % 2 == 1)
    rng = np.random.default_rng(grid)
    p = rng.integers(P_LO, P_HI, N, endpoint=True).astype(np.int32)
    p[0], p[1] = I32_MIN, I32_MAX
    return dict(p=p, q=rng.integers(-1000, 1000, N).astype(np.int32), e=np.where(minus, -m, m).astype(np.int64), d=np.zeros(N, np.int64),
                t=np.zeros(N, np.int64), k0=(slot // 2).astype(np.uint8), k1=(slot % 2).astype(np.uint8), ptype=hip.PH_I32), m, tiles_per_wg


@pytest.fixture(scope="module")
def tables(ctx):
    """grid -> (table, columns, |e|, tiles per workgroup, the Q1-shaped reference), built once for both tests"""
    made = {}

    def get(grid):
        if grid not in made:
            c, m, tpw = columns(grid)
            made[grid] = (lc_table(ctx, c), c, m, tpw, lc_want(c, P_LO, P_HI, 0, N))
        return made[grid]

    yield get
    for t, *_ in made.values():
        t.free()


@pytest.mark.parametrize("grid", GRIDS)
def test_q1_shape_merge_carries_and_borrows(ctx, monkeypatch, tables, grid):
    t, c, m, tpw, want = tables(grid)
    # what the data is for: a workgroup's partial of the largest sum is near +-3e18, both signs occur where there are three workgroups,
    # and the totals leave 64 bits from 64 B - 1 workgroups on
    partial = m * 10_000 * (tpw * WIDE_TILE - 2)
    assert 2.9e18 < partial < 2 ** 63
    ch = [g[2][3] for g in want]
    if grid >= 3:
        assert len(set(np.sign(c["e"][2:]).tolist())) == 2
    if grid >= 63:
        assert len(want) == 6
    if grid >= 64 * B - 1:      # a slot's net is a third of its 85 or more workgroups
        assert any(x >= 2 ** 64 for x in ch) and any(x <= -(2 ** 64) for x in ch)
    pl = lc_plan(ctx, t, P_LO, P_HI, c["ptype"])
    assert pl.kind == "lowcard_chain"
    monkeypatch.setenv("PH_SCAN_GRID", str(grid))
    pl.run()
    assert pl.variant == "wide" and pl.bytes_per_row == 34
    assert sorted(lc_result(pl.fetch())) == want          # fetched after one run: the merge published
    pl.run()
    pl.run()                                              # the run before was never fetched: the plain merge
    assert sorted(lc_result(pl.fetch())) == want
    pl.run()
    assert sorted(lc_result(pl.fetch())) == want          # and the publishing merge again
    pl.free()


def jit_want(c):
    """(first row, key, [Σe, Σe(1-d)(1+t), min q, max q, min e, max e], count) per group, in Python integers"""
    p, q, e, d, t = (c[k].astype(np.int64) for k in ("p", "q", "e", "d", "t"))
    m = (p >= P_LO) & (p <= P_HI)
    slot = c["k0"].astype(np.int64) * 2 + c["k1"]
    out = []
    for s in sorted(set(slot[m].tolist())):
        g = m & (slot == s)
        out.append((int(np.flatnonzero(g)[0]), (s // 2, s % 2),
                    [exact_sum(e[g]), exact_sum(e[g] * (100 - d[g]) * (100 + t[g])), int(q[g].min()), int(q[g].max()), int(e[g].min()), int(e[g].max())],
                    int(g.sum())))
    return sorted(out)


@pytest.mark.parametrize("grid", GRIDS)
def test_generated_plan_sum_min_max(ctx, monkeypatch, tables, grid):
    """a generated kernel's words merge by operation (merge_partials_ops_kernel): 128-bit sums, signed minima and maxima, first rows"""
    t, c, _, _, _ = tables(grid)
    e, d, tt, one = hip.X_COL(E), hip.X_COL(D), hip.X_COL(T), hip.X_CONST(1, 0)
    aggs = [hip.aggexpr(hip.PH_A_SUM, [e]), hip.aggexpr(hip.PH_A_SUM, [e, one, d, hip.X_SUB, hip.X_MUL, one, tt, hip.X_ADD, hip.X_MUL]),
            hip.aggexpr(hip.PH_A_MIN, [hip.X_COL(Q)]), hip.aggexpr(hip.PH_A_MAX, [hip.X_COL(Q)]), hip.aggexpr(hip.PH_A_MIN, [e]),
            hip.aggexpr(hip.PH_A_MAX, [e]), hip.aggexpr(hip.PH_A_COUNT_STAR)]
    preds = [hip.pred(P, hip.PH_GE, hip.const(hip.PH_I32, i=P_LO)), hip.pred(P, hip.PH_LE, hip.const(hip.PH_I32, i=P_HI))]
    pl = hip.ScanPlan(ctx, t, preds, [K0, K1], aggs)
    assert pl.kind == "jit"
    want = jit_want(c)
    monkeypatch.setenv("PH_SCAN_GRID", str(grid))

    def result():
        r = pl.fetch()
        return sorted((int(r["first_row"][g]), tuple(int(k) for k in r["keys"][g]), [int(x) for x in r["sum"][g][:6]], int(r["count"][g][6]))
                      for g in range(r["ngroups"]))

    pl.run()
    assert result() == want
    pl.run()
    pl.run()
    assert result() == want
    pl.free()

