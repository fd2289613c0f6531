"""The fused scans where their integer-domain arguments bind ("What pins the proof"): the overflow proof of
ph_scan_plan_run at its admission edge, the 128-bit merge of the workgroup partials with totals beyond 2^63, and the boundaries of the
32-bit multiply form over narrowed copies. The contract asserted everywhere: a run either returns exactly what Python integers give
(domain_edges.py) for every accumulator, count and first row of every group, or it raises PH_EOVERFLOW — never another number.

Forms: lowcard_chain and filter_sumprod over narrowed copies in the 32-bit form ("n32", lineitem's width tuple: the kernel instance
with compile-time widths), in the 64-bit form ("n64") and over a table whose predicate column has no copy ("wide": the wide kernels), a
hiprtc-generated plan ("jit") and the same plan under PH_SCAN_JIT=0 ("generic": the operator chain, which has no proof and detects
overflow per row). Child processes repeat the narrow cases under PH_NARROW=0 and PH_SCAN_NARROW_GENERIC=1 (read once per process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import domain_edges as DE  # noqa: E402
from domain_edges import D, E, FS_A, FS_B, FS_P, FS_Q, K0, K1, N_LADDER, P, P_HI, P_LO, Q, T  # noqa: E402
from plan_amd import hip  # noqa: E402

pytestmark = pytest.mark.gpu

LC_BYTES = {"n32": 11, "n64": 8, "wide": 34}    # bytes per row the kernel reads: which kernel family a ladder table got
FS_BYTES = {"n32": 8, "n64": 5, "wide": 24}


# ------------------------------------------------------------------ tables, plans, results

def lc_table(ctx, c):
    return hip.Table(ctx, [(hip.PH_I32, c["q"]), (hip.PH_DEC64, c["e"], 2), (hip.PH_DEC64, c["d"], 2), (hip.PH_DEC64, c["t"], 2),
                           (hip.PH_CODE8, c["k0"], 0, None, ["a", "b", "c"]), (hip.PH_CODE8, c["k1"], 0, None, ["x", "y"]),
                           (hip.PH_DATE, c["p"])], len(c["p"]))


def fs_table(ctx, c):
    return hip.Table(ctx, [(hip.PH_DATE, c["p"]), (hip.PH_I32, c["q"]), (hip.PH_DEC64, c["a"], 2), (hip.PH_DEC64, c["b"], 2)], len(c["p"]))


def p_preds(col, lo, hi):
    return [hip.pred(col, hip.PH_GE, hip.const(hip.PH_DATE, i=lo)), hip.pred(col, hip.PH_LE, hip.const(hip.PH_DATE, i=hi))]


def factors(consts):
    """f1 = A1 - d and f2 = A2 + t as programs (constants at the columns' scale 2, so A is taken as it is)"""
    A1, B1, A2, B2 = consts
    assert (B1, B2) == (-1, 1)
    return [hip.X_CONST(A1, 2), hip.X_COL(D), hip.X_SUB], [hip.X_CONST(A2, 2), hip.X_COL(T), hip.X_ADD]


def lc_plan(ctx, t, consts, lo=P_LO, hi=P_HI):
    f1, f2 = factors(consts)
    dp = [hip.X_COL(E)] + f1 + [hip.X_MUL]
    aggs = [hip.aggexpr(hip.PH_A_SUM, [hip.X_COL(Q)]), hip.aggexpr(hip.PH_A_SUM, [hip.X_COL(E)]), hip.aggexpr(hip.PH_A_SUM, dp),
            hip.aggexpr(hip.PH_A_SUM, dp + f2 + [hip.X_MUL]), hip.aggexpr(hip.PH_A_AVG, [hip.X_COL(D)]), hip.aggexpr(hip.PH_A_COUNT_STAR)]
    pl = hip.ScanPlan(ctx, t, p_preds(P, lo, hi), [K0, K1], aggs)
    assert pl.kind == "lowcard_chain"
    return pl


def jit_plan(ctx, t, consts, lo=P_LO, hi=P_HI):
    """a three-factor product, a plain sum, a MIN and a MAX: outside both precompiled shapes"""
    f1, f2 = factors(consts)
    aggs = [hip.aggexpr(hip.PH_A_SUM, [hip.X_COL(E)] + f1 + [hip.X_MUL] + f2 + [hip.X_MUL]), hip.aggexpr(hip.PH_A_SUM, [hip.X_COL(E)]),
            hip.aggexpr(hip.PH_A_MIN, [hip.X_COL(E)]), hip.aggexpr(hip.PH_A_MAX, [hip.X_COL(D)]), hip.aggexpr(hip.PH_A_COUNT_STAR)]
    return hip.ScanPlan(ctx, t, p_preds(P, lo, hi), [K0, K1], aggs)


def fs_plan(ctx, t, lo=P_LO, hi=P_HI):
    aggs = [hip.aggexpr(hip.PH_A_SUM, [hip.X_COL(FS_A), hip.X_COL(FS_B), hip.X_MUL]), hip.aggexpr(hip.PH_A_COUNT_STAR)]
    pl = hip.ScanPlan(ctx, t, p_preds(FS_P, lo, hi) + [hip.pred(FS_Q, hip.PH_LT, hip.const(hip.PH_I32, i=100))], [], aggs)
    assert pl.kind == "filter_sumprod"
    return pl


def grouped(r, nsum, cnt_idx):
    """[[first_row, [k0, k1], sums, count]] by first row; a fused plan returns its groups in that order already"""
    out = [[int(r["first_row"][g]), [int(k) for k in r["keys"][g]], [int(x) for x in r["sum"][g][:nsum]], int(r["count"][g][cnt_idx])]
           for g in range(r["ngroups"])]
    return sorted(out)


def lc_result(r):
    assert [int(x) for x in r["first_row"]] == sorted(int(x) for x in r["first_row"])
    return grouped(r, 5, 5)


def jit_result(r):
    return grouped(r, 4, 4)


def fs_result(r):
    return [int(r["sum"][0][0]), int(r["count"][0][1])] if r["ngroups"] else None


def admitted(pl, b, e):
    """runs [b, e): False when the library refuses it with PH_EOVERFLOW"""
    try:
        pl.run(b, e)
        return True
    except hip.PlanHipError as ex:
        if ex.code != hip.PH_EOVERFLOW:
            raise
        return False


def run_or_refuse(pl, b, e, result):
    """the run's result, or None when the library refuses it with PH_EOVERFLOW (at the run, or at the fetch of a generic plan)"""
    try:
        pl.run(b, e)
        return result(pl.fetch())
    except hip.PlanHipError as ex:
        if ex.code != hip.PH_EOVERFLOW:
            raise
        return None


class Tables:
    """device tables and their RowKinds, built once per process and shared by the cases"""

    def __init__(self, ctx):
        self.ctx, self.t = ctx, {}

    def get(self, key, columns, make):
        if key not in self.t:
            c = columns()
            self.t[key] = (make(self.ctx, c), c, DE.RowKinds(c))
        return self.t[key]

    def lc_ladder(self, form, n=N_LADDER):
        return self.get(("lc", form, n), lambda: DE.lc_ladder_columns(form, n), lc_table)

    def drop(self, key):
        self.t.pop(key)[0].free()

    def free(self):
        for t, _, _ in self.t.values():
            t.free()
        self.t = {}


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tabs(ctx):
    t = Tables(ctx)
    yield t
    t.free()


# ------------------------------------------------------------------ A.1 the magnitude ladder

def lc_ladder(tabs, form, sign, plan=lc_plan, result=lc_result, reference=DE.lc_reference, check=True, want_bytes=None):
    """[[k, sign, bytes per row, result or None]] of one form's ladder; every admitted step is compared with Python"""
    t, c, kinds = tabs.lc_ladder(form)
    out = []
    for k, consts, _ in DE.lc_ladder_steps(c, sign):
        pl = plan(tabs.ctx, t, consts)
        if want_bytes is not None:
            assert pl.bytes_per_row == want_bytes, (form, pl.bytes_per_row)
        res = run_or_refuse(pl, 0, len(c["p"]), result)
        if check and res is not None:
            assert res == reference(kinds.runs(0, len(c["p"])), P_LO, P_HI, *consts), (form, sign, k)
        out.append([k, sign, pl.bytes_per_row, res])
        pl.free()
    return out


def fs_ladder(tabs, form, sign, check=True, want_bytes=None):
    shared = DE.fs_ladder_shared(form)
    n = len(shared["p"])
    kinds = DE.RowKinds(dict(shared, row0=(np.arange(n) == 0)))
    out = []
    for k, b, b0, _ in DE.fs_ladder_steps(shared, sign):
        c = DE.fs_columns(shared, b, b0)
        t = fs_table(tabs.ctx, c)
        pl = fs_plan(tabs.ctx, t)
        if want_bytes is not None:
            assert pl.bytes_per_row == want_bytes, (form, pl.bytes_per_row)
        res = run_or_refuse(pl, 0, n, fs_result)
        if check and res is not None:
            assert res == DE.fs_reference(kinds.extend("b", c["b"]).runs(0, n), P_LO, P_HI, 100), (form, sign, k)
        out.append([k, sign, pl.bytes_per_row, res])
        pl.free()
        t.free()
    return out


def ladder_conditions(name, steps, bounds_products, total_of):
    """domain_edges.check_ladder over a ladder's results; prints what was admitted. steps: lc_ladder / fs_ladder output"""
    rows = [(s[0], bp[0], bp[1], None if s[3] is None else total_of(s[3])) for s, bp in zip(steps, bounds_products)]
    adm, ref, big = DE.check_ladder(name, rows, N_LADDER)
    print(f"ladder {name}: admitted 2^{adm}, refused 2^{ref}, admitted with |total| >= 2^63: 2^{big}")
    assert len(big) >= 2, f"{name}: fewer than two admitted steps carry the 128-bit merge past 2^63: {big}"
    return adm, ref, big


def lc_bounds_products(c, sign):
    return [(DE.lc_row_bound(c, *consts), prod) for _, consts, prod in DE.lc_ladder_steps(c, sign)]


def lc_total(res):
    return sum(g[2][3] for g in res)


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("form", DE.FORMS)
def test_lowcard_chain_ladder(tabs, form, sign):
    steps = lc_ladder(tabs, form, sign, want_bytes=LC_BYTES[form])
    c = tabs.lc_ladder(form)[1]
    ladder_conditions(f"lowcard_chain {form} {sign:+d}", steps, lc_bounds_products(c, sign), lc_total)


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("form", DE.FORMS)
def test_filter_sumprod_ladder(tabs, form, sign):
    steps = fs_ladder(tabs, form, sign, want_bytes=FS_BYTES[form])
    shared = DE.fs_ladder_shared(form)
    bp = [(DE.fs_row_bound(DE.fs_columns(shared, b, b0)), prod) for _, b, b0, prod in DE.fs_ladder_steps(shared, sign)]
    ladder_conditions(f"filter_sumprod {form} {sign:+d}", steps, bp, lambda r: r[0])


def jit_bounds_products(c, sign):
    """the generated plan's bound: the product of its sum's factor bounds (MIN / MAX accumulators are not sums)"""
    out = []
    for _, (A1, B1, A2, B2), prod in DE.lc_ladder_steps(c, sign):
        b = DE.affine_bound(0, 1, DE.col_range(c["e"])) * DE.affine_bound(A1, B1, DE.col_range(c["d"])) * DE.affine_bound(A2, B2, DE.col_range(c["t"]))
        out.append((b, prod))
    return out


@pytest.mark.parametrize("sign", [1, -1])
def test_generated_plan_ladder(tabs, sign):
    def plan(ctx, t, consts):
        pl = jit_plan(ctx, t, consts)
        assert pl.kind == "jit", hip.last_error()
        return pl
    steps = lc_ladder(tabs, "n32", sign, plan=plan, result=jit_result, reference=DE.jit_reference)
    ladder_conditions(f"jit {sign:+d}", steps, jit_bounds_products(tabs.lc_ladder("n32")[1], sign), lambda res: sum(g[2][0] for g in res))


@pytest.mark.parametrize("sign", [1, -1])
def test_generic_plan_ladder(tabs, sign):
    """PH_SCAN_JIT=0: the same plan through ph_filter_select / ph_expr_eval / ph_agg_sink. No proof: every step whose single row fits is
    summed in 128 bits, the others are refused by ph_expr_eval's overflow flag"""
    def plan(ctx, t, consts):
        os.environ["PH_SCAN_JIT"] = "0"
        try:
            pl = jit_plan(ctx, t, consts)
        finally:
            os.environ.pop("PH_SCAN_JIT", None)
        assert pl.kind == "generic"
        return pl
    steps = lc_ladder(tabs, "n32", sign, plan=plan, result=jit_result, reference=DE.jit_reference)
    adm, ref, _ = ladder_conditions(f"generic {sign:+d}", steps, jit_bounds_products(tabs.lc_ladder("n32")[1], sign), lambda res: sum(g[2][0] for g in res))
    assert ref == [66]      # only the step whose single row leaves int64


# ------------------------------------------------------------------ A.2 the proof is per run

N_RUNS = (1 << 21) + (1 << 19)    # more than 512 tiles of 4096 rows: the narrow kernels' two workgroups per CU get a second tile
RUN_BOUND = 95 * 10 ** 13         # 9.5e14 a row: one 4096-row tile per workgroup is inside the proof (3.9e18), a fifth 1024-row tile is not


def bisect_runs(pl, n, bound):
    """the largest admitted row_end of runs [0, row_end), found by bisection; admission must be monotone at every point probed"""
    probes = {}

    def ok(e):
        probes[e] = admitted(pl, 0, e)
        return probes[e]
    assert not ok(n), "the whole table was admitted: the case needs a larger table or magnitude on this device"
    assert ok(DE.TILE) and ok((DE.PROOF_LIMIT - 1) // bound), "a run with rows x bound < 4e18 was refused"
    lo, hi = max(e for e, a in probes.items() if a), n
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ok(mid):
            lo = mid
        else:
            hi = mid
    assert max(e for e, a in probes.items() if a) < min(e for e, a in probes.items() if not a), sorted(probes.items())
    return lo


def runs_at_the_edge(name, pl, kinds, n, bound, result, reference):
    last = bisect_runs(pl, n, bound)
    got = run_or_refuse(pl, 0, last, result)
    assert got is not None and got == reference(kinds.runs(0, last)), (name, last)
    assert not admitted(pl, 0, last + 1)
    ragged = {}
    for b in (4, 8, 12, 4100):
        got = run_or_refuse(pl, b, last, result)
        ragged[b] = got is not None
        assert got is None or got == reference(kinds.runs(b, last)), (name, b, last)
    print(f"runs {name}: largest admitted row_end {last} of {n} at bound {bound}; ragged begins admitted: {ragged}")
    assert ragged[4100], "a run that starts 4100 rows later has no more tiles"


@pytest.mark.parametrize("form", ["n32", "wide"])
def test_lowcard_chain_proof_is_per_run(tabs, form):
    t, c, kinds = tabs.lc_ladder(form, N_RUNS)
    e, f1 = int(c["e"][2]), DE.LC_A1 + DE.LC_B1 * int(c["d"][2])
    consts = (DE.LC_A1, DE.LC_B1, RUN_BOUND // (e * f1) - int(c["t"][2]), 1)
    bound = DE.lc_row_bound(c, *consts)
    assert 9 * 10 ** 14 < bound <= RUN_BOUND
    pl = lc_plan(tabs.ctx, t, consts)
    assert pl.bytes_per_row == LC_BYTES[form]
    runs_at_the_edge(f"lowcard_chain {form}", pl, kinds, N_RUNS, bound, lc_result, lambda runs: DE.lc_reference(runs, P_LO, P_HI, *consts))
    pl.free()
    if form == "n32":   # the generated plan over the same table (1024-row tiles, up to eight workgroups per CU)
        pl = jit_plan(tabs.ctx, t, consts)
        assert pl.kind == "jit"
        runs_at_the_edge("jit", pl, kinds, N_RUNS, bound, jit_result, lambda runs: DE.jit_reference(runs, P_LO, P_HI, *consts))
        pl.free()
    tabs.drop(("lc", form, N_RUNS))


@pytest.mark.parametrize("form", ["n32", "wide"])
def test_filter_sumprod_proof_is_per_run(ctx, form):
    shared = DE.fs_ladder_shared(form, N_RUNS)
    b = RUN_BOUND // int(shared["a"][2])
    c = DE.fs_columns(shared, b, b - 200)
    bound = DE.fs_row_bound(c)
    assert 9 * 10 ** 14 < bound <= RUN_BOUND
    t = fs_table(ctx, c)
    pl = fs_plan(ctx, t)
    assert pl.bytes_per_row == FS_BYTES[form]
    runs_at_the_edge(f"filter_sumprod {form}", pl, DE.RowKinds(c), N_RUNS, bound, fs_result, lambda runs: DE.fs_reference(runs, P_LO, P_HI, 100))
    pl.free()
    t.free()


SHARE_NARROW = (10 * 4096, 11 * 4096)                 # one 4096-row tile: one workgroup's share of a narrow run of 2^20 rows
SHARE_WIDE = [7 + 256 * i for i in range(4)]          # the four 1024-row tiles workgroup 7 of 256 owns in a wide run of 2^20 rows


def share_columns(form):
    """the ladder table with the predicate column rewritten: 1 in one contiguous 4096-row tile, 2 in the strided tiles of one workgroup
    of the wide kernel, 0 elsewhere — every row that passes `p = 1` (or `p = 2`) lands in one workgroup's partial"""
    c = DE.lc_ladder_columns(form)
    p = np.zeros(N_LADDER, np.int32)
    p[SHARE_NARROW[0]:SHARE_NARROW[1]] = 1
    for tile in SHARE_WIDE:
        p[tile * 1024:(tile + 1) * 1024] = 2
    if form == "wide":
        p[1] = 70_000
    return dict(c, p=p)


@pytest.mark.parametrize("form", ["n32", "n64", "wide"])
def test_one_workgroup_holds_every_qualifying_row(tabs, form):
    t, c, kinds = tabs.get(("share", form), lambda: share_columns(form), lc_table)
    e, f1 = int(c["e"][2]), DE.LC_A1 + DE.LC_B1 * int(c["d"][2])
    consts = (DE.LC_A1, DE.LC_B1, RUN_BOUND // (e * f1) - int(c["t"][2]), 1)
    assert 4096 * DE.lc_row_bound(c, *consts) < DE.PROOF_LIMIT     # 4096 rows at the bound: the largest partial the proof allows
    seen = {}
    for lo, hi in ((1, 1), (2, 2), (1, 2)):
        pl = lc_plan(tabs.ctx, t, consts, lo, hi)
        assert (pl.bytes_per_row == 34) == (form == "wide")
        got = run_or_refuse(pl, 0, N_LADDER, lc_result)
        seen[(lo, hi)] = got is not None
        assert got is None or got == DE.lc_reference(kinds.runs(0, N_LADDER), lo, hi, *consts), (form, lo, hi)
        if lo == hi == 1:   # the tile alone: 4096 rows x bound < 4e18, so the proof has to admit it
            got = run_or_refuse(pl, *SHARE_NARROW, lc_result)
            want = DE.lc_reference(kinds.runs(*SHARE_NARROW), 1, 1, *consts)
            assert got == want and sum(g[3] for g in want) == 4096 and abs(sum(g[2][3] for g in want)) > 3 * 10 ** 18
        pl.free()
    print(f"one workgroup's share, {form}: whole-table runs admitted {seen}")
    tabs.drop(("share", form))


# ------------------------------------------------------------------ A.3 mixed signs

def mixed_columns(form, block):
    """alternating blocks of +max and -max in e (a for filter_sumprod): totals near zero, every partial near its bound"""
    c = DE.lc_ladder_columns(form)
    sign = 1 - 2 * ((np.arange(N_LADDER) // block) % 2)
    return dict(c, e=c["e"][2] * sign)


@pytest.mark.parametrize("block", [1024, 4096])
@pytest.mark.parametrize("form", ["n32", "wide"])
def test_mixed_signs(tabs, form, block):
    t, c, kinds = tabs.get(("mixed", form, block), lambda: mixed_columns(form, block), lc_table)
    e, f1 = int(c["e"][2]), DE.LC_A1 + DE.LC_B1 * int(c["d"][2])
    seen = {}
    for per_row in (DE.PROOF_LIMIT // N_LADDER - 10 ** 9, RUN_BOUND):    # one the proof must admit for the whole table, one near its limit
        consts = (DE.LC_A1, DE.LC_B1, per_row // (abs(e) * f1) - int(c["t"][2]), 1)
        bound = DE.lc_row_bound(c, *consts)
        for plan, result, reference in ((lc_plan, lc_result, DE.lc_reference), (jit_plan, jit_result, DE.jit_reference)):
            pl = plan(tabs.ctx, t, consts)
            got = run_or_refuse(pl, 0, N_LADDER, result)
            seen[(per_row, pl.kind)] = got is not None
            if DE.must_admit(N_LADDER, bound):
                assert got is not None, (form, block, per_row, pl.kind)
            assert got is None or got == reference(kinds.runs(0, N_LADDER), P_LO, P_HI, *consts), (form, block, per_row, pl.kind)
            pl.free()
    print(f"mixed signs lowcard_chain/jit {form} blocks of {block}: admitted {seen}")
    tabs.drop(("mixed", form, block))
    # filter_sumprod: a alternates, b carries the magnitude
    shared = DE.fs_ladder_shared(form)
    a = int(shared["a"][2])
    shared = dict(shared, a=a * (1 - 2 * ((np.arange(N_LADDER) // block) % 2)))
    for per_row in (DE.PROOF_LIMIT // N_LADDER - 10 ** 9, RUN_BOUND):
        c = DE.fs_columns(shared, per_row // a, per_row // a - 200)
        t = fs_table(tabs.ctx, c)
        pl = fs_plan(tabs.ctx, t)
        got = run_or_refuse(pl, 0, N_LADDER, fs_result)
        if DE.must_admit(N_LADDER, DE.fs_row_bound(c)):
            assert got is not None, (form, block, per_row)
        assert got is None or got == DE.fs_reference(DE.RowKinds(c).runs(0, N_LADDER), P_LO, P_HI, 100), (form, block, per_row)
        pl.free()
        t.free()


# ------------------------------------------------------------------ A.4 partials merged across shards

@pytest.mark.parametrize("sign", [1, -1])
def test_shard_totals_beyond_2_63_merge(tabs, sign):
    """three row ranges of one table as three ranks: each rank's sums are beyond 2^63, ph_scan_plan_fetch_merged adds the 128-bit words"""
    t, c, kinds = tabs.lc_ladder("n32")
    n = len(c["p"])
    cuts = [0, 349_524, 699_052, n]
    consts = [s[1] for s in DE.lc_ladder_steps(c, sign) if s[0] == 48][0]
    for plan, result, reference, col in ((lc_plan, lc_result, DE.lc_reference, 3), (jit_plan, jit_result, DE.jit_reference, 0)):
        pl = plan(tabs.ctx, t, consts)
        words = []
        for b, e in zip(cuts[:-1], cuts[1:]):
            pl.run(b, e)
            ptr, nw = pl.partials_dev()
            words.append(tabs.ctx.download(hip.vp(ptr), np.uint64, nw))
            shard = reference(kinds.runs(b, e), P_LO, P_HI, *consts)
            assert all(abs(g[2][col]) >= 2 ** 63 for g in shard)
        merged = result(pl.fetch_merged(np.concatenate(words), 3))
        want = reference(kinds.runs(0, n), P_LO, P_HI, *consts)
        # first rows of a merged result carry the rank in their upper bits: groups compare by key here
        assert sorted(g[1:] for g in merged) == sorted(g[1:] for g in want), (pl.kind, sign)
        pl.free()
    shared = DE.fs_ladder_shared("n32")
    b, b0 = [(s[1], s[2]) for s in DE.fs_ladder_steps(shared, sign) if s[0] == 48][0]
    cf = DE.fs_columns(shared, b, b0)
    tf = fs_table(tabs.ctx, cf)
    kf = DE.RowKinds(cf)
    pl = fs_plan(tabs.ctx, tf)
    words = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        pl.run(lo, hi)
        ptr, nw = pl.partials_dev()
        words.append(tabs.ctx.download(hip.vp(ptr), np.uint64, nw))
        assert abs(DE.fs_reference(kf.runs(lo, hi), P_LO, P_HI, 100)[0]) >= 2 ** 63
    assert fs_result(pl.fetch_merged(np.concatenate(words), 3)) == DE.fs_reference(kf.runs(0, n), P_LO, P_HI, 100)
    pl.free()
    tf.free()


# ------------------------------------------------------------------ B where the 32-bit form begins and ends

def boundary_ranges(n):
    return [(b, n + e if e is not None and e < 0 else (n if e is None else e)) for b, e in DE.BOUNDARY_RANGES]


def widen(c):
    """the same rows over a predicate column without a copy (row 500, which fails the predicate either way, moves 70 000 days out): the
    wide kernels"""
    p = c["p"].copy()
    assert p[500] == P_LO
    p[500] = P_LO - 70_000
    return dict(c, p=p)


def run_boundaries(ctx, check=True):
    """{case: [[b, e, bytes per row, result]]} of every boundary case over narrowed copies, each compared with Python (row by row)"""
    out = {}
    for name, c, consts, _ in DE.lc_boundary_cases():
        t = lc_table(ctx, c)
        pl = lc_plan(ctx, t, consts, P_LO + 1, P_HI)      # p = P_LO (every 1000th row) fails: the predicate is live
        out["lc " + name] = res = []
        for b, e in boundary_ranges(len(c["p"])):
            got = run_or_refuse(pl, b, e, lc_result)
            if check:
                assert got == DE.lc_reference(DE.rows_of(c, b, e), P_LO + 1, P_HI, *consts), (name, b, e)
            res.append([b, e, pl.bytes_per_row, got])
        pl.free()
        t.free()
    for name, c, _ in DE.fs_boundary_cases():
        t = fs_table(ctx, c)
        pl = fs_plan(ctx, t, P_LO + 1, P_HI)
        out["fs " + name] = res = []
        for b, e in boundary_ranges(len(c["p"])):
            got = run_or_refuse(pl, b, e, fs_result)
            if check:
                assert got is not None and got == DE.fs_reference(DE.rows_of(c, b, e), P_LO + 1, P_HI, 100), (name, b, e)
            res.append([b, e, pl.bytes_per_row, got])
        pl.free()
        t.free()
    return out


def run_narrow_cases(ctx, check):
    """what the child processes repeat: the n32 ladders (the compile-time-width instances by default) and the boundary cases"""
    tabs = Tables(ctx)
    out = {"boundaries": run_boundaries(ctx, check)}
    for sign in (1, -1):
        out[f"lc_ladder{sign:+d}"] = lc_ladder(tabs, "n32", sign, check=check)
        out[f"fs_ladder{sign:+d}"] = fs_ladder(tabs, "n32", sign, check=check)
    tabs.free()
    return out


def child_run(**env):
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"domain_edges_child_{os.getpid()}.json")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, **env), check=True, timeout=600)
    with open(out) as f:
        res = json.load(f)
    os.remove(out)
    return res


def strip_bytes(rows):
    """results without the bytes per row (which names the kernel family that ran)"""
    return [r[:2] + r[3:] for r in rows]


def test_32_bit_form_boundaries_against_python_and_the_other_kernels(ctx):
    """Each case of domain_edges.lc_boundary_cases / fs_boundary_cases is exact against Python over narrowed copies (run_boundaries), over a
    table without them (the wide kernels) and, in child processes, under PH_SCAN_NARROW_GENERIC=1 and PH_NARROW=0 — so it holds whichever
    side of the rule the form selection falls. Predicted by scan_plan.hip's rule: be / b1 / b2 = 2^31 - 1 and be b1 = 46341 x 46340 take
    FORM_NARROW32, be / b1 / b2 = 2^31 and be b1 = 65536 x 32768 = 2^31 take FORM_NARROW; ba / bb likewise for filter_sumprod."""
    mine = json.loads(json.dumps(run_narrow_cases(ctx, True)))
    # the narrow kernels ran: p 2 bytes, q 1, the 2^31-wide column 4 and the others 1 (both factors 4 in the be b1 cases), 2 code bytes
    assert {k: v[0][2] for k, v in mine["boundaries"].items()} == {
        **{"lc " + c[0]: 14 if c[0].startswith("be_b1") else 11 for c in DE.lc_boundary_cases(n=1000)}, **{"fs " + c[0]: 11 for c in DE.fs_boundary_cases(n=1000)}}
    for name, c, consts, _ in DE.lc_boundary_cases():
        cw = widen(c)
        t = lc_table(ctx, cw)
        pl = lc_plan(ctx, t, consts, P_LO + 1, P_HI)
        assert pl.bytes_per_row == 34
        for (b, e), narrow in zip(boundary_ranges(len(c["p"])), mine["boundaries"]["lc " + name]):
            assert json.loads(json.dumps(run_or_refuse(pl, b, e, lc_result))) == narrow[3], (name, b, e)
        pl.free()
        t.free()
    for name, c, _ in DE.fs_boundary_cases():
        t = fs_table(ctx, widen(c))
        pl = fs_plan(ctx, t, P_LO + 1, P_HI)
        assert pl.bytes_per_row == 24
        for (b, e), narrow in zip(boundary_ranges(len(c["p"])), mine["boundaries"]["fs " + name]):
            assert run_or_refuse(pl, b, e, fs_result) == narrow[3], (name, b, e)
        pl.free()
        t.free()
    generic, wide = child_run(PH_SCAN_NARROW_GENERIC="1"), child_run(PH_NARROW="0")
    assert all(r[2] in (24, 34) for v in wide["boundaries"].values() for r in v) and all(s[2] in (24, 34) for k, v in wide.items() if k != "boundaries" for s in v)
    for other in (generic, wide):
        assert other.keys() == mine.keys() and other["boundaries"].keys() == mine["boundaries"].keys()
        for k, rows in mine["boundaries"].items():
            assert strip_bytes(rows) == strip_bytes(other["boundaries"][k]), k
        for k, rows in mine.items():
            if k != "boundaries":
                assert strip_bytes(rows) == strip_bytes(other[k]), k


if __name__ == "__main__":   # child_run: the narrow cases under another environment (a fresh process: the switches are read once)
    _ctx = hip.Ctx(0)
    _res = run_narrow_cases(_ctx, False)
    _ctx.close()
    with open(sys.argv[1], "w") as _f:
        json.dump(_res, _f)
