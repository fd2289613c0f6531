"""GPU parity of the fused scans over frame-of-reference narrowed column copies (ph_table_col_narrow):
every case runs with the copies (the default), is checked against a numpy restatement or the oracle, asserts through
ph_scan_plan_bytes_per_row that the narrow kernel ran, and is compared bit for bit with the same case run in a child
process under PH_NARROW=0 (the wide kernels; the switch is read once per process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import oracle_lib as O  # noqa: E402
from plan_amd import hip, queries, tpchgen  # noqa: E402

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1

# lowcard_chain shape over a lineitem-like layout: q, e, d, t, k0, k1, p (queries.lineitem_table's column order)
Q, E, D, T, K0, K1, P = range(7)


def exact_sum(x):
    """exact sum of an int64 array as a Python int (two int64 partial sums of the high and low halves)"""
    x = np.asarray(x, dtype=np.int64)
    return (int((x >> 32).sum()) << 32) + int((x & 0xFFFFFFFF).sum())


def lc_table(ctx, c):
    return hip.Table(ctx, [(hip.PH_I32, c["q"]), (hip.PH_DEC64, c["e"], 2), (hip.PH_DEC64, c["d"], 2), (hip.PH_DEC64, c["t"], 2),
                           (hip.PH_CODE8, c["k0"], 0, None, ["a", "b", "c"]), (hip.PH_CODE8, c["k1"], 0, None, ["x", "y"]),
                           (c.get("ptype", hip.PH_DATE), c["p"])], len(c["p"]))


def lc_plan(ctx, t, lo, hi, ptype):
    e, d, tt = hip.X_COL(E), hip.X_COL(D), hip.X_COL(T)
    one = hip.X_CONST(1, 0)
    dp = [e, one, d, hip.X_SUB, hip.X_MUL]
    aggs = [hip.aggexpr(hip.PH_A_SUM, [hip.X_COL(Q)]), hip.aggexpr(hip.PH_A_SUM, [e]), hip.aggexpr(hip.PH_A_SUM, dp),
            hip.aggexpr(hip.PH_A_SUM, dp + [one, tt, hip.X_ADD, hip.X_MUL]), hip.aggexpr(hip.PH_A_AVG, [d]),
            hip.aggexpr(hip.PH_A_COUNT_STAR)]
    preds = [hip.pred(P, hip.PH_GE, hip.const(ptype, i=lo)), hip.pred(P, hip.PH_LE, hip.const(ptype, i=hi))]
    return hip.ScanPlan(ctx, t, preds, [K0, K1], aggs)


def lc_want(c, lo, hi, b, e_):
    """numpy restatement: groups in first-seen order, {key: (first_row, [Σq, Σe, Σe(1-d), Σe(1-d)(1+t), Σd], count)}"""
    sl = slice(b, e_)
    p, q, e, d, t = (np.asarray(c[k][sl]).astype(np.int64) for k in ("p", "q", "e", "d", "t"))
    m = (p >= lo) & (p <= hi)
    k0, k1 = c["k0"][sl].astype(np.int64), c["k1"][sl].astype(np.int64)
    out = []
    for key in sorted(set(zip(k0[m].tolist(), k1[m].tolist()))):
        g = m & (k0 == key[0]) & (k1 == key[1])
        dp = e[g] * (100 - d[g])
        out.append((int(np.flatnonzero(g)[0]) + b, key,
                    [exact_sum(q[g]), exact_sum(e[g]), exact_sum(dp), exact_sum(dp * (100 + t[g])), exact_sum(d[g])], int(g.sum())))
    return sorted(out)


def lc_result(r):
    """(first_row, key, [Σq, Σe, Σdp, Σch, Σd], count) per group, in the result's order"""
    return [(int(r["first_row"][g]), tuple(int(k) for k in r["keys"][g]), [int(x) for x in r["sum"][g][:5]], int(r["count"][g][5]))
            for g in range(r["ngroups"])]


def run_lc(ctx, c, intervals, ranges, want_narrow):
    """runs every (interval, row range) of one table; returns the results (JSON-able) and checks them against numpy"""
    t = lc_table(ctx, c)
    ptype = c.get("ptype", hip.PH_DATE)
    n = len(c["p"])
    res = []
    for lo, hi in intervals:
        pl = lc_plan(ctx, t, lo, hi, ptype)
        assert pl.kind == "lowcard_chain"
        bpr = pl.bytes_per_row
        if want_narrow is not None:
            assert (bpr < 34) == want_narrow, (bpr, want_narrow)
        for b, e_ in ranges:
            e_ = n if e_ is None else e_
            pl.run(b, e_)
            got = lc_result(pl.fetch())
            want = lc_want(c, lo, hi, b, e_)
            assert [(g[1], g[2], g[3]) for g in got] == [(w[1], w[2], w[3]) for w in want], (lo, hi, b, e_)
            assert [g[0] for g in got] == [w[0] for w in want]
            res.append([lo, hi, b, e_, bpr, got])
        pl.free()
    t.free()
    return res


def lc_data(n, seed, p_lo, p_hi, ptype=hip.PH_DATE, q=(1, 50), e=(90_000, 10_500_000), d=(0, 10), t=(0, 8)):
    """random columns with their ranges pinned at both ends (rows 0 and 1 hold every column's min and max)"""
    rng = np.random.default_rng(seed)

    def col(lo, hi, dtype):
        v = rng.integers(lo, hi, n, endpoint=True, dtype=np.int64)
        v[0], v[1] = lo, hi
        return v.astype(dtype)

    return dict(p=col(p_lo, p_hi, np.int32), q=col(*q, np.int32), e=col(*e, np.int64), d=col(*d, np.int64), t=col(*t, np.int64),
                k0=rng.integers(0, 3, n).astype(np.uint8), k1=rng.integers(0, 2, n).astype(np.uint8), ptype=ptype)


RAGGED = [(0, None), (4, None), (8, None), (12, None), (4, -3), (4100, -7), (12, 15), (4, 9), (8, 8), (0, 1), (20, 35)]


def ragged(n):
    return [(b, n + e if e is not None and e < 0 else e) for b, e in RAGGED]


# (name, columns, intervals, narrow expected) — the widths of p / e at their boundaries, negative mins, a large base
def lc_cases():
    n = 20_000
    d0 = tpchgen.days(1994, 1, 1)
    cases = []
    for span in (255, 256, 65_535, 65_536):   # p: 1- / 2-byte codes; a DATE spanning 65 536 days needs its own 4 bytes (no copy)
        c = lc_data(n, span, d0, d0 + span)
        mid = d0 + span // 2
        cases.append((f"p_span_{span}", c, [(d0, mid), (I32_MIN, I32_MAX)], span <= 65_535))
    # the 65 536-day predicate column beside 2-byte codes elsewhere: every width tuple must take the narrow form
    c = lc_data(n, 11, d0, d0 + 300, q=(-40_000, 20_000), d=(0, 300), t=(-1, 65_534))
    cases.append(("widths_2_2_4_2_2", c, [(d0 + 10, d0 + 250)], True))
    for span in (2 ** 32 - 1, 2 ** 32):   # e: 4-byte codes / no copy (the plan keeps the wide kernel)
        c = lc_data(n, span % 1000, d0, d0 + 100, e=(-(2 ** 31), -(2 ** 31) + span))
        cases.append((f"e_span_{span}", c, [(d0, d0 + 50)], span < 2 ** 32))
    # dates before 1970 and negative quantities; predicate constants around [min, max]
    c = lc_data(n, 5, -5000, -4000, q=(-100, -1), d=(-5, 5))
    cases.append(("negative_mins", c, [(-6000, -5001), (-6000, -5000), (-4000, -3000), (-5000, -4000), (-3999, -3000), (-4500, -4600),
                                       (-4700, -4300), (I32_MIN, I32_MAX)], True))
    # an int64 decimal with a base far above 2^32 and a one-byte range (64-bit products: the 32-bit form is not proven); larger
    # values would fail the overflow proof of the aggregate (rows per workgroup x |e (1 - d)(1 + t)| < 4e18)
    c = lc_data(n, 6, d0, d0 + 30, e=(90_000_000_000, 90_000_000_255), d=(0, 0), t=(0, 0))
    cases.append(("large_base", c, [(d0, d0 + 15)], True))
    # an int32 predicate column over the whole int32 range: no copy, the wide kernel
    c = lc_data(n, 7, I32_MIN, I32_MAX, ptype=hip.PH_I32)
    cases.append(("p_full_int32", c, [(-1000, 10 ** 9)], False))
    return cases


def run_lc_cases(ctx, check_narrow):
    out = {}
    for name, c, intervals, narrow in lc_cases():
        out[name] = run_lc(ctx, c, intervals, ragged(len(c["p"])), narrow if check_narrow else None)
    return out


def fs_run(ctx, L, consts, ranges):
    t = queries.lineitem_table(ctx, L)
    pl = queries.q6_plan(ctx, t, consts)
    assert pl.kind == "filter_sumprod"
    bpr = pl.bytes_per_row
    res = []
    for b, e_ in ranges:
        pl.run(b, e_)
        r = pl.fetch()
        rc, dsum = O.q6({k: v[b:e_] for k, v in L.items()}, *consts)
        if rc == 1:
            assert r["ngroups"] == 0
        else:
            assert r["ngroups"] == 1 and r["sum"][0][0] == dsum.unscaled(4), (b, e_)
        res.append([b, e_, bpr, [int(x) for x in r["sum"][0]] if r["ngroups"] else None])
    pl.free()
    t.free()
    return res


def q6_cases(L):
    n = len(L["l_shipdate"])
    c = queries.q6_constants()
    return [("q6", L, c, [(0, n), (4, n), (8, n - 5), (12, 4111), (4, 9), (8, 8)]),
            ("q6_nothing", L, (tpchgen.days(2001, 1, 1), tpchgen.days(2002, 1, 1)) + c[2:], [(0, n)]),
            ("q6_everything", L, (tpchgen.days(1990, 1, 1), tpchgen.days(2000, 1, 1), -1e30, 1e30, 1000), [(0, n), (12, n - 1)])]


def sf1_lineitem():
    return tpchgen.lineitem((1, 1), columns=["l_quantity", "l_extendedprice", "l_discount", "l_tax", "l_returnflag",
                                             "l_linestatus", "l_shipdate"])


def run_all(ctx, check_narrow):
    out = {"lowcard": run_lc_cases(ctx, check_narrow)}
    L = sf1_lineitem()
    for name, Lc, consts, ranges in q6_cases(L):
        out[name] = fs_run(ctx, Lc, consts, ranges)
    t = queries.lineitem_table(ctx, L)
    pl = queries.q1_plan(ctx, t)
    pl.run()
    r = pl.fetch()
    out["q1_sf1"] = [pl.bytes_per_row, [[int(k) for k in r["keys"][g]] + [int(x) for x in r["sum"][g]] + [int(r["count"][g][7])]
                                        for g in range(r["ngroups"])]]
    out["narrow_bytes"] = t.narrow_bytes()
    pl.free()
    t.free()
    return out


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


def run_small(ctx):
    """the synthetic lowcard cases and Q6 over a hundredth of SF1: what a child runs to cover one more kernel instance"""
    L = tpchgen.lineitem((1, 100), columns=["l_quantity", "l_extendedprice", "l_discount", "l_tax", "l_returnflag", "l_linestatus", "l_shipdate"])
    return {"lowcard": run_lc_cases(ctx, False), "q6": [fs_run(ctx, Lc, consts, ranges) for _, Lc, consts, ranges in q6_cases(L)]}


def child_run(small=False, **env):
    """every case of this file (small: run_small) in a fresh child process under the given environment (the switches are read once per process)"""
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"narrow_child_{os.getpid()}.json")
    subprocess.run([sys.executable, os.path.abspath(__file__), out] + (["small"] if small else []), env=dict(os.environ, **env), check=True, timeout=600)
    with open(out) as f:
        res = json.load(f)
    os.remove(out)
    return res


@pytest.fixture(scope="module")
def wide():
    """PH_NARROW=0: the wide kernels"""
    return child_run(PH_NARROW="0")


@pytest.fixture(scope="module")
def generic():
    """PH_SCAN_NARROW_GENERIC=1: the narrow kernels' instance that reads the code widths at run time, for every width tuple"""
    return child_run(PH_SCAN_NARROW_GENERIC="1")


def test_copies_at_load(ctx):
    L = sf1_lineitem()
    t = queries.lineitem_table(ctx, L)
    want = {queries.L_QUANTITY: 1, queries.L_EXTENDEDPRICE: 4, queries.L_DISCOUNT: 1, queries.L_TAX: 1, queries.L_SHIPDATE: 2}
    for c, w in want.items():
        assert t.col_narrow(c) == (w, t.col_range(c)[0])
    assert t.col_narrow(queries.L_RETURNFLAG) is None   # dictionary codes are read as they are
    padded = -(-len(L["l_shipdate"]) // 8192) * 8192
    assert t.narrow_bytes() == padded * 9
    t.free()
    # a NULL-able column and a column over the whole int64 range get no copy; a base near 10^18 with a small range does
    n = 1000
    big = np.arange(n, dtype=np.int64) + 10 ** 18
    full = np.arange(n, dtype=np.int64)
    full[0], full[1] = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    valid = np.full((n + 7) // 8, 0xFF, np.uint8)
    valid[0] = 0xFE
    t = hip.Table(ctx, [(hip.PH_DEC64, big, 2), (hip.PH_I64, full), (hip.PH_I32, np.ones(n, np.int32), 0, valid)], n)
    assert t.col_narrow(0) == (2, 10 ** 18)
    assert t.col_narrow(1) is None
    assert t.col_narrow(2) is None
    t.free()


def test_q1_sf1_narrow(ctx, wide):
    L = sf1_lineitem()
    t = queries.lineitem_table(ctx, L)
    pl = queries.q1_plan(ctx, t)
    assert pl.kind == "lowcard_chain" and pl.bytes_per_row == 11
    pl.run()
    r = pl.fetch()
    want = O.q1(L, queries.q1_shipdate_cutoff())
    assert r["ngroups"] == len(want) == 4
    for g, w in enumerate(want):
        assert tuple(r["keys"][g]) == (w.returnflag, w.linestatus)
        assert r["sum"][g][:4] == [w.sum_qty.value(), w.sum_base_price.unscaled(2), w.sum_disc_price.unscaled(4), w.sum_charge.unscaled(6)]
        assert r["count"][g][7] == w.count_order
    got = [[int(k) for k in r["keys"][g]] + [int(x) for x in r["sum"][g]] + [int(r["count"][g][7])] for g in range(r["ngroups"])]
    pl.free()
    t.free()
    assert wide["q1_sf1"][0] == 34 and wide["narrow_bytes"] == 0
    assert got == wide["q1_sf1"][1]


def test_q6_sf1_narrow(ctx, wide):
    L = sf1_lineitem()
    for name, Lc, consts, ranges in q6_cases(L):
        res = fs_run(ctx, Lc, consts, ranges)
        assert all(r[2] == 8 for r in res), name
        assert all(r[2] == 24 for r in wide[name]), name
        assert [r[:2] + r[3:] for r in res] == [r[:2] + r[3:] for r in wide[name]], name


def test_lowcard_width_boundaries_and_ranges(ctx, wide):
    got = run_lc_cases(ctx, True)
    for name, res in got.items():
        w = wide["lowcard"][name]
        assert len(res) == len(w), name
        for a, b in zip(res, w):
            assert a[:4] == b[:4]
            assert b[4] == 34   # the child ran the wide kernel
            assert json.loads(json.dumps(a[5])) == b[5], (name, a[:4])


def test_fixed_width_instances_match_generic(wide, generic):
    """the instances compiled for lineitem's width tuples (Q1, Q6 and the synthetic cases with the same tuple) against the
    run-time-width instance and the wide kernels"""
    assert generic["q1_sf1"][0] == 11 and generic["q1_sf1"][1] == wide["q1_sf1"][1]
    for name, _, _, _ in q6_cases({"l_shipdate": np.zeros(1)}):
        assert all(r[2] == 8 for r in generic[name]), name
        assert [r[:2] + r[3:] for r in generic[name]] == [r[:2] + r[3:] for r in wide[name]], name
    for name, res in generic["lowcard"].items():
        assert [r[:4] + r[5:] for r in res] == [r[:4] + r[5:] for r in wide["lowcard"][name]], name


@pytest.mark.parametrize("env,bytes_q6", [({"PH_SCAN_NT": "0"}, 8), ({"PH_SCAN_NT": "0", "PH_NARROW": "0"}, 24),
                                          ({"PH_NARROW": "0", "PH_SCAN_UNROLL": "2"}, 24), ({"PH_NARROW": "0", "PH_SCAN_UNROLL": "3"}, 24)],
                         ids=["plain_loads_narrow", "plain_loads_wide", "wide_unroll_2", "wide_unroll_3"])
def test_load_form_and_unroll_instances(wide, env, bytes_q6):
    """PH_SCAN_NT=0 (plain instead of non-temporal loads; read once per process) and PH_SCAN_UNROLL=2 / 3 pick kernel instances of
    their own: a child runs the lowcard cases and a small Q6 through them (each checked against numpy / the oracle in the child)
    and its results equal the wide kernels' bit for bit."""
    res = child_run(small=True, **env)
    for name, r in res["lowcard"].items():
        assert [x[:4] + x[5:] for x in r] == [x[:4] + x[5:] for x in wide["lowcard"][name]], name
        if "PH_NARROW" in env:
            assert all(x[4] == 34 for x in r), name
    assert len(res["q6"]) == 3 and all(x[2] == bytes_q6 for case in res["q6"] for x in case)


if __name__ == "__main__":   # child_run: the cases under another environment (a fresh process: the switches are read once)
    _ctx = hip.Ctx(0)
    _res = run_small(_ctx) if sys.argv[2:] == ["small"] else run_all(_ctx, False)
    _ctx.close()
    with open(sys.argv[1], "w") as _f:
        json.dump(_res, _f)
