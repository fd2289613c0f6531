"""Which plan a scan descriptor becomes, as a table: ph_scan_plan_kind / _variant / _bytes_per_row / _row_body and the exact result of
every descriptor shape that shape matching, role matching, predicate lowering, instance choice or grid geometry (scan_lower.h,
scan_inst.h, scan_plan.hip) could take another way.

One table of 2 * 4096 + 5 rows: the smallest span with an interior tile, a masked first tile and a masked last tile for the 4096-row
kernels. Columns in lineitem's value domains: a date, an int32 quantity, three DECIMAL(·, 2) columns (price, discount, tax), two
two-symbol dictionary columns, a NULL-able int32 column and a second NULL-free int32 column (three int32 predicate columns need one).
Every descriptor is created with the narrowed copies and, in a child process, under PH_NARROW=0 (read once per process); the Q1 family
also under PH_SCAN_JIT=0 (read at every create), where a plan that names fewer columns than the kernel reads gets stand-in columns.
The four strings and the bytes per row are the recorded table EXPECT; every result is compared with numpy / Python integers over
[0, n) and [7, n - 3), or [8, n - 3) where the kernel loads 4-row vectors from row_begin on (generic plans over NULL-able columns
take whole validity bytes).

The multiplier of f1 at the 24-bit bound of the lean row body: through the ABI a factor's multiplier is a power of ten (it comes from
aligning scales), so 10^6 (admitted: narrow32_lean) and 10^7 (refused: narrow32) are the pair around 2^23. Only a constant column
lets |f1| stay inside the 32-bit form beside such a multiplier, hence the tenth column, 5 in every row, and f1 = (5 10^s + 3) - 10^s d5
= 3. The bound itself (2^23 - 1 admitted, 2^23 refused) is pinned on the host in tests/test_scan_lower.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from plan_amd import hip, tpchgen  # noqa: E402

pytestmark = pytest.mark.gpu

N = 2 * 4096 + 5
SHIP, QTY, E, D, T, K0, K1, NQ, I2, D5 = range(10)
SCALE = {E: 2, D: 2, T: 2}
D0 = tpchgen.days(1992, 1, 2)
D1 = tpchgen.days(1998, 12, 1)
CUT = D1 - 112
Y94, Y95 = tpchgen.days(1994, 1, 1), tpchgen.days(1995, 1, 1)


def columns():
    """every column's minimum in row 0 and its maximum in row 1; rows 2 .. 6 and the last three differ from their neighbours in group
    and in predicate outcome, so a run that starts at row 7 or ends at n - 3 has something to leave out"""
    rng = np.random.default_rng(20261)

    def col(lo, hi, dtype):
        v = rng.integers(lo, hi, N, endpoint=True, dtype=np.int64)
        v[0], v[1] = lo, hi
        return v.astype(dtype)

    c = {SHIP: col(D0, D1, np.int32), QTY: col(1, 50, np.int32), E: col(90_000, 10_494_950, np.int64), D: col(0, 10, np.int64),
         T: col(0, 8, np.int64), K0: rng.integers(0, 2, N).astype(np.uint8), K1: rng.integers(0, 2, N).astype(np.uint8),
         NQ: col(-5, 60, np.int32), I2: col(0, 1000, np.int32), D5: np.full(N, 5, np.int64)}
    valid = rng.integers(0, 4, N) != 0   # a quarter NULL
    valid[:2] = True
    return c, valid


def make_table(ctx, c, valid):
    bits = np.packbits(valid, bitorder="little")
    return hip.Table(ctx, [(hip.PH_DATE, c[SHIP]), (hip.PH_I32, c[QTY]), (hip.PH_DEC64, c[E], 2), (hip.PH_DEC64, c[D], 2),
                           (hip.PH_DEC64, c[T], 2), (hip.PH_CODE8, c[K0], 0, None, ["a", "b"]), (hip.PH_CODE8, c[K1], 0, None, ["x", "y"]),
                           (hip.PH_I32, c[NQ], 0, bits), (hip.PH_I32, c[I2]), (hip.PH_DEC64, c[D5], 0)], N)


# ---------------------------------------------------------------- descriptors: what goes to the library beside what numpy computes

X, K, ADD, SUB, MUL = hip.X_COL, hip.X_CONST, hip.X_ADD, hip.X_SUB, hip.X_MUL
ONE = K(1, 0)
DP = [X(E), ONE, X(D), SUB, MUL]                 # e (1 - d), scale 4
CH = DP + [ONE, X(T), ADD, MUL]                  # e (1 - d) (1 + t), scale 6


def obj(a):
    return np.asarray(a).astype(object)


def v_dp(c):
    return obj(c[E]) * (100 - obj(c[D]))


def v_ch(c):
    return v_dp(c) * (100 + obj(c[T]))


def A(kind, prog, val):
    """an aggregate: (kind, RPN program, the argument's unscaled values per row as Python integers)"""
    return (kind, prog, val)


def col_agg(kind, c_):
    return A(kind, [X(c_)], lambda c: obj(c[c_]))


SUM_Q, SUM_E, SUM_D = col_agg(hip.PH_A_SUM, QTY), col_agg(hip.PH_A_SUM, E), col_agg(hip.PH_A_SUM, D)
AVG_D = col_agg(hip.PH_A_AVG, D)
SUM_DP, SUM_CH = A(hip.PH_A_SUM, DP, v_dp), A(hip.PH_A_SUM, CH, v_ch)
STAR = A(hip.PH_A_COUNT_STAR, [], None)
SUM_ED = A(hip.PH_A_SUM, [X(E), X(D), MUL], lambda c: obj(c[E]) * obj(c[D]))
SUM_DE = A(hip.PH_A_SUM, [X(D), X(E), MUL], lambda c: obj(c[E]) * obj(c[D]))
SUM_ET = A(hip.PH_A_SUM, [X(E), X(T), MUL], lambda c: obj(c[E]) * obj(c[T]))


def q1_with_multiplier(s):
    """Q1's aggregates with f1 = (5 10^s + 3) - 10^s d5 in place of 1 - d: the multiplier of the discount column is -10^s, f1 is 3"""
    dp = [X(E), K(5 * 10 ** s + 3, s), X(D5), SUB, MUL]
    return [SUM_Q, SUM_E, A(hip.PH_A_SUM, dp, lambda c: obj(c[E]) * 3), A(hip.PH_A_SUM, dp + [ONE, X(T), ADD, MUL], lambda c: obj(c[E]) * 3 * (100 + obj(c[T]))),
            col_agg(hip.PH_A_AVG, D5), STAR]


def P_(col, op, typ, v):
    """a predicate: (column, operator, literal type, literal)"""
    return (col, op, typ, v)


F_LO, F_HI = float(np.float32(0.03) - np.float32(0.01)), float(np.float32(0.03) + np.float32(0.01))
Q6_DATES = [P_(SHIP, hip.PH_GE, hip.PH_DATE, Y94), P_(SHIP, hip.PH_LT, hip.PH_DATE, Y95)]
Q6_DISC = [P_(D, hip.PH_GE, hip.PH_F32, F_LO), P_(D, hip.PH_LE, hip.PH_F32, F_HI)]
Q6_QTY = [P_(QTY, hip.PH_LT, hip.PH_I32, 24)]
SHIP_LE = [P_(SHIP, hip.PH_LE, hip.PH_DATE, CUT)]
Q1_AGGS = [SUM_Q, SUM_E, SUM_DP, SUM_CH, AVG_D, STAR]
KEYS = [K0, K1]

# name -> (predicates, group columns, aggregates, also under PH_SCAN_JIT=0)
CASES = {
    "q6": (Q6_DATES + Q6_DISC + Q6_QTY, [], [SUM_ED], False),
    "q6_pred_on_first_factor": (Q6_DATES + Q6_DISC + Q6_QTY, [], [SUM_DE], False),
    "q6_one_int32_pred_column": (Q6_DATES + Q6_DISC, [], [SUM_ED, STAR], False),
    "three_int32_pred_columns": (Q6_DATES + Q6_QTY + [P_(I2, hip.PH_GE, hip.PH_I32, 100)], [], [SUM_ED], False),
    "two_sumprod_pairs": (Q6_DATES + Q6_QTY, [], [SUM_ED, SUM_ET], False),
    "count_star_alone": (SHIP_LE, [], [STAR], False),
    "q1": (SHIP_LE, KEYS, Q1_AGGS, True),
    "q1_reversed": (SHIP_LE, KEYS, Q1_AGGS[::-1], True),
    "q1_no_tax_chain": (SHIP_LE, KEYS, [SUM_Q, SUM_E, SUM_DP, AVG_D, STAR], True),
    "q1_no_quantity": (SHIP_LE, KEYS, [SUM_E, SUM_DP, SUM_CH, AVG_D, STAR], True),
    "q1_singles_e_d": (SHIP_LE, KEYS, [SUM_E, SUM_D], True),
    "q1_singles_d_e": (SHIP_LE, KEYS, [SUM_D, SUM_E], True),
    "chain_first_factor_1_minus_d": (SHIP_LE, KEYS, [A(hip.PH_A_SUM, [ONE, X(D), SUB, X(E), MUL, ONE, X(T), ADD, MUL], v_ch), STAR], True),
    "f1_multiplier_1e6": (SHIP_LE, KEYS, q1_with_multiplier(6), True),
    "f1_multiplier_1e7": (SHIP_LE, KEYS, q1_with_multiplier(7), True),
    "one_group_column": (SHIP_LE, [K0], [SUM_E, STAR], False),
    "two_range_columns_two_groups": (SHIP_LE + Q6_QTY, KEYS, Q1_AGGS, True),
    "min_of_column": (SHIP_LE, [K0], [col_agg(hip.PH_A_MIN, E), STAR], False),
    "min_of_expression": (SHIP_LE, [K0], [A(hip.PH_A_MIN, DP, v_dp), STAR], False),
    "nullable_argument": (SHIP_LE, [K0], [col_agg(hip.PH_A_SUM, NQ), SUM_E, STAR], False),
}


def selected(c, preds):
    m = np.ones(N, bool)
    for col, op, typ, v in preds:
        if typ == hip.PH_F32:   # DECIMAL against FLOAT: decimal -> float64 -> float32, compared as float32
            x, k = (c[col].astype(np.float64) / 10.0 ** SCALE[col]).astype(np.float32), np.float32(v)
        else:
            x, k = c[col].astype(np.int64), v
        m &= {hip.PH_LT: x < k, hip.PH_LE: x <= k, hip.PH_GT: x > k, hip.PH_GE: x >= k, hip.PH_EQ: x == k}[op]
    return m


def want(c, valid, case, b, e):
    """{key: (first row, [sum | min | None per aggregate], [count per aggregate])} over rows [b, e) in Python integers"""
    preds, groups, aggs, _ = CASES[case]
    m = selected(c, preds)
    m[:b] = False
    m[e:] = False
    keys = np.stack([c[g].astype(np.int64) for g in groups], axis=1) if groups else np.zeros((N, 0), np.int64)
    out = {}
    for key in sorted(set(map(tuple, keys[m].tolist()))):
        g = m & np.all(keys == np.array(key, np.int64), axis=1) if groups else m
        vals, cnts = [], []
        for kind, prog, val in aggs:
            ok = g & valid if prog and prog[0] == X(NQ) else g
            cnts.append(int(ok.sum()))
            if kind in (hip.PH_A_COUNT_STAR, hip.PH_A_COUNT):
                vals.append(None)
            else:
                v = val(c)[ok]
                vals.append(int(min(v)) if kind == hip.PH_A_MIN else int(sum(v)))
        out[key] = (int(np.flatnonzero(g)[0]), vals, cnts)
    return out


def got(r, case, first_rows):
    aggs = CASES[case][2]
    out = {}
    for g in range(r["ngroups"]):
        vals = [None if kind in (hip.PH_A_COUNT_STAR, hip.PH_A_COUNT) else int(r["sum"][g][a]) for a, (kind, _, _) in enumerate(aggs)]
        out[tuple(int(k) for k in r["keys"][g])] = (int(r["first_row"][g]) if first_rows else None, vals, [int(x) for x in r["count"][g]])
    return out


def make_plan(ctx, t, case):
    preds, groups, aggs, _ = CASES[case]
    return hip.ScanPlan(ctx, t, [hip.pred(col, op, hip.const(typ, i=v, f=v) if typ == hip.PH_F32 else hip.const(typ, i=v)) for col, op, typ, v in preds],
                        groups, [hip.aggexpr(kind, prog) for kind, prog, _ in aggs])


def run_case(ctx, t, c, valid, case):
    """[kind, variant, bytes_per_row, row_body] of the case's plan, after checking its results over both row ranges"""
    pl = make_plan(ctx, t, case)
    kind, variant = pl.kind, pl.variant
    # the grouped fused kinds hand back the first selected row of every group; filter_sumprod has one group and no such word, the generic
    # chain orders its groups by it without reporting it
    first_rows = kind in ("lowcard_chain", "jit")
    narrow = kind in ("filter_sumprod", "lowcard_chain") and variant != "wide"
    for b, e in [(0, N), (7 if narrow else 8, N - 3)]:
        pl.run(b, e)
        w = want(c, valid, case, b, e)
        if not first_rows:
            w = {k: (None, v[1], v[2]) for k, v in w.items()}
        assert got(pl.fetch(), case, first_rows) == w, (case, b, e)
    row = [kind, variant, pl.bytes_per_row, pl.row_body]
    pl.free()
    return row


def run_all(ctx, nojit):
    c, valid = columns()
    t = make_table(ctx, c, valid)
    out = {case: run_case(ctx, t, c, valid, case) for case, spec in CASES.items() if spec[3] or not nojit}
    t.free()
    return out


# recorded from the commit before scan_lower.h / scan_inst.h existed: [kind, variant, bytes_per_row, row_body]
EXPECT = {
    "narrow": {
        "q6": ["filter_sumprod", "narrow32", 8, "columns"],
        "q6_pred_on_first_factor": ["filter_sumprod", "narrow32", 8, "columns"],
        "q6_one_int32_pred_column": ["filter_sumprod", "narrow_rt", 9, "columns"],
        "three_int32_pred_columns": ["jit", "jit", 28, "columns"],
        "two_sumprod_pairs": ["jit", "jit", 32, "columns"],
        "count_star_alone": ["jit", "jit", 4, "columns"],
        "q1": ["lowcard_chain", "narrow32_lean", 11, "columns"],
        "q1_reversed": ["lowcard_chain", "narrow32_lean", 11, "columns"],
        "q1_no_tax_chain": ["jit", "jit", 26, "columns"],
        "q1_no_quantity": ["jit", "jit", 30, "columns"],
        "q1_singles_e_d": ["jit", "jit", 22, "columns"],
        "q1_singles_d_e": ["jit", "jit", 22, "columns"],
        "chain_first_factor_1_minus_d": ["jit", "jit", 30, "columns"],
        "f1_multiplier_1e6": ["lowcard_chain", "narrow32_lean", 11, "columns"],
        "f1_multiplier_1e7": ["lowcard_chain", "narrow32", 11, "columns"],
        "one_group_column": ["jit", "jit", 13, "columns"],
        "two_range_columns_two_groups": ["jit", "jit", 34, "columns"],
        "min_of_column": ["jit", "jit", 13, "columns"],
        "min_of_expression": ["generic", "generic", 0, "columns"],
        "nullable_argument": ["generic", "generic", 0, "columns"],
    },
    "narrow_nojit": {
        "q1": ["lowcard_chain", "narrow32_lean", 11, "columns"],
        "q1_reversed": ["lowcard_chain", "narrow32_lean", 11, "columns"],
        "q1_no_tax_chain": ["lowcard_chain", "narrow_rt", 14, "columns"],
        "q1_no_quantity": ["lowcard_chain", "narrow_rt", 12, "columns"],
        "q1_singles_e_d": ["lowcard_chain", "narrow_rt", 15, "columns"],
        "q1_singles_d_e": ["lowcard_chain", "narrow_rt", 12, "columns"],
        "chain_first_factor_1_minus_d": ["generic", "generic", 0, "columns"],
        "f1_multiplier_1e6": ["lowcard_chain", "narrow32_lean", 11, "columns"],
        "f1_multiplier_1e7": ["lowcard_chain", "narrow32", 11, "columns"],
        "two_range_columns_two_groups": ["generic", "generic", 0, "columns"],
    },
    "wide": {
        "q6": ["filter_sumprod", "wide", 24, "columns"],
        "q6_pred_on_first_factor": ["filter_sumprod", "wide", 24, "columns"],
        "q6_one_int32_pred_column": ["filter_sumprod", "wide", 24, "columns"],
        "three_int32_pred_columns": ["jit", "jit", 28, "columns"],
        "two_sumprod_pairs": ["jit", "jit", 32, "columns"],
        "count_star_alone": ["jit", "jit", 4, "columns"],
        "q1": ["lowcard_chain", "wide", 34, "columns"],
        "q1_reversed": ["lowcard_chain", "wide", 34, "columns"],
        "q1_no_tax_chain": ["jit", "jit", 26, "columns"],
        "q1_no_quantity": ["jit", "jit", 30, "columns"],
        "q1_singles_e_d": ["jit", "jit", 22, "columns"],
        "q1_singles_d_e": ["jit", "jit", 22, "columns"],
        "chain_first_factor_1_minus_d": ["jit", "jit", 30, "columns"],
        "f1_multiplier_1e6": ["lowcard_chain", "wide", 34, "columns"],
        "f1_multiplier_1e7": ["lowcard_chain", "wide", 34, "columns"],
        "one_group_column": ["jit", "jit", 13, "columns"],
        "two_range_columns_two_groups": ["jit", "jit", 34, "columns"],
        "min_of_column": ["jit", "jit", 13, "columns"],
        "min_of_expression": ["generic", "generic", 0, "columns"],
        "nullable_argument": ["generic", "generic", 0, "columns"],
    },
    "wide_nojit": {
        "q1": ["lowcard_chain", "wide", 34, "columns"],
        "q1_reversed": ["lowcard_chain", "wide", 34, "columns"],
        "q1_no_tax_chain": ["lowcard_chain", "wide", 34, "columns"],
        "q1_no_quantity": ["lowcard_chain", "wide", 34, "columns"],
        "q1_singles_e_d": ["lowcard_chain", "wide", 34, "columns"],
        "q1_singles_d_e": ["lowcard_chain", "wide", 34, "columns"],
        "chain_first_factor_1_minus_d": ["generic", "generic", 0, "columns"],
        "f1_multiplier_1e6": ["lowcard_chain", "wide", 34, "columns"],
        "f1_multiplier_1e7": ["lowcard_chain", "wide", 34, "columns"],
        "two_range_columns_two_groups": ["generic", "generic", 0, "columns"],
    },
}


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in ("PH_SCAN_JIT", "PH_SCAN_GRID", "PH_SCAN_HIST", "PH_SCAN_UNROLL"):
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def wide():
    """both tables under PH_NARROW=0, from a child process (every result checked against numpy there)"""
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"scan_shapes_child_{os.getpid()}.json")
    env = {k: v for k, v in os.environ.items() if k not in ("PH_SCAN_JIT", "PH_SCAN_GRID", "PH_SCAN_HIST", "PH_SCAN_UNROLL")}
    subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(env, PH_NARROW="0"), check=True, timeout=300)
    with open(out) as f:
        res = json.load(f)
    os.remove(out)
    return res


def test_shapes_with_narrowed_copies(ctx):
    assert run_all(ctx, False) == EXPECT["narrow"]


def test_shapes_with_narrowed_copies_without_code_generation(ctx, monkeypatch):
    monkeypatch.setenv("PH_SCAN_JIT", "0")
    assert run_all(ctx, True) == EXPECT["narrow_nojit"]


def test_shapes_over_wide_columns(wide):
    assert wide["jit"] == EXPECT["wide"]


def test_shapes_over_wide_columns_without_code_generation(wide):
    assert wide["nojit"] == EXPECT["wide_nojit"]


def test_table_has_the_edges_the_cases_need():
    c, valid = columns()
    assert N % 4096 == 5 and not valid.all() and valid[:2].all()
    for case in CASES:
        for b, e in [(0, N), (8, N - 3)]:
            w = want(c, valid, case, b, e)
            assert len(w) == 2 ** len(CASES[case][1]), case   # every group has rows: an empty one would hide its accumulators
    # rows that the shorter range leaves out are selected rows of Q1's predicate
    assert selected(c, SHIP_LE)[:7].any() and selected(c, SHIP_LE)[N - 3:].any()


if __name__ == "__main__":   # the child of `wide`: a fresh process, since PH_NARROW is read once
    _ctx = hip.Ctx(0)
    _res = {"jit": run_all(_ctx, False)}
    os.environ["PH_SCAN_JIT"] = "0"
    _res["nojit"] = run_all(_ctx, True)
    _ctx.close()
    with open(sys.argv[1], "w") as _f:
        json.dump(_res, _f)
