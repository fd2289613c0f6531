"""Inputs and plain references of the expression-layer tests (test_gpu_expr_edges.py, test_gpu_plan_exprs.py; checked on their own,
without a device, by test_expr_edges_reference.py).

Nothing here restates the arithmetic a kernel does: the calendar comes from numpy's datetime64 units (no era / day-of-era formula),
the casts of decimals from `float(Fraction)` (select_edges.cast_f64), float32 / float64 arithmetic from numpy's IEEE operations —
which the reference test checks against exact `Fraction` rounding (f32_of_fraction) —, decimal programs from Python ints
(domain_edges.eval_program, the evaluator behind domain_edges.expected_values)."""
from fractions import Fraction

import numpy as np

import domain_edges as DE
import select_edges as SE
from plan_amd import hip

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
SHIFT = 719468        # days from 0000-03-01 to 1970-01-01: what civil_from_days adds first
ERA = 146097          # days of 400 Gregorian years
DAY_0001, DAY_9999 = -719162, 2932896    # 0001-01-01 and 9999-12-31


# ------------------------------------------------------------------ dates
def civil_parts(days):
    """(year, month, day) as int64 arrays of int32 days since 1970-01-01, proleptic Gregorian: numpy truncates a datetime64[D] to its
    month and its year; the parts are differences of those (no division by 146097 or 1461 anywhere)"""
    d = np.asarray(days, dtype=np.int64).astype("datetime64[D]")
    mon = d.astype("datetime64[M]")
    yr = d.astype("datetime64[Y]")
    year = yr.astype(np.int64) + 1970
    month = mon.astype(np.int64) - yr.astype("datetime64[M]").astype(np.int64) + 1
    day = (d - mon.astype("datetime64[D]")).astype(np.int64) + 1
    return year, month, day


def _date_edges():
    named = []
    for c in (I32_MIN, I32_MAX):
        named += [c + k for k in range(-3, 4)]
    for c in (I32_MAX - SHIFT, -SHIFT):
        named += [c + k for k in range(-2, 3)]
    named += [DAY_0001, DAY_9999, 0, -1]
    k_lo, k_hi = -((-(I32_MIN + SHIFT)) // ERA), (I32_MAX + SHIFT) // ERA
    eras = [k * ERA - SHIFT + j for k in range(k_lo - 1, k_hi + 2) for j in (-1, 0, 1)]
    out, seen = [], set()
    for v in named + eras:
        if I32_MIN <= v <= I32_MAX and v not in seen:
            seen.add(v)
            out.append(v)
    return np.array(out, dtype=np.int32)


DATE_EDGES = _date_edges()              # the named edges first (22 of them), then every era boundary of the int32 domain +-1
N_NAMED_DATE_EDGES = 22
ALL_DAYS_0001_9999 = (DAY_0001, DAY_9999)   # np.arange(lo, hi + 1): 3 652 059 days


def date_selections(n, seed=0):
    """{name: int32 row ids} over a column of n rows: ascending, descending, rows repeated, a selection of one row"""
    rng = np.random.default_rng(seed + n)
    asc = np.flatnonzero(rng.random(n) < 0.5).astype(np.int32)
    return {"ascending": asc, "descending": asc[::-1].copy(), "repeated": rng.integers(0, n, n + 37).astype(np.int32),
            "one": np.array([n - 1], dtype=np.int32)}


# ------------------------------------------------------------------ FLOAT / DOUBLE programs
def f32_of_fraction(x):
    """the float32 nearest to an exact Fraction, ties to even, denormals and overflow to infinity included — integer arithmetic only"""
    x = Fraction(x)
    if x == 0:
        return np.float32(0.0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if a < Fraction(2) ** e:
        e -= 1                                   # 2^e <= a < 2^(e+1)
    e = max(e, -126)                             # below the smallest normal the spacing stays 2^-149
    unit = Fraction(2) ** (e - 23)
    q = a / unit
    m = q.numerator // q.denominator
    rem = q - m
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and m & 1):
        m += 1
    v = m * unit
    if v >= Fraction(2) ** 128:
        return np.float32(-np.inf if x < 0 else np.inf)
    return np.float32(float(-v if x < 0 else v))     # v has 24 significant bits: a double holds it exactly


def f64_of_fraction(x):
    """the float64 nearest to an exact Fraction (int / int true division is correctly rounded)"""
    x = Fraction(x)
    return np.float64(x.numerator / x.denominator)


def column(typ, values, scale=0, valid=None):
    """one operand column of float_program: values as a numpy integer array, valid a boolean array or None"""
    dt = np.int32 if typ in (hip.PH_I32, hip.PH_DATE) else np.int64
    return dict(type=typ, scale=scale, values=np.asarray(values, dtype=dt), valid=None if valid is None else np.asarray(valid, dtype=bool))


def cast_column(c, wide):
    """the binder's casts (function_cast.go:327-374): INTEGER / DATE / BIGINT -> float in one rounding; DECIMAL -> the nearest double of
    the decimal (select_edges.cast_f64: float(Fraction)), and for FLOAT that double narrowed"""
    v = c["values"]
    if c["type"] == hip.PH_DEC64:
        d = np.array([SE.cast_f64(x, c["scale"]) for x in v.tolist()], dtype=np.float64)
        return d if wide else d.astype(np.float32)
    assert c["type"] in (hip.PH_I32, hip.PH_DATE, hip.PH_I64), c["type"]
    return v.astype(np.float64 if wide else np.float32)


def hugeint_f32(v):
    """tryCastBigintToFloat32 (function_cast.go:365-374) for a HUGEINT that fits int64: Upper = 0 gives float32(Lower), Upper = -1 gives
    -float32(MaxUint64 - Lower) - 1 in float32 arithmetic; MaxUint64 - Lower = -v - 1. One rounding of the integer — no double between."""
    v = int(v)
    if v >= 0:
        return f32_of_fraction(v)
    with np.errstate(all="ignore"):
        return np.float32(-f32_of_fraction(-v - 1) - np.float32(1))


def hugeint_values():
    """scale-0 values above 2^53 beside float32 midpoints (select_edges.cast_inputs(0): every integer within a few double ulps of the
    midpoints of three binades): where one rounding and two can part"""
    v = SE.cast_inputs(0)
    return v[np.abs(v.astype(object)) >= SE.EXACT]


def float_program(prog, cols, wide):
    """ph_float_eval's program, step by step: (values, valid). Every float32 operation rounds to float32 (numpy's float32 arithmetic);
    `wide` runs it in float64. A literal is a float32 (widened for DOUBLE). Comparisons follow selectOperation: FLOAT has > >= <= as
    IEEE compares, DOUBLE has < as GreaterFloat(right, left) — false for a NaN left, true for a NaN right and a number left —, every
    other one is never true; they give 1.0 / 0.0. valid = no operand of the row is NULL."""
    dt = np.float64 if wide else np.float32
    n = len(cols[0]["values"])
    valid = np.ones(n, dtype=bool)
    st = []
    with np.errstate(all="ignore"):
        for op, col, ival, _ in prog:
            if op == hip.PH_X_COL:
                c = cols[col]
                st.append(cast_column(c, wide))
                if c["valid"] is not None:
                    valid &= c["valid"]
            elif op == hip.PH_X_CONST:
                k = np.array([ival & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0]
                st.append(np.full(n, k, dtype=np.float32).astype(dt))
            else:
                b, a = st.pop(), st.pop()
                assert a.dtype == dt and b.dtype == dt
                if op == hip.PH_X_ADD:
                    x = a + b
                elif op == hip.PH_X_SUB:
                    x = a - b
                elif op == hip.PH_X_MUL:
                    x = a * b
                elif op == hip.PH_X_DIV:
                    x = a / b
                elif wide:
                    hit = np.where(np.isnan(b), ~np.isnan(a), a < b) if op == hip.PH_X_LT else np.zeros(n, dtype=bool)
                    x = hit.astype(dt)
                else:
                    hit = {hip.PH_X_GT: a > b, hip.PH_X_GE: a >= b, hip.PH_X_LE: a <= b}.get(op, np.zeros(n, dtype=bool))
                    x = hit.astype(dt)
                assert x.dtype == dt
                st.append(x)
    assert len(st) == 1
    return st[0], valid


def float_truth(prog, cols, wide):
    """the INTEGER truth of a program that ends in a comparison: 1 where it holds and no operand is NULL"""
    v, valid = float_program(prog, cols, wide)
    return ((v != 0) & valid).astype(np.int32)


def bits(a):
    """bit patterns of a float32 / float64 array with every NaN mapped to one pattern: equal arrays = equal values, -0.0 apart from 0.0"""
    a = np.ascontiguousarray(a)
    u = a.view(np.uint32 if a.dtype == np.float32 else np.uint64).copy()
    u[np.isnan(a)] = u.dtype.type(0x7FC00000 if a.dtype == np.float32 else 0x7FF8000000000000)
    return u


F32_TINY = np.float32(2.0 ** -126)        # the smallest normal
F32_DENORM = np.float32(2.0 ** -149)      # the smallest denormal
FLOAT_LITERALS = (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(-0.0), np.float32(0.0), F32_TINY, F32_DENORM,
                  np.float32(-F32_DENORM), np.float32(1.0), np.float32(0.2))
INT32_FLOAT_EDGES = sorted({s * (2 ** 24 + d) for s in (1, -1) for d in (-1, 0, 1, 2, 3)} | {I32_MAX, -I32_MAX, I32_MIN, 0, 1, -1, 3, -7})
INT64_FLOAT_EDGES = sorted({s * (2 ** 53 + d) for s in (1, -1) for d in (-2, -1, 0, 1, 2, 3)} | {s * (2 ** 24 + d) for s in (1, -1) for d in (-1, 1)}
                           | {s * ((2 ** 24 + 1) * 2 ** 36 + d) for s in (1, -1) for d in (-1, 0, 1)}      # a float32 midpoint at 2^60, +-1
                           | {I64_MAX, -I64_MAX, I64_MIN, 0, 5, -5})


# ------------------------------------------------------------------ decimal programs, WHEN trees and CASE
def decimal_program(prog, cols, scales, rows=None):
    """domain_edges.eval_program over the rows (all, or the listed ones) of cols = {index: python list, None = NULL}: per row
    (value, scale), (None, scale) for a NULL operand, or "overflow" """
    n = len(next(iter(cols.values())))
    rows = range(n) if rows is None else rows
    return [DE.eval_program(prog, {c: v[r] for c, v in cols.items()}, scales) for r in rows]


_CMP = {hip.PH_EQ: lambda a, b: a == b, hip.PH_NE: lambda a, b: a != b, hip.PH_LT: lambda a, b: a < b, hip.PH_LE: lambda a, b: a <= b,
        hip.PH_GT: lambda a, b: a > b, hip.PH_GE: lambda a, b: a >= b}


def when_rows(tree, cols, n):
    """a WHEN / filter tree of hip.bool_tree's nested tuples, with plain Python values for the constants (same scale as the column):
    ("cmp", col, op, value) | ("colcmp", col, op, col2) | ("in", col, [values]) | ("and", ...) | ("or", ...). A NULL operand makes a
    comparison false (it is a select: there is no NOT above it). Returns a list of n bools."""
    kind = tree[0]
    if kind == "cmp":
        return [cols[tree[1]][r] is not None and _CMP[tree[2]](cols[tree[1]][r], tree[3]) for r in range(n)]
    if kind == "colcmp":
        return [cols[tree[1]][r] is not None and cols[tree[3]][r] is not None and _CMP[tree[2]](cols[tree[1]][r], cols[tree[3]][r]) for r in range(n)]
    if kind == "in":
        return [cols[tree[1]][r] is not None and cols[tree[1]][r] in tree[2] for r in range(n)]
    kids = [when_rows(k, cols, n) for k in tree[1:]]
    return [all(k[r] for k in kids) if kind == "and" else any(k[r] for k in kids) for r in range(n)]


def is_int_literal(prog):
    return len(prog) == 1 and prog[0][0] == hip.PH_X_CONST and prog[0][3] == 0


def case_rows(when, then_prog, else_prog, cols, scales):
    """CASE WHEN .. THEN .. ELSE .. END as executeCase runs it: THEN is evaluated on the WHEN-true rows ONLY and ELSE on the others, so a
    row's overflow counts only in the branch that row takes. An integer ELSE literal is multiplied to the THEN scale (an overflow of
    that cast fails the expression whatever the rows). `when` is the list of bools (when_rows). Returns (values, scale), "overflow", or
    "unsupported" when the branches' scales differ."""
    n = len(when)
    t_rows = [r for r in range(n) if when[r]]
    e_rows = [r for r in range(n) if not when[r]]
    probe = {c: 0 for c in scales}
    t_scale = DE.eval_program(then_prog, probe, scales)[1]
    if is_int_literal(else_prog):
        k = else_prog[0][2] * 10 ** t_scale
        if not DE.fits64(k):
            return "overflow"
        e_vals = [(k, t_scale)] * len(e_rows)
    else:
        if DE.eval_program(else_prog, probe, scales)[1] != t_scale:
            return "unsupported"
        e_vals = decimal_program(else_prog, cols, scales, e_rows)
    t_vals = decimal_program(then_prog, cols, scales, t_rows)
    if "overflow" in t_vals or "overflow" in e_vals:
        return "overflow"
    out = [None] * n
    for r, v in zip(t_rows, t_vals):
        out[r] = v[0]
    for r, v in zip(e_rows, e_vals):
        out[r] = v[0]
    return out, t_scale


def group_by(keys, args, kinds):
    """a dict group-by over exact ints: keys = per-row tuples, args = one per-row list per aggregate (None = NULL, skipped),
    kinds = hip.PH_A_* per aggregate. {key: [(sum or min or max or None, count)] per aggregate} — AVG is its sum and its count, COUNT
    and COUNT_STAR carry only the count (of the non-NULL values, of the rows)."""
    groups = {}
    for r, k in enumerate(keys):
        g = groups.setdefault(k, [[None, 0] for _ in kinds])
        for a, kind in enumerate(kinds):
            if kind == hip.PH_A_COUNT_STAR:
                g[a][1] += 1
                continue
            v = args[a][r]
            if v is None:
                continue
            s = g[a][0]
            if kind == hip.PH_A_COUNT:
                pass
            elif kind == hip.PH_A_MIN:
                g[a][0] = v if s is None else min(s, v)
            elif kind == hip.PH_A_MAX:
                g[a][0] = v if s is None else max(s, v)
            else:
                g[a][0] = v if s is None else s + v
            g[a][1] += 1
    return {k: [tuple(x) for x in g] for k, g in groups.items()}
