"""The references of the expression-layer tests, checked without a device: the datetime64 calendar against datetime.date, the fixed
host twins of civil_from_days against it on the date edges, the parent's 32-bit formula failing exactly on the top 719 468 days (so the
GPU test can fail), numpy's float32 / float64 arithmetic and casts against exact Fraction rounding, the HUGEINT route against the
DECIMAL route, and CASE / WHEN / group-by on hand-made rows."""
import ctypes
import datetime
from fractions import Fraction

import numpy as np

import domain_edges as DE
import expr_edges as EE
import select_edges as SE
from plan_amd import hip, tpchgen

F32 = np.float32
HUGEINT_DIFFER, HUGEINT_VALUES = 4368, 26335     # the count DESIGN.md quotes (section 4.2, Filter)


def test_civil_parts_is_the_calendar_of_datetime_date():
    days, want = [], []
    epoch = datetime.date(1970, 1, 1).toordinal()
    for y in range(1, 10000):
        for m in range(1, 13):
            first = datetime.date(y, m, 1)
            last = datetime.date(9999, 12, 31) if (y, m) == (9999, 12) else datetime.date(y + (m == 12), m % 12 + 1, 1) - datetime.timedelta(1)
            for dt in (first, last):
                days.append(dt.toordinal() - epoch)
                want.append((dt.year, dt.month, dt.day))
        feb28 = datetime.date(y, 2, 28)
        for dt in (feb28, feb28 + datetime.timedelta(1)):      # Feb 29 in a leap year, Mar 1 otherwise
            days.append(dt.toordinal() - epoch)
            want.append((dt.year, dt.month, dt.day))
    assert days[0] == EE.DAY_0001 and max(days) == EE.DAY_9999 and len(days) == 9999 * 26
    # the day numbers back through date.fromordinal: the same dates, and civil_parts agrees with them
    back = [datetime.date.fromordinal(x + epoch) for x in days]
    assert [(dt.year, dt.month, dt.day) for dt in back] == want
    y, m, d = EE.civil_parts(np.array(days))
    assert list(zip(y.tolist(), m.tolist(), d.tolist())) == want
    assert sum(1 for w in want if w[1:] == (2, 29)) == 2 * 2424                 # 2424 leap days, each as the month's last day and as Feb 28 + 1


def test_date_edges_hold_what_the_issue_lists():
    e = EE.DATE_EDGES
    assert e.dtype == np.int32 and len(set(e.tolist())) == len(e)
    named = set(e[:EE.N_NAMED_DATE_EDGES].tolist())
    for c in (EE.I32_MIN, EE.I32_MAX):
        assert {c + k for k in range(-3, 4) if EE.I32_MIN <= c + k <= EE.I32_MAX} <= named
    assert {EE.I32_MAX - EE.SHIFT + k for k in range(-2, 3)} | {-EE.SHIFT + k for k in range(-2, 3)} | {EE.DAY_0001, EE.DAY_9999, 0, -1} == \
        named - {c + k for c in (EE.I32_MIN, EE.I32_MAX) for k in range(-3, 4)}
    have = set(e.tolist())
    k = -14700
    count = 0
    while k * EE.ERA - EE.SHIFT <= EE.I32_MAX + 1:
        for j in (-1, 0, 1):
            v = k * EE.ERA - EE.SHIFT + j
            if EE.I32_MIN <= v <= EE.I32_MAX:
                assert v in have
                count += 1
        k += 1
    assert count > 3 * 29000 and len(e) >= 257
    # the calendar at the edges of the domain, by hand: 0000-03-01 is z = 0; the era before it ends on Feb 29 of year 0
    assert [int(p[0]) for p in EE.civil_parts([-EE.SHIFT])] == [0, 3, 1]
    assert [int(p[0]) for p in EE.civil_parts([-EE.SHIFT - 1])] == [0, 2, 29]
    assert [int(p[0]) for p in EE.civil_parts([EE.DAY_9999])] == [9999, 12, 31]
    assert [int(p[0]) for p in EE.civil_parts([EE.I32_MAX])] == [5881580, 7, 11]
    assert [int(p[0]) for p in EE.civil_parts([EE.I32_MIN])] == [-5877641, 6, 23]


def _host_twin(days):
    fn = tpchgen.lib().tpchgen_civil_from_days
    fn.restype = None
    out = []
    for x in days.tolist():
        y, m, d = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        fn(ctypes.c_int32(x), ctypes.byref(y), ctypes.byref(m), ctypes.byref(d))
        out.append((y.value, m.value, d.value))
    return out


def test_the_host_twin_of_civil_from_days_is_exact_on_the_date_edges():
    y, m, d = EE.civil_parts(EE.DATE_EDGES)
    assert _host_twin(EE.DATE_EDGES) == list(zip(y.tolist(), m.tolist(), d.tolist()))


def civil_from_days_wrapping(days):
    """the formula with `z += 719468` in 32 bits, as the device ran it before the fix (numpy int32 arithmetic wraps)"""
    with np.errstate(over="ignore"):
        z = (np.asarray(days, dtype=np.int64) + EE.SHIFT).astype(np.int32).astype(np.int64)     # the wrap
    era = np.where(z >= 0, z, z - 146096) // 146097
    era = np.where((z < 0) & ((z - 146096) % 146097 != 0), era + 1, era)                            # C division truncates
    doe = z - era * 146097
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
    mp = (5 * doy + 2) // 153
    d = doy - (153 * mp + 2) // 5 + 1
    m = np.where(mp < 10, mp + 3, mp - 9)
    return yoe + era * 400 + (m <= 2), m, d


def test_the_32_bit_formula_fails_on_exactly_the_top_719468_days():
    """what makes the GPU date test able to fail: sampled over the domain (every edge, every 997th day, the whole top million), the
    wrapping formula is wrong for the days above INT32_MAX - 719468 and for no other"""
    days = np.unique(np.concatenate([EE.DATE_EDGES.astype(np.int64), np.arange(EE.I32_MIN, EE.I32_MAX, 997, dtype=np.int64),
                                     np.arange(EE.I32_MAX - 1_000_000, EE.I32_MAX + 1, dtype=np.int64)]))
    y, m, d = EE.civil_parts(days)
    wy, wm, wd = civil_from_days_wrapping(days)
    wrong = (wy != y) | (wm != m) | (wd != d)
    assert np.array_equal(wrong, days > EE.I32_MAX - EE.SHIFT)
    assert int(wrong.sum()) == EE.SHIFT


# ------------------------------------------------------------------ float programs
def test_f32_of_fraction_on_hand_made_roundings():
    assert EE.f32_of_fraction(Fraction(2 ** 24 + 1)) == F32(2 ** 24)                 # a tie goes to the even mantissa
    assert EE.f32_of_fraction(Fraction(2 ** 24 + 3)) == F32(2 ** 24 + 4)
    assert EE.f32_of_fraction(Fraction(2 ** 25 + 2) + Fraction(1, 10 ** 9)) == F32(2 ** 25 + 4)
    assert EE.f32_of_fraction(Fraction(1, 2 ** 149)) == EE.F32_DENORM
    assert EE.f32_of_fraction(Fraction(1, 2 ** 150)) == F32(0.0)                     # the tie below the smallest denormal: to even, 0
    assert EE.f32_of_fraction(Fraction(3, 2 ** 150)) == F32(2.0 ** -148)
    assert EE.f32_of_fraction(Fraction(2 ** 128)) == F32(np.inf) and EE.f32_of_fraction(-Fraction(2 ** 128)) == F32(-np.inf)
    assert EE.f32_of_fraction(Fraction(2 ** 128) - Fraction(2 ** 103)) == F32(np.inf)     # half an ulp above the largest float: to even, up
    assert EE.f32_of_fraction(Fraction(1, 5)) == F32(0.2)


def test_integer_and_decimal_casts_against_exact_rounding():
    for typ, vals in ((hip.PH_I32, EE.INT32_FLOAT_EDGES), (hip.PH_DATE, EE.INT32_FLOAT_EDGES), (hip.PH_I64, EE.INT64_FLOAT_EDGES)):
        c = EE.column(typ, vals)
        assert EE.bits(EE.cast_column(c, False)).tolist() == [int(EE.bits(np.array([EE.f32_of_fraction(v)]))[0]) for v in vals]
        assert EE.cast_column(c, True).tolist() == [float(EE.f64_of_fraction(v)) for v in vals]
    for scale in (0, 2, 4):
        vals = SE.cast_inputs(scale)[::7]
        c = EE.column(hip.PH_DEC64, vals, scale)
        want64 = [EE.f64_of_fraction(Fraction(int(v), 10 ** scale)) for v in vals.tolist()]
        assert EE.cast_column(c, True).tolist() == [float(x) for x in want64]
        # FLOAT: the double, narrowed — two roundings, not the float32 nearest to the decimal
        assert EE.cast_column(c, False).tolist() == [float(EE.f32_of_fraction(Fraction(float(x)))) for x in want64]
    # the int64 column rounds ONCE: beside a float32 midpoint above 2^53 that differs from going through the double
    v = (2 ** 24 + 1) * 2 ** 36 + 1
    once, twice = EE.cast_column(EE.column(hip.PH_I64, [v]), False)[0], EE.cast_column(EE.column(hip.PH_DEC64, [v], 0), False)[0]
    assert once == F32((2 ** 24 + 2) * 2.0 ** 36) and twice == F32(2.0 ** 60)


def test_float_program_steps_round_like_exact_arithmetic():
    q = EE.column(hip.PH_I32, [3, 7, 2 ** 24 + 1, -5, 0, 1])
    s = EE.column(hip.PH_DEC64, [10, 333, 7, 1, 0, 3], 2)
    prog = [hip.X_COL(0), hip.X_F32(0.2), hip.X_MUL, hip.X_COL(1), hip.X_OP(hip.PH_X_DIV)]           # (q * 0.2f) / s
    got, valid = EE.float_program(prog, [q, s], False)
    k = Fraction(float(F32(0.2)))
    for i, (a, b) in enumerate(zip(q["values"].tolist(), s["values"].tolist())):
        fa = Fraction(float(EE.f32_of_fraction(a)))
        fb = Fraction(float(F32(SE.cast_f64(b, 2))))
        prod = Fraction(float(EE.f32_of_fraction(fa * k)))
        if fb == 0:
            assert np.isnan(got[i]) if prod == 0 else np.isinf(got[i])
        else:
            assert got[i] == EE.f32_of_fraction(prod / fb), i
    assert valid.all() and got.dtype == np.float32
    got64, _ = EE.float_program(prog, [q, s], True)
    assert got64.dtype == np.float64 and got64[0] == EE.f64_of_fraction(Fraction(float(EE.f64_of_fraction(3 * k))) / Fraction(1, 10))
    # a product in the denormal range is kept (numpy must not flush): 2^-126 * 2^-3 = 2^-129, and 3 * 2^-149
    one = EE.column(hip.PH_I32, [1, 3])
    v, _ = EE.float_program([hip.X_COL(0), hip.X_F32(EE.F32_TINY), hip.X_MUL, hip.X_F32(0.125), hip.X_MUL], [one], False)
    assert v.tolist() == [2.0 ** -129, 3 * 2.0 ** -129]
    v, _ = EE.float_program([hip.X_COL(0), hip.X_F32(EE.F32_DENORM), hip.X_MUL], [one], False)
    assert v.tolist() == [2.0 ** -149, 3 * 2.0 ** -149]


def test_float_comparisons_follow_select_operation():
    nan, inf = float("nan"), float("inf")
    a = EE.column(hip.PH_I32, [1, 2, 3, 0, 0])
    # x / y with y = 0 makes the specials: 1/0 = inf, 0/0 = NaN
    z = EE.column(hip.PH_I32, [1, 2, 3, 0, 1])

    def run(op, lit, wide):
        return EE.float_truth([hip.X_COL(0), hip.X_F32(lit), hip.X_OP(op)], [a], wide).tolist()
    assert run(hip.PH_X_GT, 2.0, False) == [0, 0, 1, 0, 0] and run(hip.PH_X_GE, 2.0, False) == [0, 1, 1, 0, 0] and run(hip.PH_X_LE, 2.0, False) == [1, 1, 0, 1, 1]
    assert run(hip.PH_X_LT, 2.0, False) == [0] * 5                                  # FLOAT has no <
    assert run(hip.PH_X_LT, 2.0, True) == [1, 0, 0, 1, 1]
    for op in (hip.PH_X_GT, hip.PH_X_GE, hip.PH_X_LE):
        assert run(op, 2.0, True) == [0] * 5                                        # DOUBLE has only <
        assert run(op, nan, False) == [0] * 5
    assert run(hip.PH_X_LT, nan, True) == [1] * 5                                   # GreaterFloat(NaN, number)
    nan_left = EE.float_truth([hip.X_COL(0), hip.X_COL(1), hip.X_OP(hip.PH_X_DIV), hip.X_F32(1.0), hip.X_OP(hip.PH_X_LT)], [a, EE.column(hip.PH_I32, [0] * 5)], True)
    assert nan_left.tolist() == [0] * 5                                             # inf < 1 and NaN < 1: never
    both = EE.float_truth([hip.X_COL(0), hip.X_COL(1), hip.X_OP(hip.PH_X_DIV), hip.X_F32(nan), hip.X_OP(hip.PH_X_LT)], [a, EE.column(hip.PH_I32, [0] * 5)], True)
    assert both.tolist() == [1, 1, 1, 0, 0]                                         # NaN < NaN is false, inf < NaN true
    v, _ = EE.float_program([hip.X_COL(0), hip.X_COL(1), hip.X_OP(hip.PH_X_DIV)], [z, EE.column(hip.PH_I32, [0, 0, 0, 0, -1])], False)
    assert v[:3].tolist() == [inf] * 3 and np.isnan(v[3]) and v[4] == -1.0
    # NULLs: the value is NULL, the truth 0 — also where the comparison itself would hold
    nul = EE.column(hip.PH_I32, [1, 1, 1, 1, 1], valid=[True, False, True, False, True])
    other = EE.column(hip.PH_DEC64, [0, 0, 0, 0, 0], 2, valid=[True, True, False, False, True])
    prog = [hip.X_COL(0), hip.X_COL(1), hip.X_OP(hip.PH_X_GT)]
    assert EE.float_truth(prog, [nul, other], False).tolist() == [1, 0, 0, 0, 1]
    assert EE.float_program(prog, [nul, other], False)[1].tolist() == [True, False, False, False, True]
    assert EE.bits(np.array([np.nan, -np.nan, 0.0, -0.0], dtype=np.float32)).tolist() == [0x7FC00000, 0x7FC00000, 0, 0x80000000]


def test_the_hugeint_route_and_the_decimal_route_part_beside_midpoints():
    """tryCastBigintToFloat32 rounds the integer once, the DECIMAL(p,0) route twice (nearest double, then float32): counted on values
    beside float32 midpoints above 2^53. DESIGN.md records the count and the example."""
    vals = EE.hugeint_values()
    huge = np.array([EE.hugeint_f32(v) for v in vals.tolist()], dtype=np.float32)
    dec = EE.cast_column(EE.column(hip.PH_DEC64, vals, 0), False)
    differ = np.flatnonzero(EE.bits(huge) != EE.bits(dec))
    i = differ[np.argmax(vals[differ] > 0)]
    print(f"HUGEINT route vs DECIMAL route: {len(differ)} of {len(vals)} crafted values differ; e.g. {int(vals[i])}: "
          f"{float(huge[i])!r} against {float(dec[i])!r}")
    assert len(vals) > 10_000 and 0 < len(differ) < len(vals)
    assert (len(differ), len(vals)) == (HUGEINT_DIFFER, HUGEINT_VALUES)
    # each differing value is one float32 ulp apart, and the HUGEINT route is the correctly rounded one of the two
    for j in differ[:50].tolist():
        assert huge[j] == EE.f32_of_fraction(int(vals[j]) if vals[j] >= 0 else -int(vals[j]) - 1) * (1 if vals[j] >= 0 else -1)
        assert np.nextafter(dec[j], huge[j]) == huge[j]
    assert EE.hugeint_f32(-1) == F32(-1.0) and EE.hugeint_f32(5) == F32(5.0) and EE.hugeint_f32(-(2 ** 24) - 4) == F32(-(2 ** 24) - 4)
    # a negative value takes two float32 steps there: -float32(2^24 + 1) - 1 = -(2^24) - 1, a tie that goes to -(2^24) — by hand
    assert EE.hugeint_f32(-(2 ** 24) - 2) == F32(-(2 ** 24))



# ------------------------------------------------------------------ decimal programs and CASE
def test_case_rows_evaluates_each_branch_on_its_own_rows():
    big = DE.I64_MAX // 100
    cols = {0: [1, 2, 3, None, 5], 1: [100, 200, big + 1, 400, 500]}
    scales = {0: 0, 1: 2}
    when = EE.when_rows(("cmp", 0, hip.PH_NE, 3), cols, 5)
    assert when == [True, True, False, False, True]                                  # the NULL makes the WHEN false
    then = [hip.X_COL(1), hip.X_CONST(100, 0), hip.X_MUL]                            # b * 100: row 2 would overflow, and does not take THEN
    vals, scale = EE.case_rows(when, then, [hip.X_CONST(-7)], cols, scales)
    assert scale == 2 and vals == [10000, 20000, -700, -700, 50000]
    assert EE.case_rows([True] * 5, then, [hip.X_CONST(-7)], cols, scales) == "overflow"
    assert EE.case_rows([not w for w in when], [hip.X_CONST(1, 2)], then, cols, scales)[0] == [10000, 20000, 1, 1, 50000]
    assert EE.case_rows([False] * 5, [hip.X_CONST(1, 2)], then, cols, scales) == "overflow"
    assert EE.case_rows(when, then, [hip.X_COL(1), hip.X_COL(1), hip.X_MUL], cols, scales) == "unsupported"   # scale 2 against 4
    assert EE.case_rows(when, [hip.X_COL(1), hip.X_COL(1), hip.X_MUL], [hip.X_CONST(10 ** 15)], {0: cols[0], 1: [1] * 5}, scales) == "overflow"
    assert EE.case_rows(when, [hip.X_CONST(1)], [hip.X_CONST(0)], cols, scales) == ([1, 1, 0, 0, 1], 0)
    tree = ("or", ("and", ("cmp", 0, hip.PH_GE, 2), ("colcmp", 1, hip.PH_GT, 0)), ("in", 0, [1, 9]))
    assert EE.when_rows(tree, cols, 5) == [True, True, True, False, True]


def test_decimal_program_and_group_by_on_hand_made_rows():
    cols = {0: [150, -250, None, DE.I64_MAX], 1: [10000, 20000, 30000, 2]}
    scales = {0: 2, 1: 4}
    prog = [hip.X_COL(0), hip.X_COL(1), hip.X_ADD]                                   # scale 2 + scale 4: the left side times 100
    assert EE.decimal_program(prog, cols, scales) == [(25000, 4), (-5000, 4), (None, 4), "overflow"]
    assert EE.decimal_program(prog, cols, scales, rows=[1]) == [(-5000, 4)]
    g = EE.group_by([(1,), (2,), (1,), (1,)], [[5, None, -7, None]] * 5 + [None],
                    [hip.PH_A_SUM, hip.PH_A_MIN, hip.PH_A_MAX, hip.PH_A_AVG, hip.PH_A_COUNT, hip.PH_A_COUNT_STAR])
    assert g == {(1,): [(-2, 2), (-7, 2), (5, 2), (-2, 2), (None, 2), (None, 3)], (2,): [(None, 0)] * 5 + [(None, 1)]}
