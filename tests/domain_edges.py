"""Case tables and arbitrary-precision references of the integer-domain edge tests (test_gpu_domain_edges_scan.py,
test_gpu_domain_edges_ops.py; checked on their own, without a device, by test_domain_edges_reference.py).

Every reference here is plain Python `int` / `fractions.Fraction` arithmetic over the values of the input arrays: numpy is used
only to hold the columns, to test predicates on them and to count how often each distinct row occurs (RowKinds) — never to
multiply or add what a kernel multiplies or adds, since int64 arithmetic wraps where these tests work."""
from fractions import Fraction

import numpy as np

from plan_amd import hip

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
PROOF_LIMIT = 4 * 10 ** 18   # ph_scan_plan_run: per-row bound x rows per workgroup < 4e18
TILE = 4096                  # the proof counts whole tiles: its must-admit rule holds for runs of at least this many rows

# ------------------------------------------------------------------ the fused scans' tables (lineitem's column order)
Q, E, D, T, K0, K1, P = range(7)
FS_P, FS_Q, FS_A, FS_B = range(4)
P_LO, P_HI = 9000, 9999      # the predicate's interval; rows 0 and 1 of every table lie outside it and pin the column ranges
N_LADDER = 1 << 20
# per-row magnitudes 2^k: a factor 16 apart from ~1e9 past 2^63, a factor 4 apart between 2^63 / n = 2^43 and 4e18 / 1024 ~ 2^51.8
LADDER_EXP = (30, 34, 38, 42, 44, 46, 48, 50, 52, 54, 58, 62, 66)
FORMS = ("n32", "n64", "wide")


def fits64(v):
    return I64_MIN <= v <= I64_MAX


class RowKinds:
    """The distinct rows of a table, each with its values as Python ints. A sum over rows [b, e) is then
    sum(count of the kind in [b, e) x the kind's term), all in Python ints; first(b, e) gives each kind's first row in the range."""

    def __init__(self, cols):
        self.names = list(cols)
        n = len(cols[self.names[0]])
        code, radix = np.zeros(n, np.int64), 1
        for name in self.names:     # one mixed-radix word per row: value - min where the ranges are small, the value's rank otherwise
            a = np.asarray(cols[name])
            lo, hi = col_range(a)
            if radix * (hi - lo + 1) < 2 ** 62:
                digit, card = a.astype(np.int64) - lo, hi - lo + 1
            else:
                u, digit = np.unique(a, return_inverse=True)
                digit, card = digit.reshape(-1), len(u)
            assert radix * card < 2 ** 62, "too many distinct rows for one word"
            code, radix = code * card + digit, radix * card
        _, idx, inv = np.unique(code, return_index=True, return_inverse=True)
        self.inv, self.first_of_kind = inv.reshape(-1), idx
        self.values = [{name: int(cols[name][i]) for name in self.names} for i in idx]
        self._cache = {}

    def extend(self, name, arr):
        """one more column that is constant within every kind (checked); the same object with the new values"""
        arr = np.asarray(arr)
        per_kind = arr[self.first_of_kind]
        assert np.array_equal(per_kind[self.inv], arr), f"column {name} varies within a kind"
        for v, x in zip(self.values, per_kind.tolist()):
            v[name] = x     # (cached runs hold these dicts: counts and first rows stay as they are)
        return self

    def runs(self, b, e):
        """[(values, count, first row)] of the kinds that occur in rows [b, e)"""
        if (b, e) not in self._cache:
            seg = self.inv[b:e]
            cnt = np.bincount(seg, minlength=len(self.values))
            kinds, first = np.unique(seg, return_index=True)
            self._cache[(b, e)] = [(self.values[k], int(cnt[k]), int(f) + b) for k, f in zip(kinds.tolist(), first.tolist())]
        return self._cache[(b, e)]


def rows_of(cols, b, e):
    """the literal form of RowKinds.runs: one entry per row (small tables)"""
    names = list(cols)
    lists = {k: np.asarray(cols[k][b:e]).tolist() for k in names}
    return [({k: lists[k][i] for k in names}, 1, b + i) for i in range(e - b)]


def lc_reference(runs, lo, hi, A1, B1, A2, B2):
    """lowcard_chain's result: [[first_row, [k0, k1], [Σq, Σe, Σe f1, Σe f1 f2, Σd], count]] in first-seen order,
    f1 = A1 + B1 d, f2 = A2 + B2 t"""
    groups = {}
    for v, cnt, first in runs:
        if not lo <= v["p"] <= hi:
            continue
        dp = v["e"] * (A1 + B1 * v["d"])
        terms = (v["q"], v["e"], dp, dp * (A2 + B2 * v["t"]), v["d"])
        g = groups.setdefault((v["k0"], v["k1"]), [first, [0] * 5, 0])
        g[0] = min(g[0], first)
        g[1] = [s + cnt * x for s, x in zip(g[1], terms)]
        g[2] += cnt
    return sorted([g[0], list(k), g[1], g[2]] for k, g in groups.items())


def fs_reference(runs, lo, hi, q_below):
    """filter_sumprod's result [Σ a b, count] over p in [lo, hi] and q < q_below; None when no row passes"""
    s = c = 0
    for v, cnt, _ in runs:
        if lo <= v["p"] <= hi and v["q"] < q_below:
            s += cnt * v["a"] * v["b"]
            c += cnt
    return [s, c] if c else None


def jit_reference(runs, lo, hi, A1, B1, A2, B2):
    """the generated plan of the ladder: [[first_row, [k0, k1], [Σ e f1 f2, Σe, MIN(e), MAX(d)], count]] in first-seen order"""
    groups = {}
    for v, cnt, first in runs:
        if not lo <= v["p"] <= hi:
            continue
        g = groups.setdefault((v["k0"], v["k1"]), [first, [0, 0, v["e"], v["d"]], 0])
        g[0] = min(g[0], first)
        g[1] = [g[1][0] + cnt * v["e"] * (A1 + B1 * v["d"]) * (A2 + B2 * v["t"]), g[1][1] + cnt * v["e"], min(g[1][2], v["e"]), max(g[1][3], v["d"])]
        g[2] += cnt
    return sorted([g[0], list(k), g[1], g[2]] for k, g in groups.items())


def col_range(a):
    return int(np.min(a)), int(np.max(a))


def affine_bound(A, B, rng):
    """scan_plan.hip affine_bound: max |A + B x| over the column's [min, max]"""
    return max(abs(A + B * rng[0]), abs(A + B * rng[1]))


def lc_row_bound(c, A1, B1, A2, B2):
    """the per-row bound ph_scan_plan_create derives for lowcard_chain from the column statistics"""
    be, b1, b2 = affine_bound(0, 1, col_range(c["e"])), affine_bound(A1, B1, col_range(c["d"])), affine_bound(A2, B2, col_range(c["t"]))
    return max(be * b1 * b2, be * b1, be, affine_bound(0, 1, col_range(c["d"])), affine_bound(0, 1, col_range(c["q"])))


def lc_form(c, A1, B1, A2, B2):
    """the form scan_plan.hip's rule picks over narrowed copies: the 32-bit multiply form when be, b1, b2 and be b1 are <= 2^31 - 1"""
    be, b1, b2 = affine_bound(0, 1, col_range(c["e"])), affine_bound(A1, B1, col_range(c["d"])), affine_bound(A2, B2, col_range(c["t"]))
    return "n32" if max(be, b1, b2, be * b1) <= I32_MAX else "n64"


def fs_row_bound(c):
    return affine_bound(0, 1, col_range(c["a"])) * affine_bound(0, 1, col_range(c["b"]))


def fs_form(c):
    return "n32" if max(affine_bound(0, 1, col_range(c["a"])), affine_bound(0, 1, col_range(c["b"]))) <= I32_MAX else "n64"


def must_admit(run_rows, bound):
    """no workgroup sees more rows than the run has, so the documented proof must let these through (runs of one tile or more)"""
    return run_rows >= TILE and run_rows * bound < PROOF_LIMIT


# ------------------------------------------------------------------ part A: the magnitude ladder

def lc_ladder_columns(form, n=N_LADDER):
    """Rows 2.. pass the predicate and hold e = max, d = min (f1 = A1 - d is then largest), t = max; rows 0 and 1 fail it and pin the other
    end of every range. n32: the width tuple (p 2, q 1, e 4, d 1, t 1) of the kernel instance compiled for lineitem, e f1 < 2^31;
    n64: e above 2^31 (64-bit products); wide: p spans 70 000 days, which denies it a copy, so the plan keeps the wide kernel."""
    i = np.arange(n)
    p = (P_LO + (i % 10) * 100).astype(np.int32)
    p[0], p[1] = P_LO - 1, (P_LO + 70_000 if form == "wide" else P_HI + 1)
    q = np.full(n, 50, np.int32)
    q[0] = 1
    e_hi = 2 ** 31 + 5 if form == "n64" else 1_000_000
    e = np.full(n, e_hi, np.int64)
    e[0] = e_hi - (200 if form == "n64" else 70_000)
    d = np.zeros(n, np.int64)
    d[1] = 10
    t = np.full(n, 8, np.int64)
    t[0] = 0
    return dict(p=p, q=q, e=e, d=d, t=t, k0=(i % 3).astype(np.uint8), k1=((i // 3) % 2).astype(np.uint8))


LC_A1, LC_B1 = 100, -1    # f1 = 1.00 - d at scale 2


def lc_ladder_steps(c, sign):
    """[(k, (A1, B1, A2, B2), per-row product of rows 2..)]: f2 = A2 + t chosen so that the product is the first multiple of e f1 at or above 2^k"""
    e, f1, t = int(c["e"][2]), LC_A1 + LC_B1 * int(c["d"][2]), int(c["t"][2])
    steps, seen = [], set()
    for k in LADDER_EXP:
        f2 = sign * max(1, -(-(2 ** k) // (e * f1)))
        if f2 in seen:
            continue
        seen.add(f2)
        steps.append((k, (LC_A1, LC_B1, f2 - t, 1), e * f1 * f2))
    return steps


def fs_ladder_shared(form, n=N_LADDER):
    """p, q, a of the filter_sumprod ladder (b changes per step). n32: the width tuple (p 2, q 1, b 1, a 4) compiled for lineitem"""
    i = np.arange(n)
    p = (P_LO + (i % 10) * 100).astype(np.int32)
    p[0], p[1] = P_LO - 1, (P_LO + 70_000 if form == "wide" else P_HI + 1)
    q = np.full(n, 50, np.int32)
    q[0] = 1
    a_hi = 2 ** 31 + 5 if form == "n64" else 1_000_000
    a = np.full(n, a_hi, np.int64)
    a[0] = a_hi - (200 if form == "n64" else 70_000)
    return dict(p=p, q=q, a=a)


def fs_ladder_steps(shared, sign):
    """[(k, b of rows 1.., b of row 0, per-row product)]: b = the first multiple at or above 2^k / a; row 0 (outside the predicate)
    holds a value up to 200 nearer zero, so b keeps a one-byte copy"""
    a = int(shared["a"][2])
    steps, seen = [], set()
    for k in LADDER_EXP:
        f = max(1, -(-(2 ** k) // a))
        if f in seen:
            continue
        seen.add(f)
        steps.append((k, sign * f, sign * (f - min(f - 1, 200)), a * sign * f))
    return steps


def fs_columns(shared, b, b0):
    col = np.full(len(shared["p"]), b, np.int64)
    col[0] = b0
    return dict(shared, b=col)


def check_ladder(name, steps, n):
    """conditions on one form's ladder, asserted before (CPU) and after (GPU) it runs. steps: [(k, per-row bound, per-row product,
    total or None when refused)]; returns (admitted ks, refused ks, ks admitted with |total| >= 2^63)"""
    adm = [s for s in steps if s[3] is not None]
    ref = [s for s in steps if s[3] is None]
    for k, bound, prod, total in steps:
        if must_admit(n, bound):
            assert total is not None, f"{name}: step 2^{k} (bound {bound}) satisfies rows x bound < 4e18 and was refused"
        if not fits64(prod):
            assert total is None, f"{name}: step 2^{k}: one row's product {prod} does not fit int64 and the run was admitted"
    if adm and ref:
        assert max(abs(s[2]) for s in adm) < min(abs(s[2]) for s in ref), f"{name}: admission is not monotone in the magnitude: {steps}"
    big = [s[0] for s in adm if abs(s[3]) >= 2 ** 63]
    return [s[0] for s in adm], [s[0] for s in ref], big


# ------------------------------------------------------------------ part B: where the 32-bit form begins and ends

def _pin(col, rows, values):
    for r, v in zip(rows, values):
        col[r] = v


def lc_boundary_cases(n=20_000):
    """[(name, columns, (A1, B1, A2, B2), form the rule in scan_plan.hip predicts)]: one case on each side of each of the four conditions
    of FORM_NARROW32 (be, b1, b2, be b1 <= 2^31 - 1), the other bounds as small as that allows. p = P_LO in rows 500, 1500, ... (a predicate
    from P_LO + 1 leaves them out); rows 0..7 hold every sign combination of the extremes of e, f1 and f2."""
    M = I32_MAX
    spec = [  # name, e range, f1 range, f2 range
        ("be_2^31-1", (-M, M), (-1, 1), (-1, 1)),
        ("be_2^31", (-M - 1, M), (-1, 1), (-1, 1)),
        ("b1_2^31-1", (-1, 1), (-M, M), (-1, 1)),
        ("b1_2^31", (-1, 1), (-M - 1, M), (-1, 1)),
        ("b2_2^31-1", (-1, 1), (-1, 1), (-M, M)),
        ("b2_2^31", (-1, 1), (-1, 1), (-M - 1, M)),
        ("be_b1_46341x46340", (-46_341, 46_341), (-46_340, 46_340), (-1, 1)),
        ("be_b1_65536x32768", (-65_536, 65_536), (-32_768, 32_768), (-1, 1)),
    ]
    out = []
    for ci, (name, er, f1r, f2r) in enumerate(spec):
        rng = np.random.default_rng(100 + ci)

        def draw(lo, hi):
            v = rng.integers(lo, hi, n, endpoint=True, dtype=np.int64)
            v[rng.integers(0, n, n // 8)] = lo      # the extremes are common, not two rows
            v[rng.integers(0, n, n // 8)] = hi
            return v
        e, f1, f2 = draw(*er), draw(*f1r), draw(*f2r)
        for r in range(8):
            e[r], f1[r], f2[r] = er[r & 1], f1r[(r >> 1) & 1], f2r[(r >> 2) & 1]
        i = np.arange(n)
        c = dict(p=(P_LO + (i + 500) % 1000).astype(np.int32), q=rng.integers(-50, 50, n, endpoint=True).astype(np.int32),
                 e=e, d=100 - f1, t=f2 - 100, k0=rng.integers(0, 3, n).astype(np.uint8), k1=rng.integers(0, 2, n).astype(np.uint8))
        consts = (100, -1, 100, 1)     # f1 = 1.00 - d, f2 = 1.00 + t at scale 2
        out.append((name, c, consts, lc_form(c, *consts)))
    return out


def fs_boundary_cases(n=20_000):
    """[(name, columns, predicted form)]: ba and bb each at 2^31 - 1 and 2^31; the other factor is the largest power of two the must-admit
    rule (run rows x ba x bb < 4e18) leaves at 2^31, so every run of these tables is one the proof has to admit"""
    M = I32_MAX
    other = 1
    while n * (M + 1) * other * 2 < PROOF_LIMIT:
        other *= 2
    spec = [("ba_2^31-1", (-M, M), (-other, other)), ("ba_2^31", (-M - 1, M), (-other, other)),
            ("bb_2^31-1", (-other, other), (-M, M)), ("bb_2^31", (-other, other), (-M - 1, M))]
    out = []
    for ci, (name, ar, br) in enumerate(spec):
        rng = np.random.default_rng(200 + ci)
        a, b = (rng.integers(lo, hi, n, endpoint=True, dtype=np.int64) for lo, hi in (ar, br))
        for r in range(4):
            a[r], b[r] = ar[r & 1], br[(r >> 1) & 1]
        a[rng.integers(4, n, n // 8)] = ar[0]
        b[rng.integers(4, n, n // 8)] = br[0]
        i = np.arange(n)
        c = dict(p=(P_LO + (i + 500) % 1000).astype(np.int32), q=rng.integers(1, 50, n, endpoint=True).astype(np.int32), a=a, b=b)
        out.append((name, c, fs_form(c)))
    return out


BOUNDARY_RANGES = ((0, None), (4, -3), (12, 4111))


# ------------------------------------------------------------------ part E: ORDER BY keys

def cents_half_even(x, scale):
    """the sort key of a DECIMAL: x / 10^scale as an exact Fraction, rounded half-even to two places; the whole number of cents"""
    v = Fraction(x, 10 ** scale) * 100
    fl = v.numerator // v.denominator
    rem = v - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1):
        fl += 1
    return fl


def sorted_rows(keys, descending, sel):
    """ORDER BY restated: keys = [(python values, bool validity or None)], NULLs first in either direction, ties in input order"""
    def key(pos_row):
        pos, r = pos_row
        out = []
        for (vals, valid), desc in zip(keys, descending):
            if valid is not None and not valid[r]:
                out.append((0, 0))
            else:
                out.append((1, -vals[r] if desc else vals[r]))
        return tuple(out) + (pos,)
    return [r for _, r in sorted(enumerate(sel), key=key)]


def dec_sort_values(scale, seed, n):
    """int64 DECIMAL values up to +-(2^63 - 1) with half-way cases (...5 / ...50 below the cents) of both signs, ties, and small values"""
    rng = np.random.default_rng(seed)
    v = rng.integers(I64_MIN + 1, I64_MAX, n, endpoint=True, dtype=np.int64)
    v[: n // 4] = rng.integers(-10 ** 6, 10 ** 6, n // 4)
    edge = [I64_MAX, -I64_MAX, I64_MAX - 1, -I64_MAX + 1, 0, 1, -1, 10 ** 17, -10 ** 17, 92 * 10 ** 15, 93 * 10 ** 15, -92 * 10 ** 15, -93 * 10 ** 15,
            92 * 10 ** 16, 93 * 10 ** 16, -92 * 10 ** 16, -93 * 10 ** 16, 9 * 10 ** 18, -9 * 10 ** 18]
    if scale > 2:
        half = 5 * 10 ** (scale - 3)
        unit = 10 ** (scale - 2)
        base = (I64_MAX // unit - 3) * unit
        for b in (0, unit, 2 * unit, 12345 * unit, base, base - unit):
            edge += [b + half, -(b + half), b + half - 1, -(b + half - 1), b + half + 1, -(b + half + 1)]
    edge = [x for x in edge if fits64(x)]
    pos = rng.choice(n, min(n, 3 * len(edge)), replace=False)
    for j, r in enumerate(pos):
        v[r] = edge[j % len(edge)]
    return v


def civil_days(y, m, d):
    """days since 1970-01-01 of a proleptic Gregorian date (negative before 1970)"""
    y -= m <= 2
    era = y // 400
    yoe = y - era * 400
    doy = (153 * (m + (-3 if m > 2 else 9)) + 2) // 5 + d - 1
    doe = yoe * 365 + yoe // 4 - yoe // 100 + doy
    return era * 146097 + doe - 719468


# ------------------------------------------------------------------ parts C and D: expressions and aggregates

def eval_program(prog, row, scales):
    """ph_expr_eval's decimal programs over one row: (value, scale), or "overflow" when any step leaves int64 (the alignment multiplies
    included), or (None, scale) when an input is NULL. prog: hip.X_* tuples; row: {col: int or None}; scales: {col: scale}"""
    st = []
    for op, col, ival, scale in prog:
        if op == hip.PH_X_COL:
            st.append((row[col], scales[col]))
        elif op == hip.PH_X_CONST:
            st.append((ival, scale))
        else:
            (y, sy), (x, sx) = st.pop(), st.pop()
            if x is None or y is None:
                st.append((None, sx + sy if op == hip.PH_X_MUL else max(sx, sy)))
                continue
            if op == hip.PH_X_MUL:
                r, s = x * y, sx + sy
            else:
                s = max(sx, sy)
                x, y = x * 10 ** (s - sx), y * 10 ** (s - sy)
                if not (fits64(x) and fits64(y)):
                    return "overflow"
                r = x + y if op == hip.PH_X_ADD else x - y
            if not fits64(r):
                return "overflow"
            st.append((r, s))
    return st[0]


def expected_values(prog, a, b, scales):
    """eval_program over every row of two operand columns: one evaluation per distinct operand pair (numpy only finds the pairs)"""
    ua, ia = np.unique(np.asarray(a), return_inverse=True)
    ub, ib = np.unique(np.asarray(b), return_inverse=True)
    assert len(ua) * len(ub) < 10_000
    table = np.empty((len(ua), len(ub)), dtype=object)
    for i, x in enumerate(ua.tolist()):
        for j, y in enumerate(ub.tolist()):
            table[i, j] = eval_program(prog, {0: x, 1: y}, {0: scales[0], 1: scales[1]})
    return table[ia.reshape(-1), ib.reshape(-1)].tolist()


_C0, _C1 = hip.X_COL(0), hip.X_COL(1)
# (name, program, scales of the two columns, operand pairs that still fit, operand pairs that overflow — each in the step the name says)
EXPR_CASES = [
    ("multiply", [_C0, _C1, hip.X_MUL], (0, 0),
     [(153_092_023, 60_247_241_209), (3_037_000_499, 3_037_000_499), (-3_037_000_499, 3_037_000_499), (I64_MIN, 1), (I64_MAX, -1), (I64_MIN // 2, 2)],
     [(3_037_000_500, 3_037_000_500), (I64_MIN, -1), (-3_037_000_500, 3_037_000_500), (I64_MIN // 2 - 1, 2)]),
    ("add", [_C0, _C1, hip.X_ADD], (2, 2),
     [(I64_MIN, 0), (I64_MAX, 0), (I64_MAX - 1, 1), (I64_MIN + 1, -1)], [(I64_MAX, 1), (I64_MIN, -1)]),
    ("subtract", [_C0, _C1, hip.X_SUB], (2, 2),
     [(I64_MAX, 0), (-1, I64_MIN), (I64_MIN, 0), (-1, I64_MAX)], [(0, I64_MIN), (I64_MIN, 1), (I64_MAX, -1)]),
    ("align_left", [_C0, _C1, hip.X_ADD], (0, 2),       # the left operand is multiplied by 100: a 10^k at and one past the limit
     [(I64_MAX // 100, 7), (I64_MIN // 100 + 1, -8)], [(I64_MAX // 100 + 1, 0), (I64_MIN // 100, 0)]),
    ("align_right", [_C0, _C1, hip.X_SUB], (4, 1),      # the right operand is multiplied by 1000
     [(807, I64_MAX // 1000), (-808, -(I64_MAX // 1000))], [(0, I64_MAX // 1000 + 1), (0, I64_MIN // 1000)]),
    ("constants", [_C0, hip.X_CONST(0, 0), hip.X_ADD, _C1, hip.X_CONST(-1, 0), hip.X_MUL, hip.X_SUB], (0, 0),   # (a + 0) - (b * -1)
     [(I64_MIN, 0), (I64_MAX, 0), (I64_MAX - 5, -5), (I64_MIN + 5, 5)], [(0, I64_MIN), (I64_MAX, 1)]),
]


class TopK:
    """ph_agg_topk restated: the groups at least as good as the k-th best; NULL aggregates (None) sort first whatever the direction.
    values: [int or None] per group; best(k) = the set of group indices"""

    def __init__(self, values, descending):
        self.rank = [(0, 0) if v is None else (1, -v if descending else v) for v in values]
        self.order = sorted(range(len(values)), key=self.rank.__getitem__)

    def best(self, k):
        if k <= 0 or not self.order:
            return set()
        kth = self.rank[self.order[min(k, len(self.order)) - 1]]
        n = len(self.order)
        if k < n:      # the ties of the k-th follow it in the order
            n = k
            while n < len(self.order) and self.rank[self.order[n]] == kth:
                n += 1
        return set(self.order[:n])


def topk_reference(values, k, descending):
    return TopK(values, descending).best(k)


def having_reference(values, op, k):
    """ph_agg_fetch_where over one conjunct with a DECIMAL constant: `>` is the one comparison the reference's selectOperation has for
    DECIMAL / HUGEINT values, every other operator selects nothing; NULL aggregates (None) fail every comparison"""
    if op != hip.PH_GT:
        return set()
    return {g for g, v in enumerate(values) if v is not None and v > k}
