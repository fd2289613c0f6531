"""Inputs and plain references of the selection-layer edge tests (test_gpu_select_layer.py; checked on their own, without a
device, by test_select_edges_reference.py).

Every reference here is Python `int` / `fractions.Fraction` arithmetic or a numpy expression over the input arrays — never the
expression a kernel evaluates: the decimal casts come from `float(Fraction(v, 10**s))` (correctly rounded by construction), the
scans from an int64 `cumsum`, the comparisons from numpy over boolean validity."""
import hashlib
from fractions import Fraction

import numpy as np

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
EXACT = 2 ** 53                      # below it an int64 is a double, and so is every 10^s the scales here use
OP_EQ, OP_NE, OP_LT, OP_LE, OP_GT, OP_GE, OP_LIKE, OP_NOTLIKE = range(1, 9)   # planhip.h's and the oracle's numbering
ALL_OPS = (OP_EQ, OP_NE, OP_LT, OP_LE, OP_GT, OP_GE)

# ------------------------------------------------------------------ DECIMAL -> DOUBLE -> FLOAT
CAST_SCALES = (0, 1, 2, 4, 6)
# float32 binades 2^e whose midpoints, times 10^s, lie between 2^53 and 2^63 (three per scale), and one far below 2^53
CAST_EXPONENTS = {0: (54, 58, 62), 1: (50, 53, 56), 2: (47, 50, 53), 4: (40, 43, 46), 6: (34, 37, 40)}
CAST_EXPONENT_BELOW = {0: 30, 1: 27, 2: 24, 4: 24, 6: 24}
CAST_MANTISSAS = (0, 1, 0x2AAAAB, 0x7FFFFE)   # the lower float of the pair: even, odd, odd, even (a tie goes to the even one)
CAST_SPECIALS = (0, 1, -1, 5, -5, 99, 100, 101, -100, 12345678, EXACT - 1, -(EXACT - 1), EXACT, -EXACT, EXACT + 1, -(EXACT + 1),
                 I64_MAX, -I64_MAX, I64_MIN)


def cast_f64(v, scale):
    """the DOUBLE of the decimal v / 10^scale: the nearest double (ties to even) of the exact quotient — what strtod gives for its text"""
    return float(Fraction(int(v), 10 ** scale))


def cast_f32(v, scale):
    """the FLOAT of the decimal: the reference's second step narrows the DOUBLE (tryCastDecimalToFloat32)"""
    return np.float32(cast_f64(v, scale))


def cast_reference(values, scale):
    """(float64 array, float32 array) of cast_f64 / cast_f32 over an int64 array"""
    d = np.array([cast_f64(v, scale) for v in values.tolist()], dtype=np.float64)
    return d, d.astype(np.float32)


def cast_midpoints(scale, below=False):
    """[(lower float, upper float, their midpoint as a Fraction)], both signs: adjacent float32 values whose midpoint the cast inputs surround"""
    out = []
    for e in ((CAST_EXPONENT_BELOW[scale],) if below else CAST_EXPONENTS[scale]):
        for j in CAST_MANTISSAS:
            lo = Fraction((2 ** 23 + j) * 2 ** e, 2 ** 23)
            hi = Fraction((2 ** 23 + j + 1) * 2 ** e, 2 ** 23)
            flo, fhi = np.float32(float(lo)), np.float32(float(hi))
            assert Fraction(float(flo)) == lo and Fraction(float(fhi)) == hi and np.nextafter(flo, np.float32(np.inf)) == fhi
            out.append((flo, fhi, (lo + hi) / 2))
            out.append((-fhi, -flo, -(lo + hi) / 2))
    return out


def cast_inputs(scale):
    """Deterministic unscaled values for one scale: every integer within 1.5 double-ulps (at most 2000 steps) of midpoint x 10^scale
    for the midpoints above and below 2^53, and the int64 / 2^53 edges. Sorted, distinct, int64."""
    vals = set(CAST_SPECIALS)
    for below in (False, True):
        for flo, fhi, mid in cast_midpoints(scale, below):
            centre = mid * 10 ** scale
            assert centre.denominator == 1, (scale, mid)
            c = int(centre)
            e = max(abs(int(mid)), 1).bit_length() - 1                     # mid in [2^e, 2^(e+1))
            ulp = Fraction(2) ** (e - 52)
            w = max(min(int(ulp * 10 ** scale * 3 / 2) + 2, 2000), 50 if below else 0)
            vals.update(range(c - w, c + w + 1))
    vals = sorted(v for v in vals if I64_MIN <= v <= I64_MAX)
    return np.array(vals, dtype=np.int64)


def cast_random(scale, n, seed):
    """n unscaled values with |v| in [2^53, 2^63), either sign"""
    rng = np.random.default_rng(seed * 31 + scale)
    mag = rng.integers(EXACT, 2 ** 63, n, dtype=np.int64)
    return np.where(rng.random(n) < 0.5, -mag, mag)


def cast_random_below(scale, n, seed):
    """n unscaled values with |v| < 2^53, either sign: where one IEEE division is already the reference"""
    rng = np.random.default_rng(seed * 37 + scale)
    return rng.integers(-(EXACT - 1), EXACT, n, dtype=np.int64) >> rng.integers(0, 40, n)


def cast_by_division(values, scale, wide):
    """What `(double)unscaled / 10^scale` gives (numpy's IEEE float64, the arithmetic the kernels used): NOT the reference above 2^53;
    the reference tests count where the two part, so that the GPU tests are known to be able to fail."""
    d = values.astype(np.float64) / np.float64(10 ** scale)
    return d if wide else d.astype(np.float32)


# ------------------------------------------------------------------ exclusive scan
SCAN_TILE = 4096
SCAN_FORMS = ("loop", "small", "lookback", "three_pass")   # ph_ctx_scan_forms' order
SCAN_KINDS = ("random", "zeros", "first", "last", "full")
SCAN_SIZES = ([0, 1, 1023, 1024, 1025, 16383, 16384, 16385] +
              [k * SCAN_TILE + d for k in (5, 4095, 4096, 4097) for d in (-1, 0, 1)] + [20_000_003])
SCAN_SIZES_ABOVE_SMALL = [n for n in SCAN_SIZES if n > 16384]
SCAN_TWICE_THREE_PASS = 16384 * SCAN_TILE + 1            # its tile sums are more than 16384 again


def scan_form(n, three_pass=False):
    """the form exclusive_scan_i32 documents for n elements"""
    if n <= 1024:
        return "loop"
    if n <= 16384:
        return "small"
    return "three_pass" if three_pass else "lookback"


def scan_input(n, kind, seed=0):
    """int32[n] with a total below 2^31 (the scan's contract): counts in 0..4096 — or as far as n allows under that total —, all
    zeros, one non-zero at either end, or a total of exactly 2^31 - 1"""
    if kind == "zeros" or n == 0:
        return np.zeros(n, np.int32)
    if kind == "random":
        top = min(4096, I32_MAX // n)
        return np.random.default_rng(seed + n).integers(0, top + 1, n).astype(np.int32)
    if kind in ("first", "last"):
        v = np.zeros(n, np.int32)
        v[0 if kind == "first" else -1] = 4096
        return v
    assert kind == "full"
    v = np.full(n, I32_MAX // n, np.int32)
    v[-1] += I32_MAX - int(v.astype(np.int64).sum())
    return v


def scan_reference(v):
    """(exclusive prefix sums as int64, total)"""
    c = np.cumsum(v.astype(np.int64))
    total = int(c[-1]) if len(v) else 0
    ex = np.zeros(len(v), np.int64)
    ex[1:] = c[:-1]
    return ex, total


def scan_digest(exclusive, total):
    """what the three-pass child prints for one input and the parent recomputes: the int32 image of the prefix sums, and the total"""
    return hashlib.sha256(np.ascontiguousarray(exclusive, dtype=np.int32).tobytes()).hexdigest() + ":" + str(int(total))


# ------------------------------------------------------------------ column OP column
COLS_SIZES = (0, 1, 255, 256, 257, 2047, 2048, 2049, 70_001)
COLS_NULLS = ("neither", "left", "right", "both")
COLS_KINDS = ("integer", "date", "decimal", "bigint", "code")
# selectOperation's (type, op) pairs for two columns: everything else selects nothing
COLS_OPS = {"integer": ALL_OPS, "date": (OP_LT, OP_LE, OP_GT, OP_GE), "decimal": (OP_GT,), "bigint": (), "code": ()}


def cols_input(kind, n, nulls, seed=0):
    """(a, b, valid_a, valid_b): two columns over a small range, so that every ordering and equality occurs, with the type's extreme
    values mixed in; valid_* is a boolean array, or None for a column without NULLs"""
    rng = np.random.default_rng(seed * 1000 + n + len(kind) * 7 + len(nulls))
    if kind == "integer":
        pool = np.array([I32_MIN, I32_MIN + 1, -1, 0, 1, 7, I32_MAX - 1, I32_MAX], np.int32)
    elif kind == "date":
        pool = np.arange(8000, 8008, dtype=np.int32)                    # days since 1970: calendar dates both witnesses can hold
    elif kind == "decimal":
        pool = np.array([I64_MIN, I64_MIN + 1, -100, 0, 100, 2 ** 53 + 1, I64_MAX - 1, I64_MAX], np.int64)
    elif kind == "bigint":
        pool = np.array([I64_MIN, -1, 0, 1, I64_MAX], np.int64)
    else:
        pool = np.array([0, 1, 2, 254, 255], np.uint8)
    a = pool[rng.integers(0, len(pool), n)]
    b = pool[rng.integers(0, len(pool), n)]
    va = rng.random(n) > 0.2 if nulls in ("left", "both") else None
    vb = rng.random(n) > 0.2 if nulls in ("right", "both") else None
    return a, b, va, vb


def cols_selection(n, seed=0):
    """an ascending selection of about two thirds of n rows (int64 row ids)"""
    rng = np.random.default_rng(seed + 17 * n)
    return np.flatnonzero(rng.random(n) < 0.66).astype(np.int64)


def cols_reference(kind, op, a, b, va, vb, sel=None):
    """rows (of sel, or all) where a OP b holds and neither side is NULL; int64 row ids in input order"""
    rows = np.arange(len(a), dtype=np.int64) if sel is None else np.asarray(sel, np.int64)
    if op not in COLS_OPS[kind]:
        return rows[:0]
    x, y = a[rows], b[rows]
    hit = {OP_EQ: x == y, OP_NE: x != y, OP_LT: x < y, OP_LE: x <= y, OP_GT: x > y, OP_GE: x >= y}[op]
    if va is not None:
        hit = hit & va[rows]
    if vb is not None:
        hit = hit & vb[rows]
    return rows[hit]


def pack(valid):
    """boolean validity -> the bitmap the columns carry (bit i of byte i / 8, least significant first)"""
    return None if valid is None else np.packbits(valid, bitorder="little")


# ------------------------------------------------------------------ FLOAT / DOUBLE columns against a constant
def float_values(dtype, k, n, seed=0):
    """n values of dtype around the constant k: NaN, both zeros, both infinities, the smallest and largest denormals, k and its two
    neighbours, and random values of both signs"""
    rng = np.random.default_rng(seed + n)
    k = dtype(k)
    tiny = np.nextafter(dtype(0), dtype(1))
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, tiny, -tiny, np.finfo(dtype).tiny - tiny, k,
                        np.nextafter(k, dtype(np.inf)), np.nextafter(k, dtype(-np.inf))], dtype=dtype)
    pick = rng.integers(0, len(special) + 6, n)
    rand = (rng.standard_normal(n) * 3).astype(dtype) + k if np.isfinite(k) else rng.standard_normal(n).astype(dtype)
    return np.where(pick < len(special), special[np.minimum(pick, len(special) - 1)], rand).astype(dtype)


def float_select_reference(dtype, op, v, k, valid=None, sel=None):
    """selectOperation's pairs: FLOAT has > >= <= (plain IEEE comparisons: false for a NaN), DOUBLE has < (GreaterFloat(k, v): false
    for a NaN value, true for a NaN constant and any other value); every other operator selects nothing."""
    rows = np.arange(len(v), dtype=np.int64) if sel is None else np.asarray(sel, np.int64)
    x = v[rows]
    with np.errstate(invalid="ignore"):
        if dtype is np.float32:
            kf = np.float32(k)
            hit = {OP_GT: x > kf, OP_GE: x >= kf, OP_LE: x <= kf}.get(op)
        else:
            hit = {OP_LT: ~np.isnan(x) if np.isnan(k) else x < np.float64(k)}.get(op)
    if hit is None:
        return rows[:0]
    if valid is not None:
        hit = hit & valid[rows]
    return rows[hit]


# ------------------------------------------------------------------ a run of dictionary codes
RUN_CASES = ((3, 9), (0, 255), (7, 7), (0, 0), (255, 255), (-5, 4), (250, 300), (-3, 400), (9, 3), (256, 300), (-9, -1))


def code_run_reference(codes, lo, hi, valid=None, sel=None):
    """rows whose code lies in lo..hi ('=' against a run of codes: a prefix LIKE or a sorted IN list over a dictionary in byte order)"""
    rows = np.arange(len(codes), dtype=np.int64) if sel is None else np.asarray(sel, np.int64)
    x = codes[rows].astype(np.int64)
    hit = (x >= lo) & (x <= hi)
    if valid is not None:
        hit = hit & valid[rows]
    return rows[hit]
