"""Inputs and the plain reference of the load-time column statistics (ctx.hip: minmax_kernel, order_stat_kernel, run_stat_kernel,
narrow_kernel behind ph_table_col_range / ph_table_col_stats / ph_table_col_run_len / ph_table_col_narrow). Every builder places ONE
defect where a kernel of 64-lane waves, 256-thread blocks and a grid capped at 2048 blocks (second grid-stride trip at row 524288) can
miss it, and says what it built: (values, claim, defect position). `reference` restates include/planhip.h in Python integers and exact
numpy compares (no value is ever subtracted from another in a fixed-width type). test_stat_edges_reference.py checks builders and
reference without a device; test_gpu_stat_edges.py compares the library with `reference`, always by equality."""
import numpy as np

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1

LIMITS = {"I32": (I32_MIN, I32_MAX), "DATE": (I32_MIN, I32_MAX), "I64": (I64_MIN, I64_MAX), "DEC64": (I64_MIN, I64_MAX), "CODE8": (0, 255)}
DTYPE = {"I32": np.int32, "DATE": np.int32, "I64": np.int64, "DEC64": np.int64, "CODE8": np.uint8, "F32": np.float32, "F64": np.float64}
WIDTH = {"I32": 4, "DATE": 4, "I64": 8, "DEC64": 8, "CODE8": 1, "F32": 4, "F64": 8}
RANGED = ("I32", "DATE", "I64", "DEC64", "CODE8")     # types with min / max
ORDERED = ("I32", "DATE", "I64", "DEC64")             # types with order flags, run length and narrowed copies

WAVE, BLOCK, GRID_CAP = 64, 256, 2048
STRIDE = GRID_CAP * BLOCK                             # 524288: the first row of a grid-stride loop's second trip
ROW_PAD = 8192
RUN_MAX = 64                                          # the longest run ph_table_col_run_len reports

N = (1, 2, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193, 524287, 524288, 524289, 1048577)
BOUNDARY = (0, 62, 63, 64, 254, 255, 256, 524286, 524287, 524288)


def positions(n):
    """the defect positions of a column of n rows: the rows beside a wave, a block and the grid-stride boundary, and the last two rows"""
    return sorted({p for p in BOUNDARY + (n - 2, n - 1) if 0 <= p < n})


def pair_positions(n):
    """positions p whose pair (p, p + 1) exists"""
    return [p for p in positions(n) if p + 1 < n]


def padded(n):
    return -(-max(n, 1) // ROW_PAD) * ROW_PAD


def null_bitmap(n, null_rows):
    """validity bits (little bit order, 1 = not NULL) of n rows with the given rows NULL"""
    bits = np.ones(n, np.uint8)
    bits[list(null_rows)] = 0
    return np.packbits(bits, bitorder="little")


# ------------------------------------------------------------------ the reference

def reference(values, typ, validity=None):
    """{range, ascending, strict, run_len, narrow} of one column as include/planhip.h defines them. range: (min, max) over every stored slot
    (NULL slots included) or None; narrow: (width, base) or None."""
    v = np.asarray(values)
    n = len(v)
    out = dict(range=None, ascending=False, strict=False, run_len=0, narrow=None)
    if typ not in RANGED or n == 0:
        return out
    mn, mx = int(v.min()), int(v.max())
    out["range"] = (mn, mx)
    if typ not in ORDERED or validity is not None:
        return out
    out["ascending"] = not bool((v[1:] < v[:-1]).any())
    out["strict"] = not bool((v[1:] <= v[:-1]).any())
    span = mx - mn + 1
    if out["ascending"] and not out["strict"] and n % span == 0 and 2 <= n // span <= RUN_MAX:
        c = n // span
        want = np.int64(mn) + np.arange(n, dtype=np.int64) // c      # at most mx: no overflow
        if bool((v.astype(np.int64) == want).all()):
            out["run_len"] = c
    w = next((w for w in (1, 2, 4) if mx - mn < 256 ** w), None)
    if w is not None and w < WIDTH[typ]:
        out["narrow"] = (w, mn)
    return out


def flags(ref):
    """ph_table_col_stats & 3 of a reference result"""
    return (1 if ref["ascending"] else 0) | (2 if ref["strict"] else 0)


def narrow_bytes(n, refs):
    """ph_table_narrow_bytes of a table of n rows whose columns have these reference results"""
    return padded(n) * sum(r["narrow"][0] for r in refs if r["narrow"])


# ------------------------------------------------------------------ builders: (values, claim, defect position)

def _array(typ, n, fill):
    return np.full(n, fill, dtype=DTYPE[typ])


VALUE_SETS = ("extremes", "inside_low", "inside_high", "constant_min", "constant_max")


def extremum_at(n, typ, p_min, p_max, value_set="extremes"):
    """a flat column whose single minimum (the type's) sits at p_min and whose single maximum (the type's) at p_max. extremes: flat in the
    middle of the type; inside_low / inside_high: flat one inside the minimum / the maximum; constant_min / constant_max: every row at that
    extreme (no position). claim: range."""
    lo, hi = LIMITS[typ]
    if value_set.startswith("constant"):
        k = lo if value_set == "constant_min" else hi
        return _array(typ, n, k), dict(range=(k, k)), None
    assert n >= 2 and p_min != p_max and 0 <= p_min < n and 0 <= p_max < n
    flat = {"extremes": (lo + hi) // 2 + 7, "inside_low": lo + 1, "inside_high": hi - 1}[value_set]
    v = _array(typ, n, flat)
    v[p_min], v[p_max] = lo, hi
    return v, dict(range=(lo, hi)), (p_min, p_max)


def _ramp(typ, n, first, step):
    """first + i * step for i < n as the type's array (exact: through uint64 wraparound for the 64-bit types)"""
    if WIDTH[typ] == 4:
        return (first + np.arange(n, dtype=np.int64) * step).astype(np.int32)
    u = np.arange(n, dtype=np.uint64) * np.uint64(step) + np.uint64(first % 2 ** 64)
    return u.view(np.int64)


ORDER_BASES = ("small", "wide", "max_to_min", "equal_at_max")
ORDER_WHOLE = ("clean", "clean_wide", "constant", "descending")


def order_defect(n, typ, p, kind, base="small"):
    """a strictly ascending column with the one pair (p, p + 1) made `equal` or `descending`. small: 0, 2, 4, ...; wide: from the type's
    minimum to its maximum in equal huge steps (b - a of the swapped pair does not fit the type); max_to_min: the pair is (type maximum, type
    minimum), the rows before it count up to the maximum and the rows after it up from the minimum; equal_at_max: the pair is (maximum,
    maximum), which only the last pair can be. claim: ascending, strict, bad_pairs."""
    lo, hi = LIMITS[typ]
    assert typ in ORDERED and 0 <= p and p + 1 < n and kind in ("equal", "descending")
    if base == "small":
        v = _ramp(typ, n, 0, 2)
        v[p + 1] = v[p] if kind == "equal" else v[p] - 1
    elif base == "wide":
        v = _ramp(typ, n, lo, (hi - lo) // (n - 1))
        v[n - 1] = hi
        if kind == "equal":
            v[p + 1] = v[p]
        else:
            v[p], v[p + 1] = v[p + 1], v[p]
    elif base == "max_to_min":
        assert kind == "descending"
        v = _array(typ, n, 0)
        v[:p + 1] = _ramp(typ, p + 1, hi - p, 1)
        v[p + 1:] = _ramp(typ, n - p - 1, lo, 1)
    else:
        assert base == "equal_at_max" and kind == "equal" and p == n - 2
        v = _ramp(typ, n, hi - (n - 2), 1)
        v[n - 1] = hi
    return v, dict(ascending=kind == "equal", strict=False, bad_pairs=[p]), p


def order_whole(n, typ, which):
    """the columns without a single defect: clean (0, 2, 4, ...), clean_wide (minimum to maximum), constant, descending (strictly)"""
    lo, hi = LIMITS[typ]
    assert typ in ORDERED and n >= 1
    if which == "clean":
        v = _ramp(typ, n, 0, 2)
    elif which == "clean_wide":
        v = _ramp(typ, n, lo, (hi - lo) // max(n - 1, 1))
        v[n - 1] = hi if n > 1 else lo
    elif which == "constant":
        v = _array(typ, n, hi)
    else:
        v = _ramp(typ, n, hi - 3 * (n - 1), 3)[::-1].copy()
    bad = [] if which.startswith("clean") else list(range(n - 1))
    return v, dict(ascending=which != "descending" or n == 1, strict=which.startswith("clean") or n == 1, bad_pairs=bad), None


RUN_LENGTHS = (2, 3, 4, 63, 64, 65)
RUNS_PAST_STRIDE = {2: 262145, 3: 174763, 4: 131073, 63: 8323, 64: 8193, 65: 8067}     # c x nruns just past 524288
# At those sizes every row from 524288 on lies in the LAST run, where no row can move without changing the maximum. Two runs more put the
# last row of a run that is not the last past the grid stride: the one place where an `uneven` defect shows whether the loop makes its second trip
RUNS_WELL_PAST_STRIDE = {c: r + 2 for c, r in RUNS_PAST_STRIDE.items()}
RUNS_ABOUT_1000 ={2: 500, 3: 333, 4: 250, 63: 16, 64: 16, 65: 15}


def run_firsts(typ, nruns):
    lo, hi = LIMITS[typ]
    return (lo, -1, 0, hi - nruns + 1)


def run_defect(c, nruns, first, p=None, defect=None, typ="I64"):
    """runs of length c over the nruns consecutive values from `first`. defect None: clean. "uneven": row p, the last row of its run, holds
    the next run's value (still ascending, not strict, same min, max and n). "last_plus_one": the very last row is one larger (p = n - 1),
    which changes the span. claim: run_len, c, min, odd_row."""
    lo, hi = LIMITS[typ]
    n = c * nruns
    assert typ in ORDERED and lo <= first and first + nruns - 1 <= hi
    v = _ramp(typ, n, 0, 1)
    v = (v // c + DTYPE[typ](first)).astype(DTYPE[typ])       # first + i // c <= hi
    if defect is None:
        return v, dict(run_len=c if 2 <= c <= RUN_MAX else 0, c=c, min=first, odd_row=None), None
    if defect == "uneven":
        assert p % c == c - 1 and p + 1 < n
        v[p] = v[p + 1]
    else:
        assert defect == "last_plus_one" and first + nruns <= hi and p in (None, n - 1)
        p = n - 1
        v[p] = first + nruns
    return v, dict(run_len=0, c=c, min=first, odd_row=p), p


def uneven_rows(c, nruns, near):
    """the rows an `uneven` defect can take beside the positions `near`: the last row of each position's run, the last run excepted"""
    n = c * nruns
    return sorted({q // c * c + c - 1 for q in near if q // c * c + c - 1 < n - c} | ({n - c - 1} if nruns > 1 else set()))


SPANS = {8: (0, 1, 255, 256, 65535, 65536, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1), 4: (0, 255, 256, 65535, 65536, 2 ** 32 - 1)}


def narrow_bases(typ, span):
    """the bases at which [base, base + span] fits the type: its minimum, one that straddles zero, zero, and the one that ends at its maximum"""
    lo, hi = LIMITS[typ]
    return [b for b in dict.fromkeys((lo, -1 - span // 2, 0, hi - span)) if lo <= b and b + span <= hi]


def narrow_span(typ, span, base, n=2, p_lo=0, p_hi=1):
    """a column flat in the middle of [base, base + span] with base at p_lo and base + span at p_hi (n = 1: span 0 only). claim: range,
    narrow = (width, base) or None."""
    lo, hi = LIMITS[typ]
    assert typ in ORDERED and lo <= base and base + span <= hi
    v = _array(typ, n, base + span // 2)
    if span:
        assert p_lo != p_hi
        v[p_lo], v[p_hi] = base, base + span
    w = 1 if span < 2 ** 8 else 2 if span < 2 ** 16 else 4 if span < 2 ** 32 else None
    return v, dict(range=(base, base + span), narrow=(w, base) if w is not None and w < WIDTH[typ] else None), (p_lo, p_hi)


def position_pairs(n):
    """(p, q) over the defect positions in a cycle: every position holds the first value once and the second once"""
    ps = positions(n)
    return [(ps[k], ps[(k + 1) % len(ps)]) for k in range(len(ps))] if len(ps) > 1 else []


def exact_sum(x):
    """the exact sum of an int64 array as a Python int"""
    x = np.asarray(x, dtype=np.int64)
    return (int((x >> 32).sum()) << 32) + int((x & 0xFFFFFFFF).sum())
