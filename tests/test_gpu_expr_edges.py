"""ph_date_extract and ph_float_eval at their edges, compared exactly: every calendar part over the whole int32 day domain against
numpy's datetime64 calendar, FLOAT / DOUBLE programs bit for bit against expr_edges.float_program — NULL operands and the validity
bitmap's documented size, every operand type at the values where a cast rounds, the IEEE special values, the comparisons
selectOperation has. Inputs and references: expr_edges.py (checked without a device by test_expr_edges_reference.py)."""
import numpy as np
import pytest

import expr_edges as EE
import select_edges as SE
from plan_amd import hip

pytestmark = pytest.mark.gpu

PARTS = (hip.PH_PART_YEAR, hip.PH_PART_MONTH, hip.PH_PART_DAY)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


# ------------------------------------------------------------------ ph_date_extract
def check_dates(ctx, days, sel=None):
    """YEAR, MONTH and DAY of rows sel (or all) of a PH_DATE column against civil_parts; the message names the wrong days"""
    col = hip.DevColumn(ctx, hip.PH_DATE, days)
    rows = np.arange(len(days)) if sel is None else sel
    dsel = None if sel is None else ctx.upload(np.ascontiguousarray(sel, dtype=np.int32))
    want = EE.civil_parts(days[rows])
    for part, w in zip(PARTS, want):
        out = hip.date_extract(ctx, part, col, dsel, len(rows))
        got = ctx.download(out, np.int32, len(rows))
        ctx.free(out)
        wrong = np.flatnonzero(got != w)
        assert len(wrong) == 0, (f"part {part}: {len(wrong)} of {len(rows)} rows differ, days {int(days[rows][wrong].min())} .. "
                                 f"{int(days[rows][wrong].max())}; first: day {int(days[rows][wrong[0]])} gave {int(got[wrong[0]])}, the calendar says {int(w[wrong[0]])}")
    if dsel is not None:
        ctx.free(dsel)
    col.free()


def test_every_day_of_the_years_1_to_9999(ctx):
    """3 652 059 rows in one column: more than the 2048 x 256 rows one pass of the grid covers, so the grid-stride loop runs"""
    days = np.arange(EE.DAY_0001, EE.DAY_9999 + 1, dtype=np.int32)
    assert len(days) == 3_652_059 > 2048 * 256
    check_dates(ctx, days)


@pytest.mark.parametrize("n", [1, 255, 257, len(EE.DATE_EDGES)])
def test_date_edges(ctx, n):
    """the ends of the int32 domain, the days around INT32_MAX - 719468 (where a 32-bit `z + 719468` wraps), z = 0, and every era boundary;
    the first 22 edges are the named ones, so n = 255 and 257 hold them all. n = 1 probes INT32_MAX itself as well as INT32_MIN."""
    check_dates(ctx, EE.DATE_EDGES[:n])
    if n == 1:
        check_dates(ctx, np.array([EE.I32_MAX], dtype=np.int32))


@pytest.mark.parametrize("name", ["ascending", "descending", "repeated", "one"])
def test_date_extract_under_a_selection(ctx, name):
    days = EE.DATE_EDGES[:4099]
    check_dates(ctx, days, EE.date_selections(len(days))[name])


# ------------------------------------------------------------------ ph_float_eval
def dev_columns(ctx, cols):
    return [hip.DevColumn(ctx, c["type"], c["values"], scale=c["scale"], validity=SE.pack(c["valid"])) for c in cols]


def take(cols, sel):
    """the rows sel of reference columns, in sel's order (what a selection shows the program)"""
    return [dict(c, values=c["values"][sel], valid=None if c["valid"] is None else c["valid"][sel]) for c in cols]


def device_values(ctx, dev, prog, sel, n, wide, validity=None):
    dsel = None if sel is None else ctx.upload(np.ascontiguousarray(sel, dtype=np.int32))
    out = hip.float_eval(ctx, dev, prog, dsel, n, truth=False, wide=wide, want_validity=validity if validity is not None else False)
    if validity is not None:
        out = out[0]
    got = ctx.download(out, np.float64 if wide else np.float32, n)
    ctx.free(out)
    if dsel is not None:
        ctx.free(dsel)
    return got


def device_truth(ctx, dev, prog, sel, n, wide):
    dsel = None if sel is None else ctx.upload(np.ascontiguousarray(sel, dtype=np.int32))
    out = hip.float_eval(ctx, dev, prog, dsel, n, truth=True, wide=wide)
    got = ctx.download(out, np.int32, n)
    ctx.free(out)
    if dsel is not None:
        ctx.free(dsel)
    return got


def same_bits(got, want, what):
    g, w = EE.bits(got), EE.bits(want)
    bad = np.flatnonzero(g != w)
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(w)} rows differ; row {bad[0]}: {got[bad[0]]!r} ({int(g[bad[0]]):#x}), the reference says {want[bad[0]]!r} ({int(w[bad[0]]):#x})"


NULL_ROWS = 5000     # the columns the selections read from


def null_columns(n):
    """three operands: two NULL-able ones whose NULLs do not coincide (every combination occurs, also within one 64-row word and in its
    first and last bit) and one without a bitmap. The comparison a > b holds in every row, so only a NULL makes the truth 0."""
    i = np.arange(n)
    va = (i % 3 != 1) & (i % 64 != 0)
    vb = (i % 5 != 2) & (i % 64 != 63)
    a = EE.column(hip.PH_I32, 5 + i % 7, valid=va)
    b = EE.column(hip.PH_DEC64, 1 + i % 11, 2, valid=vb)
    c = EE.column(hip.PH_I64, 3 + i % 13)
    return [a, b, c]


@pytest.mark.parametrize("with_sel", [False, True], ids=["rows", "sel"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4097])
def test_float_eval_null_operands(ctx, n, with_sel):
    """a NULL operand: truth 0 in exactly those rows; in value mode the bitmap's first n bits are the AND of the operand validities, the
    documented (n + 63) / 64 * 8 bytes are all that is written, and the bits of the last word past row n - 1 are 0"""
    if with_sel:
        cols = null_columns(NULL_ROWS)
        rng = np.random.default_rng(n)
        sel = rng.integers(0, NULL_ROWS, n).astype(np.int32)       # unordered, rows repeated
        sel[0] = NULL_ROWS - 1
        seen = take(cols, sel)
    else:
        cols, sel = null_columns(n), None
        seen = cols
    dev = dev_columns(ctx, cols)
    valid = seen[0]["valid"] & seen[1]["valid"]
    if n >= 63:
        assert 0 < valid.sum() < n and (seen[0]["valid"] != seen[1]["valid"]).any()
    gt = [hip.X_COL(0), hip.X_COL(1), hip.X_OP(hip.PH_X_GT)]
    got = device_truth(ctx, dev, gt, sel, n, False)
    assert np.array_equal(got, EE.float_truth(gt, seen, False)) and np.array_equal(got, valid.astype(np.int32))
    lt = [hip.X_COL(1), hip.X_COL(0), hip.X_COL(2), hip.X_MUL, hip.X_OP(hip.PH_X_LT)]      # b < a * c in DOUBLE
    got = device_truth(ctx, dev, lt, sel, n, True)
    assert np.array_equal(got, EE.float_truth(lt, seen, True)) and np.array_equal(got, valid.astype(np.int32))
    size = hip.float_eval_validity_bytes(n)
    assert size == (n + 63) // 64 * 8
    for wide in (False, True):
        prog = [hip.X_COL(0), hip.X_COL(1), hip.X_MUL, hip.X_COL(2), hip.X_OP(hip.PH_X_DIV)]
        bitmap = ctx.upload(np.full(size + 64, 0xA5, dtype=np.uint8))
        got = device_values(ctx, dev, prog, sel, n, wide, validity=bitmap)
        raw = ctx.download(bitmap, np.uint8, size + 64)
        ctx.free(bitmap)
        want, want_valid = EE.float_program(prog, seen, wide)
        assert np.array_equal(want_valid, valid)
        bits = np.unpackbits(raw[:size], bitorder="little")
        assert np.array_equal(bits[:n].astype(bool), valid), f"wide={wide}: validity bits differ in rows {np.flatnonzero(bits[:n].astype(bool) != valid)[:8]}"
        assert not bits[n:].any(), "bits past row n - 1 of the last word are set"
        assert np.all(raw[size:] == 0xA5), f"wide={wide}: bytes past the documented {size} were written: {np.flatnonzero(raw[size:] != 0xA5)}"
        same_bits(got[valid], want[valid], f"values, wide={wide}")
    # no operand with a bitmap: the caller's buffer is left alone and every row is valid
    bitmap = ctx.upload(np.full(size + 64, 0xA5, dtype=np.uint8))
    got = device_values(ctx, dev[2:], [hip.X_COL(0), hip.X_F32(0.5), hip.X_MUL], sel, n, False, validity=bitmap)
    assert np.all(ctx.download(bitmap, np.uint8, size + 64) == 0xA5)
    same_bits(got, EE.float_program([hip.X_COL(0), hip.X_F32(0.5), hip.X_MUL], seen[2:], False)[0], "values of a NULL-free operand")
    ctx.free(bitmap)
    for d in dev:
        d.free()


def test_float_eval_wants_a_bitmap_for_null_able_values(ctx):
    dev = dev_columns(ctx, null_columns(65))
    with pytest.raises(hip.PlanHipError) as e:
        hip.float_eval(ctx, dev, [hip.X_COL(0), hip.X_COL(1), hip.X_MUL], None, 65, truth=False)
    assert e.value.code == hip.PH_EINVAL
    for d in dev:
        d.free()


@pytest.mark.parametrize("wide", [False, True], ids=["float", "double"])
@pytest.mark.parametrize("typ", [hip.PH_I32, hip.PH_DATE, hip.PH_I64, hip.PH_DEC64], ids=["i32", "date", "i64", "dec0"])
def test_float_eval_operand_casts(ctx, typ, wide):
    """INTEGER and DATE at +-(2^24 +- 1), +-(2^31 - 1) and INT32_MIN; BIGINT and DECIMAL(p,0) below and above 2^53 and beside a float32
    midpoint at 2^60: an integer reaches FLOAT in one rounding, a decimal through its nearest double — bit for bit, as the value itself
    and after one arithmetic step"""
    vals = EE.INT32_FLOAT_EDGES if typ in (hip.PH_I32, hip.PH_DATE) else EE.INT64_FLOAT_EDGES
    cols = [EE.column(typ, vals)]
    dev = dev_columns(ctx, cols)
    for prog in ([hip.X_COL(0)], [hip.X_COL(0), hip.X_F32(3.0), hip.X_MUL], [hip.X_F32(1.0), hip.X_COL(0), hip.X_OP(hip.PH_X_DIV)]):
        same_bits(device_values(ctx, dev, prog, None, len(vals), wide), EE.float_program(prog, cols, wide)[0], f"type {typ} wide={wide} program {prog}")
    dev[0].free()


def test_float_eval_takes_a_hugeint_as_the_decimal_it_is_carried_as(ctx):
    """A HUGEINT sum travels as a scale-0 decimal, and the device casts it as one (nearest double, then float32), which is what it documents.
    The reference casts a HUGEINT by tryCastBigintToFloat32, in one rounding: beside float32 midpoints above 2^53 the two part — counted
    here, recorded in DESIGN.md, not asserted away."""
    vals = EE.hugeint_values()
    cols = [EE.column(hip.PH_DEC64, vals, 0)]
    dev = dev_columns(ctx, cols)
    got = device_values(ctx, dev, [hip.X_COL(0)], None, len(vals), False)
    dev[0].free()
    same_bits(got, EE.float_program([hip.X_COL(0)], cols, False)[0], "DECIMAL(p,0) route")
    huge = np.array([EE.hugeint_f32(v) for v in vals.tolist()], dtype=np.float32)
    differ = int((EE.bits(got) != EE.bits(huge)).sum())
    print(f"HUGEINT route: {differ} of {len(vals)} crafted values above 2^53 round differently from the DECIMAL route the device takes")
    assert 0 < differ < len(vals)


def special_columns():
    x = EE.column(hip.PH_I32, [0, 1, -1, 3, 2 ** 24 + 1, EE.I32_MIN, 0, 7])
    zero = EE.column(hip.PH_I32, [0] * 8)
    small = EE.column(hip.PH_DEC64, [1, -1, 3, 0, 12345, 1, 1, 1], 19)          # 10^-19: squared it is a float32 denormal, cubed it is 0
    return [x, zero, small]


@pytest.mark.parametrize("wide", [False, True], ids=["float", "double"])
def test_float_eval_special_values(ctx, wide):
    """NaN, +-Inf, -0.0, the smallest normal and denormal as literals and as results (x / 0 = +-Inf, 0 / 0 = NaN), products and quotients
    that land in the denormal range — kept, not flushed —, and every comparison over all of them. No cast can reach the denormal range by
    itself (the smallest non-zero decimal is 10^-19), so the denormals come from arithmetic and literals."""
    cols = special_columns()
    dev = dev_columns(ctx, cols)
    n = len(cols[0]["values"])
    X, Z, S = hip.X_COL(0), hip.X_COL(1), hip.X_COL(2)
    DIV = hip.X_OP(hip.PH_X_DIV)
    progs = [[X, Z, DIV],                                                        # +-Inf and NaN
             [S, S, hip.X_MUL], [S, S, hip.X_MUL, S, hip.X_MUL],                 # 1e-38 (denormal in FLOAT), 1e-57 (0 in FLOAT)
             [X, hip.X_F32(EE.F32_TINY), hip.X_MUL, hip.X_F32(0.125), hip.X_MUL],
             [hip.X_F32(EE.F32_TINY), X, DIV], [X, hip.X_F32(EE.F32_DENORM), hip.X_MUL, X, DIV],
             [X, Z, DIV, X, Z, DIV, hip.X_SUB], [X, Z, DIV, hip.X_F32(0.0), hip.X_MUL]]     # Inf - Inf, Inf * 0
    for lit in EE.FLOAT_LITERALS:
        k = hip.X_F32(lit)
        progs += [[X, k, hip.X_MUL], [X, k, hip.X_ADD], [k, X, hip.X_SUB], [X, k, DIV], [k, X, DIV], [Z, k, hip.X_MUL], [X, Z, DIV, k, hip.X_ADD]]
    denormal_results = 0
    for prog in progs:
        want = EE.float_program(prog, cols, wide)[0]
        same_bits(device_values(ctx, dev, prog, None, n, wide), want, f"wide={wide} program {prog}")
        if not wide:
            denormal_results += int(((want != 0) & (np.abs(want) < EE.F32_TINY)).sum())
    assert wide or denormal_results >= 20                                        # the FLOAT programs really produce denormals
    ops = (hip.PH_X_GT, hip.PH_X_GE, hip.PH_X_LE, hip.PH_X_LT)
    hits = 0
    for lit in EE.FLOAT_LITERALS:
        k = hip.X_F32(lit)
        for op in ops:
            for prog in ([X, Z, DIV, k, hip.X_OP(op)], [k, X, Z, DIV, hip.X_OP(op)], [X, k, hip.X_OP(op)], [S, S, hip.X_MUL, k, hip.X_OP(op)],
                         [Z, k, hip.X_MUL, k, hip.X_OP(op)]):
                want = EE.float_truth(prog, cols, wide)
                got = device_truth(ctx, dev, prog, None, n, wide)
                assert np.array_equal(got, want), f"wide={wide} program {prog} (literal {lit!r}): {got.tolist()} against {want.tolist()}"
                hits += int(want.sum())
                if (op == hip.PH_X_LT) != wide:
                    assert not want.any()                                        # FLOAT has no <, DOUBLE has nothing else
    assert hits > 100
    for d in dev:
        d.free()
