"""The selection layer (ops_select.hip) at its edges, compared exactly: the exclusive scan that places the rows of every count / scan /
write operator in each of its four forms, column OP column, FLOAT / DOUBLE columns, a run of dictionary codes, the DECIMAL -> FLOAT /
DOUBLE casts over the whole int64 domain, and the small selection-vector primitives. Inputs and references: select_edges.py (plain
Python / numpy, checked without a device by test_select_edges_reference.py); the oracle is the second witness where it has the operation."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":   # the three-pass child: no conftest.py has prepared the path
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "tests")]

import oracle_lib as O
import select_edges as SE
from plan_amd import hip

pytestmark = pytest.mark.gpu

I32 = np.int32


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


def dl(ctx, p, dtype, n):
    return ctx.download(p, dtype, n) if n else np.empty(0, dtype)


def up(ctx, arr):
    arr = np.ascontiguousarray(arr)
    return ctx.upload(arr) if arr.nbytes else ctx.alloc(8)


def forms_delta(before, after):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def scan_on_device(ctx, v):
    """(exclusive sums as the device left them, total, {form: calls})"""
    dev = up(ctx, v)
    before = ctx.scan_forms()
    total = hip.dev_exclusive_scan_i32(ctx, dev, len(v))
    delta = forms_delta(before, ctx.scan_forms())
    got = dl(ctx, dev, I32, len(v))
    ctx.free(dev)
    return got, total, delta


def check_scan(ctx, n, kind, form):
    v = SE.scan_input(n, kind)
    got, total, delta = scan_on_device(ctx, v)
    ex, want_total = SE.scan_reference(v)
    assert delta == {form: 1}, (n, kind, delta)
    assert total == want_total, (n, kind)
    assert np.array_equal(got.astype(np.int64), ex), (n, kind)


# ------------------------------------------------------------------ 1. the scan, directly

@pytest.mark.parametrize("n", SE.SCAN_SIZES)
def test_exclusive_scan_every_element_and_total(ctx, n):
    """ph_dev_exclusive_scan_i32 against numpy's int64 cumsum on both sides of every switch point (1024, 16384) and of the 4096-element
    tiles, with totals up to exactly 2^31 - 1; ph_ctx_scan_forms says that the form the size calls for is the one that ran."""
    for kind in SE.SCAN_KINDS:
        check_scan(ctx, n, kind, SE.scan_form(n))


def sorted_agg_groups(ctx, n, seed):
    """one ph_agg_sink_sorted call in its one-pass form (it takes tiles and an epoch from the scan's states): (keys, sums, counts) and numpy's"""
    rng = np.random.default_rng(seed)
    keys = np.repeat(np.arange(n // 40 + 1, dtype=np.int64), rng.integers(40, 160, n // 40 + 1))[:n]
    vals = rng.integers(-10 ** 9, 10 ** 9, n).astype(np.int64)
    K, V = hip.DevColumn(ctx, hip.PH_I64, keys), hip.DevColumn(ctx, hip.PH_I64, vals)
    agg = hip.Agg(ctx, [hip.PH_I64], [(hip.PH_A_SUM, 0), (hip.PH_A_COUNT_STAR, -1)], 1024)
    assert agg.sink_sorted([K], [V], n)
    uk, first, cnt = np.unique(keys, return_index=True, return_counts=True)
    r = agg.finalize(room=len(uk))
    ctx.check_deferred()
    agg.free()
    K.free(); V.free()
    assert np.array_equal(r["keys"][:, 0], uk) and np.array_equal(r["first_row"], first)
    assert [s[0] for s in r["sum"]] == [int(x) for x in np.add.reduceat(vals.astype(object), first)]
    assert np.array_equal(r["count"][:, 1], cnt)


def test_scan_tile_states_across_calls_reallocations_and_the_streaming_aggregate(monkeypatch):
    """One fresh context: look-back scans whose sizes grow and shrink, so that the per-context tile states (first max(2 x tiles, 4096)
    of them) are allocated and then re-allocated twice — once by the streaming aggregate, which takes tiles from the same ticket counter
    and epochs from the same sequence, once by a scan —, with one-pass ph_agg_sink_sorted calls in between. Every result is exact."""
    monkeypatch.setenv("PH_STREAM_AGG_ONE_PASS", "1")
    ctx = hip.Ctx(0)
    try:
        steps = [("scan", 20_000), ("agg", 300_000), ("scan", 16_385), ("agg", 5_000_000),   # 4883 tiles of 1024 rows > 4096: states re-allocated
                 ("scan", 20_000), ("scan", 9766 * 4096 + 7), ("agg", 300_000),               # 9767 tiles > 2 x 4883: again
                 ("scan", 17_000_001), ("scan", 16_385), ("agg", 300_000), ("scan", 40_000_000), ("scan", 70_000)]
        for k, (what, n) in enumerate(steps):
            if what == "agg":
                sorted_agg_groups(ctx, n, k)
            else:
                for kind in ("random", "full"):
                    check_scan(ctx, n, kind, "lookback")
    finally:
        ctx.close()


# ------------------------------------------------------------------ 2. the three-pass form, in a process of its own

def three_pass_cases():
    return [(n, kind) for n in SE.SCAN_SIZES_ABOVE_SMALL for kind in ("random", "full")] + [(SE.SCAN_TWICE_THREE_PASS, "random")]


def three_pass_child():
    """(child process, PH_SCAN_THREE_PASS=1) one line per case: size, kind, digest of the result, the forms that ran"""
    ctx = hip.Ctx(0)
    for n, kind in three_pass_cases():
        got, total, delta = scan_on_device(ctx, SE.scan_input(n, kind))
        print("SCAN", n, kind, SE.scan_digest(got, total), ",".join(f"{k}={v}" for k, v in sorted(delta.items())), flush=True)
    ctx.close()
    print("DONE", flush=True)


def test_three_pass_scan_in_a_child_process():
    """PH_SCAN_THREE_PASS is read once per process: a fresh child runs every size above 16384 through the three-pass form (tile sums,
    their scan, add-back) and one size above 16384 x 4096, whose tile sums take the three-pass form again; it prints a digest of every
    result, compared here with numpy's. Nothing else starts on the device in this test after a child that failed."""
    env = dict(os.environ, PH_SCAN_THREE_PASS="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "three-pass-child"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("SCAN ")]
    assert r.stdout.rstrip().endswith("DONE") and len(lines) == len(three_pass_cases())
    for (n, kind), ln in zip(three_pass_cases(), lines):
        assert (int(ln[1]), ln[2]) == (n, kind)
        ex, total = SE.scan_reference(SE.scan_input(n, kind))
        assert ln[3] == SE.scan_digest(ex, total), (n, kind)
        tiles = -(-n // SE.SCAN_TILE)
        want = {"three_pass": 2, SE.scan_form(-(-tiles // SE.SCAN_TILE)): 1} if tiles > 16384 else {"three_pass": 1, SE.scan_form(tiles): 1}
        assert ln[4] == ",".join(f"{k}={v}" for k, v in sorted(want.items())), (n, kind, ln[4])


# ------------------------------------------------------------------ 3. the scan, through the operators

@pytest.mark.parametrize("n_in,form", [(2_097_152, "loop"), (2_097_153, "small"), (33_554_432, "small"), (33_554_433, "lookback")])
def test_filter_select_block_counts_on_both_switch_points(ctx, n_in, form):
    """ph_filter_select at 2048 rows per block — with an input selection, and with '!=' — over 1024, 1025, 16384 and 16385 blocks: the
    selection is numpy's, and the scan took the form the block count calls for."""
    rng = np.random.default_rng(n_in)
    n = n_in + 1000
    v = rng.integers(0, 100, n).astype(I32)
    d = hip.DevColumn(ctx, hip.PH_I32, v)
    sel = np.arange(n_in, dtype=np.int64)
    sel[n_in // 3:] += 1000                                    # an ascending selection that leaves rows out
    dsel = ctx.upload(sel.astype(I32))
    for op, k, hit in ((hip.PH_LT, 37, v[sel] < 37), (hip.PH_NE, 5, v[sel] != 5), (hip.PH_EQ, 99, v[sel] == 99)):
        before = ctx.scan_forms()
        out, cnt = hip.filter_select(ctx, d, n, op, hip.const(hip.PH_I32, i=k), sel_in=dsel, n_in=n_in)
        assert forms_delta(before, ctx.scan_forms()) == {form: 1}, (op, n_in)
        want = sel[hit]
        assert cnt == len(want) and np.array_equal(dl(ctx, out, I32, cnt), want.astype(I32)), (op, n_in)
        ctx.free(out)
    ctx.free(dsel)
    d.free()
    v = v[:n_in]
    d = hip.DevColumn(ctx, hip.PH_I32, v)                      # '!=' without a selection: the row-per-lane path as well
    before = ctx.scan_forms()
    out, cnt = hip.filter_select(ctx, d, n_in, hip.PH_NE, hip.const(hip.PH_I32, i=5))
    assert forms_delta(before, ctx.scan_forms()) == {form: 1}
    want = np.flatnonzero(v != 5)
    assert cnt == len(want) and np.array_equal(dl(ctx, out, I32, cnt), want.astype(I32))
    ctx.free(out)
    d.free()


# ------------------------------------------------------------------ 4. column OP column

COLS_TYPES = {"integer": (hip.PH_I32, O.OT_INT32, 0), "date": (hip.PH_DATE, O.OT_DATE, 0), "decimal": (hip.PH_DEC64, O.OT_DECIMAL, 2),
              "bigint": (hip.PH_I64, O.OT_INT64, 0), "code": (hip.PH_CODE8, O.OT_CODE8, 0)}


@pytest.mark.parametrize("kind", SE.COLS_KINDS)
@pytest.mark.parametrize("nulls", SE.COLS_NULLS)
def test_filter_select_cols_against_numpy_and_the_oracle(ctx, kind, nulls):
    """ph_filter_select_cols for every type pair it knows, all six operators (the pairs selectOperation lacks select nothing), NULLs on
    either side, with and without a selection, sizes around the 256-row rounds and the 2048-row blocks, values at the types' ends."""
    ht, ot, scale = COLS_TYPES[kind]
    selected = 0
    for n in SE.COLS_SIZES:
        a, b, va, vb = SE.cols_input(kind, n, nulls)
        A = hip.DevColumn(ctx, ht, a, scale=scale, validity=SE.pack(va))
        B = hip.DevColumn(ctx, ht, b, scale=scale, validity=SE.pack(vb))
        oa, ob = O.col(ot, a, scale=scale, validity=SE.pack(va)), O.col(ot, b, scale=scale, validity=SE.pack(vb))
        for sel in (None, SE.cols_selection(n)):
            dsel = None if sel is None else up(ctx, sel.astype(I32))
            n_in = n if sel is None else len(sel)
            for op in SE.ALL_OPS:
                out, cnt = hip.filter_select_cols(ctx, A, B, n, op, sel_in=dsel, n_in=n_in)
                got = dl(ctx, out, I32, cnt).astype(np.int64)
                ctx.free(out)
                want = SE.cols_reference(kind, op, a, b, va, vb, sel)
                assert cnt == len(want) and np.array_equal(got, want), (kind, nulls, n, op, sel is not None)
                assert np.array_equal(O.select_cols(oa, op, ob, sel_in=sel, n=n), want), (kind, nulls, n, op)
                selected += cnt
            if dsel is not None:
                ctx.free(dsel)
        A.free(); B.free()
    assert (selected > 0) == bool(SE.COLS_OPS[kind])


def test_filter_select_cols_refuses_mixed_scales_and_types(ctx):
    n = 100
    cols = {"i32": hip.DevColumn(ctx, hip.PH_I32, np.arange(n, dtype=I32)), "date": hip.DevColumn(ctx, hip.PH_DATE, np.arange(n, dtype=I32)),
            "i64": hip.DevColumn(ctx, hip.PH_I64, np.arange(n, dtype=np.int64)), "dec2": hip.DevColumn(ctx, hip.PH_DEC64, np.arange(n, dtype=np.int64), scale=2),
            "dec4": hip.DevColumn(ctx, hip.PH_DEC64, np.arange(n, dtype=np.int64), scale=4), "code": hip.DevColumn(ctx, hip.PH_CODE8, np.arange(n, dtype=np.uint8))}
    for x, y in (("dec2", "dec4"), ("dec4", "dec2"), ("i32", "date"), ("i32", "i64"), ("i64", "dec2"), ("code", "i32"), ("date", "dec2")):
        for op in SE.ALL_OPS:
            with pytest.raises(hip.PlanHipError) as e:
                hip.filter_select_cols(ctx, cols[x], cols[y], n, op)
            assert e.value.code == hip.PH_EUNSUPPORTED, (x, y, op)
    for c in cols.values():
        c.free()


# ------------------------------------------------------------------ 5. FLOAT and DOUBLE columns

@pytest.mark.parametrize("dtype,ht,ot,ks", [
    (np.float32, hip.PH_F32, O.OT_FLOAT, (1.5, 0.0, -0.0, float(np.float32(1e-40)), -2.75, float("inf"), float("-inf"), float("nan"))),
    (np.float64, hip.PH_F64, O.OT_DOUBLE, (1.5, 0.0, -0.0, 5e-324, -2.75, float("inf"), float("-inf"), float("nan")))])
def test_float_and_double_columns_against_the_oracle(ctx, dtype, ht, ot, ks):
    """SK_F32 / SK_F64: every operator (FLOAT has > >= <=, DOUBLE has <; the rest select nothing) over NaN, both zeros, both infinities,
    denormals and the constant's two neighbours, with NULLs, with and without a selection. A NaN constant: never true for FLOAT's
    operators; DOUBLE's '<' is GreaterFloat(k, v), which holds for every value that is no NaN."""
    for k in ks:
        for n in (1, 257, 70_001):
            v = SE.float_values(dtype, k, n, seed=3)
            valid = np.random.default_rng(n).random(n) > 0.1
            D = hip.DevColumn(ctx, ht, v, validity=SE.pack(valid))
            oc = O.col(ot, v, validity=SE.pack(valid))
            for sel in (None, SE.cols_selection(n)):
                dsel = None if sel is None else up(ctx, sel.astype(I32))
                n_in = n if sel is None else len(sel)
                for op in SE.ALL_OPS + (SE.OP_LIKE, SE.OP_NOTLIKE):
                    out, cnt = hip.filter_select(ctx, D, n, op, hip.const(ht, f=k), sel_in=dsel, n_in=n_in)
                    got = dl(ctx, out, I32, cnt).astype(np.int64)
                    ctx.free(out)
                    want = SE.float_select_reference(dtype, op, v, k, valid, sel)
                    assert np.array_equal(got, want), (dtype, k, n, op, sel is not None)
                    assert np.array_equal(O.select(oc, op, O.const(ot, f=k), sel_in=sel, n=n), want), (dtype, k, n, op)
                if dsel is not None:
                    ctx.free(dsel)
            D.free()


# ------------------------------------------------------------------ 6. '=' against a run of dictionary codes

def test_run_of_codes_constant(ctx):
    """k.type == PH_CODE8 names the codes k.i .. k.scale: '=' selects the rows whose code lies inside (ends clipped to 0..255, an empty or
    out-of-range run selects nothing), on the four-values-per-lane path and, under a selection, on the row-per-lane path. A run has no
    order and no complement here: every other operator is refused, which is asserted."""
    rng = np.random.default_rng(6)
    for n in (1, 255, 4097, 70_001):
        codes = rng.integers(0, 256, n).astype(np.uint8)
        codes[: min(n, 4)] = np.array([0, 255, 3, 9], np.uint8)[: min(n, 4)]
        valid = rng.random(n) > 0.1
        for val in (None, valid):
            D = hip.DevColumn(ctx, hip.PH_CODE8, codes, validity=SE.pack(val))
            for sel in (None, SE.cols_selection(n)):
                dsel = None if sel is None else up(ctx, sel.astype(I32))
                n_in = n if sel is None else len(sel)
                for lo, hi in SE.RUN_CASES:
                    k = hip.const(hip.PH_CODE8, i=lo, scale=hi)
                    out, cnt = hip.filter_select(ctx, D, n, hip.PH_EQ, k, sel_in=dsel, n_in=n_in)
                    got = dl(ctx, out, I32, cnt).astype(np.int64)
                    ctx.free(out)
                    assert np.array_equal(got, SE.code_run_reference(codes, lo, hi, val, sel)), (n, lo, hi, sel is not None)
                if n_in:
                    for op in (hip.PH_NE, hip.PH_LT, hip.PH_LE, hip.PH_GT, hip.PH_GE, hip.PH_LIKE):
                        with pytest.raises(hip.PlanHipError) as e:
                            hip.filter_select(ctx, D, n, op, hip.const(hip.PH_CODE8, i=3, scale=9), sel_in=dsel, n_in=n_in)
                        assert e.value.code == hip.PH_EUNSUPPORTED
                if dsel is not None:
                    ctx.free(dsel)
            D.free()


# ------------------------------------------------------------------ 7. DECIMAL -> FLOAT / DOUBLE

def cast_column(scale):
    vals = np.concatenate([SE.cast_inputs(scale), SE.cast_random(scale, 100_000, seed=7), SE.cast_random_below(scale, 20_000, seed=7)])
    ref64, ref32 = SE.cast_reference(vals, scale)
    return vals, ref64, ref32


@pytest.mark.parametrize("scale", SE.CAST_SCALES)
def test_decimal_column_against_float_constants_beside_every_midpoint(ctx, scale):
    """ph_filter_select, DECIMAL column against a FLOAT constant (> >= <=), the constants being the two floats on either side of every
    midpoint the generated values surround: the rows are those whose reference cast — the nearest double of the decimal, narrowed —
    satisfies the comparison, for |unscaled| below and above 2^53 alike. The oracle agrees on a selection that holds every generated value."""
    vals, _, ref32 = cast_column(scale)
    n, ngen = len(vals), len(SE.cast_inputs(scale))
    D = hip.DevColumn(ctx, hip.PH_DEC64, vals, scale=scale)
    oc = O.col(O.OT_DECIMAL, vals, scale=scale)
    sel = np.concatenate([np.arange(ngen, dtype=np.int64), np.arange(ngen, n, 40, dtype=np.int64)])
    dsel = ctx.upload(sel.astype(I32))
    wrong = 0
    for flo, fhi, _ in SE.cast_midpoints(scale) + SE.cast_midpoints(scale, below=True):
        for kf in (flo, fhi):
            for op, fn in ((hip.PH_GT, np.greater), (hip.PH_GE, np.greater_equal), (hip.PH_LE, np.less_equal)):
                k = hip.const(hip.PH_F32, f=float(kf))
                out, cnt = hip.filter_select(ctx, D, n, op, k)
                got = dl(ctx, out, I32, cnt).astype(np.int64)
                ctx.free(out)
                want = np.flatnonzero(fn(ref32, kf))
                wrong += int(len(np.setxor1d(got, want)))
                out, cnt = hip.filter_select(ctx, D, n, op, k, sel_in=dsel, n_in=len(sel))
                got_sel = dl(ctx, out, I32, cnt).astype(np.int64)
                ctx.free(out)
                want_sel = sel[fn(ref32[sel], kf)]
                wrong += int(len(np.setxor1d(got_sel, want_sel)))
                assert np.array_equal(O.select(oc, op, O.const(O.OT_FLOAT, f=float(kf)), sel_in=sel), want_sel), (scale, kf, op)
    ctx.free(dsel)
    D.free()
    print(f"scale {scale}: {wrong} rows selected differently from the reference cast")
    assert wrong == 0


@pytest.mark.parametrize("scale", SE.CAST_SCALES)
@pytest.mark.parametrize("wide", [False, True])
def test_float_eval_returns_the_reference_cast(ctx, scale, wide):
    """ph_float_eval's column operand: the FLOAT (wide=False) or DOUBLE (wide=True) value of a DECIMAL column is the reference's cast, bit
    for bit, over the generated values and 100 000 random ones of at least 2^53 — and under a selection."""
    vals, ref64, ref32 = cast_column(scale)
    want = ref64 if wide else ref32
    dt = np.float64 if wide else np.float32
    n = len(vals)
    D = hip.DevColumn(ctx, hip.PH_DEC64, vals, scale=scale)
    out = hip.float_eval(ctx, [D], [hip.X_COL(0)], None, n, truth=False, wide=wide)
    got = dl(ctx, out, dt, n)
    ctx.free(out)
    diff = int((got.view(np.uint64 if wide else np.uint32) != want.view(np.uint64 if wide else np.uint32)).sum())
    small = np.abs(ref64) < 2.0 ** 52 / 10 ** scale
    print(f"scale {scale}, {'DOUBLE' if wide else 'FLOAT'}: {diff} of {n} values differ from the reference cast ({int((got[small] != want[small]).sum())} below 2^53)")
    assert diff == 0
    sel = np.arange(0, n, 3, dtype=np.int64)
    dsel = ctx.upload(sel.astype(I32))
    out = hip.float_eval(ctx, [D], [hip.X_COL(0)], dsel, len(sel), truth=False, wide=wide)
    assert np.array_equal(dl(ctx, out, dt, len(sel)), want[sel])
    ctx.free(out); ctx.free(dsel)
    D.free()


def test_float_eval_double_less_than_with_a_nan_side(ctx):
    """DOUBLE '<' is lessFloat64Op = util.GreaterFloat(right, left): a NaN on the right is greater than every number, a NaN on the left never less"""
    q = np.arange(-3, 500, dtype=I32)
    Q = hip.DevColumn(ctx, hip.PH_I32, q)
    nan = float("nan")
    for prog, want in (([hip.X_COL(0), hip.X_F32(nan), hip.X_OP(hip.PH_X_LT)], 1), ([hip.X_F32(nan), hip.X_COL(0), hip.X_OP(hip.PH_X_LT)], 0),
                       ([hip.X_F32(nan), hip.X_F32(nan), hip.X_OP(hip.PH_X_LT)], 0)):
        out = hip.float_eval(ctx, [Q], prog, None, len(q), wide=True)
        assert np.array_equal(dl(ctx, out, I32, len(q)), np.full(len(q), want, I32))
        ctx.free(out)
    Q.free()


# ------------------------------------------------------------------ 8. the primitives

@pytest.mark.parametrize("n", [1, 255, 257, 70_001])
def test_dev_iota_and_sel_mark(ctx, n):
    p = hip.dev_iota(ctx, n)
    assert np.array_equal(dl(ctx, p, I32, n), np.arange(n, dtype=I32))
    ctx.free(p)
    rng = np.random.default_rng(n)
    sel = np.flatnonzero(rng.random(n) < 0.4).astype(I32)
    sel = np.concatenate([sel, sel[: len(sel) // 2]])           # rows named twice are marked once
    marks = ctx.upload(np.zeros(n + 8, np.uint8))
    dsel = up(ctx, sel)
    hip.sel_mark(ctx, dsel, len(sel), marks)
    want = np.zeros(n + 8, np.uint8)
    want[sel] = 1
    assert np.array_equal(dl(ctx, marks, np.uint8, n + 8), want)
    ctx.free(marks); ctx.free(dsel)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 70_001])
def test_rowid_validity(ctx, n):
    rng = np.random.default_rng(n)
    ids = rng.integers(-3, 50, n).astype(I32)
    ids[0] = -1
    ids[-1] = SE.I32_MIN if n > 1 else -1
    for fill in (ids, np.full(n, 5, I32), np.full(n, -1, I32)):
        d = ctx.upload(fill)
        bm = hip.rowid_validity(ctx, d, n)
        got = dl(ctx, bm, np.uint8, (n + 7) // 8)
        assert np.array_equal(got, np.packbits(fill >= 0, bitorder="little"))      # packbits pads with zeros: no stray bit beyond n
        ctx.free(d); ctx.free(bm)


@pytest.mark.parametrize("n", [1, 255, 70_001])
def test_widen_codes(ctx, n):
    rng = np.random.default_rng(n)
    codes = rng.integers(0, 256, n).astype(np.uint8)
    codes[0] = 201
    D = hip.DevColumn(ctx, hip.PH_CODE8, codes)
    out = hip.widen_codes(ctx, D, None, n)
    assert np.array_equal(dl(ctx, out, I32, n), codes.astype(I32))
    ctx.free(out)
    sel = rng.integers(0, n, 2 * n + 3).astype(I32)
    sel[::7] = -1                                                 # a negative row id reads row 0
    sel[1::11] = SE.I32_MIN
    dsel = ctx.upload(sel)
    out = hip.widen_codes(ctx, D, dsel, len(sel))
    assert np.array_equal(dl(ctx, out, I32, len(sel)), codes[np.maximum(sel, 0)].astype(I32))
    ctx.free(out); ctx.free(dsel)
    D.free()


@pytest.mark.parametrize("n_rows", [1, 15, 17, 4097, 70_001])
def test_sel_union_overlapping_and_repeated_children(ctx, n_rows):
    rng = np.random.default_rng(n_rows)
    a = np.flatnonzero(rng.random(n_rows) < 0.5).astype(I32)
    b = np.flatnonzero(rng.random(n_rows) < 0.5).astype(I32)
    c = np.array([n_rows - 1], I32)
    empty = np.empty(0, I32)
    for children in ([a, b], [a, a], [a, b, a, c], [empty, b, empty], [c, c, c]):
        ptrs = [up(ctx, x) for x in children]
        out, cnt = hip.sel_union(ctx, ptrs, [len(x) for x in children], n_rows)
        want = np.unique(np.concatenate(children)).astype(I32)
        assert cnt == len(want) and np.array_equal(dl(ctx, out, I32, cnt), want)
        ctx.free(out)
        for p in ptrs:
            ctx.free(p)


@pytest.mark.parametrize("n_rows", [1, 17, 4097, 70_001])
def test_sel_difference_with_a_parent_selection(ctx, n_rows):
    rng = np.random.default_rng(n_rows)
    parent = np.flatnonzero(rng.random(n_rows) < 0.7).astype(I32)
    if len(parent) == 0:
        parent = np.array([0], I32)
    child = parent[rng.random(len(parent)) < 0.4]
    dpar = ctx.upload(parent)
    for ch in (child, parent, np.empty(0, I32), parent[:1], parent[-1:]):
        dch = up(ctx, ch)
        out, cnt = hip.sel_difference(ctx, dpar, len(parent), dch, len(ch), n_rows)
        want = np.setdiff1d(parent, ch).astype(I32)
        assert cnt == len(want) and np.array_equal(dl(ctx, out, I32, cnt), want)
        ctx.free(out)
        out, cnt = hip.sel_difference(ctx, None, n_rows, dch, len(ch), n_rows)      # no parent: the identity over n_rows
        want = np.setdiff1d(np.arange(n_rows, dtype=I32), ch).astype(I32)
        assert cnt == len(want) and np.array_equal(dl(ctx, out, I32, cnt), want)
        ctx.free(out); ctx.free(dch)
    ctx.free(dpar)


@pytest.mark.parametrize("ht,dt", [(hip.PH_I32, np.int32), (hip.PH_DEC64, np.int64)])
@pytest.mark.parametrize("n", [1, 257, 70_001])
def test_scatter_without_a_selection_and_for_integers(ctx, ht, dt, n):
    """ph_scatter: out[sel[i]] = values[i] (sel = None: out[i]) for the valid values only — an invalid source row leaves the target value
    and its validity bit untouched —, with and without a validity output."""
    rng = np.random.default_rng(n + int(ht))
    info = np.iinfo(dt)
    vals = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    valid = rng.random(n) > 0.3
    m = 2 * n + 5
    for vv in (None, valid):
        V = hip.DevColumn(ctx, ht, vals, scale=2 if ht == hip.PH_DEC64 else 0, validity=SE.pack(vv))
        ok = np.ones(n, bool) if vv is None else vv
        for sel in (None, rng.permutation(m)[:n].astype(I32)):
            rows = np.arange(n) if sel is None else sel
            dsel = None if sel is None else ctx.upload(sel)
            for with_validity in (False, True):
                before = rng.integers(-99, 99, m).astype(dt)
                out = ctx.upload(before)
                nbytes = (m + 31) // 32 * 4
                bits0 = rng.integers(0, 256, nbytes).astype(np.uint8)
                oval = ctx.upload(bits0) if with_validity else None
                hip.scatter(ctx, V, dsel, n, out, oval)
                want = before.copy()
                want[rows[ok]] = vals[ok]
                assert np.array_equal(dl(ctx, out, dt, m), want), (n, vv is None, sel is None)
                if with_validity:
                    wbits = np.unpackbits(bits0, bitorder="little")
                    wbits[rows[ok]] = 1
                    assert np.array_equal(dl(ctx, oval, np.uint8, nbytes), np.packbits(wbits, bitorder="little"))
                    ctx.free(oval)
                ctx.free(out)
            if dsel is not None:
                ctx.free(dsel)
        V.free()


@pytest.mark.parametrize("ht,dt", [(hip.PH_CODE8, np.uint8), (hip.PH_I32, np.int32), (hip.PH_DEC64, np.int64)])
def test_gather_negative_indices_read_row_zero(ctx, ht, dt):
    rng = np.random.default_rng(int(ht))
    src = rng.integers(0, 200, 5000).astype(dt)
    S = hip.DevColumn(ctx, ht, src)
    for n in (1, 2047, 2049, 70_001):
        idx = rng.integers(0, len(src), n).astype(I32)
        idx[::5] = -1
        idx[2::13] = SE.I32_MIN
        didx = ctx.upload(idx)
        out = hip.gather(ctx, S, didx, n)
        assert np.array_equal(dl(ctx, out, dt, n), src[np.maximum(idx, 0)])
        ctx.free(out); ctx.free(didx)
    S.free()


if __name__ == "__main__":
    assert sys.argv[1:] == ["three-pass-child"] and os.environ.get("PH_SCAN_THREE_PASS")
    three_pass_child()
