"""The references of the selection-layer edge tests, checked without a device: the Python cast agrees with the oracle's odec_float64 on
every generated value, the generated values really separate `(double)unscaled / 10^scale` from the reference's cast (so the GPU tests can
fail), the scan inputs keep the scan's contract, and the numpy column comparison agrees with the oracle's."""
import numpy as np
import pytest

import oracle_lib as O
import select_edges as SE


@pytest.mark.parametrize("scale", SE.CAST_SCALES)
def test_cast_reference_is_the_oracles_decimal_to_double(scale):
    vals = np.concatenate([SE.cast_inputs(scale), SE.cast_random(scale, 2000, seed=1)])
    want64, want32 = SE.cast_reference(vals, scale)
    got = np.array([O.dec_float64(v, scale) for v in vals.tolist()], dtype=np.float64)
    assert np.array_equal(got, want64)
    assert np.array_equal(got.astype(np.float32), want32)
    # the int64 / 2^53 edges are among the inputs, on both sides of zero
    for v in (SE.EXACT - 1, SE.EXACT, SE.EXACT + 1, SE.I64_MAX):
        assert v in vals and -v in vals


def test_cast_inputs_are_deterministic_and_surround_every_midpoint():
    for scale in SE.CAST_SCALES:
        a, b = SE.cast_inputs(scale), SE.cast_inputs(scale)
        assert np.array_equal(a, b) and np.all(np.diff(a) > 0)
        _, ref32 = SE.cast_reference(a, scale)
        for flo, fhi, _ in SE.cast_midpoints(scale) + SE.cast_midpoints(scale, below=True):
            assert (ref32 == flo).any() and (ref32 == fhi).any(), (scale, flo, fhi)    # values that round to either neighbour


@pytest.mark.parametrize("scale", [s for s in SE.CAST_SCALES if s >= 1])
def test_generated_values_separate_the_division_from_the_reference(scale):
    vals = SE.cast_inputs(scale)
    ref64, ref32 = SE.cast_reference(vals, scale)
    d32 = int((SE.cast_by_division(vals, scale, wide=False) != ref32).sum())
    d64 = int((SE.cast_by_division(vals, scale, wide=True) != ref64).sum())
    print(f"scale {scale}: {len(vals)} generated values, division differs from the reference in {d32} FLOAT and {d64} DOUBLE results")
    assert d32 >= 1 and d64 >= 1
    # below 2^53 the division IS the reference: those rows must keep their path
    small = np.abs(vals.astype(object)) < SE.EXACT
    assert small.sum() > 500
    assert np.array_equal(SE.cast_by_division(vals[small.astype(bool)], scale, wide=True), ref64[small.astype(bool)])
    below = SE.cast_random_below(scale, 20_000, seed=7)
    assert np.all(np.abs(below) < SE.EXACT) and np.array_equal(SE.cast_by_division(below, scale, wide=True), SE.cast_reference(below, scale)[0])


@pytest.mark.parametrize("scale", [1, 2, 4, 6])
def test_random_values_above_2_53_differ_in_a_real_share(scale):
    vals = SE.cast_random(scale, 100_000, seed=7)
    assert np.all(np.abs(vals.astype(object)) >= SE.EXACT)
    ref64, ref32 = SE.cast_reference(vals, scale)
    d64 = int((SE.cast_by_division(vals, scale, wide=True) != ref64).sum())
    d32 = int((SE.cast_by_division(vals, scale, wide=False) != ref32).sum())
    print(f"scale {scale}: DOUBLE differs in {d64} of {len(vals)} random values ({100.0 * d64 / len(vals):.2f} %), FLOAT in {d32}")
    assert d64 > 0


def test_the_issues_example_values():
    """100 * (2^50 + 2^26) + 9 .. 12 at scale 2: the reference gives 2^50, the division the next float up"""
    vals = np.arange(112589997395148809, 112589997395148813, dtype=np.int64)
    assert int(vals[0]) == 100 * (2 ** 50 + 2 ** 26) + 9
    _, ref32 = SE.cast_reference(vals, 2)
    assert np.all(ref32 == np.float32(1125899906842624.0))
    assert np.all(SE.cast_by_division(vals, 2, wide=False) == np.float32(1125900041060352.0))
    assert all(v in SE.cast_inputs(2) for v in vals)


def test_scan_inputs_keep_the_contract():
    for n in SE.SCAN_SIZES:
        for kind in SE.SCAN_KINDS:
            if n > 2_000_000 and (n, kind) != (SE.SCAN_SIZES[-1], "full"):      # the large sizes follow the same rule: one stands for them
                continue
            v = SE.scan_input(n, kind)
            ex, total = SE.scan_reference(v)
            assert len(v) == n and v.dtype == np.int32 and (n == 0 or v.min() >= 0)
            assert 0 <= total <= SE.I32_MAX and (n == 0 or int(ex[-1]) + int(v[-1]) == total)
            if kind == "full" and n:
                assert total == SE.I32_MAX
    assert [SE.scan_form(n) for n in (0, 1024, 1025, 16384, 16385)] == ["loop", "loop", "small", "small", "lookback"]
    assert {SE.scan_form(n) for n in SE.SCAN_SIZES} == {"loop", "small", "lookback"}
    assert -(-SE.SCAN_TWICE_THREE_PASS // SE.SCAN_TILE) > 16384


KIND_TYPES = {"integer": (O.OT_INT32, 0), "date": (O.OT_DATE, 0), "decimal": (O.OT_DECIMAL, 2), "bigint": (O.OT_INT64, 0)}


@pytest.mark.parametrize("kind", ["integer", "date", "decimal", "bigint"])
def test_select_cols_binding_equals_the_numpy_reference(kind):
    ot, scale = KIND_TYPES[kind]
    seen = 0
    for n in SE.COLS_SIZES:
        for nulls in SE.COLS_NULLS:
            a, b, va, vb = SE.cols_input(kind, n, nulls)
            ca, cb = O.col(ot, a, scale=scale, validity=SE.pack(va)), O.col(ot, b, scale=scale, validity=SE.pack(vb))
            for sel in (None, SE.cols_selection(n)):
                for op in SE.ALL_OPS:
                    got = O.select_cols(ca, op, cb, sel_in=sel, n=n)
                    want = SE.cols_reference(kind, op, a, b, va, vb, sel)
                    assert np.array_equal(got, want), (kind, n, nulls, op, sel is not None)
                    seen += len(want)
    assert (seen > 0) == bool(SE.COLS_OPS[kind])


def test_float_select_reference_equals_the_oracle():
    """FLOAT / DOUBLE columns against a constant: the numpy restatement and the oracle agree, NaN and the zeros included"""
    for dtype, ot, ks in ((np.float32, O.OT_FLOAT, (1.5, 0.0, -0.0, float(np.float32(1e-40)), float("inf"), float("nan"))),
                          (np.float64, O.OT_DOUBLE, (1.5, 0.0, -0.0, 5e-324, float("-inf"), float("nan")))):
        for k in ks:
            v = SE.float_values(dtype, k, 5000)
            assert np.isnan(v).any() and (v == 0).any() and np.isinf(v).any()
            valid = np.random.default_rng(3).random(len(v)) > 0.1
            c = O.col(ot, v, validity=SE.pack(valid))
            for op in SE.ALL_OPS + (SE.OP_LIKE, SE.OP_NOTLIKE):
                got = O.select(c, op, O.const(ot, f=k), n=len(v))
                assert np.array_equal(got, SE.float_select_reference(dtype, op, v, k, valid)), (dtype, k, op)
