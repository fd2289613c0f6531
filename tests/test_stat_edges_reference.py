"""The inputs and the reference of the column-statistics edge tests (stat_edges.py), checked without a device: `reference` against a
brute-force restatement in plain Python loops, every built column against the defect it claims, and the sizes and positions against the
boundaries they are there for. A GPU test over inputs that lost their defect would still pass; this file is what fails."""
import numpy as np
import pytest

import stat_edges as S

SMALL = [n for n in S.N if n <= 300]


def brute(values, typ, validity=None):
    """include/planhip.h's definitions once more, row by row over Python integers (written apart from stat_edges.reference)"""
    x = [int(a) for a in values]
    n = len(x)
    out = dict(range=None, ascending=False, strict=False, run_len=0, narrow=None)
    if typ in ("F32", "F64", "STR") or n == 0:
        return out
    lo = hi = x[0]
    for a in x:
        if a < lo:
            lo = a
        if a > hi:
            hi = a
    out["range"] = (lo, hi)
    if typ == "CODE8" or validity is not None:
        return out
    asc = strict = True
    for i in range(n - 1):
        if x[i + 1] < x[i]:
            asc = False
        if x[i + 1] <= x[i]:
            strict = False
    out["ascending"], out["strict"] = asc, strict
    if asc and not strict:
        for c in range(2, 65):
            if c * (hi - lo + 1) == n and all(x[i] == lo + i // c for i in range(n)):
                out["run_len"] = c
    width = {"I32": 4, "DATE": 4, "I64": 8, "DEC64": 8}[typ]
    for w in (4, 2, 1):
        if hi - lo <= 2 ** (8 * w) - 1 and w < width:
            out["narrow"] = (w, lo)
    return out


def all_cases(n):
    """(name, type, values, claim, position) of every builder at n rows"""
    for typ in S.RANGED:
        for vs in S.VALUE_SETS:
            if vs.startswith("constant"):
                yield (f"extremum {vs}", typ) + S.extremum_at(n, typ, None, None, vs)
            else:
                for p, q in S.position_pairs(n):
                    yield (f"extremum {vs} {p} {q}", typ) + S.extremum_at(n, typ, p, q, vs)
    for typ in S.ORDERED:
        for p in S.pair_positions(n):
            for base, kind in (("small", "equal"), ("small", "descending"), ("wide", "equal"), ("wide", "descending"), ("max_to_min", "descending")):
                yield (f"order {base} {kind} {p}", typ) + S.order_defect(n, typ, p, kind, base)
        if n >= 2:
            yield ("order equal_at_max", typ) + S.order_defect(n, typ, n - 2, "equal", "equal_at_max")
        for which in S.ORDER_WHOLE:
            yield (f"order {which}", typ) + S.order_whole(n, typ, which)
        for span in S.SPANS[S.WIDTH[typ]]:
            for base in S.narrow_bases(typ, span):
                if span == 0:
                    yield (f"narrow {span} {base}", typ) + S.narrow_span(typ, span, base, n)
                for p, q in S.position_pairs(n):
                    yield (f"narrow {span} {base} {p} {q}", typ) + S.narrow_span(typ, span, base, n, p, q)


def run_cases(max_rows):
    """(name, type, values, claim, position) of the run builder at every (c, nruns) of at most max_rows rows"""
    for c in S.RUN_LENGTHS:
        for nruns in (1, S.RUNS_ABOUT_1000[c], S.RUNS_PAST_STRIDE[c]):
            if c * nruns > max_rows:
                continue
            for typ in S.ORDERED:
                for first in S.run_firsts(typ, nruns):
                    yield (f"run {c}x{nruns} from {first}", typ) + S.run_defect(c, nruns, first, typ=typ)
                    for p in S.uneven_rows(c, nruns, S.positions(c * nruns)):
                        yield (f"run {c}x{nruns} from {first} uneven {p}", typ) + S.run_defect(c, nruns, first, p, "uneven", typ)
                    if first + nruns <= S.LIMITS[typ][1]:
                        yield (f"run {c}x{nruns} from {first} last+1", typ) + S.run_defect(c, nruns, first, None, "last_plus_one", typ)


def check_claim(name, typ, v, claim, pos):
    x = [int(a) for a in v]
    n = len(x)
    assert v.dtype == S.DTYPE[typ], name
    if "range" in claim:
        assert (min(x), max(x)) == claim["range"], name
        if name.startswith("extremum") and pos is not None:   # one minimum, one maximum, where the builder says
            assert [i for i in range(n) if x[i] == claim["range"][0]] == [pos[0]], name
            assert [i for i in range(n) if x[i] == claim["range"][1]] == [pos[1]], name
        if name.startswith("narrow") and claim["range"][0] != claim["range"][1]:
            assert x[pos[0]] == claim["range"][0] and x[pos[1]] == claim["range"][1], name
    if "bad_pairs" in claim:
        assert [i for i in range(n - 1) if x[i + 1] <= x[i]] == list(claim["bad_pairs"]), name
        assert claim["ascending"] == (not any(x[i + 1] < x[i] for i in range(n - 1))), name
        assert claim["strict"] == (not claim["bad_pairs"]), name
        if pos is not None:
            assert list(claim["bad_pairs"]) == [pos], name
    if "odd_row" in claim:
        c = claim["c"]
        assert [i for i in range(n) if x[i] != claim["min"] + i // c] == ([] if claim["odd_row"] is None else [claim["odd_row"]]), name
        assert claim["odd_row"] == pos and min(x) == claim["min"], name


def check_reference(name, typ, v, claim):
    ref = S.reference(v, typ)
    assert ref == brute(v, typ), name
    for k in ("range", "ascending", "strict", "run_len", "narrow"):
        if k in claim:
            assert ref[k] == claim[k], (name, k)


@pytest.mark.parametrize("n", SMALL)
def test_builders_hold_their_claim_and_reference_equals_brute_force(n):
    count = 0
    for name, typ, v, claim, pos in all_cases(n):
        assert len(v) == n
        check_claim(name, typ, v, claim, pos)
        check_reference(name, typ, v, claim)
        count += 1
    assert count > 20


def test_run_builder_and_reference_up_to_1040_rows():
    seen = set()
    for name, typ, v, claim, pos in run_cases(1040):
        check_claim(name, typ, v, claim, pos)
        check_reference(name, typ, v, claim)
        seen.add((claim["c"], len(v) // claim["c"], claim["odd_row"] is None, claim["run_len"] > 0))
    assert {(c, 1, True, c <= 64) for c in S.RUN_LENGTHS} <= seen                    # one run: a constant column of c rows
    assert {(c, S.RUNS_ABOUT_1000[c], False, False) for c in S.RUN_LENGTHS} <= seen  # defects at about 1000 rows
    assert S.reference(np.zeros(65, np.int64), "I64")["run_len"] == 0 and S.reference(np.zeros(64, np.int64), "I64")["run_len"] == 64
    assert S.reference(np.zeros(1, np.int64), "I64")["run_len"] == 0


def test_large_cases_hold_their_claim():
    """the builders at the sizes past the grid stride, by numpy (the loops above stop at about 1000 rows)"""
    for c, nruns in [(c, S.RUNS_PAST_STRIDE[c]) for c in S.RUN_LENGTHS] + [(c, S.RUNS_WELL_PAST_STRIDE[c]) for c in S.RUN_LENGTHS]:
        n = c * nruns
        assert S.STRIDE < n <= S.STRIDE + 4 * c
        rows = S.uneven_rows(c, nruns, S.positions(n))
        assert any(S.STRIDE - c <= p <= S.STRIDE + c for p in rows) and n - c - 1 in rows and c - 1 in rows
        # a misplaced row that only the second trip of a grid-stride loop reads
        assert max(rows) >= S.STRIDE if nruns == S.RUNS_WELL_PAST_STRIDE[c] else (max(rows) < S.STRIDE or c > S.RUN_MAX)
        first = S.run_firsts("I64", nruns)[c % 4]
        for p in [None] + rows:
            v, claim, pos = S.run_defect(c, nruns, first, p, None if p is None else "uneven")
            odd = np.flatnonzero(v != np.int64(first) + np.arange(n) // c)
            assert odd.tolist() == ([] if p is None else [p]) and pos == p
            assert S.reference(v, "I64")["run_len"] == claim["run_len"] == (c if p is None and c <= 64 else 0)
    n = S.N[-1]
    for typ in S.ORDERED:
        for p in pair_positions_past_stride(n):
            for base, kind in (("small", "equal"), ("wide", "descending"), ("max_to_min", "descending")):
                v, claim, _ = S.order_defect(n, typ, p, kind, base)
                assert np.flatnonzero(v[1:] <= v[:-1]).tolist() == [p]
                ref = S.reference(v, typ)
                assert (ref["ascending"], ref["strict"]) == (claim["ascending"], False) == (kind == "equal", False)
        v, claim, _ = S.order_whole(n, typ, "clean_wide")
        assert S.flags(S.reference(v, typ)) == 3 and (int(v[0]), int(v[-1])) == S.LIMITS[typ]


def pair_positions_past_stride(n):
    return [p for p in S.pair_positions(n) if p >= S.STRIDE - 2]


def test_reference_on_types_without_statistics_and_nullable_columns():
    none = dict(range=None, ascending=False, strict=False, run_len=0, narrow=None)
    for typ in ("F32", "F64", "STR"):
        assert S.reference(np.arange(5), typ) == none
    for typ in S.RANGED:
        assert S.reference(np.zeros(0, S.DTYPE[typ]), typ) == none
        assert S.reference(np.arange(5, dtype=S.DTYPE[typ]), typ, S.null_bitmap(5, [0, 4])) == dict(none, range=(0, 4))
    assert S.reference(np.arange(5, dtype=np.uint8), "CODE8") == dict(none, range=(0, 4))
    one = S.reference(np.array([7], np.int32), "I32")
    assert one == dict(range=(7, 7), ascending=True, strict=True, run_len=0, narrow=(1, 7))
    assert S.null_bitmap(10, [0, 9]).tolist() == [0xFE, 0x01]
    # spans from 2^63 upward (a signed max - min overflows) give no copy; 2^32 - 1 is the last that does
    for span, want in ((2 ** 32 - 1, 4), (2 ** 32, None), (2 ** 63 - 1, None), (2 ** 63, None), (2 ** 64 - 1, None)):
        v, claim, _ = S.narrow_span("I64", span, S.I64_MIN)
        assert (claim["narrow"] and claim["narrow"][0]) == want and S.reference(v, "I64")["narrow"] == claim["narrow"]
    assert S.padded(0) == S.padded(1) == S.padded(8192) == 8192 and S.padded(8193) == 16384
    assert S.narrow_bytes(8193, [dict(narrow=(2, 0)), dict(narrow=None), dict(narrow=(4, 1))]) == 16384 * 6
    assert S.exact_sum(np.array([S.I64_MAX, S.I64_MAX, S.I64_MIN, -1], np.int64)) == S.I64_MAX - 2


def test_sizes_and_positions_cover_the_boundaries():
    """a later edit of N or BOUNDARY cannot quietly drop what they are there for"""
    assert (S.WAVE, S.BLOCK, S.STRIDE) == (64, 256, 524288)
    for edge in (S.WAVE, S.BLOCK, S.ROW_PAD, S.STRIDE):
        assert {edge - 1, edge, edge + 1} <= set(S.N), edge
    assert {1, 2, 2 * S.STRIDE + 1} <= set(S.N)
    n = S.N[-1]
    # the pair one thread reads across a wave, a block and the grid stride; the last pair under `i + 1 < n`
    assert {S.WAVE - 1, S.BLOCK - 1, S.STRIDE - 1, n - 2} <= set(S.pair_positions(n))
    # the first row of the next wave / block / grid-stride trip and the rows on either side of it; the first and the last row
    assert {0, S.WAVE - 2, S.WAVE, S.BLOCK - 2, S.BLOCK, S.STRIDE - 2, S.STRIDE, n - 1} <= set(S.positions(n))
    for m in S.N:
        ps = S.positions(m)
        assert ps and ps[-1] == m - 1 and all(0 <= p < m for p in ps)
        assert m < 2 or (m - 2 in ps and S.pair_positions(m)[-1] == m - 2)
        assert all(p in ps for p in S.BOUNDARY if p < m)
    assert S.pair_positions(1) == [] and S.position_pairs(1) == []
    for c in S.RUN_LENGTHS:
        assert S.STRIDE < c * S.RUNS_PAST_STRIDE[c] and 900 <= c * S.RUNS_ABOUT_1000[c] <= 1040
    assert set(S.RUN_LENGTHS) >= {2, S.RUN_MAX - 1, S.RUN_MAX, S.RUN_MAX + 1}
    for w in (4, 8):
        assert {255, 256, 65535, 65536, 2 ** 32 - 1} <= set(S.SPANS[w])
    assert {2 ** 32, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1} <= set(S.SPANS[8])
