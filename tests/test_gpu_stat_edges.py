"""The statistics ph_table_create gathers for every integer column (ctx.hip: minmax_kernel, order_stat_kernel, run_stat_kernel,
narrow_kernel) against stat_edges.reference, by equality: the range, the order flags, the run length and the narrowed copy of columns with
ONE defect beside a wave, a block and the grid-stride boundary, in the last pair, and at the extremes of the types. One table per (size,
type) holds one column per defect position or value set. Every column of every table is compared in full (range, flags, run length, copy),
whichever statistic its test is named after.

Sizes past 8193 rows keep the columns a table few: every position still gets one order defect (an equal pair), the other order shapes
start at the grid-stride boundary (the earlier positions sit in the first trip of the loop exactly as they do in the tables of up to
8193 rows), the range columns take one value set, the copy columns one base a span."""
import numpy as np
import pytest

import stat_edges as S
from plan_amd import hip

pytestmark = pytest.mark.gpu

T = {"I32": hip.PH_I32, "DATE": hip.PH_DATE, "I64": hip.PH_I64, "DEC64": hip.PH_DEC64, "CODE8": hip.PH_CODE8, "F32": hip.PH_F32, "F64": hip.PH_F64}
SMALL_MAX = 8193


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


def spec(typ, v, validity=None):
    return dict(typ=T[typ], arr=v, scale=2 if typ == "DEC64" else 0, validity=validity)


def observe(t, c):
    """what the library reports for column c, in the form of stat_edges.reference"""
    try:
        rng = t.col_range(c)
    except hip.PlanHipError as ex:
        if ex.code != hip.PH_EUNSUPPORTED:
            raise
        rng = None
    f = hip.table_col_stats(t, c)
    assert f & ~3 == 0
    return dict(range=rng, ascending=bool(f & hip.PH_STAT_ASCENDING), strict=bool(f & hip.PH_STAT_STRICT), run_len=t.col_run_len(c), narrow=t.col_narrow(c))


def check_table(ctx, n, cols):
    """cols: [(name, type, values, validity, claim)]. One table; every column equals the reference, which equals the builder's claim"""
    assert cols and all(len(c[2]) == n for c in cols)
    t = hip.Table(ctx, [spec(typ, v, validity) for _, typ, v, validity, _ in cols], n)
    refs = []
    for c, (name, typ, v, validity, claim) in enumerate(cols):
        ref = S.reference(v, typ, validity)
        for k, want in claim.items():   # a NULL-able column keeps the range it claims and nothing else
            if k in ref and (validity is None or k == "range"):
                assert ref[k] == want, (name, typ, n, k)
        assert observe(t, c) == ref, (name, typ, n)
        refs.append(ref)
    assert t.narrow_bytes() == S.narrow_bytes(n, refs), (n, [c[0] for c in cols])
    t.free()
    return refs


# ------------------------------------------------------------------ range

def range_columns(n, typ):
    cols = []
    for vs in S.VALUE_SETS:
        if vs.startswith("constant"):
            v, claim, _ = S.extremum_at(n, typ, None, None, vs)
            cols.append((vs, typ, v, None, claim))
            cols.append((vs + " nullable", typ, v, S.null_bitmap(n, {0, n - 1}), claim))
        elif vs == "extremes" or n <= SMALL_MAX:
            for p, q in S.position_pairs(n):
                v, claim, _ = S.extremum_at(n, typ, p, q, vs)
                cols.append((f"{vs} min at {p} max at {q}", typ, v, None, claim))
                cols.append((f"{vs} min at {p} max at {q}, both NULL", typ, v, S.null_bitmap(n, {p, q}), claim))
    return cols


@pytest.mark.parametrize("typ", S.RANGED)
def test_range_finds_the_extremes_wherever_they_sit(ctx, typ):
    for n in S.N:
        cols = range_columns(n, typ)
        refs = check_table(ctx, n, cols)
        for (name, _, _, validity, claim), ref in zip(cols, refs):
            assert ref["range"] == claim["range"]
            if validity is not None:    # the range of the stored slots, and nothing else
                assert (ref["ascending"], ref["strict"], ref["run_len"], ref["narrow"]) == (False, False, 0, None), name


# ------------------------------------------------------------------ order flags

def order_columns(n, typ):
    shapes = (("small", "equal"), ("small", "descending"), ("wide", "equal"), ("wide", "descending"), ("max_to_min", "descending"))
    cols = []
    for p in S.pair_positions(n):
        for base, kind in shapes:
            if n > SMALL_MAX and (base, kind) != ("small", "equal") and ((base, kind) in shapes[1:3] or p < S.STRIDE - 2):
                continue    # past 8193 rows: one shape at every position, three from the grid-stride boundary on
            v, claim, _ = S.order_defect(n, typ, p, kind, base)
            cols.append((f"{base} {kind} at {p}", typ, v, None, claim))
    if n >= 2:
        v, claim, _ = S.order_defect(n, typ, n - 2, "equal", "equal_at_max")
        cols.append(("equal_at_max", typ, v, None, claim))
    for which in S.ORDER_WHOLE if n <= SMALL_MAX else ("clean", "clean_wide"):
        v, claim, _ = S.order_whole(n, typ, which)
        cols.append((which, typ, v, None, claim))
    return cols


@pytest.mark.parametrize("typ", S.ORDERED)
def test_order_flags_see_one_defect_at_every_boundary(ctx, typ):
    for n in S.N:
        cols = order_columns(n, typ)
        if n <= 256:    # dictionary codes have a range and no order: 0, 1, 2, ... reports neither flag
            cols.append(("codes ascending", "CODE8", np.arange(n, dtype=np.uint8), None, dict(ascending=False, strict=False, range=(0, n - 1))))
        refs = check_table(ctx, n, cols)
        for (name, _, _, _, claim), ref in zip(cols, refs):
            assert S.flags(ref) == (1 if claim["ascending"] else 0) | (2 if claim["strict"] else 0), (name, n)


# ------------------------------------------------------------------ run length

def run_columns(c, nruns, typ, firsts, near):
    cols = []
    for first in firsts:
        v, claim, _ = S.run_defect(c, nruns, first, typ=typ)
        cols.append((f"runs of {c} from {first}", typ, v, None, claim))
    rows = S.uneven_rows(c, nruns, near)
    for k, p in enumerate(rows):
        first = firsts[k % len(firsts)]
        v, claim, _ = S.run_defect(c, nruns, first, p, "uneven", typ)
        cols.append((f"runs of {c} from {first}, row {p} early", typ, v, None, claim))
    for first in firsts:
        if first + nruns <= S.LIMITS[typ][1]:
            v, claim, _ = S.run_defect(c, nruns, first, None, "last_plus_one", typ)
            cols.append((f"runs of {c} from {first}, last row + 1", typ, v, None, claim))
    return cols


@pytest.mark.parametrize("c", S.RUN_LENGTHS)
def test_run_length_refuses_one_misplaced_row(ctx, c):
    big = ("I32", "I64")
    for nruns, types in ((1, S.ORDERED), (S.RUNS_ABOUT_1000[c], S.ORDERED), (S.RUNS_PAST_STRIDE[c], big), (S.RUNS_WELL_PAST_STRIDE[c], big)):
        n = c * nruns
        for typ in types:
            firsts = S.run_firsts(typ, nruns)
            cols = run_columns(c, nruns, typ, firsts, S.positions(n))
            refs = check_table(ctx, n, cols)
            clean = [r["run_len"] for (_, _, _, _, claim), r in zip(cols, refs) if claim["odd_row"] is None]
            assert clean == [c if c <= S.RUN_MAX else 0] * len(firsts)
            assert [r["run_len"] for (_, _, _, _, claim), r in zip(cols, refs) if claim["odd_row"] is not None].count(0) == len(cols) - len(firsts)
            assert nruns == 1 or len(cols) > 2 * len(firsts)    # both defects are there


# ------------------------------------------------------------------ narrowed copies: width and base

def narrow_columns(n, typ):
    pairs = S.position_pairs(n)
    cols, k = [], 0
    for span in S.SPANS[S.WIDTH[typ]]:
        bases = S.narrow_bases(typ, span)
        if n > SMALL_MAX:   # one base a span, in turn
            bases = [bases[k % len(bases)]]
        for base in bases:
            if span and not pairs:
                continue
            p, q = pairs[k % len(pairs)] if span else (0, 0)
            k += 1
            v, claim, _ = S.narrow_span(typ, span, base, n, p, q)
            cols.append((f"span {span} from {base} at {p}, {q}", typ, v, None, claim))
    return cols


@pytest.mark.parametrize("typ", S.ORDERED)
def test_narrow_width_and_base_at_the_span_edges(ctx, typ):
    for n in (1, 2, 257, 8193, 524289):
        cols = narrow_columns(n, typ)
        refs = check_table(ctx, n, cols)
        for (name, _, _, _, claim), ref in zip(cols, refs):
            assert ref["narrow"] == claim["narrow"] and ref["range"] == claim["range"], name
        if n > 1:
            widths = {r["narrow"][0] if r["narrow"] else None for r in refs}
            assert widths == ({1, 2, 4, None} if S.WIDTH[typ] == 8 else {1, 2, None})


# ------------------------------------------------------------------ narrowed copies: contents

PROOF_LIMIT = 4 * 10 ** 18                         # ph_scan_plan_run: per-row bound x rows per workgroup (4096 at these sizes) < 4e18
A_MAX = 3
DEC_BASE_MIN = -((PROOF_LIMIT - 1) // (4096 * A_MAX))    # -325 520 833 333 333


def fs_sum_count(pl):
    pl.run()
    r = pl.fetch()
    return (int(r["sum"][0][0]), int(r["count"][0][1])) if r["ngroups"] else (0, 0)


def fs_aggs(a, b):
    return [hip.aggexpr(hip.PH_A_SUM, [hip.X_COL(a), hip.X_COL(b), hip.X_MUL]), hip.aggexpr(hip.PH_A_COUNT_STAR)]


def edge_codes(n, w, phase, seed):
    """codes of w bytes: 0 and the largest code in turn at the defect positions (phase 1: the other way round), anything between elsewhere"""
    top = 256 ** w - 1
    code = np.random.default_rng(seed).integers(1, top, n, dtype=np.int64)     # 1 .. top - 1
    ps = S.positions(n)
    code[ps[phase::2]] = 0
    code[ps[1 - phase::2]] = top
    return code, top


def lc_sum_of_q(ctx, q, w):
    """a 4-byte source in the summed slot: lowcard_chain's SUM(q) by (k0, k1) under a DATE range, every other column a one-byte copy
    (q is PH_I32: a DATE has no sum)"""
    n = len(q)
    i = np.arange(n, dtype=np.int64)
    e, d, tx, k0, k1, p = 1000 + i % 251, i % 11, i % 9, (i % 3).astype(np.uint8), (i % 2).astype(np.uint8), (9000 + i % 200).astype(np.int32)
    t = hip.Table(ctx, [spec("I32", q), spec("DEC64", e), spec("DEC64", d), spec("DEC64", tx), dict(typ=hip.PH_CODE8, arr=k0, dictionary=["a", "b", "c"]),
                        dict(typ=hip.PH_CODE8, arr=k1, dictionary=["x", "y"]), spec("DATE", p)], n)
    one = hip.X_CONST(1, 0)
    dp = [hip.X_COL(1), one, hip.X_COL(2), hip.X_SUB, hip.X_MUL]
    aggs = [hip.aggexpr(hip.PH_A_SUM, [hip.X_COL(0)]), hip.aggexpr(hip.PH_A_SUM, [hip.X_COL(1)]), hip.aggexpr(hip.PH_A_SUM, dp),
            hip.aggexpr(hip.PH_A_SUM, dp + [one, hip.X_COL(3), hip.X_ADD, hip.X_MUL]), hip.aggexpr(hip.PH_A_AVG, [hip.X_COL(2)]), hip.aggexpr(hip.PH_A_COUNT_STAR)]
    for lo, hi in ((9000, 9199), (9050, 9149)):
        pl = hip.ScanPlan(ctx, t, [hip.pred(6, hip.PH_GE, hip.const(hip.PH_DATE, i=lo)), hip.pred(6, hip.PH_LE, hip.const(hip.PH_DATE, i=hi))], [4, 5], aggs)
        assert pl.kind == "lowcard_chain" and pl.bytes_per_row == 1 + w + 1 + 1 + 1 + 2, (pl.kind, pl.bytes_per_row)
        pl.run()
        r = pl.fetch()
        got = sorted((tuple(int(k) for k in r["keys"][g]), r["sum"][g][0], r["sum"][g][1], r["count"][g][5]) for g in range(r["ngroups"]))
        keep = (p >= lo) & (p <= hi)
        groups = [(key, keep & (k0 == key[0]) & (k1 == key[1])) for key in ((a, b) for a in range(3) for b in range(2))]
        want = [(key, S.exact_sum(q[m]), S.exact_sum(e[m]), int(m.sum())) for key, m in groups if m.any()]
        assert [g for g in got if g[3]] == want, (n, w, lo, hi)
        pl.free()
    t.free()


@pytest.mark.parametrize("src_w,w", [(8, 1), (8, 2), (8, 4), (4, 1), (4, 2)])
def test_narrow_copy_contents_through_a_fused_scan(ctx, src_w, w):
    """The copy is read the way production reads it: a filter_sumprod plan (SUM(a * b), COUNT(*), range predicates) whose bytes per row
    say that the narrow kernel ran. 8-byte sources sit in the summed and filtered slot b (DEC64; the one 64-bit comparison is `>`), beside
    a = 1..3 and an int32 predicate column; 4-byte sources in the filtered slot p, and in the summed slot q of a lowcard_chain plan
    (lc_sum_of_q). Bases: the plan's overflow proof bounds |a b| x 4096 rows
    below 4e18, which refuses a DEC64 base at the type minimum; the most negative base it admits with a <= 3 is -325 520 833 333 333
    (3 x 325 520 833 333 333 x 4096 = 3 999 999 999 999 995 904), and that one is used. The int32 sources, which are not summed, start at
    INT32_MIN."""
    span = 256 ** w - 1
    assert A_MAX * -DEC_BASE_MIN * 4096 < PROOF_LIMIT <= A_MAX * (-DEC_BASE_MIN + 1) * 4096
    if src_w == 8:
        bases = (DEC_BASE_MIN, -1 - span // 2, 0, -DEC_BASE_MIN - span)
    else:
        bases = (S.I32_MIN, -1 - span // 2, 0, S.I32_MAX - span)
    for n in (65, 8193, 524289):
        i = np.arange(n, dtype=np.int64)
        a = 1 + i % A_MAX
        for k, base in enumerate(bases):
            for phase in (0, 1):
                code, top = edge_codes(n, w, phase, 1000 * w + 10 * k + phase)
                lo, hi = base, base + top
                if src_w == 8:
                    p, b = (i % 4).astype(np.int32), base + code
                    t = hip.Table(ctx, [spec("I32", p), spec("DEC64", a), spec("DEC64", b)], n)
                    assert t.col_narrow(2) == (w, base) and t.col_range(2) == (lo, hi)
                    cases = [((plo, phi), kk) for plo, phi in ((0, 3), (1, 2)) for kk in (None, lo - 1, lo, hi - 1, hi)]
                    want_bytes = 1 + 1 + w + 1
                else:
                    typ = ("I32", "DATE")[k % 2]
                    p, b = (base + code).astype(np.int32), 1000 + i % 251
                    t = hip.Table(ctx, [spec(typ, p), spec("DEC64", a), spec("DEC64", b)], n)
                    assert t.col_narrow(0) == (w, base) and t.col_range(0) == (lo, hi)
                    cases = [(r, None) for r in ((lo, hi), (lo + 1, hi), (lo, hi - 1), (lo + 1, hi - 1), (lo, lo), (hi, hi), (S.I32_MIN, S.I32_MAX))]
                    want_bytes = w + w + 1 + 1
                    lc_sum_of_q(ctx, p, w)
                ptyp = t.col(0).type
                prod = a * b
                for (plo, phi), kk in cases:
                    preds = [hip.pred(0, hip.PH_GE, hip.const(ptyp, i=plo)), hip.pred(0, hip.PH_LE, hip.const(ptyp, i=phi))]
                    keep = (p >= plo) & (p <= phi)
                    if kk is not None:
                        preds.append(hip.pred(2, hip.PH_GT, hip.const(hip.PH_DEC64, i=kk, scale=2)))
                        keep &= b > kk
                    pl = hip.ScanPlan(ctx, t, preds, [], fs_aggs(1, 2))
                    assert pl.kind == "filter_sumprod" and pl.bytes_per_row == want_bytes, (pl.kind, pl.bytes_per_row, want_bytes)
                    assert fs_sum_count(pl) == (S.exact_sum(prod[keep]), int(keep.sum())), (n, base, phase, plo, phi, kk)
                    pl.free()
                t.free()


# ------------------------------------------------------------------ no statistics, no rows, padding

def str_spec(strings):
    off = np.zeros(len(strings) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(s) for s in strings])
    return dict(typ=hip.PH_STR, arr=off, aux=np.frombuffer(b"".join(strings), dtype=np.uint8))


def test_types_without_statistics_and_the_empty_table(ctx):
    none = dict(range=None, ascending=False, strict=False, run_len=0, narrow=None)
    n = 5
    t = hip.Table(ctx, [spec("F32", np.arange(n, dtype=np.float32)), spec("F64", np.arange(n, dtype=np.float64)), str_spec([b"a", b"b", b"c", b"d", b"e"])], n)
    empty = hip.Table(ctx, [spec(typ, np.zeros(0, S.DTYPE[typ])) for typ in T] + [str_spec([])], 0)
    for tab, types in ((t, ("F32", "F64", "STR")), (empty, tuple(T) + ("STR",))):
        for c, typ in enumerate(types):
            with pytest.raises(hip.PlanHipError) as ex:
                tab.col_range(c)
            assert ex.value.code == hip.PH_EUNSUPPORTED
            assert hip.table_col_stats(tab, c) == 0 and tab.col_run_len(c) == 0 and tab.col_narrow(c) is None
            assert observe(tab, c) == none == S.reference(np.zeros(0 if tab is empty else n), typ)
        assert tab.narrow_bytes() == 0
        tab.free()


@pytest.mark.parametrize("n", [1, 8191, 8193])
def test_padding_past_the_last_row_is_zero(ctx, n):
    """rows n .. padded(n) of every column's data and bytes ceil(n / 8) .. padded(n) / 8 of its validity are zero, whatever the rows hold
    (here every bit of every row and of the caller's validity bytes is set)"""
    types = [typ for typ in T]
    ones = {typ: np.frombuffer(b"\xff" * (n * S.WIDTH[typ]), dtype=S.DTYPE[typ]) for typ in types}
    valid = np.full((n + 7) // 8, 0xFF, np.uint8)
    t = hip.Table(ctx, [spec(typ, ones[typ], valid) for typ in types] + [spec(typ, ones[typ]) for typ in types], n)
    pad = S.padded(n)
    for c, typ in enumerate(types + types):
        col = t.col(c)
        w = S.WIDTH[typ]
        assert not ctx.download(hip.vp(col.data + n * w), np.uint8, (pad - n) * w).any(), (typ, c)
        assert ctx.download(hip.vp(col.data), np.uint8, n * w).all()
        assert (col.validity is not None) == (c < len(types))
        if col.validity is not None:
            assert not ctx.download(hip.vp(col.validity + (n + 7) // 8), np.uint8, pad // 8 - (n + 7) // 8).any(), (typ, c)
    t.free()
