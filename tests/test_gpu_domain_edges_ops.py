"""The operator-granular kernels at the edges of their integer domains, each against plain Python integers (domain_edges.py):
ph_sort_rows keys (E), ph_expr_eval's per-row overflow detection (C) and the aggregate sinks' 128-bit sums, MIN/MAX seeds, top-k and
HAVING (D). A call returns the exact result or an error code; it never returns another number."""
import datetime
from fractions import Fraction

import numpy as np
import pytest

import domain_edges as DE
import oracle_lib as O
from domain_edges import I32_MAX, I32_MIN, I64_MAX, I64_MIN
from plan_amd import hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


def bits(valid):
    return None if valid is None else np.packbits(valid, bitorder="little")


# ------------------------------------------------------------------ E. sort keys

def oracle_sort(cols, desc, sel, n):
    """O.sort_rows, or None where the oracle reports an error (dec.Int64's `ok`)"""
    arr = (O.OCol * len(cols))(*cols)
    d = (O.i32 * len(cols))(*[1 if x else 0 for x in desc])
    rows = np.empty(max(n, 1), np.int64)
    s = None if sel is None else np.ascontiguousarray(sel, dtype=np.int64)
    rc = O.lib().oracle_sort_rows(arr, d, O.i32(len(cols)), O.ptr(s), O.i64(n), O.ptr(rows), None, None)
    return rows[:n].tolist() if rc == 0 else None


def sort_columns(n, seed):
    """{name: (hip type, oracle type, array, scale, bool validity or None, python key per row)}"""
    rng = np.random.default_rng(seed)
    i32 = rng.integers(I32_MIN, I32_MAX, n, endpoint=True, dtype=np.int64).astype(np.int32)
    day_lo, day_hi = DE.civil_days(1, 1, 1), DE.civil_days(9999, 12, 31)
    date = rng.integers(day_lo, day_hi, n, endpoint=True, dtype=np.int64).astype(np.int32)
    for j, r in enumerate(rng.choice(n, min(n, 24), replace=False)):
        i32[r] = (I32_MIN, -1, 0, I32_MAX, I32_MIN + 1, I32_MAX - 1)[j % 6]
        date[r] = (day_lo, day_hi, -1, 0, 1, day_lo + 1)[j % 6]
    valid = rng.random(n) > 0.1
    epoch = datetime.date(1970, 1, 1).toordinal()

    def ymd(days):   # the reference's DATE key is (year, month, day)
        d = datetime.date.fromordinal(epoch + int(days))
        return d.year * 10_000 + d.month * 100 + d.day
    cols = {"i32": (hip.PH_I32, O.OT_INT32, i32, 0, None, i32.tolist()),
            "i32n": (hip.PH_I32, O.OT_INT32, i32, 0, valid, i32.tolist()),
            "date": (hip.PH_DATE, O.OT_DATE, date, 0, None, [ymd(x) for x in date]),
            "daten": (hip.PH_DATE, O.OT_DATE, date, 0, ~valid | (rng.random(n) > 0.5), [ymd(x) for x in date])}
    for scale in (0, 1, 2, 4, 6):
        v = DE.dec_sort_values(scale, seed * 16 + scale, n)
        cents = [DE.cents_half_even(x, scale) for x in v.tolist()]
        cols[f"dec{scale}"] = (hip.PH_DEC64, O.OT_DECIMAL, v, scale, None, cents)
        cols[f"dec{scale}n"] = (hip.PH_DEC64, O.OT_DECIMAL, v, scale, rng.random(n) > 0.1, cents)
    return cols


def test_sort_rows_keys_at_the_domain_edges(ctx):
    """PH_I32 keys with INT32_MIN / -1 / 0 / INT32_MAX, PH_DATE keys from 0001-01-01 to 9999-12-31, PH_DEC64 keys up to +-(2^63 - 1) at scales
    0, 1, 2, 4, 6 with half-way cases of both signs: ASC and DESC, NULL-able, with a selection, against Python's sorted over (null flag, value
    rounded half-even to cents as a Fraction, input position), and against the oracle wherever it returns without error.
    (Scale > 2: the rounding step q += +-1 cannot reach INT64_MAX / INT64_MIN, |q| <= |x| / 10 — nothing to test. Scale < 2 ordered
    large DECIMAL(18,0) values wrongly before round_cents stopped multiplying.)"""
    with_oracle = 0
    for n, seed in ((1, 1), (300, 2), (20_000, 3)):
        cols = sort_columns(n, seed)
        dev = {k: hip.DevColumn(ctx, c[0], c[2], c[3], validity=bits(c[4])) for k, c in cols.items()}
        rng = np.random.default_rng(seed)
        sel = np.sort(rng.choice(n, max(1, n // 2), replace=False))
        sel_dev = ctx.upload(sel.astype(np.int32))
        cases = [([k], [d]) for k in cols for d in (False, True)]
        cases += [(["dec0", "daten", "i32"], [True, False, True]), (["dec6n", "dec1"], [False, True]), (["date", "dec4n", "i32n"], [True, True, False]),
                  (["i32n", "dec2n", "dec0n"], [True, False, False])]
        for names, desc in cases:
            for s, sd, m in ((None, None, n), (sel, sel_dev, len(sel))):
                out = hip.sort_rows(ctx, [dev[k] for k in names], desc, sd, m)
                got = ctx.download(out, np.int32, m).tolist()
                ctx.free(out)
                rows = range(n) if s is None else s.tolist()
                assert got == DE.sorted_rows([(cols[k][5], cols[k][4]) for k in names], desc, rows), (n, names, desc, s is not None)
                want = oracle_sort([O.col(cols[k][1], cols[k][2], cols[k][3], validity=bits(cols[k][4])) for k in names], desc, s, m)
                if want is not None:
                    with_oracle += 1
                    assert got == want, (n, names, desc, s is not None)
        ctx.free(sel_dev)
        for c in dev.values():
            c.free()
    assert with_oracle > 0


# ------------------------------------------------------------------ C. ph_expr_eval

N_EXPR = (1 << 18) + 777     # at or above 2^18 rows PH_EXPR_JIT=1 runs the generated kernel: 1024 rows per workgroup step, 4 per thread


class Shifted:
    """Two operand columns of 2 n - 1 rows, harmless everywhere but in row n - 1: the view that starts at row n - 1 - pos has that row at
    position pos, without another upload"""

    def __init__(self, ctx, n, a, b, scales, types=(hip.PH_DEC64, hip.PH_DEC64)):
        i = np.arange(2 * n - 1)
        self.n, self.scales, self.types = n, scales, types
        self.host = [(i % 7 - 3).astype(np.int64), (i % 5 - 2).astype(np.int64)]
        self.host[0][n - 1], self.host[1][n - 1] = a, b
        self.dev = [ctx.upload(h) for h in self.host]
        self.ctx = ctx

    def cols(self, pos):
        out = []
        for d, t, s in zip(self.dev, self.types, self.scales):
            c = hip.Col()
            c.type, c.scale, c.data = t, s, d.value + 8 * (self.n - 1 - pos)
            out.append(c)
        return out

    def rows(self, pos):
        s = self.n - 1 - pos
        return [h[s:s + self.n] for h in self.host]

    def free(self):
        for d in self.dev:
            self.ctx.free(d)


def tail_positions(n):
    """index 0, n - 1, the last row of the last full 1024-row block, and positions in every 256-row quarter of the ragged tail"""
    full = n // 1024 * 1024
    return sorted({0, n - 1, full - 1, full, full + 255, full + 256, full + 511, full + 512, full + 767, full + 768, full + (n - full) // 2})


def eval_call(ctx, cols, prog, sel, n, validity=False):
    out, val = hip.expr_eval(ctx, cols, prog, sel, n, want_validity=validity)
    got = ctx.download(out, np.int64, n).tolist()
    v = None
    if validity:
        v = np.unpackbits(ctx.download(val, np.uint8, (n + 7) // 8), bitorder="little")[:n].astype(bool)
        ctx.free(val)
    ctx.free(out)
    return got, v


@pytest.mark.parametrize("jit", ["1", "0"])
def test_expr_eval_finds_overflow_in_exactly_the_rows_that_overflow(ctx, jit, monkeypatch):
    """domain_edges.EXPR_CASES through the generated kernel (PH_EXPR_JIT=1) and the interpreter (0): the largest operands that still fit
    are exact; one overflowing row among n harmless ones raises PH_EOVERFLOW wherever it stands (every row of the ragged tail for the
    multiply) and whichever step overflows; outside the selection vector or with a NULL input it raises nothing; the flag does not stick"""
    monkeypatch.setenv("PH_EXPR_JIT", jit)
    n = N_EXPR
    places = tail_positions(n)
    for name, prog, scales, fit, overflow in DE.EXPR_CASES:
        # the largest operands that still fit, one pair at each of the places: exact values, no error
        i = np.arange(n)
        a, b = (i % 7 - 3).astype(np.int64), (i % 5 - 2).astype(np.int64)
        for j, pos in enumerate(places):
            a[pos], b[pos] = fit[j % len(fit)]
        fa, fb = hip.DevColumn(ctx, hip.PH_DEC64, a, scales[0]), hip.DevColumn(ctx, hip.PH_DEC64, b, scales[1])
        fit_want = DE.expected_values(prog, a, b, scales)
        assert "overflow" not in fit_want
        got, _ = eval_call(ctx, [fa, fb], prog, None, n)
        assert got == [w[0] for w in fit_want], name
        for j, (x, y) in enumerate(overflow):
            # one overflowing row among n harmless ones is refused wherever it stands
            sh = Shifted(ctx, n, x, y, scales)
            positions = places if j else sorted(set(places) | set(range(n // 1024 * 1024, n, 1 if name == "multiply" else 37)))
            for pos in positions:
                with pytest.raises(hip.PlanHipError) as e:
                    hip.expr_eval(ctx, sh.cols(pos), prog, None, n)
                assert e.value.code == hip.PH_EOVERFLOW, (name, x, y, pos)
            if j:
                sh.free()
                continue
            # the flag does not stick: the next call on the same context is clean and exact
            got, _ = eval_call(ctx, [fa, fb], prog, None, n)
            assert got == [w[0] for w in fit_want], name
            # the same row outside the selection vector: nothing is raised and the selected rows are exact
            pos = n - 3
            sel = np.delete(np.arange(n, dtype=np.int32), pos)
            sel_dev = ctx.upload(sel)
            got, _ = eval_call(ctx, sh.cols(pos), prog, sel_dev, n - 1)
            assert got == [w[0] for w in DE.expected_values(prog, *[h[sel] for h in sh.rows(pos)], scales)], (name, x, y)
            ctx.free(sel_dev)
            # the same row with either input NULL: nothing is raised, the other rows are exact and the validity bits right
            a, b = sh.rows(pos)
            want = np.array([0 if w == "overflow" else w[0] for w in DE.expected_values(prog, a, b, scales)], dtype=object)
            for null_col in (0, 1):
                va, vb = np.ones(n, bool), np.ones(n, bool)
                (va, vb)[null_col][pos] = False
                va[[3, 1000]] = False
                vb[[4, 1000, n - 1]] = False
                da = hip.DevColumn(ctx, hip.PH_DEC64, a, scales[0], validity=bits(va))
                db = hip.DevColumn(ctx, hip.PH_DEC64, b, scales[1], validity=bits(vb))
                got, valid = eval_call(ctx, [da, db], prog, None, n, validity=True)
                live = va & vb
                assert np.array_equal(valid, live), (name, null_col)
                assert np.array(got, dtype=object)[live].tolist() == want[live].tolist(), (name, x, y, null_col)
                da.free()
                db.free()
            sh.free()
        fa.free()
        fb.free()
    # deferred errors: the refused call is reported once by the next read-back, and the call after it is clean
    name, prog, scales, fit, overflow = DE.EXPR_CASES[0]
    bad, good = Shifted(ctx, n, *overflow[0], scales), Shifted(ctx, n, *fit[0], scales)
    ctx.set_deferred_errors(True)
    try:
        out, _ = hip.expr_eval(ctx, bad.cols(n - 1), prog, None, n)
        with pytest.raises(hip.PlanHipError) as e:
            ctx.download(out, np.int64, 1)
        assert e.value.code == hip.PH_EOVERFLOW
        ctx.free(out)
        out, _ = hip.expr_eval(ctx, good.cols(n - 1), prog, None, n)
        assert ctx.download(out, np.int64, n).tolist() == [w[0] for w in DE.expected_values(prog, *good.rows(n - 1), scales)]
        ctx.check_deferred()
        ctx.free(out)
    finally:
        ctx.set_deferred_errors(False)
    bad.free()
    good.free()


# ------------------------------------------------------------------ D. aggregates

EDGE = [I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX, 12_345, -987_654_321, 10 ** 17]
K_MIN, K_MAX = 0, 6                      # EDGE's INT64_MIN and INT64_MAX
AGGS = [(hip.PH_A_SUM, 0), (hip.PH_A_AVG, 0), (hip.PH_A_MIN, 0), (hip.PH_A_MAX, 0), (hip.PH_A_COUNT, 0), (hip.PH_A_COUNT_STAR, -1)]


def agg_rows(n, ngroups, seed, ordered=False):
    """(key, kind, valid): the argument of row i is EDGE[kind[i]], NULL where valid is False. Group 0 holds only INT64_MIN (its MAX is
    MAX's seed), group 1 only INT64_MAX (its MIN is MIN's seed), group 2 alternates the two, every input of group 3 is NULL; each of the
    four has more than a thousand rows; the other groups mix all of EDGE with a tenth of NULLs"""
    rng = np.random.default_rng(seed)
    key = rng.integers(0, ngroups, n).astype(np.int64)
    key[:4096] = np.arange(4096) % 4
    if ordered:
        key = np.sort(key)
    kind = rng.integers(0, len(EDGE), n)
    kind[key == 0] = K_MIN
    kind[key == 1] = K_MAX
    kind[key == 2] = np.where(np.arange(int((key == 2).sum())) % 2 == 0, K_MAX, K_MIN)
    valid = rng.random(n) > 0.1
    valid[key == 3] = False
    valid[key == 2] = True
    return key, kind, valid


def agg_reference(key, kind, valid, row_base=0):
    """{group key: (first row, sum, count of non-NULL inputs, min, max, rows)} in Python integers; numpy only counts how often each
    value of EDGE occurs in each group"""
    K = len(EDGE)
    uk, first, inv = np.unique(key, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    cnt = np.bincount(inv[valid] * K + kind[valid], minlength=len(uk) * K).reshape(len(uk), K).tolist()
    rows = np.bincount(inv, minlength=len(uk)).tolist()
    out = {}
    for g, k in enumerate(uk.tolist()):
        seen = [EDGE[j] for j in range(K) if cnt[g][j]]
        out[k] = (int(first[g]) + row_base, sum(c * v for c, v in zip(cnt[g], EDGE)), sum(cnt[g]), min(seen, default=None), max(seen, default=None), rows[g])
    return out


def signed64(v):
    lo = v & (2 ** 64 - 1)
    return lo - 2 ** 64 if lo >= 2 ** 63 else lo


def check_groups(r, want, name):
    assert r["ngroups"] == len(want), name
    assert np.all(np.diff(r["first_row"]) > 0)
    for g in range(r["ngroups"]):
        first, s, c, mn, mx, rows = want[int(r["keys"][g][0])]
        cnts, sums = [int(x) for x in r["count"][g]], r["sum"][g]
        assert int(r["first_row"][g]) == first and cnts[5] == rows and cnts[:5] == [c] * 5, (name, g)
        if c:
            assert sums[0] == s and Fraction(sums[1], cnts[1]) == Fraction(s, c), (name, g, sums[0], s)
            assert (signed64(sums[2]), signed64(sums[3])) == (mn, mx), (name, g)


def dev_cols(ctx, key, kind, valid):
    vals = np.array(EDGE, np.int64)[kind]
    return hip.DevColumn(ctx, hip.PH_I64, key), hip.DevColumn(ctx, hip.PH_I64, vals, validity=bits(valid))


# (name, rows, groups, ph_agg_create's hint, environment, the kind ph_agg_sink_kind reports): the sink forms the suite reaches elsewhere
# with ordinary values
SINK_FORMS = [
    ("row by row", 5_000, 40, 16, {}, "generic"),
    ("LDS pre-aggregation", 300_000, 700, 1024, {}, "generic"),
    ("bulk build", 200_000, 60_000, 100_000, {}, "bulk1"),
    ("bulk build, second form", 4_300_000, 11_000, 50_000, {}, "bulk2_spec"),
    ("specialised sink", (1 << 20) + 12_345, 175, 1024, {"PH_AGG_JIT": "1"}, "spec"),
    ("generic sink of 2^20 rows", (1 << 20) + 12_345, 175, 1024, {"PH_AGG_JIT": "0"}, "generic"),
]


@pytest.mark.parametrize("form", SINK_FORMS, ids=[f[0].replace(" ", "_") for f in SINK_FORMS])
def test_sink_forms_carry_128_bits_and_keep_min_max_seeds(ctx, form, monkeypatch):
    """SUM / AVG of m x INT64_MIN, m x INT64_MAX and alternating extremes, MIN = INT64_MAX and MAX = INT64_MIN with count > 0, groups
    whose every input is NULL (count 0), through one sink form"""
    name, n, ngroups, hint, env, sink_kind = form
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    key, kind, valid = agg_rows(n, ngroups, len(name))
    dk, dv = dev_cols(ctx, key, kind, valid)
    agg = hip.Agg(ctx, [hip.PH_I64], AGGS, hint)
    assert agg.sink_kind == ""
    agg.sink([dk], [dv], None, n)
    assert agg.sink_kind == sink_kind
    r = agg.finalize(room=ngroups)
    want = agg_reference(key, kind, valid)
    check_groups(r, want, name)
    assert want[0][1] == want[0][2] * I64_MIN and want[1][1] == want[1][2] * I64_MAX and want[0][2] > 900 and want[3][2] == 0
    assert want[1][3] == I64_MAX and want[0][4] == I64_MIN and abs(want[2][1]) <= 2 ** 63
    agg.free()
    dk.free()
    dv.free()


@pytest.mark.parametrize("hint", [1024, 100_000], ids=["into_an_ordinary_table", "into_a_bulk_built_table"])
def test_second_sink_into_a_filled_table(ctx, hint):
    n, ngroups = 300_000, (700 if hint == 1024 else 60_000)
    key, kind, valid = agg_rows(n, ngroups, 77)
    half = 180_000
    agg = hip.Agg(ctx, [hip.PH_I64], AGGS, hint)
    cols = []
    for b, e in ((0, half), (half, n)):
        dk, dv = dev_cols(ctx, key[b:e], kind[b:e], valid[b:e])
        agg.sink([dk], [dv], None, e - b, row_base=b)
        cols += [dk, dv]
    check_groups(agg.finalize(room=ngroups), agg_reference(key, kind, valid), f"second sink, hint {hint}")
    agg.free()
    for c in cols:
        c.free()


@pytest.mark.parametrize("form", ["PH_STREAM_AGG_ONE_PASS", "PH_STREAM_AGG_TWO_PASS"])
def test_streaming_aggregate_carries_across_tiles_and_workgroups(ctx, form, monkeypatch):
    """ph_agg_sink_sorted: random runs with the extreme groups of agg_rows, then a run that starts on the last row of a 2048-row tile and
    holds 100 001 x INT64_MAX (its sum carries in the middle of the run, across tiles and workgroups), directly followed by 100 000 x
    INT64_MIN, by one-row groups over all of EDGE, and by 50 001 rows that alternate the extremes"""
    monkeypatch.setenv(form, "1")
    key, kind, valid = agg_rows(300_000, 9_000, 5, ordered=True)
    lead = 2048 * 150 - 1 - len(key)       # pad with one ordinary group so that the long run starts on the last row of tile 149
    assert lead > 0
    parts = [(key, kind, valid), (np.full(lead, 10_000), np.full(lead, 7), np.ones(lead, bool)),
             (np.full(100_001, 10_001), np.full(100_001, K_MAX), np.ones(100_001, bool)),
             (np.full(100_000, 10_002), np.full(100_000, K_MIN), np.ones(100_000, bool)),
             (10_003 + np.arange(5_000), np.arange(5_000) % len(EDGE), np.arange(5_000) % 13 != 0),
             (np.full(50_001, 20_000), np.where(np.arange(50_001) % 2 == 0, K_MAX, K_MIN), np.ones(50_001, bool))]
    key, kind, valid = (np.concatenate([p[i] for p in parts]) for i in range(3))
    key = key.astype(np.int64)
    assert int(np.flatnonzero(key == 10_001)[0]) % 2048 == 2047
    n = len(key)
    dk, dv = dev_cols(ctx, key, kind, valid)
    agg = hip.Agg(ctx, [hip.PH_I64], AGGS, 1024)
    assert agg.sink_sorted([dk], [dv], n)
    want = agg_reference(key, kind, valid)
    check_groups(agg.finalize(room=len(want)), want, form)
    ctx.check_deferred()
    assert want[10_001][1] == 100_001 * I64_MAX and want[10_002][1] == 100_000 * I64_MIN and want[20_000][1] == I64_MAX - 25_000
    agg.free()
    dk.free()
    dv.free()


TOPK_AGGS = [(hip.PH_A_SUM, 0), (hip.PH_A_MIN, 0), (hip.PH_A_MAX, 0), (hip.PH_A_COUNT_STAR, -1)]


def one_row_groups(ctx, ngroups, seed):
    """one row per group, so SUM = MIN = MAX = the row's value: both int64 extremes, -1, 0, ties at the extremes, NULL aggregates"""
    rng = np.random.default_rng(seed)
    vals = rng.integers(-10 ** 12, 10 ** 12, ngroups).astype(np.int64)
    special = [I64_MIN, I64_MIN, I64_MIN + 1, -1, 0, 0, 1, I64_MAX - 1, I64_MAX, I64_MAX]
    where = rng.choice(ngroups, 3 * len(special), replace=False)
    for j, g in enumerate(where):
        vals[g] = special[j % len(special)]
    valid = np.ones(ngroups, bool)
    valid[rng.choice(ngroups, 5, replace=False)] = False
    key = np.arange(ngroups, dtype=np.int64) * 3 + 1
    dk, dv = hip.DevColumn(ctx, hip.PH_I64, key), hip.DevColumn(ctx, hip.PH_I64, vals, validity=bits(valid))
    agg = hip.Agg(ctx, [hip.PH_I64], TOPK_AGGS, ngroups)
    agg.sink([dk], [dv], None, ngroups)
    dk.free()
    dv.free()
    return agg, [int(v) if ok else None for v, ok in zip(vals.tolist(), valid.tolist())]


@pytest.mark.parametrize("ngroups", [1000, 3000, 150_000], ids=["one_chunk", "a_few_chunks", "pruned_final_stage"])
def test_topk_over_the_whole_int64_domain(ctx, ngroups):
    """ph_agg_topk, ascending and descending, k in {1, 2, 40, ngroups - 1, ngroups, ngroups + 1} (40 x 147 chunks: more than the 4096
    candidates the last workgroup holds in LDS): every group at least as good as the k-th comes back (NULL aggregates first) with its exact
    value, and nothing else — except that a live value equal to the best possible one (INT64_MIN ascending, INT64_MAX descending) shares the
    NULLs' key and may come back with them, which ph_agg_topk's contract allows."""
    agg, values = one_row_groups(ctx, ngroups, ngroups)
    nnull = sum(v is None for v in values)
    live = np.array([v is not None for v in values])
    dense = np.array([0 if v is None else v for v in values], np.int64)
    for a in (0, 1):
        for desc in (True, False):
            ref = DE.TopK(values, desc)
            for k in (1, 2, 40, ngroups - 1, ngroups, ngroups + 1):
                r = agg.topk(a, k, descending=desc, cap=ngroups)
                idx = (r["keys"][:, 0] - 1) // 3
                got, want = set(idx.tolist()), ref.best(k)
                assert len(got) == r["ngroups"] and want <= got, (a, desc, k, len(want), len(got))
                best = I64_MAX if desc else I64_MIN
                assert all(values[g] == best for g in got - want) and (not (got - want) or k <= nnull), (a, desc, k)
                assert np.all(np.diff(r["first_row"]) > 0)
                cnt = r["count"][:, a]
                assert np.array_equal(cnt, live[idx].astype(np.int64))
                assert np.array_equal(r["sum_lo"][:, a].view(np.int64)[cnt > 0], dense[idx][cnt > 0])
    agg.free()


def test_having_at_the_extremes_and_sums_too_wide_for_int64(ctx):
    """ph_agg_fetch_where with constants at and next to the int64 extremes, every operator, against domain_edges.having_reference; and its
    answer — PH_EOVERFLOW, as ph_agg_topk's — when a SUM named by a conjunct does not fit int64, in the first, a middle or the last group"""
    ngroups = 3000
    agg, values = one_row_groups(ctx, ngroups, 31)
    full = agg.finalize(room=ngroups)
    assert [(int(x) - 1) // 3 for x in full["keys"][:, 0]] == list(range(ngroups))
    for a in (0, 2):
        for k in (I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX):
            for op in (hip.PH_EQ, hip.PH_NE, hip.PH_LT, hip.PH_LE, hip.PH_GT, hip.PH_GE):
                r = agg.finalize(room=ngroups, where=[(a, op, hip.const(hip.PH_DEC64, i=k, scale=0), 0)])
                want = sorted(DE.having_reference(values, op, k))
                assert [(int(x) - 1) // 3 for x in r["keys"][:, 0]] == want, (a, k, op)          # first-seen order kept
                assert [signed64(s[a]) for s in r["sum"]] == [values[g] for g in want]
    agg.free()
    for wide_group in (0, ngroups // 2, ngroups - 1):
        key = np.arange(ngroups + 1, dtype=np.int64)
        key[ngroups] = wide_group                       # one more row of INT64_MAX for that group: its SUM is 2^64 - 2
        vals = np.full(ngroups + 1, 5, np.int64)
        vals[wide_group] = vals[ngroups] = I64_MAX
        dk, dv = hip.DevColumn(ctx, hip.PH_I64, key), hip.DevColumn(ctx, hip.PH_I64, vals)
        agg = hip.Agg(ctx, [hip.PH_I64], TOPK_AGGS, ngroups)
        agg.sink([dk], [dv], None, ngroups + 1)
        r = agg.finalize(room=ngroups)
        assert r["sum"][wide_group][0] == 2 * I64_MAX and sum(s[0] for s in r["sum"]) == 2 * I64_MAX + 5 * (ngroups - 1)
        for call in (lambda: agg.finalize(room=ngroups, where=[(0, hip.PH_GT, hip.const(hip.PH_DEC64, i=7, scale=0), 0)]),
                     lambda: agg.topk(0, 3, cap=ngroups), lambda: agg.topk(0, 3, descending=False, cap=ngroups)):
            with pytest.raises(hip.PlanHipError) as e:
                call()
            assert e.value.code == hip.PH_EOVERFLOW, wide_group
        # MAX of the same groups fits: the refusal is about the aggregate the call names
        r = agg.finalize(room=ngroups, where=[(2, hip.PH_GT, hip.const(hip.PH_DEC64, i=I64_MAX - 1, scale=0), 0)])
        assert r["keys"][:, 0].tolist() == [wide_group]
        assert {int(x) for x in agg.topk(2, 1, cap=ngroups)["keys"][:, 0]} == {wide_group}
        agg.free()
        dk.free()
        dv.free()
