"""Every PH_PE_* expression form inside a ph_plan, on fixed small tables, one form per check, compared exactly with expr_edges
(Python ints, Fractions, numpy IEEE arithmetic): as the columns of a Project root — over the whole table (identity rows), under a scan
predicate (row ids) and over no rows —, below an INNER join that repeats probe rows (one-sided operands through row ids, mixed ones
gathered positionally), CASE with each branch evaluated on its own rows, overflow raised exactly when a kept row overflows, the forms
as group keys and aggregate arguments (streaming and hash aggregate), and NULL-able operands (a bitmap column, a LEFT join's build
side): NULL, truth 0, or PH_EUNSUPPORTED — never a wrong value."""
import numpy as np
import pytest

import domain_edges as DE
import expr_edges as EE
from plan_amd import hip

pytestmark = pytest.mark.gpu

N = 4099                                   # ragged against 256, 1024 and 4096
ID, D, A, B, Q, W, S = range(7)            # the main table's columns; every scan below emits all of them in this order
SCALES = {ID: 0, D: 0, A: 2, B: 4, Q: 0, W: 0}
W_BIG_ROWS = {7: DE.I64_MAX // 100, 8: -(DE.I64_MAX // 100), 4098: DE.I64_MAX // 100 - 1}    # w * 100 still fits
OV = 2500                                  # the row that overflows w * 100 in the overflow variants
K, JID, V, U, DD, SS = range(6)            # the second table's columns


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


def q_of(r):
    """q of row r: scattered over -2048 .. 6143, so that q against id, against constants and against the second table's u all split the rows"""
    return (r * 2654435761) % 8192 - 2048


def main_columns(dates="shuffled", a_nulls=False, overflow=False):
    """the main table as {column: python list} (None = NULL) — the reference's view and, through make_table, the device's"""
    i = np.arange(N)
    edge = np.concatenate([EE.DATE_EDGES[:EE.N_NAMED_DATE_EDGES + 200], (8000 + (i[:N - EE.N_NAMED_DATE_EDGES - 200] * 7) % 2600).astype(np.int32)])
    d = np.sort(edge) if dates == "sorted" else edge[np.random.default_rng(3).permutation(N)]
    a = ((i * 37) % 2001 - 1000).astype(np.int64)
    b = ((i * i) % 100003 - 50000).astype(np.int64)
    q = np.array([q_of(r) for r in range(N)], dtype=np.int32)
    w = (i % 97 - 48).astype(np.int64)
    for r, v in W_BIG_ROWS.items():
        w[r] = v
    if overflow:
        w[OV] = DE.I64_MAX // 100 + 1
    cols = {ID: i.tolist(), D: d.tolist(), A: a.tolist(), B: b.tolist(), Q: q.tolist(), W: w.tolist(), S: ["k%d" % (r % 13) for r in range(N)]}
    if a_nulls:
        cols[A] = [None if r % 5 == 3 else v for r, v in enumerate(cols[A])]
    return cols


def str_col(values):
    raw = [v.encode() for v in values]
    off = np.zeros(len(raw) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(x) for x in raw])
    return dict(typ=hip.PH_STR, arr=off, aux=np.frombuffer(b"".join(raw), dtype=np.uint8))


def fixed_col(typ, values, scale=0):
    valid = np.array([v is not None for v in values])
    arr = np.array([0 if v is None else v for v in values], dtype=hip.NP_TYPES[typ])
    return dict(typ=typ, arr=arr, scale=scale, validity=None if valid.all() else np.packbits(valid, bitorder="little"))


def make_table(ctx, cols):
    return hip.Table(ctx, [fixed_col(hip.PH_I32, cols[ID]), fixed_col(hip.PH_DATE, cols[D]), fixed_col(hip.PH_DEC64, cols[A], 2), fixed_col(hip.PH_DEC64, cols[B], 4),
                           fixed_col(hip.PH_I32, cols[Q]), fixed_col(hip.PH_I64, cols[W]), str_col(cols[S])], N)


def second_columns():
    """keys that hit the even ids once, the multiples of 6 twice and the odd ids never"""
    k = np.concatenate([np.arange(0, N, 2), np.arange(0, N, 6)])
    j = np.arange(len(k))
    return {K: k.tolist(), JID: j.tolist(), V: (j * 11 - 5000).tolist(), U: (j % 9).tolist(), DD: (9000 + j % 400).tolist(), SS: ["s%d" % (x % 5) for x in j.tolist()]}


def make_second(ctx, cols):
    return hip.Table(ctx, [fixed_col(hip.PH_I32, cols[K]), fixed_col(hip.PH_I32, cols[JID]), fixed_col(hip.PH_DEC64, cols[V], 2), fixed_col(hip.PH_I32, cols[U]),
                           fixed_col(hip.PH_DATE, cols[DD]), str_col(cols[SS])], len(cols[K]))


@pytest.fixture(scope="module")
def main(ctx):
    cols = main_columns()
    t = make_table(ctx, cols)
    yield t, cols
    t.free()


@pytest.fixture(scope="module")
def second(ctx):
    cols = second_columns()
    t = make_second(ctx, cols)
    yield t, cols
    t.free()


def run_plan(ctx, build, rows=True, created=None):
    """create, run, fetch: (result, explain). build(p) adds the nodes and returns nothing; created(p) runs on the created plan."""
    p = hip.Plan(ctx)
    try:
        build(p)
        p.create()
        if created:
            created(p)
        p.run()
        r = p.fetch_rows() if rows else p.fetch()
        return r, p.explain()
    finally:
        p.free()


def error_code(ctx, build, rows=True, created=None):
    """the code create, run or fetch raises (None when nothing is raised)"""
    try:
        run_plan(ctx, build, rows, created)
    except hip.PlanHipError as e:
        return e.code
    return None


def I(v):
    return hip.const(hip.PH_I32, i=v)


SUBSETS = {"all": ([], lambda c, r: True), "subset": ([hip.pred(Q, hip.PH_GT, I(5))], lambda c, r: c[Q][r] > 5),
           "none": ([hip.pred(ID, hip.PH_LT, I(0))], lambda c, r: False)}


def by_id(r, ncols):
    """the fetched rows as {id: tuple of the other columns} — ids are unique below a scan"""
    ids = r["columns"][0].tolist()
    assert len(set(ids)) == len(ids)
    lists = [c if isinstance(c, list) else c.tolist() for c in r["columns"][1:ncols]]
    return {i: tuple(col[k] for col in lists) for k, i in enumerate(ids)}


def vals(res):
    assert "overflow" not in res
    return [v[0] for v in res]


def f32_bits(a):
    return EE.bits(np.asarray(a, dtype=np.float32)).astype(np.int64).tolist()


def float_cols(cols, rows, spec):
    """EE.column operands of the listed rows: spec = [(column, type, scale)]"""
    out = []
    for c, typ, scale in spec:
        v = [cols[c][r] for r in rows]
        out.append(EE.column(typ, [0 if x is None else x for x in v], scale, valid=None if None not in v else [x is not None for x in v]))
    return out


# ------------------------------------------------------------------ the forms as columns of a Project root
@pytest.mark.parametrize("subset", list(SUBSETS))
def test_project_rooted_forms(ctx, main, subset):
    """pe_col, pe_dec (add and sub at mixed scales, mul, constants, the largest operands that fit), pe_year, pe_case (decimal and
    result_int), pe_float as FLOAT values and as FLOAT / DOUBLE truth: over the identity rows, over row ids, over no rows"""
    t, cols = main
    preds, keep_row = SUBSETS[subset]
    rows = [r for r in range(N) if keep_row(cols, r)]
    one = hip.X_CONST(1)
    progs = {"add": [hip.X_COL(A), hip.X_COL(B), hip.X_ADD], "sub": [hip.X_COL(B), hip.X_COL(A), hip.X_SUB], "mul": [hip.X_COL(A), hip.X_COL(Q), hip.X_MUL],
             "const": [one, hip.X_COL(A), hip.X_SUB, hip.X_COL(B), hip.X_MUL, hip.X_CONST(-250, 2), hip.X_ADD], "big": [hip.X_COL(W), hip.X_CONST(100), hip.X_MUL]}
    when = ("and", ("cmp", Q, hip.PH_GT, 5), ("cmp", ID, hip.PH_NE, 77))
    fv = [hip.X_COL(Q), hip.X_COL(A), hip.X_MUL, hip.X_F32(0.3), hip.X_ADD]
    ft = [hip.X_COL(Q), hip.X_F32(0.5), hip.X_COL(B), hip.X_MUL, hip.X_OP(hip.PH_X_GT)]
    fw = [hip.X_COL(W), hip.X_F32(0.2), hip.X_COL(B), hip.X_COL(Q), hip.X_OP(hip.PH_X_DIV), hip.X_MUL, hip.X_OP(hip.PH_X_LT)]

    def build(p):
        s = p.scan(t, list(range(7)), preds)
        tree = hip.bool_tree(("and", ("cmp", Q, hip.PH_GT, I(5)), ("cmp", ID, hip.PH_NE, I(77))))
        p.project(s, [hip.pe_col(ID), hip.pe_col(D), hip.pe_col(S)] + [hip.pe_dec(progs[k]) for k in ("add", "sub", "mul", "const", "big")] +
                  [hip.pe_year(D), hip.pe_case(tree, progs["mul"], [hip.X_CONST(-7)], keep=p._keep),
                   hip.pe_case(tree, [one], [hip.X_CONST(0)], result_int=True, keep=p._keep),
                   hip.pe_float(fv, truth=False), hip.pe_float(ft), hip.pe_float(fw, wide=True)])
    r, ex = run_plan(ctx, build)
    assert r["nrows"] == len(rows), ex
    if subset == "subset":
        assert 0 < len(rows) < N
    got = by_id(r, 14)
    want = {}
    year = EE.civil_parts(np.array([cols[D][x] for x in rows], dtype=np.int64))[0].tolist() if rows else []
    wh = EE.when_rows(when, cols, N)
    case_dec, case_scale = EE.case_rows(wh, progs["mul"], [hip.X_CONST(-7)], cols, SCALES)
    case_int, _ = EE.case_rows(wh, [one], [hip.X_CONST(0)], cols, SCALES)
    dec = {k: vals(EE.decimal_program(progs[k], cols, SCALES, rows)) for k in progs}
    fc = float_cols(cols, rows, [(c, hip.PH_I32 if c in (ID, Q) else hip.PH_I64 if c == W else hip.PH_DEC64, SCALES[c]) for c in range(7) if c not in (D, S)] if rows else [])
    remap = {ID: 0, A: 1, B: 2, Q: 3, W: 4}
    re = lambda prog: [(op, remap.get(c, c), iv, sc) if op == hip.PH_X_COL else (op, c, iv, sc) for op, c, iv, sc in prog]
    if rows:
        v32 = f32_bits(EE.float_program(re(fv), fc, False)[0])
        t32, t64 = EE.float_truth(re(ft), fc, False).tolist(), EE.float_truth(re(fw), fc, True).tolist()
        assert subset != "all" or (0 < sum(t32) < N and 0 < sum(t64) < N)
    for k, x in enumerate(rows):
        want[cols[ID][x]] = (cols[D][x], cols[S][x], dec["add"][k], dec["sub"][k], dec["mul"][k], dec["const"][k], dec["big"][k], year[k],
                             case_dec[x], case_int[x], v32[k], t32[k], t64[k])
    assert r["scales"][3:8] == [4, 4, 2, 6, 0] and case_scale == 2 and r["scales"][9] == 2 and r["scales"][10] == 0, (r["scales"], ex)
    # a FLOAT column comes back as its bits in the low 32 bits: compare those (NaNs do not occur here)
    got = {i: v[:10] + (v[10] & 0xFFFFFFFF,) + v[11:] for i, v in got.items()}
    bad = [i for i in want if got.get(i) != want[i]]
    assert not bad and got.keys() == want.keys(), (len(bad), bad[:3], [(got.get(i), want[i]) for i in bad[:3]], ex)


def test_forms_below_a_join_that_repeats_probe_rows(ctx, main, second):
    """INNER join, the main table probing: the multiples of 6 come out twice. Operands of one side are read through that side's row ids,
    operands of both sides are gathered positionally first — pe_dec, pe_year, pe_case and pe_float over each arrangement"""
    t, cols = main
    t2, c2 = second
    # join output: id, d, a, b, q | jid, v, u
    JO = dict(id=0, d=1, a=2, b=3, q=4, jid=5, v=6, u=7)
    sc = {0: 0, 1: 0, 2: 2, 3: 4, 4: 0, 5: 0, 6: 2, 7: 0}
    pairs = [(i, j) for j, i in enumerate(c2[K])]
    jc = {0: [cols[ID][i] for i, _ in pairs], 1: [cols[D][i] for i, _ in pairs], 2: [cols[A][i] for i, _ in pairs], 3: [cols[B][i] for i, _ in pairs],
          4: [cols[Q][i] for i, _ in pairs], 5: [c2[JID][j] for _, j in pairs], 6: [c2[V][j] for _, j in pairs], 7: [c2[U][j] for _, j in pairs]}
    m = len(pairs)
    probe_only = [hip.X_COL(2), hip.X_COL(3), hip.X_MUL]                    # a * b
    build_only = [hip.X_COL(6), hip.X_COL(7), hip.X_MUL]                    # v * u
    mixed = [hip.X_COL(2), hip.X_COL(6), hip.X_ADD, hip.X_COL(4), hip.X_MUL]          # (a + v) * q
    when = ("colcmp", 4, hip.PH_GT, 7)                                      # q > u: a probe column against a build column
    ft_mixed = [hip.X_COL(4), hip.X_F32(0.5), hip.X_COL(6), hip.X_MUL, hip.X_OP(hip.PH_X_GT)]
    ft_probe = [hip.X_COL(4), hip.X_F32(0.01), hip.X_COL(2), hip.X_MUL, hip.X_OP(hip.PH_X_GE)]

    def build(p):
        probe = p.scan(t, list(range(7)))
        bld = p.scan(t2, list(range(6)))
        j = p.join(probe, bld, [ID], [K], [0, 1, 2, 3, 4, 7 + JID, 7 + V, 7 + U])
        p.project(j, [hip.pe_col(0), hip.pe_col(5), hip.pe_dec(probe_only), hip.pe_dec(build_only), hip.pe_dec(mixed), hip.pe_year(1),
                      hip.pe_case(hip.bool_tree(("colcmp", 4, hip.PH_GT, 7)), mixed, probe_only[:1] + [hip.X_CONST(0), hip.X_MUL, hip.X_COL(4), hip.X_MUL], keep=p._keep),
                      hip.pe_float(ft_mixed), hip.pe_float(ft_probe)])
    r, ex = run_plan(ctx, build)
    assert r["nrows"] == m == len(c2[K]), ex
    got = sorted(zip(*[c.tolist() for c in r["columns"]]))
    wh = EE.when_rows(when, jc, m)
    case, cs = EE.case_rows(wh, mixed, probe_only[:1] + [hip.X_CONST(0), hip.X_MUL, hip.X_COL(4), hip.X_MUL], jc, sc)
    assert cs == 2 and 0 < sum(wh) < m
    fc = [EE.column(hip.PH_I32, jc[4]), EE.column(hip.PH_DEC64, jc[6], 2), EE.column(hip.PH_DEC64, jc[2], 2)]
    tm = EE.float_truth([hip.X_COL(0), hip.X_F32(0.5), hip.X_COL(1), hip.X_MUL, hip.X_OP(hip.PH_X_GT)], fc, False).tolist()
    tp = EE.float_truth([hip.X_COL(0), hip.X_F32(0.01), hip.X_COL(2), hip.X_MUL, hip.X_OP(hip.PH_X_GE)], fc, False).tolist()
    assert 0 < sum(tm) < m and 0 < sum(tp) < m
    year = EE.civil_parts(np.array(jc[1], dtype=np.int64))[0].tolist()
    want = sorted(zip(jc[0], jc[5], vals(EE.decimal_program(probe_only, jc, sc)), vals(EE.decimal_program(build_only, jc, sc)),
                      vals(EE.decimal_program(mixed, jc, sc)), year, case, tm, tp))
    assert len({x[0] for x in want}) < m                                    # probe rows really repeat
    bad = [k for k in range(m) if got[k] != want[k]]
    assert not bad, (len(bad), [(got[k], want[k]) for k in bad[:3]], ex)


# ------------------------------------------------------------------ CASE
WHENS = {
    "all_true": ("cmp", ID, hip.PH_GE, 0), "all_false": ("cmp", ID, hip.PH_LT, 0), "mixed": ("cmp", Q, hip.PH_GT, 5),
    "and": ("and", ("cmp", Q, hip.PH_GT, 5), ("cmp", Q, hip.PH_LE, 3000), ("cmp", ID, hip.PH_NE, 1023)),
    "or": ("or", ("cmp", Q, hip.PH_LT, -5), ("cmp", ID, hip.PH_EQ, 4098), ("and", ("cmp", Q, hip.PH_GE, 20), ("cmp", ID, hip.PH_LT, 2000))),
    "in": ("in", Q, [q_of(r) for r in range(0, N, 350)] + [100000]), "colcmp": ("colcmp", Q, hip.PH_GT, ID), "colcmp_le": ("colcmp", ID, hip.PH_LE, Q),
    "null": ("cmp", A, hip.PH_GT, 0),
}


def device_tree(tree):
    """the same tree with ph_const constants (I32 for the integer columns, DECIMAL scale 2 for a)"""
    if tree[0] == "cmp":
        return ("cmp", tree[1], tree[2], hip.const(hip.PH_DEC64, i=tree[3], scale=2) if tree[1] == A else I(tree[3]))
    if tree[0] == "in":
        return ("in", tree[1], [I(v) for v in tree[2]])
    if tree[0] == "colcmp":
        return tree
    return (tree[0],) + tuple(device_tree(k) for k in tree[1:])


@pytest.fixture(scope="module")
def main_nulls(ctx):
    cols = main_columns(a_nulls=True)
    t = make_table(ctx, cols)
    yield t, cols
    t.free()


@pytest.mark.parametrize("name", list(WHENS))
def test_case_when_shapes(ctx, main, main_nulls, name):
    """WHEN all true, all false, mixed, as AND / OR / IN trees, column against column, and over a NULL-able column (a NULL takes ELSE);
    THEN and ELSE both programs (the two scatters), evaluated on their own rows"""
    t, cols = main_nulls if name == "null" else main
    then, other = [hip.X_COL(B), hip.X_COL(Q), hip.X_MUL], [hip.X_COL(B), hip.X_CONST(3), hip.X_SUB]

    def build(p):
        s = p.scan(t, list(range(7)))
        p.project(s, [hip.pe_col(ID), hip.pe_case(hip.bool_tree(device_tree(WHENS[name])), then, other, keep=p._keep)])
    r, ex = run_plan(ctx, build)
    wh = EE.when_rows(WHENS[name], cols, N)
    if name == "all_true":
        assert all(wh)
    elif name == "all_false":
        assert not any(wh)
    else:
        assert 0 < sum(wh) < N
    if name == "null":
        assert any(cols[A][x] is None for x in range(N)) and not any(wh[x] for x in range(N) if cols[A][x] is None)
    want, scale = EE.case_rows(wh, then, other, cols, SCALES)
    got = by_id(r, 2)
    assert r["nrows"] == N and r["scales"][1] == scale == 4, ex
    bad = [x for x in range(N) if got[x] != (want[x],)]
    assert not bad, (len(bad), [(x, got[x], want[x], wh[x]) for x in bad[:4]], ex)


def test_case_else_integer_literals_are_cast_to_the_then_scale(ctx, main):
    """ELSE 0 (the memset), 1 and -7 at THEN scales 0, 2 and 4: nine CASE columns of one Project"""
    t, cols = main
    thens = {0: [hip.X_COL(Q)], 2: [hip.X_COL(A)], 4: [hip.X_COL(B)]}
    combos = [(s, k) for s in (0, 2, 4) for k in (0, 1, -7)]

    def build(p):
        s = p.scan(t, list(range(7)))
        tree = hip.bool_tree(device_tree(WHENS["mixed"]))
        p.project(s, [hip.pe_col(ID)] + [hip.pe_case(tree, thens[sc], [hip.X_CONST(k)], keep=p._keep) for sc, k in combos])
    r, ex = run_plan(ctx, build)
    wh = EE.when_rows(WHENS["mixed"], cols, N)
    got = by_id(r, 10)
    assert r["scales"][1:] == [sc for sc, _ in combos], ex
    for c, (sc, k) in enumerate(combos):
        want, scale = EE.case_rows(wh, thens[sc], [hip.X_CONST(k)], cols, SCALES)
        assert scale == sc and want[[x for x in range(N) if not wh[x]][0]] == k * 10 ** sc
        bad = [x for x in range(N) if got[x][c] != want[x]]
        assert not bad, (sc, k, len(bad), [(x, got[x][c], want[x]) for x in bad[:4]], ex)


def case_plan(t, when, then, other, preds=()):
    def build(p):
        s = p.scan(t, list(range(7)), list(preds))
        p.project(s, [hip.pe_col(ID), hip.pe_case(hip.bool_tree(device_tree(when)), then, other, keep=p._keep)])
    return build


def test_case_refusals(ctx, main, main_nulls):
    t, _ = main
    # an ELSE literal whose cast to the THEN scale leaves int64: 10^15 at scale 4
    assert error_code(ctx, case_plan(t, WHENS["mixed"], [hip.X_COL(B)], [hip.X_CONST(10 ** 15)])) == hip.PH_EOVERFLOW
    assert error_code(ctx, case_plan(t, WHENS["mixed"], [hip.X_COL(B)], [hip.X_CONST(-(10 ** 15))])) == hip.PH_EOVERFLOW
    assert error_code(ctx, case_plan(t, WHENS["mixed"], [hip.X_COL(B)], [hip.X_CONST(10 ** 14)])) is None
    # branches of different scales
    assert error_code(ctx, case_plan(t, WHENS["mixed"], [hip.X_COL(A)], [hip.X_COL(B)])) == hip.PH_EUNSUPPORTED
    # a NULL-able operand in a branch
    tn, _ = main_nulls
    assert error_code(ctx, case_plan(tn, WHENS["mixed"], [hip.X_COL(A)], [hip.X_CONST(0)])) == hip.PH_EUNSUPPORTED
    assert error_code(ctx, case_plan(tn, WHENS["mixed"], [hip.X_COL(B)], [hip.X_COL(A), hip.X_CONST(100), hip.X_MUL])) == hip.PH_EUNSUPPORTED


@pytest.fixture(scope="module")
def main_overflow(ctx):
    cols = main_columns(overflow=True)
    t = make_table(ctx, cols)
    yield t, cols
    t.free()


TIMES_100 = [hip.X_COL(W), hip.X_CONST(100), hip.X_MUL]


@pytest.mark.parametrize("branch", ["then", "else"])
def test_case_branch_overflow_counts_only_on_its_own_rows(ctx, main_overflow, branch):
    """w * 100 overflows in row OV alone. While that row takes the other branch nothing is raised and every value is exact; when it takes
    the overflowing branch the plan raises PH_EOVERFLOW, and the next plan on the context is clean"""
    t, cols = main_overflow
    not_ov, is_ov = ("cmp", ID, hip.PH_NE, OV), ("cmp", ID, hip.PH_EQ, OV)
    flat = [hip.X_COL(Q)]
    if branch == "then":
        safe, unsafe = (not_ov, TIMES_100, flat), (WHENS["all_true"], TIMES_100, flat)
    else:
        safe, unsafe = (is_ov, flat, TIMES_100), (WHENS["all_false"], flat, TIMES_100)
    r, ex = run_plan(ctx, case_plan(t, *safe))
    want, scale = EE.case_rows(EE.when_rows(safe[0], cols, N), safe[1], safe[2], cols, SCALES)
    got = by_id(r, 2)
    assert scale == 0 and want[OV] == cols[Q][OV] and want[7] == W_BIG_ROWS[7] * 100
    assert [got[x][0] for x in range(N)] == want, ex
    assert EE.case_rows(EE.when_rows(unsafe[0], cols, N), unsafe[1], unsafe[2], cols, SCALES) == "overflow"
    assert error_code(ctx, case_plan(t, *unsafe)) == hip.PH_EOVERFLOW
    r2, ex = run_plan(ctx, case_plan(t, *safe))
    got2 = by_id(r2, 2)
    assert [got2[x][0] for x in range(N)] == want, ex
    # ... and under a scan predicate that drops the row, the unsafe CASE is safe as well
    r3, ex = run_plan(ctx, case_plan(t, *unsafe, preds=[hip.pred(ID, hip.PH_NE, I(OV))]))
    assert r3["nrows"] == N - 1 and by_id(r3, 2)[7][0] == W_BIG_ROWS[7] * 100, ex


# ------------------------------------------------------------------ overflow in pe_dec
def test_pe_dec_overflow_is_raised_exactly_when_a_kept_row_overflows(ctx, main_overflow):
    t, cols = main_overflow

    def project(preds):
        def build(p):
            s = p.scan(t, list(range(7)), preds)
            p.project(s, [hip.pe_col(ID), hip.pe_dec(TIMES_100)])
        return build

    def agg(preds):
        def build(p):
            s = p.scan(t, list(range(7)), preds)
            p.agg(s, [hip.pe_year(D)], [(hip.PH_A_SUM, hip.pe_dec(TIMES_100)), (hip.PH_A_COUNT_STAR, None)])
        return build
    drop = [hip.pred(ID, hip.PH_NE, I(OV))]
    r, ex = run_plan(ctx, project(drop))
    want = vals(EE.decimal_program(TIMES_100, cols, SCALES, [x for x in range(N) if x != OV]))
    got = by_id(r, 2)
    assert [got[x][0] for x in range(N) if x != OV] == want and OV not in got, ex
    assert error_code(ctx, project([])) == hip.PH_EOVERFLOW
    assert error_code(ctx, project([hip.pred(ID, hip.PH_GE, I(OV))])) == hip.PH_EOVERFLOW
    # under an aggregate the error must surface from run or fetch — not be taken for a broken statistic and answered by a second run
    ra, ex = run_plan(ctx, agg(drop), rows=False)
    year = EE.civil_parts(np.array(cols[D], dtype=np.int64))[0].tolist()
    ref = EE.group_by([(year[x],) for x in range(N) if x != OV], [want, None], [hip.PH_A_SUM, hip.PH_A_COUNT_STAR])
    assert {(int(ra["keys"][g][0]),): [(ra["sum"][g][0], ra["count"][g][0]), (None, ra["count"][g][1])] for g in range(ra["ngroups"])} == ref, ex
    assert error_code(ctx, agg([]), rows=False) == hip.PH_EOVERFLOW
    # ... nor for a sum beyond int64 under a top-k preselection, which is no error and is fetched again without the preselection
    assert error_code(ctx, agg([]), rows=False, created=lambda p: p.set_topk(0, 5)) == hip.PH_EOVERFLOW
    rt, ex = run_plan(ctx, agg(drop), rows=False, created=lambda p: p.set_topk(0, 5))
    best = sorted((v[0][0] for v in ref.values()), reverse=True)[:5]
    assert sorted((rt["sum"][g][0] for g in range(rt["ngroups"])), reverse=True)[:5] == best, ex
    ra2, ex = run_plan(ctx, agg(drop), rows=False)
    assert ra2["ngroups"] == len(ref) and sum(ra2["sum"][g][0] for g in range(ra2["ngroups"])) == sum(want), ex


# ------------------------------------------------------------------ group keys and aggregate arguments
KINDS = [hip.PH_A_SUM, hip.PH_A_MIN, hip.PH_A_MAX, hip.PH_A_AVG, hip.PH_A_COUNT, hip.PH_A_COUNT_STAR]
MUL_AQ = [hip.X_COL(A), hip.X_COL(Q), hip.X_MUL]
NEG_KEY = [hip.X_COL(Q), hip.X_CONST(25), hip.X_SUB]                        # a pe_dec group key that goes negative
FT = [hip.X_COL(Q), hip.X_F32(0.5), hip.X_COL(B), hip.X_MUL, hip.X_OP(hip.PH_X_GT)]


def reference_forms(cols):
    """per-row values of every form, as exact ints"""
    year = EE.civil_parts(np.array(cols[D], dtype=np.int64))[0].tolist()
    wh = EE.when_rows(WHENS["mixed"], cols, N)
    fc = [EE.column(hip.PH_I32, cols[Q]), EE.column(hip.PH_DEC64, cols[B], 4)]
    truth = EE.float_truth([hip.X_COL(0), hip.X_F32(0.5), hip.X_COL(1), hip.X_MUL, hip.X_OP(hip.PH_X_GT)], fc, False).tolist()
    return {"col": cols[A], "dec": vals(EE.decimal_program(MUL_AQ, cols, SCALES)), "year": year,
            "case": EE.case_rows(wh, MUL_AQ, [hip.X_CONST(-7)], cols, SCALES)[0], "case_int": EE.case_rows(wh, [hip.X_CONST(1)], [hip.X_CONST(0)], cols, SCALES)[0],
            "truth": truth, "neg": vals(EE.decimal_program(NEG_KEY, cols, SCALES))}


def device_forms(p):
    tree = hip.bool_tree(device_tree(WHENS["mixed"]))
    return {"col": hip.pe_col(A), "dec": hip.pe_dec(MUL_AQ), "year": hip.pe_year(D), "case": hip.pe_case(tree, MUL_AQ, [hip.X_CONST(-7)], keep=p._keep),
            "case_int": hip.pe_case(tree, [hip.X_CONST(1)], [hip.X_CONST(0)], result_int=True, keep=p._keep), "truth": hip.pe_float(FT), "neg": hip.pe_dec(NEG_KEY)}


def groups_of(r, nkeys):
    """{key: [(value, count)]} as expr_edges.group_by gives it: the sum word is the SUM / MIN / MAX / AVG's sum, None for the counts and
    for an aggregate that saw no value"""
    counts = (hip.PH_A_COUNT, hip.PH_A_COUNT_STAR)
    return {tuple(int(k) for k in r["keys"][g][:nkeys]): [(None if kind in counts or r["count"][g][a] == 0 else r["sum"][g][a], r["count"][g][a])
                                                          for a, kind in enumerate(KINDS)] for g in range(r["ngroups"])}


@pytest.fixture(scope="module")
def main_sorted(ctx):
    cols = main_columns(dates="sorted")
    t = make_table(ctx, cols)
    yield t, cols
    t.free()


@pytest.mark.parametrize("key", ["year", "case_int", "neg"])
def test_forms_as_group_keys_and_aggregate_arguments(ctx, main, main_sorted, key):
    """GROUP BY extract(year), a result_int CASE or a pe_dec that goes negative; SUM / MIN / MAX / AVG (sum and count) / COUNT / COUNT(*)
    over each form against a dict group-by of exact ints. By year, the table sorted by date takes the streaming aggregate and the
    shuffled one the hash aggregate (named by explain()): the same groups either way."""
    results = {}
    for order, (t, cols) in (("shuffled", main), ("sorted", main_sorted)):
        ref = reference_forms(cols)
        for arg in ("col", "dec", "year", "case", "case_int", "truth"):
            def build(p):
                s = p.scan(t, list(range(7)))
                f = device_forms(p)
                p.agg(s, [f[key]], [(k, None if k == hip.PH_A_COUNT_STAR else f[arg]) for k in KINDS])
            r, ex = run_plan(ctx, build, rows=False)
            want = EE.group_by([(k,) for k in ref[key]], [ref[arg]] * 5 + [None], KINDS)
            got = groups_of(r, 1)
            assert got == want, (order, arg, [(k, got.get(k), want[k]) for k in want if got.get(k) != want[k]][:3], ex)
            if key == "year":
                assert ("streaming aggregate" in ex) == (order == "sorted"), ex
                assert ("hash aggregate" in ex) == (order == "shuffled"), ex
            results[(order, arg)] = got
        if key == "neg":
            assert min(ref["neg"]) < 0 < max(ref["neg"])
    # the two tables hold the same rows but for the order of d: grouped by a key that does not read d, arguments that do not read d agree
    if key != "year":
        for arg in ("col", "dec", "case", "case_int", "truth"):
            assert results[("sorted", arg)] == results[("shuffled", arg)]


def test_group_by_year_gives_the_same_groups_streaming_and_hashed(ctx, main, main_sorted):
    """d holds the same dates in both tables, sorted in one and shuffled in the other: COUNT(*), MIN(d) and MAX(d) per year are the
    same answer from the streaming aggregate and from the hash aggregate"""
    out = []
    for t, _ in (main, main_sorted):
        def build(p):
            s = p.scan(t, list(range(7)))
            p.agg(s, [hip.pe_year(D)], [(hip.PH_A_COUNT_STAR, None), (hip.PH_A_MIN, hip.pe_col(D)), (hip.PH_A_MAX, hip.pe_col(D))])
        r, ex = run_plan(ctx, build, rows=False)
        out.append(({int(r["keys"][g][0]): (r["count"][g][0], r["sum"][g][1], r["sum"][g][2]) for g in range(r["ngroups"])}, ex))
    assert out[0][0] == out[1][0]
    assert "hash aggregate" in out[0][1] and "streaming aggregate" in out[1][1], (out[0][1], out[1][1])
    assert min(out[0][0]) < -5_000_000 and max(out[0][0]) > 5_000_000              # the years at both ends of the int32 day domain are groups


# ------------------------------------------------------------------ NULL-able operands
def test_null_able_column_gives_null_and_truth_zero(ctx, main_nulls):
    """the bitmap variant of a: pe_dec over it is NULL and pe_float's truth 0 in the NULL rows. Through an Agg grouped by id: count(x) is 0
    (finalised as NULL) and the sums skip the row; a Filter on truth = 1 drops the NULL rows."""
    t, cols = main_nulls
    add = [hip.X_COL(A), hip.X_COL(B), hip.X_ADD]
    ft = [hip.X_COL(A), hip.X_F32(-5.0), hip.X_OP(hip.PH_X_GT)]             # true in three rows of four

    def build(p):
        s = p.scan(t, list(range(7)))
        p.agg(s, [hip.pe_col(ID)], [(hip.PH_A_COUNT, hip.pe_dec(add)), (hip.PH_A_SUM, hip.pe_dec(add)), (hip.PH_A_SUM, hip.pe_float(ft)), (hip.PH_A_COUNT_STAR, None),
                                    (hip.PH_A_MIN, hip.pe_col(A))])
    r, ex = run_plan(ctx, build, rows=False)
    res = EE.decimal_program(add, cols, SCALES)
    fc = float_cols(cols, range(N), [(A, hip.PH_DEC64, 2)])
    truth = EE.float_truth([hip.X_COL(0), hip.X_F32(-5.0), hip.X_OP(hip.PH_X_GT)], fc, False).tolist()
    assert r["ngroups"] == N, ex
    nulls = 0
    for g in range(N):
        x = int(r["keys"][g][0])
        if cols[A][x] is None:
            nulls += 1
            assert res[x][0] is None and truth[x] == 0
            assert (r["count"][g][0], r["count"][g][1], r["count"][g][4]) == (0, 0, 0), (x, ex)
        else:
            assert (r["count"][g][0], r["sum"][g][1], r["count"][g][4], r["sum"][g][4]) == (1, res[x][0], 1, cols[A][x]), (x, ex)
        assert r["sum"][g][2] == truth[x] and r["count"][g][3] == 1, (x, ex)
    assert nulls == len([x for x in range(N) if x % 5 == 3]) and 0 < sum(truth) < N - nulls

    def filtered(p):
        s = p.scan(t, list(range(7)))
        pr = p.project(s, [hip.pe_col(ID), hip.pe_float(ft)])
        p.filter(pr, [hip.pred(1, hip.PH_EQ, I(1))])
    r, ex = run_plan(ctx, filtered)
    assert sorted(r["columns"][0].tolist()) == [x for x in range(N) if truth[x]], ex


def test_left_join_build_side_gives_null_and_truth_zero(ctx, main, second):
    """LEFT join, the main table probing: the odd ids have no match, the multiples of 6 two. Expressions over the build side's columns —
    alone and mixed with probe columns — are NULL / truth 0 in the unmatched rows"""
    t, cols = main
    t2, c2 = second
    mixed = [hip.X_COL(1), hip.X_COL(3), hip.X_ADD]                          # a + v over the join's output id, a, q, v
    ft = [hip.X_COL(3), hip.X_F32(-1000.0), hip.X_OP(hip.PH_X_GT)]
    ftm = [hip.X_COL(2), hip.X_COL(3), hip.X_MUL, hip.X_F32(-1e9), hip.X_OP(hip.PH_X_GE)]

    def build(p):
        probe = p.scan(t, list(range(7)))
        bld = p.scan(t2, list(range(6)))
        j = p.join(probe, bld, [ID], [K], [ID, A, Q, 7 + V], join_type=hip.PH_JT_LEFT)
        p.agg(j, [hip.pe_col(0)], [(hip.PH_A_COUNT, hip.pe_dec(mixed)), (hip.PH_A_SUM, hip.pe_dec(mixed)), (hip.PH_A_SUM, hip.pe_float(ft)),
                                   (hip.PH_A_SUM, hip.pe_float(ftm)), (hip.PH_A_COUNT_STAR, None), (hip.PH_A_COUNT, hip.pe_col(3))])
    r, ex = run_plan(ctx, build, rows=False)
    matches = {}
    for j, k in enumerate(c2[K]):
        matches.setdefault(k, []).append(c2[V][j])
    assert r["ngroups"] == N, ex
    seen = {0: 0, 1: 0, 2: 0}
    for g in range(N):
        x = int(r["keys"][g][0])
        vs = matches.get(x, [])
        seen[len(vs)] += 1
        fc = [EE.column(hip.PH_I32, [cols[Q][x]] * len(vs)), EE.column(hip.PH_DEC64, vs, 2)]
        t1 = int(EE.float_truth([hip.X_COL(1), hip.X_F32(-1000.0), hip.X_OP(hip.PH_X_GT)], fc, False).sum()) if vs else 0
        t2_ = int(EE.float_truth([hip.X_COL(0), hip.X_COL(1), hip.X_MUL, hip.X_F32(-1e9), hip.X_OP(hip.PH_X_GE)], fc, False).sum()) if vs else 0
        want_sum = sum(cols[A][x] + v for v in vs)
        got = (r["count"][g][0], r["sum"][g][1] if vs else 0, r["sum"][g][2], r["sum"][g][3], r["count"][g][4], r["count"][g][5])
        assert got == (len(vs), want_sum, t1, t2_, max(len(vs), 1), len(vs)), (x, got, ex)
        if not vs:
            assert r["count"][g][1] == 0                                     # the sum of no value: NULL
    assert seen[0] > 2000 and seen[1] > 1000 and seen[2] > 600

    def filtered(p):
        probe = p.scan(t, list(range(7)))
        bld = p.scan(t2, list(range(6)))
        j = p.join(probe, bld, [ID], [K], [ID, A, Q, 7 + V], join_type=hip.PH_JT_LEFT)
        pr = p.project(j, [hip.pe_col(0), hip.pe_float(ft)])
        p.filter(pr, [hip.pred(1, hip.PH_EQ, I(1))])
    r, ex = run_plan(ctx, filtered)
    assert sorted(r["columns"][0].tolist()) == sorted(c2[K]), ex              # every match (v > -1000.00 holds for all), no unmatched row


def test_null_able_shapes_outside_the_device_path_are_refused(ctx, main, main_nulls, second):
    """where NULL-able support ends the answer is PH_EUNSUPPORTED — the code is pinned, not the text: pe_year and pe_substr over a LEFT
    join's build side, a NULL-able column among fetched rows"""
    t, _ = main
    tn, _ = main_nulls
    t2, _ = second

    def left(exprs, root_agg=False):
        def build(p):
            probe = p.scan(t, list(range(7)))
            bld = p.scan(t2, list(range(6)))
            j = p.join(probe, bld, [ID], [K], [ID, 7 + V, 7 + DD, 7 + SS], join_type=hip.PH_JT_LEFT)
            if root_agg:
                p.agg(j, [hip.pe_col(0)], [(hip.PH_A_SUM, exprs[0])])
            else:
                p.project(j, exprs)
        return build
    assert error_code(ctx, left([hip.pe_col(0), hip.pe_year(2)])) == hip.PH_EUNSUPPORTED
    assert error_code(ctx, left([hip.pe_year(2)], root_agg=True), rows=False) == hip.PH_EUNSUPPORTED
    assert error_code(ctx, left([hip.pe_col(0), hip.pe_substr(3, 1, 1)])) == hip.PH_EUNSUPPORTED
    assert error_code(ctx, left([hip.pe_col(0), hip.pe_col(1)])) == hip.PH_EUNSUPPORTED          # a NULL-able column in fetch_rows
    assert error_code(ctx, left([hip.pe_col(0), hip.pe_dec([hip.X_COL(1), hip.X_CONST(1), hip.X_ADD])])) == hip.PH_EUNSUPPORTED
    assert error_code(ctx, left([hip.pe_col(0)])) is None                                        # the probe side alone is fetched

    def bitmap(exprs):
        def build(p):
            s = p.scan(tn, list(range(7)))
            p.project(s, exprs)
        return build
    assert error_code(ctx, bitmap([hip.pe_col(ID), hip.pe_col(A)])) == hip.PH_EUNSUPPORTED
    assert error_code(ctx, bitmap([hip.pe_col(ID), hip.pe_dec([hip.X_COL(A), hip.X_COL(B), hip.X_ADD])])) == hip.PH_EUNSUPPORTED
    assert error_code(ctx, bitmap([hip.pe_col(ID), hip.pe_float([hip.X_COL(A), hip.X_F32(2.0), hip.X_MUL], truth=False)])) == hip.PH_EUNSUPPORTED
    assert error_code(ctx, bitmap([hip.pe_col(ID), hip.pe_col(B)])) is None
