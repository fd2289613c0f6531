"""The references of the integer-domain edge tests, checked without a device: the Python restatements in domain_edges.py agree with
the oracle on seeded inputs at magnitudes the oracle accepts, and the case tables of the GPU tests satisfy their own conditions — so a
wrong reference can neither pass as a kernel bug nor hide one."""
from decimal import ROUND_HALF_EVEN, Decimal

import numpy as np

import domain_edges as DE
import oracle_lib as O
from domain_edges import I32_MAX, I64_MAX, I64_MIN  # noqa: F401
from plan_amd import hip, queries, tpchgen


def lineitem_columns(L):
    return dict(p=L["l_shipdate"], q=L["l_quantity"], e=L["l_extendedprice"], d=L["l_discount"], t=L["l_tax"],
                k0=L["l_returnflag"], k1=L["l_linestatus"])


def test_q1_and_q6_restatements_match_the_oracle(sf001):
    L = sf001["lineitem"]
    n = len(L["l_shipdate"])
    c = lineitem_columns(L)
    cutoff = queries.q1_shipdate_cutoff()
    mine = DE.lc_reference(DE.rows_of(c, 0, n), DE.I32_MIN, cutoff, 100, -1, 100, 1)     # f1 = 1.00 - d, f2 = 1.00 + t at scale 2
    want = O.q1(L, cutoff)
    by_key = {tuple(g[1]): g for g in mine}
    assert len(want) == len(mine) == 4
    for w in want:
        g = by_key[(w.returnflag, w.linestatus)]
        assert g[2][:4] == [w.sum_qty.value(), w.sum_base_price.unscaled(2), w.sum_disc_price.unscaled(4), w.sum_charge.unscaled(6)]
        assert g[3] == w.count_order
        m = (L["l_returnflag"] == w.returnflag) & (L["l_linestatus"] == w.linestatus) & (L["l_shipdate"] <= cutoff)
        assert g[2][4] == int(L["l_discount"][m].sum()) and g[0] == int(np.flatnonzero(m)[0])      # (values below 11: no wrap to fear)
    # the counted form of the same sums (RowKinds) equals the row-by-row form, whole table and ragged ranges
    kinds = DE.RowKinds(c)
    for b, e in ((0, n), (4, n - 3), (4100, 20_000), (8, 8)):
        assert DE.lc_reference(kinds.runs(b, e), 9000, cutoff, 100, -1, 100, 1) == DE.lc_reference(DE.rows_of(c, b, e), 9000, cutoff, 100, -1, 100, 1)
        assert DE.jit_reference(kinds.runs(b, e), 9000, cutoff, 77, -1, -5, 1) == DE.jit_reference(DE.rows_of(c, b, e), 9000, cutoff, 77, -1, -5, 1)
    # Q6: the discount's float32 compares are the oracle's own selection (not what is restated here); quantity < 24, one year of ship dates
    d1, d2, lo, hi, qty = queries.q6_constants()
    dcol = O.col(O.OT_DECIMAL, L["l_discount"], 2)
    keep = np.zeros(n, bool)
    keep[O.select(dcol, O.OP_LE, O.const(O.OT_FLOAT, f=hi), O.select(dcol, O.OP_GE, O.const(O.OT_FLOAT, f=lo), n=n))] = True
    fc = dict(p=L["l_shipdate"][keep], q=L["l_quantity"][keep], a=L["l_extendedprice"][keep], b=L["l_discount"][keep])
    rc, dsum = O.q6(L, d1, d2, lo, hi, qty)
    got = DE.fs_reference(DE.rows_of(fc, 0, int(keep.sum())), d1, d2 - 1, qty)
    assert rc == 0 and got[0] == dsum.unscaled(4)
    assert DE.fs_reference(DE.RowKinds(fc).runs(0, int(keep.sum())), d1, d2 - 1, qty) == got


def oracle_program(prog):
    out = []
    for op, col, ival, scale in prog:
        if op == hip.PH_X_COL:
            out.append((O.OX_COL, col, 0, 0))
        elif op == hip.PH_X_CONST:
            out.append((O.OX_CONST_INT, 0, ival, 0) if scale == 0 else (O.OX_CONST_DEC, 0, ival, scale))
        else:
            out.append(({hip.PH_X_ADD: O.OX_ADD, hip.PH_X_SUB: O.OX_SUB, hip.PH_X_MUL: O.OX_MUL}[op], 0, 0, 0))
    return out


def test_expression_programs_match_the_oracle():
    rng = np.random.default_rng(9)
    n = 4000
    a = rng.choice(rng.integers(-10 ** 6, 10 ** 6, 60), n).astype(np.int64)
    b = rng.choice(rng.integers(-10 ** 5, 10 ** 5, 40), n).astype(np.int64)
    for name, prog, scales, fit, overflow in DE.EXPR_CASES:
        ocols = [O.col(O.OT_DECIMAL, a, scales[0]), O.col(O.OT_DECIMAL, b, scales[1])]
        rc, want = O.eval_decimal(ocols, oracle_program(prog), None, n)
        assert rc == 0
        mine = DE.expected_values(prog, a, b, scales)
        assert len({w[1] for w in mine}) == 1
        assert [w[0] for w in mine] == O.odec_unscaled(want, mine[0][1]), name
        assert mine[:50] == [DE.eval_program(prog, {0: int(x), 1: int(y)}, dict(enumerate(scales))) for x, y in zip(a[:50], b[:50])]
        # the case table: every pair is on the side it is listed on, and the listed step is the one that overflows
        for x, y in fit + overflow:
            assert (DE.eval_program(prog, {0: x, 1: y}, dict(enumerate(scales))) == "overflow") == ((x, y) in overflow), (name, x, y)
    assert 153_092_023 * 60_247_241_209 == I64_MAX and 3_037_000_499 ** 2 <= I64_MAX < 3_037_000_500 ** 2
    # NULL in, NULL out
    assert DE.eval_program(DE.EXPR_CASES[0][1], {0: None, 1: I64_MIN}, {0: 0, 1: 0})[0] is None


def test_half_even_cents_and_sorted_rows_match_the_oracle():
    rng = np.random.default_rng(5)
    n = 3000
    for scale in (0, 1, 2, 4, 6):
        v = rng.integers(-5 * 10 ** 9, 5 * 10 ** 9, n).astype(np.int64)
        unit = 10 ** max(scale - 2, 0)
        v[: n // 3] = rng.integers(-2000, 2000, n // 3) * unit + (unit // 2) * rng.integers(-1, 2, n // 3)      # half-way cases of both signs
        cents = [DE.cents_half_even(int(x), scale) for x in v]
        assert cents == [int((Decimal(int(x)) / Decimal(10 ** scale)).quantize(Decimal("0.01"), rounding=ROUND_HALF_EVEN) * 100) for x in v]
        valid = rng.random(n) > 0.1
        date = rng.integers(DE.civil_days(1, 1, 1), DE.civil_days(9999, 12, 31), n).astype(np.int32)
        sel = np.sort(rng.choice(n, n // 2, replace=False)).astype(np.int64)
        for desc in ([False, True], [True, False]):
            for s in (None, sel):
                m = n if s is None else len(s)
                want, _ = O.sort_rows([O.col(O.OT_DECIMAL, v, scale, validity=np.packbits(valid, bitorder="little")), O.col(O.OT_DATE, date)], desc, sel=s, n=m)
                mine = DE.sorted_rows([(cents, valid), (date.tolist(), None)], desc, range(n) if s is None else s.tolist())
                assert mine == want.tolist(), (scale, desc)
    assert DE.cents_half_even(1234550, 4) == 12346 and DE.cents_half_even(1234450, 4) == 12344 and DE.cents_half_even(-1234550, 4) == -12346
    assert DE.cents_half_even(I64_MAX, 0) == I64_MAX * 100 and DE.cents_half_even(-I64_MAX, 1) == -I64_MAX * 10     # no wrap: Fractions
    # the generated sort columns hold what the GPU test is about: values whose cents leave int64 at scales 0 and 1
    for scale in (0, 1):
        v = DE.dec_sort_values(scale, 7, 300)
        assert any(not DE.fits64(int(x) * 10 ** (2 - scale)) for x in v) and any(abs(int(x)) < 10 ** 6 for x in v)
    assert DE.civil_days(1970, 1, 1) == 0 and DE.civil_days(1969, 12, 31) == -1 and DE.civil_days(1998, 12, 1) == tpchgen.days(1998, 12, 1)


def test_topk_and_having_filters_match_the_oracle():
    rng = np.random.default_rng(21)
    n, card = 20_000, 300
    keys = rng.integers(0, card, n).astype(np.int32)
    vals = rng.integers(-50_000, 50_000, n).astype(np.int64)
    valid = keys % 50 != 7                      # groups 7, 57, ...: every input NULL
    rc, od = O.eval_decimal([O.col(O.OT_DECIMAL, vals, 2)], [(O.OX_COL, 0, 0, 0)], None, n)
    ng, first, gk, gn, gv = O.groupby([O.col(O.OT_INT32, keys)], [O.col(O.OT_ODEC, od, validity=np.packbits(valid, bitorder="little"))],
                                      [(O.OA_SUM, 0)], None, n, card + 8)
    assert ng == card
    sums = [None if gv[g].kind == O.OV_NULL else gv[g].d.unscaled(2) for g in range(ng)]
    for g in range(ng):      # the oracle's sums are Python's
        m = (keys == gk[g][0]) & valid
        assert sums[g] == (sum(vals[m].tolist()) if m.any() else None)
    live = [g for g in range(ng) if sums[g] is not None]
    dense = np.array([sums[g] for g in live], np.int64)
    for k in (-10 ** 6, -1, 0, 12_345, 10 ** 7):
        sel = O.select(O.col(O.OT_DECIMAL, dense, 2), O.OP_GT, O.const(O.OT_DECIMAL, i=k, scale=2), n=len(dense))
        assert DE.having_reference(sums, hip.PH_GT, k) == {live[i] for i in sel.tolist()}
        for op, oop in ((hip.PH_GE, O.OP_GE), (hip.PH_LT, O.OP_LT), (hip.PH_LE, O.OP_LE), (hip.PH_EQ, O.OP_EQ), (hip.PH_NE, O.OP_NE)):
            assert len(O.select(O.col(O.OT_DECIMAL, dense, 2), oop, O.const(O.OT_DECIMAL, i=k, scale=2), n=len(dense))) == 0
            assert DE.having_reference(sums, op, k) == set()
    nulls = {g for g in range(ng) if sums[g] is None}
    for desc in (True, False):
        order = sorted(live, key=lambda g: -sums[g] if desc else sums[g])
        for k in (1, 2, len(nulls), len(nulls) + 1, len(nulls) + 5, ng - 1, ng, ng + 1):
            got = DE.topk_reference(sums, k, desc)
            if k <= len(nulls):
                assert got == nulls                 # NULLs first, all of them tie
            else:
                kth = sums[order[min(k - len(nulls), len(order)) - 1]]
                assert got == nulls | {g for g in live if (sums[g] >= kth if desc else sums[g] <= kth)}
    assert DE.topk_reference([I64_MIN, None, I64_MAX, -1, 0, I64_MAX], 1, True) == {1}
    assert DE.topk_reference([I64_MIN, None, I64_MAX, -1, 0, I64_MAX], 2, True) == {1, 2, 5}
    assert DE.topk_reference([I64_MIN, None, I64_MAX, -1, 0, I64_MAX], 2, False) == {0, 1}


def test_ladder_tables_satisfy_their_own_conditions():
    """the must-admit set is non-empty for every form, at least two steps that the documented rule admits on 256 CUs total 2^63 or more,
    the last step's single row does not fit int64, and the bounds the tests compute are the bounds the rows attain"""
    n = DE.N_LADDER
    for form in DE.FORMS:
        c = DE.lc_ladder_columns(form, 8192)
        shared = DE.fs_ladder_shared(form, 8192)
        for sign in (1, -1):
            lc = [(k, DE.lc_row_bound(c, *consts), prod) for k, consts, prod in DE.lc_ladder_steps(c, sign)]
            fs = [(k, DE.fs_row_bound(DE.fs_columns(shared, b, b0)), prod) for k, b, b0, prod in DE.fs_ladder_steps(shared, sign)]
            for name, steps in (("lc", lc), ("fs", fs)):
                assert all(abs(prod) <= bound and (k < 46 or bound < abs(prod) + abs(prod) // 8) for k, bound, prod in steps), (name, form)   # rows 2.. attain (nearly) the bound
                assert all((prod > 0) == (sign > 0) for _, _, prod in steps)
                assert [k for k, bound, _ in steps if DE.must_admit(n, bound)], (name, form)
                assert [k for k, _, prod in steps if not DE.fits64(prod)] == [66], (name, form)
                # what ph_scan_plan_run's rule predicts at 2^20 rows on 256 CUs: 4096 rows per workgroup in the wide and the narrow forms
                carried = [k for k, bound, prod in steps if 4096 * bound < DE.PROOF_LIMIT and n * abs(prod) >= 2 ** 63]
                assert len(carried) >= 2, (name, form, sign, carried)
                assert sorted(abs(p) for _, _, p in steps) == [abs(p) for _, _, p in steps]
        # the counted reference equals the row-by-row one on the ladder's own tables
        consts = DE.lc_ladder_steps(c, -1)[4][1]
        assert DE.lc_reference(DE.RowKinds(c).runs(4, 8000), DE.P_LO, DE.P_HI, *consts) == DE.lc_reference(DE.rows_of(c, 4, 8000), DE.P_LO, DE.P_HI, *consts)
        fc = DE.fs_columns(shared, -12345, -12300)
        kinds = DE.RowKinds(dict(shared, row0=np.arange(8192) == 0)).extend("b", fc["b"])
        assert DE.fs_reference(kinds.runs(0, 8192), DE.P_LO, DE.P_HI, 100) == DE.fs_reference(DE.rows_of(fc, 0, 8192), DE.P_LO, DE.P_HI, 100)
    # the forms the ladder tables are built for
    assert DE.lc_form(DE.lc_ladder_columns("n32", 64), 100, -1, 2 ** 31 - 9, 1) == "n32" and DE.lc_form(DE.lc_ladder_columns("n64", 64), 100, -1, 3, 1) == "n64"
    assert DE.fs_form(DE.fs_columns(DE.fs_ladder_shared("n32", 64), I32_MAX, I32_MAX - 200)) == "n32"
    assert DE.fs_form(DE.fs_columns(DE.fs_ladder_shared("n64", 64), 5, 4)) == "n64"


def test_boundary_cases_hit_their_bounds_exactly():
    M = I32_MAX
    want = {"be_2^31-1": (M, 1, 1, "n32"), "be_2^31": (M + 1, 1, 1, "n64"), "b1_2^31-1": (1, M, 1, "n32"), "b1_2^31": (1, M + 1, 1, "n64"),
            "b2_2^31-1": (1, 1, M, "n32"), "b2_2^31": (1, 1, M + 1, "n64"), "be_b1_46341x46340": (46_341, 46_340, 1, "n32"),
            "be_b1_65536x32768": (65_536, 32_768, 1, "n64")}
    assert 46_341 * 46_340 == 2_147_441_940 <= M < 65_536 * 32_768 == 2 ** 31
    for name, c, (A1, B1, A2, B2), form in DE.lc_boundary_cases():
        n = len(c["p"])
        be, b1, b2 = (DE.affine_bound(0, 1, DE.col_range(c["e"])), DE.affine_bound(A1, B1, DE.col_range(c["d"])), DE.affine_bound(A2, B2, DE.col_range(c["t"])))
        assert (be, b1, b2, form) == want[name], name
        # every narrowed copy exists (a span below 2^32) and the proof admits every run of the table
        assert all(DE.col_range(c[k])[1] - DE.col_range(c[k])[0] < 2 ** 32 for k in "qedt") and n * DE.lc_row_bound(c, A1, B1, A2, B2) < DE.PROOF_LIMIT
        f1, f2 = A1 + B1 * c["d"].astype(object), A2 + B2 * c["t"].astype(object)
        signs = {(int(np.sign(e)), int(np.sign(x)), int(np.sign(y))) for e, x, y in zip(c["e"][:8].tolist(), f1[:8].tolist(), f2[:8].tolist())}
        assert len(signs) == 8          # rows 0..7 pass the predicate and hold every sign combination of the extremes
        assert sorted({abs(int(x)) for x in c["e"][:8]}) == sorted({abs(DE.col_range(c["e"])[0]), abs(DE.col_range(c["e"])[1])})
        assert all(DE.P_LO + 1 <= int(p) <= DE.P_HI for p in c["p"][:8]) and int(c["p"][500]) == DE.P_LO
    fwant = {"ba_2^31-1": (M, "n32"), "ba_2^31": (M + 1, "n64"), "bb_2^31-1": (M, "n32"), "bb_2^31": (M + 1, "n64")}
    for name, c, form in DE.fs_boundary_cases():
        ba, bb = DE.affine_bound(0, 1, DE.col_range(c["a"])), DE.affine_bound(0, 1, DE.col_range(c["b"]))
        assert (max(ba, bb), form) == fwant[name] and DE.must_admit(len(c["p"]), ba * bb) and 2 * len(c["p"]) * (M + 1) * min(ba, bb) >= DE.PROOF_LIMIT
        assert {(int(np.sign(a)), int(np.sign(b))) for a, b in zip(c["a"][:4].tolist(), c["b"][:4].tolist())} == {(-1, -1), (1, -1), (-1, 1), (1, 1)}
