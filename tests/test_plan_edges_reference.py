"""The references and inputs of the ph_plan edge tests, checked without a device so that the device tests (test_gpu_plan_edges.py) cannot
inherit a mistake from them or pass vacuously: ref_join against the oracle's join on every table maker's output, ref_agg against fractions and
Python ints near the ends of int64, three tiny cases written out by hand, and for every case the device file runs the conditions on its
inputs that make it a test (something is kept and something is dropped; the cases labelled empty keep nothing; misses and fan-out past 16
are there where they are the point)."""
import fractions

import numpy as np
import pytest

import oracle_lib as O
import plan_edges as E

I64_MAX = E.I64_MAX


# ------------------------------------------------------------------ ref_join against the oracle's join
def _ocol(c):
    return O.col(O.OT_INT32 if c["typ"] == "i32" else O.OT_INT64, np.ascontiguousarray(c["arr"]))


def _small_pairs():
    """(name, probe key columns, build key columns) for every maker at n <= 4099"""
    out = []
    for place in ("i32_min", "i32_max", "i64_sparse", "i64_max"):
        for nd in (1, 255, 4099):
            d = E.dim(nd, place, shuffle=nd == 255)
            for order in ("shuffled", "ascending", "strict"):
                for dangling in ("none", "some", "all"):
                    f = E.fact(nd if order == "strict" else min(4099, nd * 3 + 1), d, order, dangling)
                    out.append((f"dim-{place}-{nd}-{order}-{dangling}", [f["cols"][E.F_KEY]], [d["cols"][E.DIM_KEY]]))
        dd = E.dupdim(255, place)
        out.append((f"dupdim-{place}", [E.fact(4099, dd, "shuffled", "some")["cols"][E.F_KEY]], [dd["cols"][0]]))
    for run_len in (3, 4):
        r = E.runs(1025, run_len)
        for dangling in ("none", "some", "all"):
            f = E.fact2(4099, r, dangling)
            out.append((f"runs{run_len}-{dangling}", [f["cols"][E.F2_K1], f["cols"][E.F2_K2]], [r["cols"][E.R_K1], r["cols"][E.R_K2]]))
    return out


PAIRS = _small_pairs()


@pytest.mark.parametrize("name", [p[0] for p in PAIRS])
def test_ref_join_equals_the_oracle_join(name):
    _, pk, bk = next(p for p in PAIRS if p[0] == name)
    np_, nb = len(pk[0]["arr"]), len(bk[0]["arr"])
    oj = O.Join([_ocol(c) for c in bk], None, nb)
    m, op, ob = oj.probe_inner([_ocol(c) for c in pk], None, np_, 1 << 20)
    found = oj.probe_mark([_ocol(c) for c in pk], None, np_).astype(bool)
    pa, ba = [c["arr"] for c in pk], [c["arr"] for c in bk]
    pr, br = E.ref_join("inner", pa, ba)
    assert m == len(pr) and sorted(zip(op.tolist(), ob.tolist())) == sorted(zip(pr.tolist(), br.tolist()))
    assert E.ref_join("semi", pa, ba).tolist() == np.nonzero(found)[0].tolist()
    assert E.ref_join("anti", pa, ba).tolist() == np.nonzero(~found)[0].tolist()
    lp, lb = E.ref_join("left", pa, ba)
    assert sorted(zip(lp.tolist(), lb.tolist())) == sorted(list(zip(op.tolist(), ob.tolist())) + [(int(i), -1) for i in np.nonzero(~found)[0]])
    if "-all" in name:
        assert m == 0 and not found.any()
    if "-some" in name and np_ >= 5:
        assert 0 < found.sum() < np_


def test_makers_have_the_shapes_they_promise():
    for place in ("i32_min", "i32_max", "i64_sparse", "i64_max"):
        d = E.dim(4099, place)
        k = d["cols"][E.DIM_KEY]["arr"].astype(object)
        assert all(b > a for a, b in zip(k[:-1], k[1:]))
        assert {"i32_min": k[0] == E.I32_MIN, "i32_max": k[-1] == E.I32_MAX, "i64_sparse": all(int(x) % (1 << 33) == 0 for x in k), "i64_max": k[-1] == I64_MAX}[place]
        s = E.dim(4099, place, shuffle=True)["cols"][E.DIM_KEY]["arr"]
        assert sorted(s.tolist()) == sorted(k.tolist()) and not np.all(s[1:] > s[:-1])
        a = E.fact(4099, d, "ascending", "some")["cols"][E.F_KEY]["arr"]
        assert np.all(a[1:] >= a[:-1]) and np.any(a[1:] == a[:-1])
        st = E.fact(255, d, "strict", "some")["cols"][E.F_KEY]["arr"]
        assert np.all(st[1:] > st[:-1])
    for run_len in (3, 4):
        r = E.runs(1025, run_len)
        k1 = r["cols"][E.R_K1]["arr"].astype(np.int64)
        assert np.array_equal(k1, k1[0] + np.arange(len(k1)) // run_len)                       # what ph_table_col_run_len measures
        assert len(set(zip(k1.tolist(), r["cols"][E.R_K2]["arr"].tolist()))) == len(k1)
    big = E.clustered()
    k = big["cols"][E.BIG_KEY]["arr"]
    assert big["n"] == (1 << 22) + 3 and k.dtype == np.int32 and np.all(k[1:] >= k[:-1]) and k[0] == 0
    lens = np.bincount(k)
    assert lens[:10].tolist() == [1, 2, 16, 17, 40, 1, 2, 16, 17, 40] and set(lens[:-1].tolist()) == {1, 2, 16, 17, 40}


# ------------------------------------------------------------------ ref_agg against fractions / Python ints
def test_ref_agg_sums_are_exact_near_the_ends_of_int64():
    vals = np.array([I64_MAX, I64_MAX, I64_MAX - 1, -I64_MAX, -I64_MAX, 5, -(2 ** 63)], dtype=np.int64)
    keys = np.array([1, 1, 1, 2, 2, 3, 2], dtype=np.int64)
    valid = np.array([1, 1, 1, 1, 1, 0, 1], dtype=bool)
    g = E.ref_agg([(keys, None)], [("sum", vals, valid), ("avg", vals, valid), ("min", vals, valid), ("max", vals, valid), ("count", vals, valid), ("count_star", None, None)], 7)
    assert g[(1,)] == [3 * I64_MAX - 1, (3 * I64_MAX - 1, 3), I64_MAX - 1, I64_MAX, 3, 3]
    assert g[(2,)] == [-2 * I64_MAX - 2 ** 63, (-2 * I64_MAX - 2 ** 63, 3), -(2 ** 63), -I64_MAX, 3, 3]
    assert g[(3,)] == [None, None, None, None, 0, 1]                                          # every input NULL: NULL, count 0
    assert 3 * I64_MAX - 1 > 2 ** 64                                                          # wider than 64 bits, kept exactly
    s, c = g[(1,)][1]
    assert fractions.Fraction(s, c) == sum(fractions.Fraction(int(v)) for v in vals[:3]) / 3
    # no group column: one group, also over zero rows
    assert E.ref_agg([], [("count_star", None, None), ("sum", vals[:0], None), ("min", vals[:0], None)], 0) == {(): [0, None, None]}
    # a NULL group key is its own group
    gk = E.ref_agg([(keys, valid)], [("count_star", None, None)], 7)
    assert gk == {(1,): [3], (2,): [3], (None,): [1]}


def test_the_vectorised_aggregate_equals_the_loop():
    rng = np.random.default_rng(7)
    k, x = rng.integers(-50, 50, 20_000), rng.integers(-10 ** 9, 10 ** 9, 20_000)
    aggs = [("sum", x, None), ("avg", x, None), ("min", x, None), ("max", x, None), ("count", x, None), ("count_star", None, None)]
    assert E._ref_agg_big([(k, None)], aggs, len(k)) == E.ref_agg([(k, None)], aggs, len(k))


def test_count_distinct_and_varchar_groups_equal_a_dict_group_by():
    """the two extensions of ref_agg against a plain dict of sets, on the columns the cases use and on a NULL-able VARCHAR-keyed toy"""
    t, a = E.distinct_input(), E.distinct_args()
    g, sel = t["cols"][E.D_G]["arr"], t["cols"][E.D_SEL]["arr"]
    ok = sel < E.DISTINCT_ARGS                                                                # the argument as the LEFT join of the cases makes it
    x = np.where(ok, a["cols"][1]["arr"][np.minimum(sel, E.DISTINCT_ARGS - 1)], 0)
    seen = {}
    for gi, xi, v in zip(g.tolist(), x.tolist(), ok.tolist()):
        seen.setdefault(gi, set())
        if v:
            seen[gi].add(xi)
    got = E.ref_agg([(g, None)], [("count_distinct", x, ok), ("count", x, ok)], t["n"])
    assert {k[0]: r[0] for k, r in got.items()} == {k: len(s) for k, s in seen.items()}
    assert all(1 < r[0] < r[1] for r in got.values())                                         # duplicates inside every group
    assert E.ref_agg([], [("count_distinct", x, ok)], t["n"]) == {(): [6]} and E.ref_agg([], [("count_distinct", x[:0], None)], 0) == {(): [0]}
    assert not ok.all() and len(set(x[~ok].tolist()) & set(x[ok].tolist())) > 0                 # a NULL hides a value that counts elsewhere
    s = E.named()["cols"][E.S_STR]["arr"]
    rows = {}
    for i, v in enumerate(s):
        rows.setdefault(v, []).append(i)
    got = E.ref_agg([(s, None)], [("count_star", None, None), ("min", np.arange(len(s)), None)], len(s))
    assert got == {(k,): [len(r), r[0]] for k, r in rows.items()} and set(rows) == set(E.STRING_POOL)
    assert b"" in rows and any(max(k) >= 0x80 for k in rows if k) and any(a != b and b.startswith(a) and a for a in rows for b in rows)
    toy = E.ref_agg([(E.strings([b"a", b"", b"a", b"ab"]), np.array([1, 1, 0, 1], dtype=bool))], [("count_distinct", [5, 5, 5, 6], None)], 4)
    assert toy == {(b"a",): [1], (b"",): [1], (None,): [1], (b"ab",): [1]}


def test_the_packed_key_columns_hold_the_domain_ends_in_both_halves():
    t = E.keyed()
    hi, lo, hi2 = (t["cols"][c] for c in (E.K_HI, E.K_DATE, E.K_HI2))
    assert {(int(a), int(b)) for a, b in zip(hi["arr"], lo["arr"])} == {(a, b) for a in E.EDGE4 for b in E.EDGE4}
    assert set(hi2["arr"].tolist()) == set(E.EDGE4) and lo["typ"] == "date" and t["cols"][E.K_CODE]["typ"] == "code"
    (_, groups, _), _ = E.reference("packed-keys")
    assert len(groups) == 512 and sum(k[5] is None for k in groups) == 128 and all(r[0] > 1 for r in groups.values())


def test_a_left_join_residual_is_part_of_the_on_condition():
    probe, build = np.array([5, 7, 9]), np.array([7, 5, 5])
    x, z = np.array([1, 1, 1]), np.array([0, 0, 2])                                          # keep the pairs with x <= z: (0, 2) only
    lp, lb = E.ref_join("left", probe, build, lambda p, b: x[p] <= z[b])
    assert sorted(zip(lp.tolist(), lb.tolist())) == [(0, 2), (1, -1), (2, -1)]


# ------------------------------------------------------------------ three cases by hand
def test_hand_computed_inner_and_left_join():
    probe, build = np.array([5, 7, 5, 9]), np.array([7, 5, 5])
    pr, br = E.ref_join("inner", probe, build)
    assert sorted(zip(pr.tolist(), br.tolist())) == [(0, 1), (0, 2), (1, 0), (2, 1), (2, 2)]
    lp, lb = E.ref_join("left", probe, build)
    assert sorted(zip(lp.tolist(), lb.tolist())) == [(0, 1), (0, 2), (1, 0), (2, 1), (2, 2), (3, -1)]
    assert E.ref_join("semi", probe, build).tolist() == [0, 1, 2] and E.ref_join("anti", probe, build).tolist() == [3]


def test_hand_computed_residual_and_two_column_keys():
    pk, bk = [np.array([1, 1, 2]), np.array([10, 11, 10])], [np.array([1, 2, 1, 1]), np.array([10, 10, 11, 10])]
    pr, br = E.ref_join("inner", pk, bk)
    assert sorted(zip(pr.tolist(), br.tolist())) == [(0, 0), (0, 3), (1, 2), (2, 1)]
    x, z = np.array([3, 9, 1]), np.array([3, 0, 9, 2])                                       # keep the pairs with x <= z
    res = lambda p, b: x[p] <= z[b]   # noqa: E731
    pr, br = E.ref_join("inner", pk, bk, res)
    assert sorted(zip(pr.tolist(), br.tolist())) == [(0, 0), (1, 2)]
    assert E.ref_join("semi", pk, bk, res).tolist() == [0, 1] and E.ref_join("anti", pk, bk, res).tolist() == [2]


def test_hand_computed_plan_with_a_left_join_under_an_aggregate():
    f = E.T([E.C("i32", [4, 6, 4, 8]), E.C("dec", [100, 200, 300, 400], 2)])
    d = E.T([E.C("i32", [4, 4, 6, 7]), E.C("dec", [-5, 15, 25, 35], 2), E.C("i32", [0, 1, 0, 1])])
    plan = E.agg(E.join(E.scan("f"), E.scan("d", [(2, "eq", 0)]), [0], [0], [0, 1, 2 + 1], kind="left"), [0],
                 [("count", 2), ("count_star", None), ("sum", 2), ("sum", 1), ("avg", 2)])
    (kind, groups, scales), facts = E.ref_plan(plan, dict(f=f, d=d))
    assert kind == "groups" and scales == [2, None, 2, 2, 2]
    assert groups == {(4,): [2, 2, -10, 400, (-10, 2)], (6,): [1, 1, 25, 200, (25, 1)], (8,): [0, 1, None, 400, None]}
    assert facts["joins"][0]["pairs"] == 3 and facts["joins"][0]["matched"] == 3 and facts["total"] == 4 and facts["kept"] == 4
    (kind, rows, kinds), _ = E.ref_plan(E.join(E.scan("f", [(1, "gt", 100)]), E.scan("d"), [0], [0], [0, 1, 2 + 1], kind="inner"), dict(f=f, d=d))
    assert kind == "rows" and rows == [(4, 300, -5), (4, 300, 15), (6, 200, 25)] and kinds == [("i32", 0), ("dec", 2), ("dec", 2)]


# ------------------------------------------------------------------ every device case is a test
def test_every_form_has_its_cases():
    forms = {c["form"] for c in E.CASES.values()}
    assert {"lookup", "merge", "run3", "run4", "fusedbuild", "gated", "selrows", "intermediate", "fprobe", "probe", "semi", "anti", "marks-for-build",
            "residual-inner", "residual-semi", "residual-anti", "left", "children", "groups-below", "stream", "hash", "sideways", "swap", "notable", "scan-agg",
            "exists-pairs-semi", "exists-pairs-anti", "late-filter", "key-pushdown-inner", "key-pushdown-semi", "string-keys", "packed-keys", "distinct",
            "string-group-key"} <= forms
    switches = {e for c in E.CASES.values() for e in c["env"]}
    assert switches == {"PH_PLAN_NO_MERGE", "PH_PLAN_NO_RUN_LOOKUP", "PH_PLAN_NO_LATE_FILTER", "PH_PLAN_NO_COUNT_PUSHDOWN", "PH_PLAN_NO_KEY_PUSHDOWN",
                        "PH_PLAN_NO_STREAM_AGG", "PH_PLAN_NO_SWAP", "PH_PLAN_NO_SORTED_PAIRS", "PH_PLAN_NO_EXISTS_PAIRS", "PH_PLAN_NO_ROW_CODES"}
    for c in E.CASES.values():
        assert c["phrases"] or c["absent"] or c["error"], c["name"]
        if c["env"]:
            assert c["absent"] or c["codes"], c["name"]        # a switch is witnessed by the absence of the form's phrase (or by the key's codes)


@pytest.mark.parametrize("name", list(E.CASES))
def test_case_inputs_make_it_a_test(name):
    c = E.CASES[name]
    (kind, result, _), f = E.reference(name)
    if c["label"] == "ordinary":
        assert 0 < f["kept"] < f["total"], f
    elif c["label"] == "empty":
        assert f["kept"] == 0 and f["input"] == 0, f
        if c["variant"] == "global_empty":                     # one group: every count 0, everything else NULL
            assert list(result) == [()] and set(result[()]) == {0, None}, result
        else:
            assert len(result) == 0
    elif c["label"] == "all":
        assert f["kept"] == f["scans"][0]["kept"] > 0, f
    else:
        assert c["label"] == "any"
    if c["variant"] in ("global", "global_empty") and c["form"] != "children":   # (children: the aggregate BELOW the root loses its group key)
        assert kind == "groups" and list(result) == [()]
    if c["variant"] == "all_miss":
        assert f["joins"][-1]["pairs"] == 0 and f["joins"][-1]["probe"] > 0 or c["form"] in ("sideways", "children", "groups-below"), f
    if c["variant"] == "build_empty":
        assert any(s["kept"] == 0 for s in f["scans"][1:]), f
    if c["variant"] == "one_row":
        assert all(s["rows"] == 1 for s in f["scans"]), f
    if c["point"] == "misses":
        assert any(j["matched"] < j["probe"] for j in f["joins"]), f
    if c["point"] in ("childless", "childless+several"):       # the LEFT join under the counts: parents (its probe side) and their children
        j = f["joins"][0]
        assert j["kind"] == "left" and j["probe"] > 0 and (j["matched"] == 0 if c["point"] == "childless" else 0 < j["matched"] < j["probe"] and j["max_fan"] > 1), f
    if c["point"] == "dups":
        assert any(j["max_fan"] > 16 for j in f["joins"]), f
