"""Which form every ph_plan join takes: the `join#` lines of ph_plan_explain for every plan builder of plan_amd/tpch.py over the SF1
database, with no switch set and with each single lowering switch set, against tests/golden/plan_join_forms_sf1.json. The lines carry
the form's name and its row counts, so a join that takes another block of the lowering (or another number of rows through it) shows.

The fixture holds, per plan, the lines with no switch set under "" and a switch's lines only where they differ from those. It was
recorded twice on the commit before the join lowering was split into one function per strategy; the two recordings were equal, so no
line is left out (UNSTABLE is empty).

The same runs pin the rest of the lowering: the lines that start with `agg#`, `scan#`, `filter#`, `project#` or `rows:` against
tests/golden/plan_agg_forms_sf1.json, in the same format, with the three switches of the aggregate lowering added to the matrix. That
fixture was recorded twice on the commit before the aggregate lowering was split into one function per step; UNSTABLE_AGG lists what
differed between the two (nothing did). Under the three new switches the `join#` lines are those of no switch, with one exception found
while recording (JOIN_UNDER_AGG_SWITCH): without the count push-down Q13's LEFT join runs as a join and reports itself. No line of any plan
shows PH_PLAN_NO_ROW_CODES: explain does not say how a VARCHAR group key got its codes (tests/plan_edges.py tells by the fetched keys).
`PYTHONPATH=.:tests python tests/test_gpu_plan_forms.py JOIN.json AGG.json` records both again."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
from plan_amd import hip, tpch

FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "plan_join_forms_sf1.json")
AGG_FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "plan_agg_forms_sf1.json")

SWITCHES = ("", "PH_PLAN_NO_KEY_PUSHDOWN", "PH_PLAN_NO_SORTED_PAIRS", "PH_PLAN_NO_EXISTS_PAIRS", "PH_PLAN_NO_LATE_FILTER",
            "PH_PLAN_NO_RUN_LOOKUP", "PH_PLAN_NO_MERGE", "PH_PLAN_NO_SWAP", "PH_PLAN_GATED_SMALL")
AGG_SWITCHES = ("PH_PLAN_NO_COUNT_PUSHDOWN", "PH_PLAN_NO_STREAM_AGG", "PH_PLAN_NO_ROW_CODES")
# the join fixture has no entry for the three switches above: their `join#` lines are those of "", but for what is written down here
JOIN_UNDER_AGG_SWITCH = {("q13", "PH_PLAN_NO_COUNT_PUSHDOWN"):
                         ["join#2: LEFT OUTER: table=direct, 1483615 pairs + 50005 probe rows without a match (their build side NULL)"]}
OTHER = ("agg#", "scan#", "filter#", "project#", "rows:")

PLANS = {
    "q1": tpch.q1_plan,
    "q2": tpch.q2_plan,
    "q3": tpch.q3_plan,
    "q4": tpch.q4_plan,
    "q5": tpch.q5_plan,
    "q7": tpch.q7_plan,
    "q8": tpch.q8_plan,
    "q9": tpch.q9_plan,
    "q10": tpch.q10_plan,
    "q11_grouped": lambda db: _one_of(tpch.q11_plans(db), 0),
    "q11_total": lambda db: _one_of(tpch.q11_plans(db), 1),
    "q12": tpch.q12_plan,
    "q13": tpch.q13_plan,
    "q14": tpch.q14_plan,
    "q15": tpch.q15_plan,
    "q15_rows": tpch.q15_rows_plan,
    "q16": tpch.q16_plan,
    "q17": tpch.q17_plan,
    "q17_whole": tpch.q17_whole_plan,
    "q18": tpch.q18_plan,
    "q19": tpch.q19_plan,
    "q20_groups": lambda db: _one_of(tpch.q20_plans(db), 0),
    "q20_suppliers": lambda db: _one_of(tpch.q20_plans(db), 1),
    "q20_whole": tpch.q20_whole_plan,
    "q21": tpch.q21_plan,
    "q21_no_residual": lambda db: tpch.q21_plan(db, residual=False),
    "q22_scalar": tpch.q22_scalar_plan,
    "q22": lambda db: tpch.q22_plan(db, q22_threshold(db)),
}
ROWS_ROOT = ("q2", "q15_rows", "q20_whole")   # plans whose root is a join: ph_plan_fetch_rows

# `join#` lines that differed between two recordings of the same commit, as (plan, switch, line index): none did
UNSTABLE = ()
UNSTABLE_AGG = ()

# every block of the join lowering is reached by at least one plan of the matrix ...
PHRASES = ("run lookup", "merge lookup", "roles swapped", "no table — the build side is clustered", "through the pairs of the table-less join",
           "with a residual condition", "evaluated BEHIND the join", "reduced by the probe key's domain",
           "semi-join marks in one pass", "(marks + selection)", "strict N:1 lookup", "fused filter+probe")
# ... but for these two, which no plan of the matrix showed when the fixture was recorded: the hand-built plans at the end of this file
HAND_BUILT = ("residual condition over the pairs", "LEFT OUTER")
# every step of the aggregate lowering too
AGG_PHRASES = ("children per parent", "input reduced to the rows the keys of join#", "groups stay on the device as a relation", "streaming aggregate",
               "hash aggregate", "count(distinct)", "fused scan plan")


def _one_of(plans, i):
    for k, p in enumerate(plans):
        if k != i:
            p.free()
    return plans[i]


_threshold = {}


def q22_threshold(db):
    if id(db) not in _threshold:
        p = tpch.q22_scalar_plan(db)
        p.run()
        _threshold[id(db)] = tpch.q22_threshold(p.fetch())
        p.free()
    return _threshold[id(db)]


_lines = {}


def explain_lines(db, name, switch):
    """(the `join#` lines, the OTHER lines) of plan `name` under `switch`: one run serves both comparisons"""
    key = (id(db), name, switch)
    if key not in _lines:
        ex = run_explain(db, name, switch).split("\n")
        _lines[key] = ([l for l in ex if l.startswith("join#")], [l for l in ex if l.startswith(OTHER)])
    return _lines[key]


def run_explain(db, name, switch):
    """ph_plan_explain after one run of plan `name` with `switch` set in the environment (the lowering reads it at run time)"""
    old = os.environ.pop(switch, None) if switch else None
    if switch:
        os.environ[switch] = "1"
    p = None
    try:
        p = PLANS[name](db)
        p.run()
        p.fetch_rows() if name in ROWS_ROOT else p.fetch()
        return p.explain()
    finally:
        if p is not None:
            p.free()
        if switch:
            del os.environ[switch]
            if old is not None:
                os.environ[switch] = old


def record(db):
    """(the join fixture, the fixture of the other lines): per plan the lines under "" and a switch's lines where they differ from those"""
    out = ({}, {})
    for name in PLANS:
        base = explain_lines(db, name, "")
        for o, b in zip(out, base):
            o[name] = {"": b}
        for sw in SWITCHES[1:] + AGG_SWITCHES:
            for o, b, lines in zip(out, base, explain_lines(db, name, sw)):
                if lines != b:
                    o[name][sw] = lines
    return out


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def db(ctx, sf1):
    d = tpch.Database(ctx, sf1)
    yield d
    d.free()


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(FIXTURE, encoding="utf-8"))


@pytest.fixture(scope="module")
def agg_fixture():
    return json.load(open(AGG_FIXTURE, encoding="utf-8"))


def test_fixture_covers_every_block():
    """the recorded matrix shows every form of the lowering at least once (else no plan would witness that block)"""
    fx = json.load(open(FIXTURE, encoding="utf-8"))
    assert sorted(fx) == sorted(PLANS)
    text = "\n".join(l for per in fx.values() for lines in per.values() for l in lines)
    for phrase in PHRASES:
        assert phrase in text, phrase
    for phrase in HAND_BUILT:
        assert phrase not in text, phrase   # (a plan that shows one makes its hand-built plan redundant)


def test_agg_fixture_covers_every_step():
    """the recorded matrix shows every step of the aggregate lowering at least once, and pins at least one `agg#` line of every plan"""
    fx = json.load(open(AGG_FIXTURE, encoding="utf-8"))
    assert sorted(fx) == sorted(PLANS)
    text = "\n".join(l for per in fx.values() for lines in per.values() for l in lines)
    for phrase in AGG_PHRASES:
        assert phrase in text, phrase
    for name, per in fx.items():
        for sw, lines in per.items():
            skip = {i for (n, s, i) in UNSTABLE_AGG if n == name and s == sw}
            assert name in ROWS_ROOT or any(l.startswith("agg#") and i not in skip for i, l in enumerate(lines)), (name, sw)
            assert any(i not in skip for i in range(len(lines))), (name, sw)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES + AGG_SWITCHES)
@pytest.mark.parametrize("name", list(PLANS))
def test_join_forms_equal_the_recording(db, fixture, name, switch):
    want = JOIN_UNDER_AGG_SWITCH.get((name, switch), fixture[name].get(switch, fixture[name][""]))
    got = explain_lines(db, name, switch)[0]
    skip = {i for (n, s, i) in UNSTABLE if n == name and s == switch}
    assert [l for i, l in enumerate(got) if i not in skip] == [l for i, l in enumerate(want) if i not in skip]


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES + AGG_SWITCHES)
@pytest.mark.parametrize("name", list(PLANS))
def test_aggregate_and_scan_lines_equal_the_recording(db, agg_fixture, name, switch):
    want = agg_fixture[name].get(switch, agg_fixture[name][""])
    got = explain_lines(db, name, switch)[1]
    skip = {i for (n, s, i) in UNSTABLE_AGG if n == name and s == switch}
    assert [l for i, l in enumerate(got) if i not in skip] == [l for i, l in enumerate(want) if i not in skip]


# ---- the two blocks no TPC-H plan of the matrix reaches (an INNER join with a residual condition; Q13's LEFT join runs as "children per
# parent" ahead of the join lowering): one small hand-built plan each, its rows against the oracle's join

N_LEFT = 4099                              # ragged against 256, 1024 and 4096


@pytest.fixture(scope="module")
def small(ctx):
    """left(id, a) and right(k, v): k hits the even ids once, the multiples of 6 twice and the odd ids never"""
    lid = np.arange(N_LEFT, dtype=np.int32)
    a = ((lid.astype(np.int64) * 2654435761) % 8192 - 2048).astype(np.int32)
    k = np.concatenate([np.arange(0, N_LEFT, 2), np.arange(0, N_LEFT, 6)]).astype(np.int32)
    v = ((np.arange(len(k)) * 37) % 8192 - 2048).astype(np.int32)
    left = hip.Table(ctx, [dict(typ=hip.PH_I32, arr=lid), dict(typ=hip.PH_I32, arr=a)], N_LEFT)
    right = hip.Table(ctx, [dict(typ=hip.PH_I32, arr=k), dict(typ=hip.PH_I32, arr=v)], len(k))
    oj = O.Join([O.col(O.OT_INT32, k)], None, len(k))
    m, op, ob = oj.probe_inner([O.col(O.OT_INT32, lid)], None, N_LEFT, 2 * len(k))
    assert m == len(k)
    found = oj.probe_mark([O.col(O.OT_INT32, lid)], None, N_LEFT)
    yield dict(left=left, right=right, lid=lid, a=a, k=k, v=v, op=op, ob=ob, found=found)
    left.free()
    right.free()


def _rows(ctx, build):
    p = hip.Plan(ctx)
    try:
        build(p)
        p.create()
        p.run()
        return p.fetch_rows(), p.explain()
    finally:
        p.free()


@pytest.mark.gpu
def test_inner_join_with_a_residual_condition_filters_the_pairs(ctx, small):
    """left x right on id = k where a < v: the oracle's pairs, filtered by the oracle's column-vs-column select"""
    s = small

    def build(p):
        l = p.scan(s["left"], [0, 1])
        r = p.scan(s["right"], [0, 1])
        p.join(l, r, [0], [0], [0, 1, 3], residual=hip.bool_tree(("colcmp", 1, hip.PH_LT, 3)))   # [left: 0 id, 1 a | right: 2 k, 3 v]
    got, ex = _rows(ctx, build)
    assert "residual condition over the pairs" in ex, ex
    pa, pv = np.ascontiguousarray(s["a"][s["op"]]), np.ascontiguousarray(s["v"][s["ob"]])
    keep = O.select_cols(O.col(O.OT_INT32, pa), O.OP_LT, O.col(O.OT_INT32, pv), n=len(pa))
    want = sorted(zip(s["lid"][s["op"]][keep].tolist(), pa[keep].tolist(), pv[keep].tolist()))
    assert 0 < len(want) < len(pa)
    assert sorted(zip(*(c.tolist() for c in got["columns"]))) == want, ex


@pytest.mark.gpu
def test_left_outer_join_keeps_the_unmatched_probe_rows(ctx, small):
    """left LEFT JOIN right on id = k, the probe side's id fetched: once per pair of the oracle's inner probe, once per row its mark probe leaves
    unmarked"""
    s = small

    def build(p):
        l = p.scan(s["left"], [0, 1])
        r = p.scan(s["right"], [0, 1])
        j = p.join(l, r, [0], [0], [0, 3], join_type=hip.PH_JT_LEFT)
        p.project(j, [hip.pe_col(0)])
    got, ex = _rows(ctx, build)
    assert "LEFT OUTER" in ex, ex
    want = np.sort(np.concatenate([s["lid"][s["op"]], s["lid"][s["found"] == 0]]))
    assert (s["found"] == 0).sum() == N_LEFT // 2 and len(want) == len(s["k"]) + N_LEFT // 2
    assert np.array_equal(np.sort(got["columns"][0]), want), ex


if __name__ == "__main__":
    import sys

    import tpch_data

    c = hip.Ctx(0)
    d = tpch.Database(c, tpch_data.load(1, 1, text=True))
    for path, fx in zip(sys.argv[1:3], record(d)):
        with open(path, "w", encoding="utf-8") as f:
            json.dump(fx, f, indent=1, ensure_ascii=False, sort_keys=True)
            f.write("\n")
    d.free()
    c.close()
