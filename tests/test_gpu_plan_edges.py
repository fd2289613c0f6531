"""ph_plan results form by form on small edge-shaped tables: every case of plan_edges.CASES is lowered into a hip.Plan and run, and
  (a) the phrase of ph_plan_explain that names the form the case was built to reach is there (under a PH_PLAN_NO_* switch: it is absent and
      the fallback's phrase is there) — a case whose phrase does not appear fails, it never skips;
  (b) the rows (join-rooted plans: every fetched column and its scale) or the groups (count, sum, min, max, avg as (sum, count), NULL as
      None) equal plan_edges.ref_plan's, the plain numpy / Python-int evaluation of the same description. Integers: no tolerance.
test_plan_edges_reference.py checks, without a device, that every case keeps and drops what its label says.

The forms and their cases (the degenerate variants of each: the probe side emptied by its filter, the build side emptied, every probe row
missing, one row against one row, the join under a GLOBAL aggregate with and without input rows):
  strict N:1 lookup / merge lookup / run lookup            lookup*, merge*, run3*, run4*, placement-lookup-* (four key-domain placements x sizes)
  counted N:1 lookup + conservative rerun                  counted-lookup / -merge / -run, every *-all_miss of the three lookups,
                                                           test_a_second_run_starts_conservative; declared-unique-has-duplicates (PH_ECONSTRAINT)
  filter fused into the direct build / gated sorted fill   fusedbuild*, gated* (a filtered build side never takes a lookup: the build-emptied
                                                           shapes of the lookups are gated-build_empty-under-* and selrows-build_empty-two-keys)
  build: selected rows / intermediate rows                 selrows*, intermediate*
  fused filter+probe / plain probe (N:M, fan-out 1/2/17)   fprobe*, probe*
  semi / anti (marks + selection)                          semi*, anti*
  filter + semi-join marks in one pass                     marks-for-build*
  residual condition (INNER pairs, SEMI, ANTI)             residual-inner*, residual-semi*, residual-anti*
  LEFT OUTER / children per parent                         left*, children*
  groups stay on the device / keys pushed into them        groups-below*, key-pushdown-inner*, key-pushdown-semi
  streaming / hash aggregate                               stream*, hash*
  fused scan plan (Agg <- Scan at the root, no GROUP BY)   scan-agg-global, scan-agg-global_empty; HAVING over the group without input:
                                                           test_a_having_judges_the_ungrouped_aggregate_without_input
  build side reduced by the probe key's domain             sideways*
  roles swapped / table-less clustered join / SEMI, ANTI   swap*, notable*, exists-pairs-semi*, exists-pairs-anti*, late-filter* (BEHIND the join)
  through its pairs (the 2^22 + 3-row clustered table)
  VARCHAR key pair, chains                                 string-keys, chain-empty-second-join, chain-pairs-then-lookup
  packed key words / too many group keys                   packed-keys (six keys in four words, INT32_MIN .. INT32_MAX in both halves, a NULL-able
                                                           key), packed-keys-five-words, packed-keys-five-below-a-join (PH_EUNSUPPORTED)
  count(distinct) through a side table                     distinct, distinct-global, distinct-empty, distinct-global-empty,
                                                           distinct-no-key-word-left (PH_EUNSUPPORTED)
  VARCHAR group key: row ids as codes / interned           string-group-key, string-group-key-NO_ROW_CODES, string-group-key-interned
  LEFT join with a residual condition under count()        children-residual (PH_EUNSUPPORTED: not counted as children per parent)"""
import numpy as np
import pytest

import plan_edges as E
from plan_amd import hip

pytestmark = pytest.mark.gpu

OP = {"lt": hip.PH_LT, "le": hip.PH_LE, "gt": hip.PH_GT, "ge": hip.PH_GE, "eq": hip.PH_EQ, "ne": hip.PH_NE}
JT = {"inner": hip.PH_JT_INNER, "semi": hip.PH_JT_SEMI, "anti": hip.PH_JT_ANTI, "left": hip.PH_JT_LEFT}
AGG = {"count_star": hip.PH_A_COUNT_STAR, "count": hip.PH_A_COUNT, "sum": hip.PH_A_SUM, "min": hip.PH_A_MIN, "max": hip.PH_A_MAX, "avg": hip.PH_A_AVG,
       "count_distinct": hip.PH_A_COUNT_DISTINCT}
COUNTS = ("count", "count_star", "count_distinct")


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


def device_table(ctx, t):
    specs = []
    for c in t["cols"]:
        if c["typ"] == "str":
            off = np.zeros(len(c["arr"]) + 1, dtype=np.int32)
            off[1:] = np.cumsum([len(s) for s in c["arr"]])
            specs.append(dict(typ=hip.PH_STR, arr=off, aux=np.frombuffer(b"".join(c["arr"]), dtype=np.uint8)))
        elif c["typ"] == "code":
            specs.append(dict(typ=hip.PH_CODE8, arr=c["arr"], dictionary=c["dictionary"]))
        else:
            specs.append(dict(typ={"i32": hip.PH_I32, "date": hip.PH_DATE, "i64": hip.PH_I64, "dec": hip.PH_DEC64}[c["typ"]], arr=c["arr"], scale=c["scale"]))
    d = hip.Table(ctx, specs, t["n"])
    for u in t["unique"]:
        hip.table_declare_unique(d, u)
    return d


@pytest.fixture(scope="module")
def big(ctx):
    """the clustered table on the device: uploaded once for all the cases that read it"""
    d = device_table(ctx, E.clustered())
    yield d
    d.free()


def lower(p, node, tabs, hosts):
    if node["op"] == "scan":
        t = hosts[node["table"]]
        preds = []
        for c, op, k in node["preds"]:
            col = t["cols"][c]
            preds.append(hip.pred(c, OP[op], hip.const(hip.PH_DEC64, i=k, scale=col["scale"]) if col["typ"] == "dec" else hip.const(hip.PH_I32, i=k)))
        bools = hip.bool_tree(("colcmp", node["colcmp"][0], OP[node["colcmp"][1]], node["colcmp"][2])) if node["colcmp"] else None
        return p.scan(tabs[node["table"]], list(range(len(t["cols"]))), preds, bools)
    if node["op"] == "join":
        probe, build = lower(p, node["probe"], tabs, hosts), lower(p, node["build"], tabs, hosts)
        res = hip.bool_tree(("colcmp", node["residual"][0], OP[node["residual"][1]], node["residual"][2])) if node["residual"] else None
        return p.join(probe, build, node["pkeys"], node["bkeys"], node["out"], join_type=JT[node["kind"]], residual=res)
    child = lower(p, node["child"], tabs, hosts)
    return p.agg(child, [hip.pe_col(g) for g in node["groups"]], [(AGG[k], None if c is None else hip.pe_col(c)) for k, c in node["aggs"]])


def run_case(ctx, build_plan, rooted):
    """build a hip.Plan, run it, fetch its groups (rooted == "groups") or rows: (result, explain()). The plan is always freed.
    A VARCHAR group key comes back as rows of a table column: r["key_strings"][k] holds the bytes of those rows, read while the plan lives."""
    p = hip.Plan(ctx)
    try:
        build_plan(p)
        p.create()
        p.run()
        r = p.fetch() if rooted == "groups" else p.fetch_rows()
        if rooted == "groups":
            r["key_strings"] = {}
            for k in range(r["keys"].shape[1]):
                typ, _scale, table, col = hip.plan_key_info(p, k)
                if typ == hip.PH_STR:
                    r["key_strings"][k] = hip.table_strings_bytes(ctx, table, col, r["keys"][:, k])
        return r, p.explain()
    finally:
        p.free()


def comparable(r, root):
    """the fetched result in ref_plan's terms: sorted row tuples and scales, or {key tuple: [per aggregate]} and scales"""
    if root["op"] != "agg":
        cols = [[s.encode() for s in c] if isinstance(c, list) else c.tolist() for c in r["columns"]]
        return sorted(zip(*cols)) if r["nrows"] else [], list(r["scales"])
    groups = {}
    for g in range(r["ngroups"]):
        key = tuple(None if r["key_null"] is not None and r["key_null"][g][k] else r["key_strings"][k][g] if k in r["key_strings"] else int(r["keys"][g][k])
                    for k in range(len(root["groups"])))
        row = []
        for a, (kind, _) in enumerate(root["aggs"]):
            cnt = r["count"][g][a]
            row.append(cnt if kind in COUNTS else None if cnt == 0 else (r["sum"][g][a], cnt) if kind == "avg" else r["sum"][g][a])
        assert key not in groups, key
        groups[key] = row
    return groups, list(r["scale"])


def check_case(ctx, monkeypatch, name, tabs):
    c = E.CASES[name]
    for sw in c["env"]:
        monkeypatch.setenv(sw, "1")
    (kind, want, kinds), _ = E.reference(name)
    root = c["plan"]
    if c["error"]:
        with pytest.raises(hip.PlanHipError) as e:
            run_case(ctx, lambda p: lower(p, root, tabs, c["tables"]), kind)
        assert e.value.code == getattr(hip, c["error"][0]) and c["error"][1] in str(e.value), str(e.value)
        return
    r, ex = run_case(ctx, lambda p: lower(p, root, tabs, c["tables"]), kind)
    for phrase in c["phrases"]:
        assert phrase in ex, (phrase, ex)
    for phrase in c["absent"]:
        assert phrase not in ex, (phrase, ex)
    got, scales = comparable(r, root)
    if kind == "rows":
        assert len(got) == len(want), (len(got), len(want), ex)
        assert got == want, ([(g, w) for g, w in zip(got, want) if g != w][:3], ex)
        assert scales == [s for _, s in kinds], ex
    else:
        assert got == want, ([(k, got.get(k), want[k]) for k in want if got.get(k) != want[k]][:3], [k for k in got if k not in want][:3], ex)
        for (agg, _), s, w in zip(root["aggs"], scales, kinds):
            if agg not in COUNTS:
                assert s == w, (agg, s, w, ex)
        if c["codes"]:                                 # which rows stand for the strings of a VARCHAR key: every group's own, or one per string
            k, how = c["codes"]
            ids = {int(x) for x in r["keys"][:, k]}
            assert len(ids) == (r["ngroups"] if how == "rows" else len(set(r["key_strings"][k]))), (how, len(ids), r["ngroups"])
            assert how == "rows" or len(ids) < r["ngroups"] or len(root["groups"]) == 1


@pytest.mark.parametrize("name", E.SMALL_CASES)
def test_small_tables(ctx, monkeypatch, name):
    c = E.CASES[name]
    tabs = {}
    try:
        for k, t in c["tables"].items():
            tabs[k] = device_table(ctx, t)
        check_case(ctx, monkeypatch, name, tabs)
    finally:
        for t in tabs.values():
            t.free()


@pytest.mark.parametrize("name", E.BIG_CASES)
def test_clustered_table(ctx, big, monkeypatch, name):
    c = E.CASES[name]
    tabs = {}
    try:
        for k, t in c["tables"].items():
            tabs[k] = big if t is E.clustered() else device_table(ctx, t)
        check_case(ctx, monkeypatch, name, tabs)
    finally:
        for t in tabs.values():
            if t is not big:
                t.free()


def test_the_tables_have_the_statistics_the_forms_rest_on(ctx, big):
    """what the lowering reads of the makers' tables: the order of the keys, the run length, the clustered table's size and order"""
    assert big.nrows >= 1 << 22 and hip.table_col_stats(big, E.BIG_KEY) & 3 == hip.PH_STAT_ASCENDING
    for place in ("i32_min", "i64_sparse", "i64_max"):
        d = E.dim(E.NDIM, place)
        t, s, a = device_table(ctx, d), device_table(ctx, E.dim(E.NDIM, place, shuffle=True)), device_table(ctx, E.fact(E.NFACT, d, "ascending"))
        try:
            assert hip.table_col_stats(t, E.DIM_KEY) == hip.PH_STAT_ASCENDING | hip.PH_STAT_STRICT | hip.PH_STAT_DECLARED_UNIQUE
            assert hip.table_col_stats(s, E.DIM_KEY) == hip.PH_STAT_DECLARED_UNIQUE
            assert hip.table_col_stats(a, E.F_KEY) == hip.PH_STAT_ASCENDING
            assert t.col_range(E.DIM_KEY) == (d["first"], d["first"] + (E.NDIM - 1) * d["step"])
        finally:
            t.free(); s.free(); a.free()
    for run_len in (3, 4):
        t = device_table(ctx, E.runs(1025, run_len))
        try:
            assert t.col_run_len(E.R_K1) == run_len and t.col_run_len(E.R_K2) == 0
        finally:
            t.free()


def test_a_second_run_starts_conservative(ctx):
    """a plan whose first run met dangling foreign keys in a strict lookup: the fetch reruns it in the conservative forms, and the next run() of
    the same plan starts there — no strict lookup any more, the same rows"""
    c = E.CASES["counted-lookup"]
    (_, want, _), _ = E.reference("counted-lookup")
    tabs = {k: device_table(ctx, t) for k, t in c["tables"].items()}
    p = hip.Plan(ctx)
    try:
        lower(p, c["plan"], tabs, c["tables"])
        p.create()
        p.run()
        r1, ex1 = p.fetch_rows(), p.explain()
        p.run()
        r2, ex2 = p.fetch_rows(), p.explain()
    finally:
        p.free()
        for t in tabs.values():
            t.free()
    assert ex1.startswith("plan run (optimistic forms)") and E.LOOK in ex1 and "a statistic did not hold" in ex1 and E.COUNTED in ex1, ex1
    assert ex2.startswith("plan run (conservative forms)") and E.LOOK not in ex2 and E.COUNTED in ex2 and E.MISSCOMP in ex2, ex2
    assert comparable(r1, c["plan"])[0] == want and comparable(r2, c["plan"])[0] == want


def test_a_having_judges_the_ungrouped_aggregate_without_input(ctx):
    """count(*), count(x), sum, min, max, avg without GROUP BY over a join whose probe side is empty: the one group (counts 0, the rest NULL)
    passes a HAVING over a count that 0 satisfies and fails every other one — a NULL aggregate passes no comparison. With input rows the same
    HAVING forms keep or drop the real group."""
    I = lambda v: hip.const(hip.PH_I32, i=v)   # noqa: E731
    D = lambda v: hip.const(hip.PH_DEC64, i=v, scale=2)   # noqa: E731
    conjuncts = [([hip.pred(0, hip.PH_EQ, I(0))], True, False), ([hip.pred(0, hip.PH_GT, I(0))], False, True),
                 ([hip.pred(1, hip.PH_LE, I(0)), hip.pred(0, hip.PH_GE, I(0))], True, False), ([hip.pred(2, hip.PH_GT, D(-10 ** 15))], False, True),
                 ([hip.pred(0, hip.PH_EQ, I(0)), hip.pred(3, hip.PH_GT, D(-10 ** 15))], False, False), ([hip.pred(1, hip.PH_LT, I(0))], False, False)]
    for name, column in (("lookup-global_empty", 1), ("lookup-global", 2)):
        c = E.CASES[name]
        (_, want, _), _ = E.reference(name)
        tabs = {k: device_table(ctx, t) for k, t in c["tables"].items()}
        try:
            for having, *keeps in conjuncts:
                p = hip.Plan(ctx)
                try:
                    lower(p, c["plan"], tabs, c["tables"])
                    p.create()
                    p.set_having(having)
                    p.run()
                    got = comparable(p.fetch(), c["plan"])[0]
                finally:
                    p.free()
                assert got == (want if keeps[column - 1] else {}), (name, [(h.col, h.op, h.k.i) for h in having], got)
        finally:
            for t in tabs.values():
                t.free()
    assert E.reference("lookup-global_empty")[0][1] == {(): [0, 0, None, None, None, None]}
