"""The hash aggregate's sink forms over constructed keys (agg_edges.py; its claims are checked without a device by
test_agg_edges_reference.py): key values at the edges of their domains, tuples that differ in one column, one half or their NULL mask
only, and keys built through the inverse of the table hash so that they share one global slot, one partition or one LDS slot. Every
comparison is exact: the group count, every group's key tuple and NULL flags, its first row, SUM / AVG (as sum and count) / MIN / MAX /
COUNT / COUNT(*), and first rows strictly increasing. Groups are matched to the reference by key tuple.

Why the loops these inputs drive end (read from agg_sink.inc / ops_agg.hip, not tried):
  * find_or_create probes linearly through a table of cap = 2 x gcap slots that holds at most gcap groups, so an EMPTY slot ends every
    walk after at most the chain's length; a lane that locks a slot publishes its id in the same iteration (nobody waits inside a branch),
    a LOCKED slot is looked at again at most 2^22 times, and every 256th step reads the error flag that an exhausted table sets;
  * every LDS insert loop runs `probes < 16 | 32 | 256 && spins < 1 << 16` and each iteration ends the loop or adds one to either;
  * the write-outs claim slots with `guard < 1 << 24` in the same half-full table; the host tries a bulk build at most 6 times, and the
    growing sink's relaunch loop doubles the table until every workgroup's next chunk fits, then every workgroup advances."""
import numpy as np
import pytest

import agg_edges as A
from join_edges import I32_MAX, I32_MIN, I64_MAX, I64_MIN
from plan_amd import hip

pytestmark = pytest.mark.gpu

TYPE = {"i64": hip.PH_I64, "dec64": hip.PH_DEC64, "i32": hip.PH_I32, "date": hip.PH_DATE, "code8": hip.PH_CODE8}
AGGS = [(hip.PH_A_SUM, 0), (hip.PH_A_AVG, 0), (hip.PH_A_MIN, 0), (hip.PH_A_MAX, 0), (hip.PH_A_COUNT, 0), (hip.PH_A_COUNT_STAR, -1)]
NA = len(AGGS)
# name: (rows, ph_agg_create's hint, environment, the kind ph_agg_sink_kind reports afterwards) — the forms of
# test_gpu_domain_edges_ops.SINK_FORMS, reached the same way. A test whose keys make a bulk build hand over names the kind it ends on.
FORMS = {
    "row": (5_000, 16, {}, "generic"),
    "lds": (300_000, 1024, {}, "generic"),
    "bulk1": (200_000, 100_000, {}, "bulk1"),
    "bulk2": (4_300_000, 50_000, {"PH_AGG_JIT": "1"}, "bulk2_spec"),
    "bulk2_generic": (4_300_000, 50_000, {"PH_AGG_JIT": "0"}, "bulk2"),
    "two_level": (4_300_000, 600_000, {}, "two_level"),
    "spec": ((1 << 20) + 12_345, 1024, {"PH_AGG_JIT": "1"}, "spec"),
    "generic_2^20": ((1 << 20) + 12_345, 1024, {"PH_AGG_JIT": "0"}, "generic"),
}


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


def bits(valid):
    return None if valid is None else np.packbits(valid, bitorder="little")


def signed64(v):
    lo = v & (2 ** 64 - 1)
    return lo - 2 ** 64 if lo >= 2 ** 63 else lo


def check_groups(r, want, name):
    nk = r["keys"].shape[1]
    assert r["ngroups"] == len(want), (name, r["ngroups"], len(want))
    assert np.all(np.diff(r["first_row"]) > 0), name
    keys, nulls, firsts, counts = r["keys"].tolist(), r["key_null"].tolist(), r["first_row"].tolist(), r["count"].tolist()
    seen = set()
    for g in range(r["ngroups"]):
        key = tuple(None if nulls[g][c] else keys[g][c] for c in range(nk))
        assert key in want and key not in seen, (name, g, key)
        seen.add(key)
        first, s, c, mn, mx, rows = want[key]
        cnts, sums = counts[g], r["sum"][g]
        assert firsts[g] == first and cnts[5] == rows and cnts[:5] == [c] * 5, (name, key, firsts[g], first, cnts, c, rows)
        if c:
            assert sums[0] == s and sums[1] == s, (name, key, sums[0], sums[1], s)
            assert (signed64(sums[2]), signed64(sums[3])) == (mn, mx), (name, key)


def env_of(monkeypatch, form):
    n, hint, env, kind = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return n, hint, kind


def rows_for(groups, n, dup=3, seed=41):
    return A.tiled(groups, n, seed, dup) if n >= A.TILE_FROM else A.rows_of(groups, n, seed, dup)


class Sunk:
    """key and argument columns of `rows` on the device, sunk into one table"""

    def __init__(self, ctx, rows, hint, key_validity="all", arg_nulls=True, sel=None, row_base=0, agg=None, sorted_form=False, kind=None):
        self.ctx, self.rows = ctx, rows
        nk = len(rows.types)
        which = range(nk) if key_validity == "all" else key_validity
        self.valid = [rows.valid[c] if c in which else None for c in range(nk)]
        self.arg_valid = rows.arg_valid if arg_nulls else np.ones(rows.n, bool)
        self.cols = [hip.DevColumn(ctx, TYPE[t], rows.cols[c], validity=bits(self.valid[c])) for c, t in enumerate(rows.types)]
        self.cols.append(hip.DevColumn(ctx, hip.PH_I64, rows.args(), validity=bits(rows.arg_valid) if arg_nulls else None))
        self.sel, self.row_base = sel, row_base
        self.agg = agg or hip.Agg(ctx, [TYPE[t] for t in rows.types], AGGS, hint)
        self.own = agg is None
        sel_dev = ctx.upload(sel.astype(np.int32)) if sel is not None else None
        if sorted_form:
            assert self.agg.sink_sorted(self.cols[:-1], self.cols[-1:], rows.n, row_base=row_base)
        else:
            self.agg.sink(self.cols[:-1], self.cols[-1:], sel_dev, rows.n if sel is None else len(sel), row_base=row_base)
        assert kind is None or self.agg.sink_kind == kind, (self.agg.sink_kind, kind)
        self.sel_dev = sel_dev

    def reference(self, src=True):
        r = self.rows
        return A.group_reference(r.cols, self.valid, r.kind, self.arg_valid, sel=self.sel, row_base=self.row_base, src=r.src if src else None)

    def check(self, name, want=None):
        want = self.reference() if want is None else want
        check_groups(self.agg.finalize(room=len(want)), want, name)
        return want

    def free(self):
        if self.own:
            self.agg.free()
        for c in self.cols:
            c.free()
        if self.sel_dev is not None:
            self.ctx.free(self.sel_dev)


def run(ctx, groups, n, hint, name, dup=3, **kw):
    s = Sunk(ctx, rows_for(groups, n, dup), hint, **kw)
    try:
        return s.check(name)
    finally:
        s.free()


# ------------------------------------------------------------------ 1. single-key domain edges
def key_column_values(ctx, agg, c, typ):
    """[(value or None)] of key column c of all groups from ph_agg_keys_dev, at the key's own width"""
    data, valid, ng, _ = agg.key_column(c, TYPE[typ])
    vals = ctx.download(data, A._DT[typ], ng)
    ok = np.unpackbits(ctx.download(valid, np.uint8, (ng + 7) // 8), bitorder="little")[:ng].astype(bool)
    ctx.free_many([data, valid])
    return [int(v) if o else None for v, o in zip(vals.tolist(), ok.tolist())]


@pytest.mark.parametrize("typ", ["i64", "dec64", "i32", "date", "code8"])
@pytest.mark.parametrize("form", list(FORMS))
def test_single_key_domain_edges(ctx, monkeypatch, form, typ):
    """every value of edge_table(type) is a group of its own in every sink form; the keys come back exactly from ph_agg_fetch and from
    ph_agg_keys_dev. No key has a validity bitmap; in bulk2 and two_level the argument has none either: only then does the second
    form count its partitions through the copy of the key switch in bulk_keys_batch (its PLAIN instances)"""
    n, hint, kind = env_of(monkeypatch, form)
    edges = A.edge_table(typ)
    s = Sunk(ctx, rows_for(A.single_key(typ, edges), n), hint, key_validity=(), arg_nulls=form not in ("bulk2", "two_level"), kind=kind)
    want = s.check(f"{form}/{typ}")
    assert sorted(k for (k,) in want) == sorted(edges)
    assert sorted(key_column_values(ctx, s.agg, 0, typ)) == sorted(edges)
    s.free()


@pytest.mark.parametrize("typ", ["i64", "dec64", "i32", "date", "code8"])
@pytest.mark.parametrize("stream", ["PH_STREAM_AGG_ONE_PASS", "PH_STREAM_AGG_TWO_PASS"])
def test_single_key_domain_edges_streaming(ctx, monkeypatch, stream, typ):
    """ph_agg_sink_sorted over the same values in ascending order (signed; CODE8 unsigned): runs of 1 .. 700 rows, accepted as ordered"""
    monkeypatch.setenv(stream, "1")
    edges = sorted(A.edge_table(typ))
    rng = np.random.default_rng(len(edges))
    lens = rng.integers(1, 700, len(edges))
    lens[:3] = [1, 2, 1023]
    g = A.single_key(typ, edges)
    rows = A.rows_of(g, int(lens.sum()), dup=0)
    src = np.repeat(np.arange(len(edges)), lens)
    rows = A.Rows(g, src, rows.kind, rows.arg_valid, [g.cols[0][src]])
    s = Sunk(ctx, rows, 1024, key_validity=(), sorted_form=True, kind="sorted")
    want = s.check(f"{stream}/{typ}")
    ctx.check_deferred()
    assert [k for (k,) in sorted(want, key=lambda k: want[k][0])] == edges
    assert key_column_values(ctx, s.agg, 0, typ) == edges          # (the streaming form numbers the groups in row order)
    s.free()


# ------------------------------------------------------------------ 2. tuple edges
MODES = [("all", "all", True, False), ("first", (0,), True, False), ("none", (), False, False), ("all+sel", "all", True, True)]


def run_tuples(ctx, types, form, n, hint, modes, kind):
    for mode, which, arg_nulls, with_sel in modes:
        g = A.tuple_edges(types)
        g = g if which == "all" else g.keep_validity(which)
        total = int(n / 0.59) if with_sel else n     # a selection of 60 % still sinks n rows and more: the form is the one named
        rows = rows_for(g, total)
        sel = np.flatnonzero(np.random.default_rng(7).random(total) < 0.6) if with_sel else None
        assert sel is None or len(sel) >= n
        s = Sunk(ctx, rows, hint, key_validity=which, arg_nulls=arg_nulls, sel=sel, row_base=1000, kind=kind)
        want = s.check(f"{form}/{'-'.join(types)}/{mode}")
        s.free()
        if which == "all":      # the NULL groups are there, each once, over rows whose bytes under the NULL differ
            for base in g.info["null_base"]:
                for mask in range(1, 1 << len(types)):
                    key = tuple(None if (mask >> c) & 1 else base[c] for c in range(len(types)))
                    assert want[key][5] >= (3 if sel is None else 1)


@pytest.mark.parametrize("types", A.TUPLE_TYPES, ids=["-".join(t) for t in A.TUPLE_TYPES])
@pytest.mark.parametrize("form", ["row", "lds", "bulk1"])
def test_tuple_edges(ctx, monkeypatch, form, types):
    """tuples that differ in one column (or one half of one column) only, transposed tuples and all 2^nk NULL patterns, with validity
    bitmaps on all key columns, on the first only, on none (and no NULL arguments: the instances without validity), and under a selection"""
    n, hint, kind = env_of(monkeypatch, form)
    run_tuples(ctx, types, form, n, hint, MODES, kind)


@pytest.mark.parametrize("form,types,modes", [("bulk2", ("i32", "date", "i64"), [MODES[0], MODES[2]]), ("bulk2_generic", ("i64", "code8", "i32", "date"), MODES[3:]),
                                              ("spec", ("i64", "code8", "i32", "date"), [MODES[1], MODES[3]])],
                         ids=["bulk2", "bulk2_generic", "spec"])
def test_tuple_edges_big_forms(ctx, monkeypatch, form, types, modes):
    n, hint, kind = env_of(monkeypatch, form)
    run_tuples(ctx, types, form, n, hint, modes, kind)


# ------------------------------------------------------------------ 3. one global probe chain
def ordinary(n, seed):
    rng = np.random.default_rng(seed)
    return A.Groups(["i64"], [np.unique(rng.integers(I64_MIN, I64_MAX, n, endpoint=True, dtype=np.int64))])


@pytest.mark.parametrize("form,m,two_key", [("row", 300, False), ("lds", 300, False), ("bulk1", 300, False), ("row", 2000, False), ("row", 300, True)],
                         ids=["row-300", "lds-300", "bulk1-300", "row-2000", "row-300-two-keys"])
def test_one_global_probe_chain(ctx, monkeypatch, form, m, two_key):
    """m keys with one home slot in the global table, 40 more whose home lies inside their chain: every lookup walks the chain (past
    the error-flag guard of every 256th step) and compares keys whose hashes agree in the low 24 bits"""
    n, hint, kind = env_of(monkeypatch, form)
    g = A.one_global_slot(m, 40, two_key=two_key)
    if not two_key:
        g = g.concat(ordinary(200, m))
    run(ctx, g, n, hint, f"chain/{form}/{m}", dup=min(3, n // len(g)), kind=kind)     # (2 240 groups in 5 000 rows: twice each)


def test_one_global_probe_chain_survives_a_resize(ctx):
    """the chain's 340 groups first, then a sink of 30 000 rows over them and 8 000 new groups: the table grows (agg_resize + the
    rehash kernel) while the chain exists, and the chain's groups are found again afterwards"""
    chain = A.one_global_slot(300, 40)
    first = A.rows_of(chain, 5_000)
    both = A.rows_of(chain.concat(ordinary(8_000, 5)), 30_000, seed=43)
    s1 = Sunk(ctx, first, 16)
    before = s1.agg.group_count()
    s2 = Sunk(ctx, both, 16, agg=s1.agg, row_base=first.n)
    assert before == 340 and s1.agg.group_count() > 8_000
    cols = [np.concatenate([a, b]) for a, b in zip(first.cols, both.cols)]
    want = A.group_reference(cols, None, np.concatenate([first.kind, both.kind]), np.concatenate([first.arg_valid, both.arg_valid]))
    check_groups(s1.agg.finalize(room=len(want)), want, "chain, two sinks")
    s2.free()
    s1.free()


# ------------------------------------------------------------------ 4. one partition
T1 = A.bulk_T(1, NA)


@pytest.mark.parametrize("form,m", [("bulk1", 100), ("bulk1", 3 * T1), ("bulk1", 60_000), ("bulk2", 60_000), ("two_level", 60_000)],
                         ids=["bulk1-100", "bulk1-3T", "bulk1-60000", "bulk2-60000", "two_level-60000"])
def test_all_groups_in_one_partition(ctx, monkeypatch, form, m):
    """every group in ONE partition (hash bits 40..53 equal): one build workgroup sees all rows. 100 groups fit its LDS table; 3 T close it
    (T - T/4 entries) and the other rows take find_or_create inside the build, decided in phase 1; 60 000 do the same at scale, void the
    second form's attempt (the host falls back to the first form) and overflow the two-level form's one bin. Every group has at least 3
    rows: a group created twice shows as a wrong count."""
    n, hint, kind = env_of(monkeypatch, form)
    assert m == 100 or m > A.closes_at(T1)
    run(ctx, A.one_partition(m), n, hint, f"partition/{form}/{m}", kind="bulk1" if form in ("bulk2", "two_level") else kind)


# ------------------------------------------------------------------ 5. the 32-probe window
@pytest.mark.parametrize("form,m", [("bulk1", 31), ("bulk1", 32), ("bulk1", 33), ("bulk1", 100), ("bulk2", 33)], ids=lambda x: str(x))
def test_probe_window_of_the_build_tables(ctx, monkeypatch, form, m):
    """probe_window_rows: m keys of one partition that share ONE slot of its LDS table, 50 rows each and more, among 2 000 ordinary
    groups of the same partition; the rows of the same-slot keys lead the input, so they meet in the empty table of their build
    workgroup (test_agg_edges_reference.py replays the insert rule over this very row order). 31 and 32 keys all enter, the 32nd at
    the window's last place, where a phase-1 lookup that stops one probe early would create it a second time; of 33 and 100 keys
    exactly 32 enter and the others leave with the window exhausted, are flagged and take find_or_create in phase 1. In bulk2 the
    33rd key voids the attempt in its first step and the host falls back to the first form. The ordinary groups close the table
    later. Exactly m + 2000 groups come back, each once."""
    n, hint, kind = env_of(monkeypatch, form)
    rows = A.probe_window_rows(m, n)
    s = Sunk(ctx, rows, hint, kind="bulk1" if form == "bulk2" else kind)
    want = s.check(f"window/{form}/{m}")
    s.free()
    assert len(want) == m + 2000 and min(v[5] for v in want.values()) >= 50


# ------------------------------------------------------------------ 6. one LDS slot in the pre-aggregating sink
@pytest.mark.parametrize("form", ["lds", "spec", "generic_2^20"])
@pytest.mark.parametrize("m", [100, "half+50"])
def test_one_lds_slot_of_the_sink(ctx, monkeypatch, form, m):
    """m keys in ONE slot of every workgroup's LDS table: the first 16 probes find room, the others go to the global table row by row
    while their neighbours stay in LDS; with half the table + 50 keys most rows do"""
    n, hint, kind = env_of(monkeypatch, form)
    # (the specialised table keeps per-aggregate counts — agg_spec_need_cnt — because Sunk gives the argument a validity bitmap)
    slots = A.spec_slots(1, NA, True, hint) if form == "spec" else A.sink_slots(1, NA)
    m = slots // 2 + 50 if m == "half+50" else m
    assert m > A.SINK_PROBE_WINDOW
    run(ctx, A.one_lds_slot(m).concat(ordinary(40, m)), n, hint, f"lds slot/{form}/{m}", kind=kind)


# ------------------------------------------------------------------ 7. streaming aggregate keys
STREAM_TYPES = ("i32", "date", "code8", "i64")
HEADS = [4, 256, 1024, 2048]


def stream_rows(cols, seed=3):
    g = A.Groups(STREAM_TYPES[: len(cols)] if len(cols) > 1 else ["i64"], cols)
    n = len(g)
    rng = np.random.default_rng(seed)
    return A.Rows(g, np.arange(n), rng.integers(0, len(A.VALUES), n), rng.random(n) > 0.1, g.cols)


def boundary_columns():
    """3000 rows, four key columns: run heads on rows 4, 256, 1024 and 2048 where only the LAST column changes (through the int64 edges,
    ascending), a head on row 2500 where the first column goes -1 -> 0 while every later column drops to its lowest value"""
    n = 3000
    i = np.arange(n)
    step = sum((i >= h).astype(np.int64) for h in HEADS)
    last = np.array([I64_MIN, -2 ** 32, -1, 0, 2 ** 32], np.int64)[step]
    late = i >= 2500
    return [np.where(late, 0, -1).astype(np.int32), np.where(late, I32_MIN, I32_MAX).astype(np.int32), np.where(late, 0, 255).astype(np.uint8),
            np.where(late, I64_MIN, last)]


@pytest.mark.parametrize("stream", ["PH_STREAM_AGG_ONE_PASS", "PH_STREAM_AGG_TWO_PASS"])
def test_streaming_aggregate_key_boundaries(ctx, monkeypatch, stream):
    monkeypatch.setenv(stream, "1")
    rows = stream_rows(boundary_columns())
    s = Sunk(ctx, rows, 1024, key_validity=(), sorted_form=True)
    want = s.check(stream, s.reference(src=False))
    ctx.check_deferred()
    assert sorted(v[0] for v in want.values()) == [0] + HEADS + [2500]
    s.free()
    # ascending over the whole int32 domain, -1 -> 0 included
    col = np.repeat(np.array(A.I32_EDGES, np.int32), 300)
    g = A.Groups(["i32"], [col])
    rows = A.Rows(g, np.arange(len(col)), rows.kind[: len(col)], rows.arg_valid[: len(col)], g.cols)
    s = Sunk(ctx, rows, 1024, key_validity=(), sorted_form=True)
    want = s.check(stream + "/i32", s.reference(src=False))
    ctx.check_deferred()
    assert len(want) == len(A.I32_EDGES)
    s.free()


def descents():
    wrap = [np.repeat(np.array([0, I64_MAX, I64_MIN], np.int64), 700)]            # INT64_MAX -> INT64_MIN: a descent, not a wrap upwards
    fourth = boundary_columns()
    fourth[3] = fourth[3].copy()
    fourth[3][1024:2048] = -2                                                    # ... -1 | -2: below its predecessor in the fourth column only
    return [("int64 max to min", wrap), ("fourth column", fourth)]


@pytest.mark.parametrize("stream", ["PH_STREAM_AGG_ONE_PASS", "PH_STREAM_AGG_TWO_PASS"])
@pytest.mark.parametrize("case", [0, 1], ids=["int64_max_to_min", "fourth_column_only"])
def test_streaming_aggregate_refuses_descending_keys(ctx, monkeypatch, stream, case):
    """rows that are not ordered by the key tuple are a deferred PH_ECONSTRAINT; ph_agg_sink over the same rows then gives the reference"""
    monkeypatch.setenv(stream, "1")
    name, cols = descents()[case]
    rows = stream_rows(cols)
    s = Sunk(ctx, rows, 1024, key_validity=(), sorted_form=True)
    with pytest.raises(hip.PlanHipError) as e:
        s.agg.group_count()
    assert e.value.code == hip.PH_ECONSTRAINT, name
    s.free()
    ctx.check_deferred()                                                          # reported once
    s = Sunk(ctx, rows, 1024, key_validity=())
    want = s.check(name, s.reference(src=False))
    assert len(want) == (3 if case == 0 else 6)
    s.free()


# ------------------------------------------------------------------ 8. device-side columns
SMALL_KINDS = np.array([2, 3, 4, 7, 8])          # VALUES -1, 0, 1, 12 345, -987 654 321: sums that fit int64


def column_rows(ng, typ, seed):
    """ng groups of two rows each, in shuffled order: key 0 is a distinct PH_I64 (the int64 edge values first), key 1 a value of
    edge_table(typ); in every third group key 1 and every argument are NULL"""
    rng = np.random.default_rng(seed)
    e64, e = A.edge_table("i64"), A.edge_table(typ)
    k0 = np.array([e64[i] if i < len(e64) else 3 * i + (i << 33) for i in range(ng)], dtype=np.int64)
    assert len(np.unique(k0)) == ng
    k1 = np.array([e[i % len(e)] for i in range(ng)], dtype=np.int64).astype(A._DT[typ])
    third = np.arange(ng) % 3 == 2
    g = A.Groups(["i64", typ], [k0, k1], [None, ~third])
    src = rng.permutation(np.repeat(np.arange(ng), 2))
    rows = A.Rows(g, src, SMALL_KINDS[rng.integers(0, len(SMALL_KINDS), 2 * ng)], ~third[src], [k0[src], k1[src]])
    return rows, third


def packed_bits(ctx, ptr, ng):
    raw = ctx.download(ptr, np.uint8, (ng + 7) // 8)
    return raw, np.unpackbits(raw, bitorder="little")[:ng].astype(bool)


@pytest.mark.parametrize("ng", [1, 7, 8, 9, 63, 64, 65, 16_385, 70_001])
def test_device_side_key_and_value_columns(ctx, ng):
    """ph_agg_keys_dev / ph_agg_values_dev: data exact at the key's own width, every validity byte exact (the bits past the last group
    of the last byte are 0), NULL keys and NULL aggregates (COUNT of a group without inputs among them) clear their bit"""
    for typ in ("i32", "code8", "date") if ng < 1000 else (("i32", "code8", "date")[ng % 3],):
        rows, third = column_rows(ng, typ, ng)
        s = Sunk(ctx, rows, 1024)
        want = s.reference()
        assert len(want) == ng and s.agg.group_count() == ng
        d0, v0, n0, _ = s.agg.key_column(0, hip.PH_I64)
        d1, v1, n1, _ = s.agg.key_column(1, TYPE[typ])
        assert n0 == n1 == ng
        key0 = ctx.download(d0, np.int64, ng)
        key1 = ctx.download(d1, A._DT[typ], ng)
        raw0, ok0 = packed_bits(ctx, v0, ng)
        raw1, ok1 = packed_bits(ctx, v1, ng)
        tail = (1 << (ng % 8)) - 1 if ng % 8 else 0xFF
        assert ok0.all() and raw0[-1] == tail and (raw0[:-1] == 0xFF).all()
        g = rows.groups
        of = {int(k): i for i, k in enumerate(g.cols[0].tolist())}
        idx = np.array([of[int(k)] for k in key0.tolist()])
        assert len(set(idx.tolist())) == ng
        assert np.array_equal(ok1, ~third[idx])
        assert np.array_equal(key1[ok1], g.cols[1][idx][ok1]) and key1.dtype == A._DT[typ]
        assert np.array_equal(raw1, np.packbits(~third[idx], bitorder="little"))
        with pytest.raises(hip.PlanHipError) as e:
            s.agg.value_column(1)
        assert e.value.code == hip.PH_EUNSUPPORTED                                    # AVG
        for a, (kind, _) in enumerate(AGGS):
            if kind == hip.PH_A_AVG:
                continue
            dv, vv, nv = s.agg.value_column(a)
            assert nv == ng
            vals = ctx.download(dv, np.int64, ng)
            raw, ok = packed_bits(ctx, vv, ng)
            ref = [want[(int(k0), None if third[i] else int(g.cols[1][i]))] for k0, i in zip(key0.tolist(), idx.tolist())]
            expect = [{hip.PH_A_SUM: r[1], hip.PH_A_MIN: r[3], hip.PH_A_MAX: r[4], hip.PH_A_COUNT: r[2], hip.PH_A_COUNT_STAR: r[5]}[kind] if r[2] or
                      kind == hip.PH_A_COUNT_STAR else None for r in ref]
            assert ok.tolist() == [x is not None for x in expect], (typ, a)
            assert vals[ok].tolist() == [x for x in expect if x is not None], (typ, a)
            assert np.array_equal(raw, np.packbits(ok, bitorder="little"))
            assert (kind == hip.PH_A_COUNT_STAR) == bool(ok.all()) or ng < 3
            ctx.free_many([dv, vv])
        ctx.free_many([d0, v0, d1, v1])
        s.free()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_value_column_reports_a_sum_wider_than_int64(ctx, where):
    """one group of 16 385 (first seen first, in the middle or last) sums 2 x INT64_MAX: PH_EOVERFLOW for SUM, MIN / MAX / COUNT unaffected"""
    ng = 16_385
    wide = {"first": 0, "middle": ng // 2, "last": ng - 1}[where]
    key = np.repeat(np.arange(ng, dtype=np.int64) * 7 - 50_000, 2)
    kind = np.full(2 * ng, 7)
    kind[2 * wide: 2 * wide + 2] = 6                                                  # VALUES[6] = INT64_MAX
    g = A.Groups(["i64"], [key])
    rows = A.Rows(g, np.arange(2 * ng), kind, np.ones(2 * ng, bool), g.cols)
    s = Sunk(ctx, rows, 1024)
    with pytest.raises(hip.PlanHipError) as e:
        s.agg.value_column(0)
    assert e.value.code == hip.PH_EOVERFLOW
    for a, expect in ((2, 12_345), (3, 12_345), (4, 2), (5, 2)):
        dv, vv, nv = s.agg.value_column(a)
        vals = ctx.download(dv, np.int64, ng)
        assert nv == ng and packed_bits(ctx, vv, ng)[1].all()
        assert sorted(vals.tolist()) == sorted([expect] * (ng - 1) + [I64_MAX if a in (2, 3) else 2])
        ctx.free_many([dv, vv])
    s.check("wide sum", s.reference(src=False))                                       # (the 128-bit sum itself is exact)
    s.free()


# ------------------------------------------------------------------ 9. DISTINCT composition at the edges
def test_distinct_composition_over_edge_values(ctx):
    """count(distinct x), sum(distinct x) per group by the documented route — a side table keyed by (group key, x), its key columns
    through ph_agg_keys_dev, re-sunk with ph_agg_sink_masked — with x over the int64 edge values and NULL, the group key NULL-able"""
    rng = np.random.default_rng(9)
    n = 40_000
    e = np.array(A.edge_table("i64"), np.int64)
    gk = np.array([I32_MIN, -1, 0, 1, I32_MAX, 77], np.int32)[rng.integers(0, 6, n)]
    gv = rng.random(n) > 0.1
    x = e[rng.integers(0, len(e), n)]
    x[gk == 77] = e[rng.integers(0, 3, int((gk == 77).sum()))]
    xv = rng.random(n) > 0.15
    xv[gk == 1] = False                                                               # a group whose every x is NULL
    dg, dx = hip.DevColumn(ctx, hip.PH_I32, gk, validity=bits(gv)), hip.DevColumn(ctx, hip.PH_I64, x, validity=bits(xv))
    main = hip.Agg(ctx, [hip.PH_I32], [(hip.PH_A_COUNT, 0), (hip.PH_A_SUM, 0), (hip.PH_A_COUNT_STAR, -1)], 64)
    dist = hip.Agg(ctx, [hip.PH_I32, hip.PH_I64], [], 1024)
    main.sink([dg], [dx], None, n, mask=0b100)
    dist.sink([dg, dx], [], None, n)
    p0, v0, nd, c0 = dist.key_column(0, hip.PH_I32)
    p1, v1, nd1, c1 = dist.key_column(1, hip.PH_I64)
    main.sink([c0], [c1], None, nd, mask=0b011)
    r = main.finalize()
    want = {}
    for k, kv, xx, xok in zip(gk.tolist(), gv.tolist(), x.tolist(), xv.tolist()):
        d = want.setdefault(k if kv else None, [set(), 0])
        d[1] += 1
        if xok:
            d[0].add(xx)
    assert nd == nd1 == len({(k if kv else None, xx if xok else None) for k, kv, xx, xok in zip(gk.tolist(), gv.tolist(), x.tolist(), xv.tolist())})
    got = {}
    for i in range(r["ngroups"]):
        k = None if r["key_null"][i][0] else int(r["keys"][i][0])
        got[k] = (int(r["count"][i][0]), r["sum"][i][1] if r["count"][i][1] else None, int(r["count"][i][2]))
    assert got == {k: (len(s), sum(s) if s else None, rows) for k, (s, rows) in want.items()}
    assert None in got and got[1][0] == 0 and any(abs(v[1] or 0) > 2 ** 63 for v in got.values())
    ctx.free_many([p0, v0, p1, v1])
    main.free()
    dist.free()
    dg.free()
    dx.free()
