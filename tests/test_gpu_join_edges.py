"""Every join form against inputs that random small keys never produce (join_edges.py; its constructions are pinned on the CPU by
test_join_edges_reference.py): A. adversarial hash structure — one bucket, one head slice, one radix bin filled to its limit, one
radix bucket, one tag, fan-out beyond the staged pairs; B. keys at the edges of the int32 / int64 domains through the chained,
partitioned, node, radix, direct and flag tables; C. the table-less joins of ops_merge.hip at the same edges.
The reference of every check is join_edges.Ref: sort / searchsorted over the key values."""
import ctypes
import functools

import numpy as np
import pytest

import join_edges as J
from join_edges import I32_MAX, I32_MIN, I64_MAX, I64_MIN
from plan_amd import hip

pytestmark = pytest.mark.gpu

HT = {"i64": hip.PH_I64, "i32": hip.PH_I32, "date": hip.PH_DATE, "code8": hip.PH_CODE8}
NEVER = str(1 << 40)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


def bits(v):
    return None if v is None else np.packbits(v, bitorder="little")


def ints(*v):
    """exact int64 values (a concatenation with an empty Python list would go through float64)"""
    return np.array(v, dtype=np.int64)


def dl(ctx, p, dtype, n):
    out = ctx.download(p, dtype, n) if n else np.empty(0, dtype)
    ctx.free(p)
    return out


def force(monkeypatch, form):
    """the switches ph_join_build reads per call; the sizes of the callers decide between the atomic and the partitioned chained build"""
    for k in ("PH_JOIN_RADIX_MIN", "PH_JOIN_RADIX", "PH_JOIN_BIG_MIN", "PH_JOIN_AUTO_RANGE", "PH_JOIN_DIRECT", "PH_JOIN_RADIX_PART_MIN"):
        monkeypatch.delenv(k, raising=False)
    if form in ("atomic", "part", "chained"):
        monkeypatch.setenv("PH_JOIN_RADIX", "0")
        monkeypatch.setenv("PH_JOIN_BIG_MIN", NEVER)
        return ("chained+bloom",)
    if form == "nodes":
        monkeypatch.setenv("PH_JOIN_RADIX", "0")
        monkeypatch.setenv("PH_JOIN_BIG_MIN", "1")
        return ("nodes",)
    if form in ("radix", "radix-part"):
        monkeypatch.setenv("PH_JOIN_RADIX_MIN", "1")
        monkeypatch.setenv("PH_JOIN_BIG_MIN", NEVER)
        monkeypatch.setenv("PH_JOIN_RADIX_PART_MIN", "1" if form == "radix-part" else NEVER)
        return ("radix",)
    assert form == "auto"
    return None


def check_join(ctx, types, bcols, pcols, bvalid=None, pvalid=None, bsel=None, psel=None, kinds=None, not_kind=None, strict_clean=False,
               **build):
    """the checks common to every test: ph_join_count, the inner probe as a set of pairs (in probe-row order where the form says so),
    the mark exactly, the lookup's rows among the allowed ones with exact (misses, multi); strict_clean: ph_join_lookup_strict is clean.
    Returns (kind, reference)."""
    nk = len(types)
    bvalid, pvalid = bvalid or [None] * nk, pvalid or [None] * nk
    r = J.Ref(bcols, pcols, bvalid, pvalid, bsel, psel)
    db = [hip.DevColumn(ctx, HT[t], a, validity=bits(v)) for t, a, v in zip(types, bcols, bvalid)]
    dp = [hip.DevColumn(ctx, HT[t], a, validity=bits(v)) for t, a, v in zip(types, pcols, pvalid)]
    bs = ctx.upload(np.asarray(bsel, np.int32)) if bsel is not None else None
    ps = ctx.upload(np.asarray(psel, np.int32)) if psel is not None else None
    mb, mp = len(r.brows), len(r.prows)
    j = hip.Join(ctx, db, bs, mb, **build)
    try:
        kind = j.kind
        assert kinds is None or kind in kinds, kind
        assert kind != not_kind
        assert j.pairs_ordered() == (kind != "radix")
        flags_only = kind == "bitmap"
        want = r.pairs()
        if not flags_only:
            assert j.count() == r.build_count, hip.last_error()
            m, op, ob = j.probe_inner(dp, ps, mp, max(4 * len(want), 1 << 16))     # (room for a wrong count to be reported as a count)
            assert m == len(want)
            got = np.stack([dl(ctx, op, np.int32, m), dl(ctx, ob, np.int32, m)], 1).astype(np.int64)
            if j.pairs_ordered():      # (the selections of these tests are ascending: probe order is probe-row order)
                assert np.all(np.diff(got[:, 0]) >= 0)
            assert np.array_equal(got[np.lexsort((got[:, 1], got[:, 0]))], want)
        assert np.array_equal(dl(ctx, j.probe_mark(dp, ps, mp), np.uint8, mp), r.mark())
        if not flags_only:
            stats = ctx.upload(np.zeros(2, np.int32))
            out = dl(ctx, j.lookup(dp, ps, mp, stats), np.int32, mp)
            assert r.lookup_ok(out).all()
            assert dl(ctx, stats, np.int32, 2).tolist() == r.lookup_stats()
            if strict_clean:
                assert r.lookup_stats() == [0, 0]
                out = dl(ctx, j.lookup_strict(dp, ps, mp), np.int32, mp)
                ctx.check_deferred()
                assert r.lookup_ok(out).all()
    finally:
        j.free()
        for d in db + dp:
            d.free()
        for s in (bs, ps):
            if s is not None:
                ctx.free(s)
    return kind, r


def check_case(ctx, c, kinds, plain=True, full=True, **build):
    if plain:
        check_join(ctx, c.types, c.bcols, c.pcols, kinds=kinds, **build)
    if full:
        check_join(ctx, c.types, c.bcols, c.pcols, c.bvalid, c.pvalid, c.bsel, c.psel, kinds=kinds, **build)


def strict_part(ctx, types, bcols, pcols, present, kinds, **build):
    """the probe rows whose keys are present (each exactly once): a clean strict lookup"""
    check_join(ctx, types, bcols, [c[present] for c in pcols], kinds=kinds, strict_clean=True, **build)


# ------------------------------------------------------------------ A. hash structure

@functools.lru_cache(maxsize=None)
def bucket_input(n_build, L, packed):
    return J.one_bucket(n_build, L, packed=packed)


@pytest.mark.parametrize("L", [64, 2048])
@pytest.mark.parametrize("form,n_build,packed", [("atomic", 20_000, False), ("part", 131_072, False), ("nodes", 40_000, False), ("nodes", 40_000, True)])
def test_one_bucket_chain_of_distinct_keys(ctx, monkeypatch, form, n_build, packed, L):
    """L distinct keys in one bucket, probed by themselves and by absent keys that share bucket, Bloom word, Bloom mask and coarse bit
    with one of them: only the chain's key compare can say no, L times per probe"""
    kinds = force(monkeypatch, form)
    b, p, info = bucket_input(n_build, L, packed)
    types = ["i32", "i32"] if packed else ["i64"]
    kind, r = check_join(ctx, types, b, p, kinds=kinds)
    cls = info["probe_class"]
    assert np.array_equal(r.cnt, np.isin(cls, info["present"]).astype(np.int64))       # (so pairs, marks and lookups above said no to every look-alike)
    assert (cls == 1).sum() == L
    strict_part(ctx, types, b, p, np.isin(cls, info["present"]), kinds)


@pytest.mark.parametrize("form,slice_log,packed", [("part", J.PB_SLICE_LOG, False), ("nodes", J.BG_SLICE_LOG, False), ("nodes", J.BG_SLICE_LOG, True)])
def test_every_build_row_in_one_head_slice(ctx, monkeypatch, form, slice_log, packed):
    """the partitioned builds with ONE non-empty partition: one workgroup links all rows, every other head slice stays empty"""
    kinds = force(monkeypatch, form)
    b, p, info = J.one_slice(131_072, slice_log, packed=packed)
    types = ["i32", "i32"] if packed else ["i64"]
    kind, r = check_join(ctx, types, b, p, kinds=kinds)
    assert np.array_equal(r.cnt, (info["probe_class"] == 0).astype(np.int64))
    strict_part(ctx, types, b, p, info["probe_class"] == 0, kinds)


@pytest.mark.parametrize("half", ["low", "high"])
@pytest.mark.parametrize("form,n_build", [("atomic", 20_000), ("part", 131_072), ("nodes", 40_000), ("radix", 20_000)])
def test_keys_equal_in_one_half_share_a_bucket(ctx, monkeypatch, form, n_build, half):
    """an absent int64 key that agrees with a build key in its low (or high) 32 bits, lies in the same bucket and passes the Bloom and
    coarse bitmaps: a key compare over half of the key would call it a match"""
    kinds = force(monkeypatch, form)
    b, p, info = J.half_twins(n_build, half)
    kind, r = check_join(ctx, ["i64"], b, p, kinds=kinds)
    assert np.array_equal(r.cnt, np.isin(info["probe_class"], info["present"]).astype(np.int64)) and (info["probe_class"] == 1).sum() == len(info["A2"]) == 32


@functools.lru_cache(maxsize=None)
def radix_input(m, same_bucket, same_tag, packed):
    return J.one_radix_bin(20_000, m, same_bucket, same_tag, packed=packed)


@pytest.mark.parametrize("probe", ["radix", "radix-part"])
@pytest.mark.parametrize("m,same_bucket,same_tag,packed", [(7168, False, False, False), (7168, True, False, False), (7168, True, True, False),
                                                            (7169, False, False, False), (7169, True, True, False), (7168, True, True, True)])
def test_radix_bin_at_its_limit(ctx, monkeypatch, probe, m, same_bucket, same_tag, packed):
    """a bin of exactly 7168 rows keeps the radix form, 7169 rows give it up — which also proves that the Python hash is the device's;
    with all of them in one bucket the insertion spills over 448 consecutive buckets and every probe walks them, with one tag every
    slot on the way is a candidate. Probed straight from the columns and through the partitioned probe."""
    force(monkeypatch, probe)
    b, p, info = radix_input(m, same_bucket, same_tag, packed)
    types = ["i32", "i32"] if packed else ["i64"]
    over = m > J.RJ_BIN_LIMIT
    kind, r = check_join(ctx, types, b, p, kinds=None if over else ("radix",), not_kind="radix" if over else None)
    assert np.array_equal(r.cnt, np.isin(info["probe_class"], [0, 2]).astype(np.int64))
    if probe == "radix":
        # NULL keys and unselected rows do not count toward the bin: 7169 rows of the bin offered, one of them NULL / unselected
        hot = np.flatnonzero(J.rj_bin_of(info["build_hash"], info["log_bins"]) == np.uint64(info["bin"]))
        n = len(b[0])
        valid = np.ones(n, bool)
        sel = np.arange(n)
        if over:
            valid[hot[0]] = False
            kind, _ = check_join(ctx, types, b, p, [valid] + [None] * (len(b) - 1), None, None, None, kinds=("radix",))
            kind, _ = check_join(ctx, types, b, p, None, None, np.delete(sel, hot[1]), None, kinds=("radix",))
        else:
            valid[hot[:3]] = False
            valid[np.flatnonzero(J.rj_bin_of(info["build_hash"], info["log_bins"]) != np.uint64(info["bin"]))[:5]] = False
            check_join(ctx, types, b, p, [valid] + [None] * (len(b) - 1), None, np.delete(sel, hot[5:9]), None, kinds=("radix",))


@pytest.mark.parametrize("probe", ["radix", "radix-part"])
@pytest.mark.parametrize("dup", [4, 16])
def test_radix_fan_out_beyond_the_staged_pairs(ctx, monkeypatch, probe, dup):
    """dup pairs per probe row: every chunk of 4096 probe rows emits more pairs than the 8192 it stages in LDS (the rest reserve their
    places one by one), and the dup equal keys fill one bucket with one tag; a capacity below the count reports the true count"""
    force(monkeypatch, probe)
    b, p, info = J.fan_out(65_536, dup)
    kind, r = check_join(ctx, ["i64"], b, p, kinds=("radix",))
    assert int(r.cnt.sum()) == info["pairs"] and info["pairs"] > 2 * J.RJ_STAGE
    db, dp = hip.DevColumn(ctx, hip.PH_I64, b[0]), hip.DevColumn(ctx, hip.PH_I64, p[0])
    j = hip.Join(ctx, [db], None, len(b[0]))
    assert j.kind == "radix"
    op, ob, m = ctx.alloc(1000 * 4), ctx.alloc(1000 * 4), hip.i64()
    rc = hip.lib().ph_join_probe_inner(j.h, hip._cols([dp]), None, hip.i64(len(p[0])), op, ob, hip.i64(1000), ctypes.byref(m))
    assert rc == hip.PH_ECAPACITY and m.value == info["pairs"]
    head = set(zip(dl(ctx, op, np.int32, 1000).tolist(), dl(ctx, ob, np.int32, 1000).tolist()))      # nothing lost but the tail
    assert len(head) == 1000 and head <= set(map(tuple, r.pairs().tolist()))
    j.free()
    db.free(); dp.free()


# ------------------------------------------------------------------ B. key-domain edges

@functools.lru_cache(maxsize=None)
def single_case(typ, big):
    return J.single_key_case(typ, *((240_000, 60_000) if big else (40_000, 30_000)))


@pytest.mark.parametrize("form", ["atomic", "part", "nodes", "radix", "radix-part"])
@pytest.mark.parametrize("typ", ["i64", "i32", "date"])
def test_single_key_domain_edges(ctx, monkeypatch, typ, form):
    """negative keys, keys beyond 2^32, the extremes of the type, int64 keys that differ in one half only — with filler, duplicates,
    NULLs and selections on both sides — through every hash-table form"""
    kinds = force(monkeypatch, form)
    c = single_case(typ, form == "part")
    assert (form == "part") == (len(c.bsel) >= 131_072) and len(c.bsel) > 16_384
    check_case(ctx, c, kinds)
    r = J.Ref(c.bcols, c.pcols)
    for v in c.info["absent"]:
        assert r.cnt[c.pcols[0].astype(np.int64) == v].sum() == 0


def test_code8_keys_0_and_255(ctx, monkeypatch):
    kinds = force(monkeypatch, "chained")
    check_case(ctx, J.single_key_case("code8"), kinds)


@functools.lru_cache(maxsize=None)
def pair_case(big):
    return J.i32_pair_case(*((240_000, 60_000) if big else (40_000, 30_000)))


@pytest.mark.parametrize("form", ["atomic", "part", "nodes", "radix", "radix-part"])
def test_int32_pair_domain_edges(ctx, monkeypatch, form):
    """two int32 keys over the int32 edge values in both columns — (0,-1), (5,-1), (-1,-1), (-1,0), (0,0) are distinct build keys whose
    packed forms differ only because the second column is masked to 32 bits; the chained fast kernels (no NULLs), the generic ones
    (NULLs), the node table and the radix form"""
    kinds = force(monkeypatch, form)
    c = pair_case(form == "part")
    check_case(ctx, c, kinds)
    r = J.Ref(c.bcols, c.pcols)
    for a, b in J.I32_PAIRS_REQUIRED:
        at = (c.pcols[0] == a) & (c.pcols[1] == b)
        nb = int(((c.bcols[0] == a) & (c.bcols[1] == b)).sum())
        assert at.any() and nb >= 3 and (r.cnt[at] == nb).all()


@pytest.mark.parametrize("types", [("i32", "i64"), ("i64", "i32"), ("i32", "date", "i64"), ("i64", "code8", "i32", "date")], ids="-".join)
def test_generic_chained_mixed_widths_and_many_keys(ctx, monkeypatch, types):
    kinds = force(monkeypatch, "chained")
    check_case(ctx, J.multi_key_case(list(types)), kinds)


@pytest.mark.parametrize("dups", [False, True], ids=["unique", "dups"])
@pytest.mark.parametrize("rng", J.dense_ranges(), ids=[d[0] for d in J.dense_ranges()])
def test_direct_table_at_the_domain_edges(ctx, monkeypatch, rng, dups):
    """the direct table over a dense range that ends at an edge of the type: exact range and strict supersets (for the int32 column at
    I32_MIN one whose key_lo lies below the int32 domain), build and probe selections, NULL probe keys; probes at lo, hi, lo - 1,
    hi + 1 and the opposite end of the domain, where key - lo wraps"""
    force(monkeypatch, "auto")
    name, typ, lo, hi = rng
    c = J.dense_case(name, typ, lo, hi, dups)
    dlo, dhi = (I64_MIN, I64_MAX) if typ == "i64" else (I32_MIN, I32_MAX)
    supersets = [(max(dlo, lo - 1000), min(dhi, hi + 1000)), (max(dlo, lo - 1), hi), (lo, min(dhi, hi + 1))]
    if name == "i32-at-min":
        supersets.append((I32_MIN - 1000, hi + 7))
    if name == "i32-at-max":
        supersets.append((lo - 7, I32_MAX + 1000))
    for kr in [(lo, hi)] + supersets:
        check_case(ctx, c, ("direct",), key_range=kr)
    if not dups:                           # unique build keys, every probe key present: a clean strict lookup
        strict_part(ctx, c.types, c.bcols, c.pcols, np.isin(c.pcols[0], c.bcols[0]), ("direct",), key_range=(lo, hi))
    if not dups and typ == "i64":          # declared sorted and unique: the gated sorted fill where lo + range does not wrap, the general fill at I64_MAX
        check_case(ctx, c, ("direct",), full=False, key_range=(lo, hi), sorted_unique=True)
        ctx.check_deferred()


@pytest.mark.parametrize("rng", J.dense_ranges(), ids=[d[0] for d in J.dense_ranges()])
def test_direct_table_fused_filters_and_range_errors(ctx, monkeypatch, rng):
    """ph_join_probe_inner_where / ph_join_probe_mark_where with one date filter over the edge ranges, and the documented error for a
    build key outside the declared range at both ends of it"""
    force(monkeypatch, "auto")
    name, typ, lo, hi = rng
    c = J.dense_case(name, typ, lo, hi, True)
    npr = c.np_
    w = np.random.default_rng(5).integers(8000, 10_000, npr).astype(np.int32)
    keep = w < 9000
    db, dp, dw = hip.DevColumn(ctx, HT[typ], c.bcols[0]), hip.DevColumn(ctx, HT[typ], c.pcols[0]), hip.DevColumn(ctx, hip.PH_DATE, w)
    j = hip.Join(ctx, [db], None, c.nb, key_range=(lo, hi))
    assert j.kind == "direct"
    r = J.Ref(c.bcols, c.pcols, None, None, None, np.flatnonzero(keep))
    want = r.pairs()
    got = j.probe_inner_where([dp], dw, hip.PH_LT, hip.const(hip.PH_DATE, i=9000), None, npr, len(want) + 16)
    assert got is not None and got[0] == len(want)
    pairs = np.stack([dl(ctx, got[1], np.int32, got[0]), dl(ctx, got[2], np.int32, got[0])], 1).astype(np.int64)
    assert np.all(np.diff(pairs[:, 0]) >= 0) and np.array_equal(pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))], want)
    f = j.probe_mark_where([dp], dw, hip.PH_LT, hip.const(hip.PH_DATE, i=9000), npr)
    assert f is not None
    mark = np.zeros(npr, np.uint8)
    mark[np.flatnonzero(keep)] = r.mark()
    assert np.array_equal(dl(ctx, f, np.uint8, npr), mark)
    j.free()
    for kr in ((lo + 1, hi), (lo, hi - 1)):
        jb = hip.Join(ctx, [db], None, c.nb, key_range=kr)
        assert jb.kind == "direct" and jb.count() == -1 and "outside the stated range" in hip.last_error()
        jb.free()
    for d in (db, dp, dw):
        d.free()


@pytest.mark.parametrize("rng", [J.dense_ranges()[0], J.dense_ranges()[4]], ids=["i64-at-min", "i32-at-max"])
def test_flag_table_at_the_domain_edges(ctx, monkeypatch, rng):
    """PH_JOIN_EXISTS_ONLY over a big build side whose range ends at an edge of the type: one byte per key value, marks exact"""
    force(monkeypatch, "auto")
    name, typ, lo, hi = rng
    c = J.dense_case(name, typ, lo, hi, False)
    g = np.random.default_rng(6)
    b = c.bcols[0][g.integers(0, c.nb, 300_000)]
    b[:2] = (lo, hi)
    bv = g.random(len(b)) > 0.05
    bsel = np.flatnonzero(g.random(len(b)) < 0.95).astype(np.int32)
    assert len(bsel) >= 262_144
    check_join(ctx, [typ], [b], c.pcols, [bv], c.pvalid, bsel, c.psel, kinds=("bitmap",), key_range=(lo, hi), exists_only=True)
    check_join(ctx, [typ], [b], c.pcols, kinds=("bitmap",), key_range=(lo, hi), exists_only=True)


def test_auto_range_when_the_span_does_not_fit_int64(ctx, monkeypatch):
    """2^20 build rows without a stated range: the library reads min / max off the column. With I64_MIN and I64_MAX among the keys
    key_hi - key_lo is 2^64 - 1, which must not pass for a dense range"""
    force(monkeypatch, "auto")
    g = np.random.default_rng(7)
    n = 1 << 20
    b = g.integers(I64_MIN, I64_MAX, n, endpoint=True, dtype=np.int64)
    b[g.choice(n, 4, replace=False)] = (I64_MIN, I64_MAX, I64_MIN, I64_MAX)
    p = np.concatenate([b[g.integers(0, n, 50_000)], g.integers(I64_MIN, I64_MAX, 50_000, endpoint=True, dtype=np.int64),
                        np.array([I64_MIN, I64_MAX, I64_MIN + 1, I64_MAX - 1, 0, -1], np.int64)])
    kind, r = check_join(ctx, ["i64"], [b], [p], not_kind="direct")
    assert kind != "bitmap" and r.cnt[-6:].tolist() == [2, 2, 0, 0, 0, 0]


def test_auto_range_dense_at_int64_min(ctx, monkeypatch):
    force(monkeypatch, "auto")
    g = np.random.default_rng(8)
    n = 1 << 20
    off = np.sort(g.choice((1 << 21) + 1, n, replace=False))
    off[0], off[-1] = 0, 1 << 21
    b = g.permutation(np.array(I64_MIN, np.int64) + off)
    p = np.concatenate([b[g.integers(0, n, 50_000)], np.array(I64_MIN, np.int64) + g.integers(0, 1 << 22, 50_000),
                        np.array([I64_MIN, I64_MIN + (1 << 21), I64_MIN + (1 << 21) + 1, I64_MAX, 0, -1], np.int64)])
    kind, r = check_join(ctx, ["i64"], [b], [p], kinds=("direct",))
    assert r.cnt[-6:].tolist() == [1, 1, 0, 0, 0, 0]


# ------------------------------------------------------------------ C. the table-less joins

@pytest.mark.parametrize("typ", ["i64", "i32"])
def test_sorted_pairs_runs_at_the_extremes(ctx, typ):
    """ph_join_sorted_pairs: runs of 1, 16, 17 and 40 rows at the lowest and the highest value of the type (a run of more than 16 rows is
    finished with a second search, which must not form key + 1 at the maximum); pairs in probe order, a run's rows ascending"""
    p = J.sorted_probe_column(typ)
    keep = np.random.default_rng(9).random(len(p)) < 0.5
    keep[[int(np.argmin(p)), int(np.argmax(p))]] = True                      # a row of each extreme stays selected
    sel = np.flatnonzero(keep).astype(np.int32)
    dp = hip.DevColumn(ctx, HT[typ], p)
    ds = ctx.upload(sel)
    for run, b in J.sorted_runs_column(typ):
        db = hip.DevColumn(ctx, HT[typ], b)
        for s, dsel in ((None, None), (sel, ds)):
            rows = np.arange(len(p)) if s is None else s
            r = J.Ref([b], [p], None, None, None, s)
            want = [(int(rows[i]), int(x)) for i in range(len(rows)) for x in np.flatnonzero(b == p[rows[i]])]    # probe order, rows ascending
            assert sorted(want) == [tuple(x) for x in r.pairs().tolist()] and int(r.cnt.max()) == run
            op, ob, m = hip.join_sorted_pairs(ctx, db, len(b), dp, dsel, len(rows), len(want) + 8)
            assert m == len(want)
            got = list(zip(dl(ctx, op, np.int32, m).tolist(), dl(ctx, ob, np.int32, m).tolist()))
            assert got == want, (typ, run)
        db.free()
    dp.free()
    ctx.free(ds)


@pytest.mark.parametrize("typ", ["i64", "i32"])
def test_merge_lookup_from_the_lowest_to_the_highest_key(ctx, typ):
    """ph_merge_lookup over unique ascending build keys from the type's minimum to its maximum: dense probes (the LDS streaming
    branch; the last build key, the type's maximum, lies next to the chunk's INT64_MAX padding) and sparse probes (the column search)"""
    lo, hi = (I64_MIN, I64_MAX) if typ == "i64" else (I32_MIN, I32_MAX)
    dt = np.int64 if typ == "i64" else np.int32
    g = np.random.default_rng(10)
    # dense: 20 000 keys in two clusters at the two ends; sparse: 600 000 keys over the whole domain (slices longer than 64 chunks)
    ends = np.concatenate([np.arange(lo, lo + 30_000, 3, dtype=np.int64), np.arange(hi - 29_997, hi + 1, 3, dtype=np.int64)])
    wide = np.unique(np.concatenate([g.integers(lo, hi, 600_000, endpoint=True, dtype=np.int64), [lo, hi]]))
    for name, b in (("dense", ends), ("sparse", wide)):
        assert b[0] == lo and b[-1] == hi and (b[1:] > b[:-1]).all()
        k = 6000 if name == "dense" else 1000
        src = b[g.integers(0, len(b), k)]
        near = np.concatenate([src, src[src < hi][: k // 2] + 1, [lo, lo + 1, lo + 2, hi - 2, hi - 1, hi]])      # present keys and absent neighbours
        p = np.sort(np.concatenate([near, b[-2100:], b[:2100]])) if name == "dense" else np.sort(near)
        db, dp = hip.DevColumn(ctx, HT[typ], b.astype(dt)), hip.DevColumn(ctx, HT[typ], p.astype(dt))
        at = np.searchsorted(b, p)
        want = np.where((at < len(b)) & (b[np.minimum(at, len(b) - 1)] == p), at, -1)
        assert (want >= 0).sum() >= 1000 and (want < 0).sum() > 100 and want[-1] == len(b) - 1 and want[0] == 0
        got = dl(ctx, hip.merge_lookup(ctx, db, len(b), dp, None, len(p)), np.int32, len(p))
        ctx.check_deferred()
        assert np.array_equal(got, want), name
        hit = np.flatnonzero(want >= 0).astype(np.int32)
        ds = ctx.upload(hit)
        got = dl(ctx, hip.merge_lookup(ctx, db, len(b), dp, ds, len(hit), strict=True), np.int32, len(hit))
        ctx.check_deferred()
        assert np.array_equal(got, want[hit])
        ctx.free(ds)
        db.free(); dp.free()


@pytest.mark.parametrize("run_len", [4, 3])
@pytest.mark.parametrize("typ,typ2", [("i64", "i32"), ("i32", "i32"), ("i64", "i64"), ("i32", "i64")])
def test_run_lookup_at_the_domain_edges(ctx, typ, typ2, run_len):
    """ph_join_run_lookup with the first key's runs starting at the type's minimum and ending at its maximum; probes from the opposite
    extreme, where k - key1_min wraps; second keys at the extremes of their type"""
    lo, hi = (I64_MIN, I64_MAX) if typ == "i64" else (I32_MIN, I32_MAX)
    lo2, hi2 = (I64_MIN, I64_MAX) if typ2 == "i64" else (I32_MIN, I32_MAX)
    nruns = 1001
    g = np.random.default_rng(11)
    second = np.array([lo2, -1, hi2, 0, 7][:run_len] if run_len == 3 else [lo2, -1, 0, hi2], dtype=np.int64)
    b2 = np.tile(second, nruns)
    dt, dt2 = (np.int64 if typ == "i64" else np.int32), (np.int64 if typ2 == "i64" else np.int32)
    for kmin in (lo, hi - nruns + 1):
        k1 = np.concatenate([np.array(kmin, np.int64) + g.integers(0, nruns, 4000), ints(lo, hi, kmin, kmin + nruns - 1, 0, -1, 1),
                             ints(kmin - 1) if kmin > lo else ints(), ints(kmin + nruns) if kmin + nruns - 1 < hi else ints()])
        k2 = np.concatenate([second, ints(lo2 + 1, hi2 - 1, 1)])[g.integers(0, run_len + 3, len(k1))]
        pv = g.random(len(k1)) > 0.1
        inr = np.array([kmin <= int(k) < kmin + nruns for k in k1.tolist()])
        slot = np.array([{int(v): i for i, v in enumerate(second)}.get(int(x), -1) for x in k2.tolist()])
        want = np.where(inr & (slot >= 0) & pv, np.array([(int(k) - kmin) * run_len for k in k1.tolist()], dtype=object) + slot, -1).astype(np.int64)
        assert (want >= 0).sum() > 500 and (~inr).sum() >= 3
        db = hip.DevColumn(ctx, HT[typ2], b2.astype(dt2))
        d1, d2 = hip.DevColumn(ctx, HT[typ], k1.astype(dt), validity=bits(pv)), hip.DevColumn(ctx, HT[typ2], k2.astype(dt2))
        got = dl(ctx, hip.join_run_lookup(ctx, db, len(b2), kmin, run_len, [d1, d2], None, len(k1)), np.int32, len(k1))
        assert np.array_equal(got, want), (kmin, run_len)
        hit = np.flatnonzero(want >= 0).astype(np.int32)
        ds = ctx.upload(hit)
        got = dl(ctx, hip.join_run_lookup(ctx, db, len(b2), kmin, run_len, [d1, d2], ds, len(hit), strict=True), np.int32, len(hit))
        ctx.check_deferred()
        assert np.array_equal(got, want[hit])
        ctx.free(ds)
        for d in (db, d1, d2):
            d.free()


@pytest.mark.parametrize("typ", ["i64", "i32"])
def test_count_by_key_at_the_domain_edges(ctx, typ):
    """ph_count_by_key with the counted range starting at the type's minimum and ending at its maximum; child keys from the opposite
    extreme (key - key_min wraps), NULL keys and selections on both sides"""
    lo, hi = (I64_MIN, I64_MAX) if typ == "i64" else (I32_MIN, I32_MAX)
    dt = np.int64 if typ == "i64" else np.int32
    g = np.random.default_rng(12)
    R = 3001
    for kmin in (lo, hi - R + 1):
        child = np.concatenate([np.array(kmin, np.int64) + g.integers(0, R, 20_000), ints(lo, hi, lo, hi, 0, -1, kmin, kmin + R - 1),
                                ints(kmin - 1) if kmin > lo else ints(), ints(kmin + R) if kmin + R - 1 < hi else ints()])
        child = g.permutation(child)
        parent = np.concatenate([np.array(kmin, np.int64) + np.arange(R), ints(lo, hi, 0, -1)])
        cv, pv = g.random(len(child)) > 0.1, g.random(len(parent)) > 0.1
        csel = np.flatnonzero(g.random(len(child)) < 0.7).astype(np.int32)
        psel = np.flatnonzero(g.random(len(parent)) < 0.8).astype(np.int32)
        dc, dp = hip.DevColumn(ctx, HT[typ], child.astype(dt), validity=bits(cv)), hip.DevColumn(ctx, HT[typ], parent.astype(dt), validity=bits(pv))
        for cs, ps in ((None, None), (csel, psel)):
            want = J.ref_counts(child, cv, cs, kmin, R, parent, pv, ps)
            assert want.sum() > 5000 and (want == 0).any()
            dcs, dps = (None if cs is None else ctx.upload(cs)), (None if ps is None else ctx.upload(ps))
            out, val = hip.count_by_key(ctx, dc, dcs, len(child) if cs is None else len(cs), kmin, R, dp, dps, len(want))
            assert np.array_equal(dl(ctx, out, np.int64, len(want)), want)
            vb = np.unpackbits(dl(ctx, val, np.uint8, (len(want) + 63) // 64 * 8), bitorder="little")[: len(want)]
            assert np.array_equal(vb.astype(bool), want > 0)
            for s in (dcs, dps):
                if s is not None:
                    ctx.free(s)
        dc.free(); dp.free()
