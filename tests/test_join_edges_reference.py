"""The constructed inputs and the plain references of the join edge tests (join_edges.py), checked without a device: the hash
inverse, the hash bits every builder claims, the values every edge table must hold, and the references against the oracle's join
and a double loop. A GPU test over inputs that lost their structure would still pass; this file is what would fail."""
import numpy as np
import pytest

import join_edges as J
import oracle_lib as O
from join_edges import I32_MAX, I32_MIN, I64_MAX, I64_MIN

OT = {"i64": O.OT_INT64, "i32": O.OT_INT32, "date": O.OT_DATE, "code8": O.OT_CODE8}
CODES = O.cdict([f"code{i:03d}" for i in range(256)])     # the oracle compares CODE8 keys through their dictionary strings


def bits(v):
    return None if v is None else np.packbits(v, bitorder="little")


def test_hash_inverse_round_trips():
    rng = np.random.default_rng(0)
    h = np.concatenate([rng.integers(0, 2 ** 64, 100_000, dtype=np.uint64),
                        np.array([0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1, J.SEED, 2 ** 32 - 1, 2 ** 32], dtype=np.uint64)])
    assert np.array_equal(J.mix64(J.inv_mix64(h)), h) and np.array_equal(J.inv_mix64(J.mix64(h)), h)
    for x in h[-8:].tolist() + h[:50].tolist():
        assert J.mix64_int(J.inv_mix64_int(x)) == x and J.inv_mix64_int(J.mix64_int(x)) == x
        assert int(J.mix64(np.array([x], dtype=np.uint64))[0]) == J.mix64_int(x)
        assert int(J.inv_mix64(np.array([x], dtype=np.uint64))[0]) == J.inv_mix64_int(x)
    assert (J.MUL1 * J.INV1) % 2 ** 64 == 1 and (J.MUL2 * J.INV2) % 2 ** 64 == 1
    assert J.mix64_int(0) == 0 and J.mix64_int(J.SEED) == 0xE220A8397B1DCDAF     # splitmix64's first output for seed 0
    k = J.keys_with_hash(h)
    assert np.array_equal(J.key_hash(k), h) and len(np.unique(k)) == len(np.unique(h))
    assert J.key_hash_int(-1) == int(J.key_hash(np.array([-1], np.int32))[0]) == int(J.key_hash(np.array([-1], np.int64))[0])   # sign-extended
    assert int(J.key_hash(np.array([255], np.uint8))[0]) == J.key_hash_int(255)                                                  # zero-extended
    a, b = J.keys_with_hash(h, packed=True)
    assert a.dtype == b.dtype == np.int32 and np.array_equal(J.pack_hash(a, b), h)
    assert int(J.pack(np.array([5], np.int32), np.array([-1], np.int32))[0]) == (5 << 32) | 0xFFFFFFFF
    assert int(J.hash2(np.array([3], np.int32), np.array([-4], np.int32))[0]) == J.mix64_int(J.mix64_int(J.SEED ^ 3) ^ (-4 & J.M64))


def test_layout_constants():
    assert [J.chained_cap(n) for n in (0, 1, 512, 513, 131_072, 131_073)] == [1024, 1024, 1024, 2048, 262_144, 524_288]
    assert J.RJ_BIN_LIMIT == 7168 and J.RJ_BUCKETS == 512 and J.RJ_STAGE == 8192
    assert [J.rj_log_bins(n) for n in (1, 64 * 4608, 64 * 4608 + 1, 1 << 20)] == [6, 6, 7, 8]
    # bits 0..59 cover the bucket, the Bloom word and mask and the coarse bit of every table that has a bitmap (<= 4 M rows)
    assert J.chained_cap(4 << 20).bit_length() - 1 <= J.LOOKALIKE_SHIFT
    assert J.BLOOM_WORD_SHIFT + (J.bloom_bits_of(4 << 20) // 32).bit_length() - 1 <= J.LOOKALIKE_SHIFT
    assert J.COARSE_SHIFT + J.COARSE_BITS <= J.LOOKALIKE_SHIFT and J.BLOOM_MASK_SHIFT + 10 <= J.BLOOM_WORD_SHIFT


def hashes(cols, packed):
    return J.pack_hash(*cols) if packed else J.key_hash(cols[0])


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("n_build,L", [(3000, 64), (20_000, 2048), (131_072, 2048)])
def test_one_bucket_has_its_structure(n_build, L, packed):
    b, p, info = J.one_bucket(n_build, L, packed=packed)
    hb, hp, cls = hashes(b, packed), hashes(p, packed), info["probe_class"]
    assert np.array_equal(hb, info["build_hash"]) and np.array_equal(hp, info["probe_hash"])
    assert len(hb) == n_build and len(np.unique(hb)) == n_build                    # distinct hashes = distinct keys
    cap = info["cap"]
    assert cap == J.chained_cap(n_build)
    hot = hb[J.bucket_of(hb, cap) == info["bucket"]]
    assert len(hot) == L
    assert set(hp[cls == 0].tolist()) == set(hot.tolist())
    look = hp[cls == 1]
    assert len(look) == L and not np.isin(look, hb).any()
    low = np.uint64((1 << 60) - 1)
    assert np.array_equal(np.sort(look & low), np.sort(hot & low))                 # one per present key, differing above bit 59 only
    partner = hot[np.argsort(hot & low)][np.searchsorted(np.sort(hot & low), look & low)]
    for f in (lambda h: J.bucket_of(h, cap), lambda h: J.bloom_word_of(h, n_build), J.bloom_mask_of, J.coarse_of,
              lambda h: J.bucket_of(h, cap) >> np.uint64(J.PB_SLICE_LOG)):
        assert np.array_equal(f(look), f(partner))
    empty = hp[cls == 2]
    assert len(empty) and not np.isin(J.bucket_of(empty, cap), J.bucket_of(hb, cap)).any()
    assert np.isin(hp[cls == 3], hb).all() and (J.bucket_of(hp[cls == 3], cap) != info["bucket"]).all()


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("slice_log", [J.PB_SLICE_LOG, J.BG_SLICE_LOG])
def test_one_slice_has_its_structure(slice_log, packed):
    n = 131_072
    b, p, info = J.one_slice(n, slice_log, packed=packed)
    hb, hp, cls = hashes(b, packed), hashes(p, packed), info["probe_class"]
    cap = info["cap"]
    assert cap >> slice_log >= 2 and len(np.unique(hb)) == n
    sl = lambda h: J.bucket_of(h, cap) >> np.uint64(slice_log)
    assert (sl(hb) == info["slice"]).all()
    assert len(np.unique(J.bucket_of(hb, cap))) > (1 << slice_log) // 2             # spread inside the slice
    assert np.isin(hp[cls == 0], hb).all()
    assert (sl(hp[cls == 1]) == info["slice"]).all() and not np.isin(hp[cls == 1], hb).any() and (cls == 1).sum() > 1000
    assert (sl(hp[cls == 2]) != info["slice"]).all() and not np.isin(hp[cls == 2], hb).any()


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("m,same_bucket,same_tag", [(7168, False, False), (7168, True, False), (7168, True, True), (7169, False, False), (7169, True, True)])
def test_one_radix_bin_has_its_structure(m, same_bucket, same_tag, packed):
    n = 20_000
    b, p, info = J.one_radix_bin(n, m, same_bucket, same_tag, packed=packed)
    hb, hp, cls = hashes(b, packed), hashes(p, packed), info["probe_class"]
    lb = info["log_bins"]
    assert lb == 6 and len(np.unique(hb)) == n
    inbin = J.rj_bin_of(hb, lb) == info["bin"]
    assert inbin.sum() == m                                                        # exactly m keys, and no other key, in the bin
    assert np.bincount(J.rj_bin_of(hb, lb).astype(np.int64), minlength=64).max() == m
    hot = hb[inbin]
    if same_bucket:
        assert (J.rj_bucket_of(hot) == info["bucket"]).all()
    else:
        assert len(np.unique(J.rj_bucket_of(hot))) == 512
    if same_tag:
        assert (J.rj_tag_of(hot) == info["tag"]).all()
    assert set(hp[cls == 0].tolist()) == set(hot.tolist())
    absent = hp[cls == 1]
    assert len(absent) > 500 and not np.isin(absent, hb).any() and (J.rj_bin_of(absent, lb) == info["bin"]).all()
    if same_bucket:
        assert (J.rj_bucket_of(absent) == info["bucket"]).all()
    if same_tag:
        assert (J.rj_tag_of(absent) == info["tag"]).all()
    assert np.isin(hp[cls == 2], hb).all()
    if not packed:   # the keys themselves: distinct, and of both signs
        assert len(np.unique(b[0])) == n and 0.4 < (b[0] < 0).mean() < 0.6


@pytest.mark.parametrize("half", ["low", "high"])
@pytest.mark.parametrize("n_build", [20_000, 131_072])
def test_half_twins_have_their_structure(n_build, half):
    b, p, info = J.half_twins(n_build, half)
    A, A2, cap = info["A"], info["A2"], info["cap"]
    hb, hA, hA2 = J.key_hash(b[0]), J.key_hash(A), J.key_hash(A2)
    assert len(A) == 32 and np.isin(A, b[0]).all() and not np.isin(A2, b[0]).any() and len(np.unique(b[0])) == n_build
    x = A.view(np.uint64) ^ A2.view(np.uint64)
    assert (x != 0).all() and ((x & np.uint64(0xFFFFFFFF)) == 0).all() if half == "low" else ((x >> np.uint64(32)) == 0).all()
    assert np.array_equal(J.bucket_of(hA, cap), J.bucket_of(hA2, cap))
    # the bitmaps let every A' through: its Bloom word holds its two mask bits and its coarse bit is set (by the helper key)
    words = np.zeros(J.bloom_bits_of(n_build) // 32, np.uint64)
    np.bitwise_or.at(words, J.bloom_word_of(hb, n_build).astype(np.int64), J.bloom_mask_of(hb))
    m = J.bloom_mask_of(hA2)
    assert ((words[J.bloom_word_of(hA2, n_build).astype(np.int64)] & m) == m).all()
    assert np.isin(J.coarse_of(hA2), J.coarse_of(hb)).all()
    hh = J.key_hash(info["helper"])
    assert (J.bucket_of(hh, cap) != J.bucket_of(hA2, cap)).all()
    assert np.array_equal(J.bucket_of(hh, cap) >> np.uint64(J.PB_SLICE_LOG), J.bucket_of(hA2, cap) >> np.uint64(J.PB_SLICE_LOG))   # same head slice: same slice of the partitioned bitmap
    r = J.Ref(b, p)
    assert np.array_equal(r.cnt, np.isin(info["probe_class"], info["present"]).astype(np.int64))


def test_fan_out_has_its_structure():
    for dup in (4, 16):
        b, p, info = J.fan_out(65_536, dup)
        u, c = np.unique(b[0], return_counts=True)
        assert (c == dup).all() and np.isin(p[0], u).all() and info["pairs"] == len(p[0]) * dup
        assert J.RJ_CH * dup > J.RJ_STAGE and len(p[0]) >= 2 * J.RJ_CH
        assert np.bincount(J.rj_bin_of(J.key_hash(b[0]), 6).astype(np.int64)).max() <= J.RJ_BIN_LIMIT


def edge_cases():
    return ([J.single_key_case(t) for t in ("i64", "i32", "date", "code8")] + [J.i32_pair_case()] +
            [J.multi_key_case(ts) for ts in (["i32", "i64"], ["i64", "i32"], ["i32", "date", "i64"], ["i64", "code8", "i32", "date"])] +
            [J.dense_case(*d, dups) for d in J.dense_ranges() for dups in (False, True)])


def test_edge_tables_hold_every_listed_value_on_both_sides():
    for typ, want in (("i64", J.I64_EDGES), ("i32", J.I32_EDGES), ("date", J.I32_EDGES), ("code8", J.CODE8_EDGES)):
        c = J.single_key_case(typ)
        for side, col, valid, sel in (("build", c.bcols[0], c.bvalid[0], c.bsel), ("probe", c.pcols[0], c.pvalid[0], c.psel)):
            for v in want:
                at = np.flatnonzero(col.astype(np.int64) == v)
                assert len(at) >= 2, (typ, side, v)                                         # (placed three times, filler may overwrite none)
                assert (valid[at] & np.isin(at, sel)).any(), (typ, side, v, "never valid and selected")
        assert (~c.bvalid[0]).any() and (~c.pvalid[0]).any() and len(c.bsel) < c.nb and len(c.psel) < c.np_
    c = J.single_key_case("i64")
    for a, b in J.I64_HIGH_ONLY:
        assert (a ^ b) & 0xFFFFFFFF == 0 and a != b and a in c.bcols[0] and b in c.pcols[0] and b not in c.bcols[0]
    for a, b in J.I64_LOW_ONLY:
        assert (a >> 32) == (b >> 32) and a != b and a in c.bcols[0] and b in c.pcols[0] and b not in c.bcols[0]
    c = J.i32_pair_case()
    bset, pset = set(zip(c.bcols[0].tolist(), c.bcols[1].tolist())), set(zip(c.pcols[0].tolist(), c.pcols[1].tolist()))
    for pr in [(a, b) for a in J.I32_EDGES for b in J.I32_EDGES] + J.I32_PAIRS_REQUIRED:
        assert pr in bset and pr in pset
    assert all(a in pset and a not in bset for a in c.info["absent"])
    assert len({int(J.pack(np.array([a], np.int32), np.array([b], np.int32))[0]) for a, b in J.I32_PAIRS_REQUIRED}) == 5
    for name, typ, lo, hi in J.dense_ranges():
        assert (hi - lo + 1) % 64 != 0
        for dups in (False, True):
            c = J.dense_case(name, typ, lo, hi, dups)
            b, p = c.bcols[0].astype(np.int64), c.pcols[0].astype(np.int64)
            assert b.min() == lo and b.max() == hi and (len(np.unique(b)) < len(b)) == dups
            if not dups:
                assert (np.diff(b) > 0).all()                                               # sorted and unique: the sorted-fill claim holds
            dlo, dhi = (I64_MIN, I64_MAX) if typ == "i64" else (I32_MIN, I32_MAX)
            for v in [lo, hi, dlo, dhi] + ([lo - 1] if lo > dlo else []) + ([hi + 1] if hi < dhi else []):
                at = np.flatnonzero(p == v)
                assert len(at) and (c.pvalid[0][at] & np.isin(at, c.psel)).any(), (c.name, v)
            assert (~c.pvalid[0]).any()


def oracle_join(c, with_nulls_and_sels):
    bv, pv = (c.bvalid, c.pvalid) if with_nulls_and_sels else ([None] * len(c.bcols), [None] * len(c.pcols))
    bs, ps = (c.bsel, c.psel) if with_nulls_and_sels else (None, None)
    ob = [O.col(OT[t], a, validity=bits(v), dictionary=CODES if t == "code8" else None) for t, a, v in zip(c.types, c.bcols, bv)]
    op = [O.col(OT[t], a, validity=bits(v), dictionary=CODES if t == "code8" else None) for t, a, v in zip(c.types, c.pcols, pv)]
    mb, mp = (len(bs) if bs is not None else c.nb), (len(ps) if ps is not None else c.np_)
    oj = O.Join(ob, None if bs is None else bs.astype(np.int64), mb)
    cap = 1 << 21
    m, wp, wb = oj.probe_inner(op, None if ps is None else ps.astype(np.int64), mp, cap)
    assert m <= cap
    want = np.stack([wp, wb], 1)
    mark = oj.probe_mark(op, None if ps is None else ps.astype(np.int64), mp)
    return oj.count(), want[np.lexsort((want[:, 1], want[:, 0]))], mark, (bv, pv, bs, ps)


def test_references_agree_with_the_oracle_on_every_edge_table():
    for c in edge_cases():
        for full in (False, True):
            cnt, pairs, mark, (bv, pv, bs, ps) = oracle_join(c, full)
            r = J.Ref(c.bcols, c.pcols, bv, pv, bs, ps)
            assert r.build_count == cnt, c.name
            assert np.array_equal(r.pairs(), pairs), c.name
            assert np.array_equal(J.ref_pairs(c.bcols, c.pcols, bv, pv, bs, ps), pairs)
            assert np.array_equal(J.ref_mark(c.bcols, c.pcols, bv, pv, bs, ps), mark), c.name
            assert len(pairs) > 100


def test_references_agree_with_the_oracle_on_every_builder():
    built = [J.one_bucket(3000, 64), J.one_bucket(3000, 64, packed=True), J.one_slice(32_768, J.PB_SLICE_LOG, n_probe=512),
             J.one_slice(32_768, J.BG_SLICE_LOG, packed=True, n_probe=512), J.one_radix_bin(9000, 7168, True, True),
             J.one_radix_bin(9000, 7168, packed=True), J.half_twins(3000, "low", 8), J.half_twins(3000, "high", 8),
             J.fan_out(4096, 4, n_probe=512), J.fan_out(4096, 16, n_probe=512)]
    for b, p, info in built:
        t = "i32" if len(b) == 2 else "i64"
        c = J.Case("built", [t] * len(b), b, p)
        cnt, pairs, mark, _ = oracle_join(c, False)
        r = J.Ref(b, p)
        assert r.build_count == cnt and np.array_equal(r.pairs(), pairs) and np.array_equal(r.mark(), mark)
        if "probe_class" in info:      # present classes match exactly once, absent classes never
            present = np.isin(info["probe_class"], info["present"])
            assert np.array_equal(r.cnt, present.astype(np.int64))
        else:
            assert len(pairs) == info["pairs"]


def test_ref_pairs_against_a_double_loop():
    T, F = True, False
    hand = [
        # duplicates on both sides, a NULL on each side, the extremes
        dict(bcols=[np.array([I64_MIN, 5, 5, I64_MAX, 0, 5], np.int64)], pcols=[np.array([5, I64_MAX, I64_MIN, 7, 5, 0], np.int64)],
             bvalid=[np.array([T, T, F, T, T, T])], pvalid=[np.array([T, T, T, T, F, T])]),
        # two int32 keys whose packed forms would collide without the mask, with selections
        dict(bcols=[np.array([0, 5, -1, -1, 0], np.int32), np.array([-1, -1, -1, 0, 0], np.int32)],
             pcols=[np.array([5, 0, -1, 0, -1, 7], np.int32), np.array([-1, -1, -1, 0, 0, 7], np.int32)],
             bsel=np.array([0, 1, 2, 4]), psel=np.array([5, 4, 2, 1, 0])),
        # mixed widths, NULLs in the second column
        dict(bcols=[np.array([I32_MIN, I32_MAX, 1, 1], np.int32), np.array([2 ** 32, -2 ** 32, 1, 1], np.int64)],
             pcols=[np.array([1, I32_MIN, I32_MAX, I32_MAX], np.int32), np.array([1, 2 ** 32, -2 ** 32, 0], np.int64)],
             bvalid=[None, np.array([T, T, T, F])], pvalid=[None, np.array([T, T, T, T])]),
    ]
    for h in hand:
        want = J.brute_pairs(**h)
        assert len(want) >= 3
        assert J.ref_pairs(**h).tolist() == [list(x) for x in want]
        r = J.Ref(**h)
        assert r.mark().tolist() == [int(any(p == w[0] for w in want)) for p in r.prows.tolist()]
        ok, misses, multi = J.ref_lookup(**h)
        per = [[w[1] for w in want if w[0] == p] for p in r.prows.tolist()]
        assert misses == sum(not x for x in per) and multi == sum(len(x) > 1 for x in per)
        for pick in (0, -1):       # any matching row is allowed, nothing else is
            out = np.array([x[pick] if x else -1 for x in per])
            assert ok(out).all()
        assert not ok(np.full(len(per), -1)).all() and not ok(np.zeros(len(per), np.int64)).all()


def test_ref_counts_and_sorted_columns():
    child = np.array([I64_MIN, I64_MIN, I64_MIN + 2, I64_MAX, 0, I64_MIN + 3], np.int64)
    cv = np.array([True, True, True, True, True, False])
    parent = np.array([I64_MIN, I64_MIN + 1, I64_MIN + 2, I64_MIN + 3, I64_MAX, 0], np.int64)
    got = J.ref_counts(child, cv, None, I64_MIN, 4, parent, np.array([True] * 5 + [False]), None)
    assert got.tolist() == [2, 0, 1, 0, 0, 0]
    got = J.ref_counts(child, None, np.array([3, 4]), I64_MAX - 3, 4, parent, None, np.array([4, 0]))
    assert got.tolist() == [1, 0]
    for typ, lo, hi in (("i64", I64_MIN, I64_MAX), ("i32", I32_MIN, I32_MAX)):
        for r, col in J.sorted_runs_column(typ):
            assert (np.diff(col.astype(object)) >= 0).all() and (col == lo).sum() == r and (col == hi).sum() == r
        p = J.sorted_probe_column(typ)
        assert {lo, hi, lo + 2, hi - 2} <= set(p.tolist())
