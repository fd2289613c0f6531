"""Which table form ph_join_build* chooses, as ph_join_kind reports it: one case on each side of every threshold of the choice
(key-range pass, density rule, small-range rule, exists-only bitmap, radix and node-table minimums, key packing) and every
switch that turns a form off. Each case builds, checks the kind, and marks 1 024 probe keys against numpy membership, so
that the table is also known to be usable. A radix table that has grown its node table stays a radix table."""
import numpy as np
import pytest

from plan_amd import hip

pytestmark = pytest.mark.gpu

K, M = 1 << 10, 1 << 20
NEVER = str(1 << 40)
KNOBS = ("PH_JOIN_RADIX_MIN", "PH_JOIN_RADIX", "PH_JOIN_BIG_MIN", "PH_JOIN_AUTO_RANGE", "PH_JOIN_DIRECT", "PH_JOIN_RADIX_PART_MIN")
HT = {np.dtype(np.int32): hip.PH_I32, np.dtype(np.int64): hip.PH_I64, np.dtype(np.uint8): hip.PH_CODE8}


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


def rng_of(name):
    return np.random.default_rng(sum(name.encode()) + 20240)


def dense(n, dtype=np.int32, lo=0):
    """a permutation of lo .. lo + n - 1"""
    return (rng_of("dense").permutation(n) + lo).astype(dtype)


def sparse64(n):
    """random 62-bit keys: no range rule ever takes them"""
    return rng_of("sparse64").integers(0, 1 << 62, n, dtype=np.int64)


def spread(n, lo, span):
    """n distinct keys of [lo, lo + span] that include both ends, in random order"""
    step = span // (n - 1)
    k = lo + np.arange(n, dtype=np.int64) * step
    k[-1] = lo + span
    return rng_of("spread").permutation(k).astype(np.int32)


def composite(cols):
    """one int64 per row of up to two key columns of at most 32 bits each (or one column of any width)"""
    if len(cols) == 1:
        return cols[0].astype(np.int64)
    return (cols[0].astype(np.int64) << 32) | (cols[1].astype(np.int64) & 0xFFFFFFFF)


def probe_keys(cols, m, rng):
    """m probe rows: every other one a build row's key, the others random values of the key's type (most of them absent)"""
    rows = rng.integers(0, len(cols[0]), m)
    out = []
    for c in cols:
        info = np.iinfo(c.dtype)
        p = rng.integers(info.min, info.max, m, dtype=c.dtype, endpoint=True)
        p[::2] = c[rows[::2]]
        out.append(p)
    return out


def build_and_mark(ctx, monkeypatch, cols, env=None, **build):
    """the kind of the table built over cols under env, after one mark probe of 1 024 keys is checked against numpy"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    n = len(cols[0])
    pk = probe_keys(cols, K, rng_of("probe"))
    db = [hip.DevColumn(ctx, HT[c.dtype], c) for c in cols]
    dp = [hip.DevColumn(ctx, HT[c.dtype], c) for c in pk]
    j = hip.Join(ctx, db, None, n, **build)
    try:
        kind = j.kind
        f = j.probe_mark(dp, None, K)
        found = ctx.download(f, np.uint8, K)
        ctx.free(f)
        assert np.array_equal(found != 0, np.isin(composite(pk), composite(cols))), kind
        assert j.kind == kind
    finally:
        j.free()
        for d in db + dp:
            d.free()
    return kind


RADIX_OFF = {"PH_JOIN_RADIX": "0"}
LOW_RADIX = {"PH_JOIN_RADIX_MIN": "100000"}

NO_RANGE = [
    # id, key columns, environment, expected kind
    ("auto_range_at", lambda: [dense(M)], None, "direct"),
    ("auto_range_below", lambda: [dense(M - 1)], None, "chained+bloom"),
    ("auto_range_off", lambda: [dense(M)], {"PH_JOIN_AUTO_RANGE": "0"}, "chained+bloom"),
    ("radix_at", lambda: [sparse64(4 * M + 1)], None, "radix"),
    ("radix_below", lambda: [sparse64(4 * M)], None, "chained+bloom"),
    ("radix_off", lambda: [sparse64(4 * M + 1)], RADIX_OFF, "nodes"),
    ("radix_and_nodes_off", lambda: [sparse64(4 * M + 1)], {**RADIX_OFF, "PH_JOIN_BIG_MIN": NEVER}, "chained"),   # (no bitmap above 4 M rows)
    ("two_int32_at", lambda: two_int32(100_000), LOW_RADIX, "radix"),
    ("two_int32_below", lambda: two_int32(99_999), LOW_RADIX, "chained+bloom"),
    ("not_packable", lambda: [two_int32(100_000)[0], sparse64(100_000)], LOW_RADIX, "chained+bloom"),
]


def two_int32(n):
    r = rng_of("two_int32")
    return [r.integers(-(1 << 31), 1 << 31, n).astype(np.int32), r.integers(-(1 << 31), 1 << 31, n).astype(np.int32)]


@pytest.mark.parametrize("cols,env,want", [pytest.param(*c[1:], id=c[0]) for c in NO_RANGE])
def test_form_without_range(ctx, monkeypatch, cols, env, want):
    assert build_and_mark(ctx, monkeypatch, cols(), env) == want


N1, N0 = 256 * K + 1, 256 * K
LO = -1000

RANGED = [
    # id, rows, span (key_hi - key_lo), environment, build flags, expected kind
    ("dense_at", N1, 8 * N1 - 1, None, {}, "direct"),                       # span + 1 = 8 n
    ("dense_above", N1, 8 * N1, None, {}, "chained+bloom"),                 # span + 1 = 8 n + 1
    ("dense_at_direct_off", N1, 8 * N1 - 1, {"PH_JOIN_DIRECT": "0"}, {}, "chained+bloom"),
    ("small_range_at", N0, 4 * M - 1, None, {}, "direct"),
    ("small_range_above", N0, 4 * M, None, {}, "chained+bloom"),            # (not direct)
    ("exists_at", N0, 64 * M - 1, None, {"exists_only": True}, "bitmap"),
    ("exists_below_dense", N0 - 1, 8 * (N0 - 1) - 1, None, {"exists_only": True}, "direct"),
    ("exists_below_sparse", N0 - 1, 8 * M, None, {"exists_only": True}, "chained+bloom"),
    ("exists_wide_span", N0, 64 * M, None, {"exists_only": True}, "chained+bloom"),   # (not bitmap)
]


@pytest.mark.parametrize("n,span,env,flags,want", [pytest.param(*c[1:], id=c[0]) for c in RANGED])
def test_form_with_range(ctx, monkeypatch, n, span, env, flags, want):
    assert build_and_mark(ctx, monkeypatch, [spread(n, LO, span)], env, key_range=(LO, LO + span), **flags) == want


def test_narrow_key_is_never_direct(ctx, monkeypatch):
    """a PH_CODE8 key with a range that a wider key would get a direct table for"""
    codes = rng_of("code8").integers(0, 256, 5000).astype(np.uint8)
    assert build_and_mark(ctx, monkeypatch, [codes], key_range=(0, 255)) == "chained+bloom"


@pytest.mark.parametrize("n,want", [(32 * K, "nodes"), (32 * K - 1, "chained+bloom")])
def test_fk_probes_threshold(ctx, monkeypatch, n, want):
    assert build_and_mark(ctx, monkeypatch, [sparse64(n)], fk_probes=True) == want


def test_build_where_over_a_sparse_range_is_unsupported(ctx, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    n = 1000
    keys = spread(n, 0, 10**9)
    gate = np.ones(n, np.uint8)
    dk, dg = hip.DevColumn(ctx, hip.PH_I32, keys), hip.DevColumn(ctx, hip.PH_CODE8, gate)
    try:
        j = hip.Join.build_where(ctx, [dk], dg, hip.PH_EQ, hip.const(hip.PH_I32, i=1), None, n, (0, 10**9))
        assert j is None                                                   # PH_EUNSUPPORTED
        assert hip.last_error() == ("ph_join_build_where: the key range [0, 1000000000] does not give a direct table for 1000 build rows; "
                                    "run ph_filter_select and ph_join_build")
    finally:
        dk.free(); dg.free()


def test_radix_stays_radix_after_mark(ctx, monkeypatch):
    """ph_join_probe_mark builds the node table of a radix table; the table still reports 'radix', its inner probes still come
    from the radix images (unordered pairs), and they equal the pairs of sort / searchsorted"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PH_JOIN_RADIX_MIN", "100000")
    cols = two_int32(100_000)
    cols[0][:500], cols[1][:500] = cols[0][500:1000], cols[1][500:1000]     # some keys twice
    r = rng_of("radix_mark")
    pm, pi = probe_keys(cols, K, r), probe_keys(cols, 4 * K, r)
    db = [hip.DevColumn(ctx, hip.PH_I32, c) for c in cols]
    dm = [hip.DevColumn(ctx, hip.PH_I32, c) for c in pm]
    di = [hip.DevColumn(ctx, hip.PH_I32, c) for c in pi]
    j = hip.Join(ctx, db, None, len(cols[0]))
    try:
        assert j.kind == "radix"
        f = j.probe_mark(dm, None, K)
        found = ctx.download(f, np.uint8, K)
        ctx.free(f)
        assert np.array_equal(found != 0, np.isin(composite(pm), composite(cols)))
        assert j.kind == "radix" and not j.pairs_ordered()
        bk, pk = composite(cols), composite(pi)
        order = np.argsort(bk, kind="stable")
        lo, hi = np.searchsorted(bk[order], pk, "left"), np.searchsorted(bk[order], pk, "right")
        want = np.array([(p, order[q]) for p in range(len(pk)) for q in range(lo[p], hi[p])], np.int64).reshape(-1, 2)
        m, op, ob = j.probe_inner(di, None, 4 * K, 1 << 16)
        assert m == len(want)
        got = np.stack([ctx.download(op, np.int32, m), ctx.download(ob, np.int32, m)], 1).astype(np.int64)
        ctx.free(op); ctx.free(ob)
        assert np.array_equal(got[np.lexsort((got[:, 1], got[:, 0]))], want[np.lexsort((want[:, 1], want[:, 0]))])
        assert j.kind == "radix"
    finally:
        j.free()
        for d in db + dm + di:
            d.free()
