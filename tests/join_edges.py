"""Constructed inputs and plain references of the join edge tests (test_gpu_join_edges.py; checked on their own, without a device, by
test_join_edges_reference.py).

Two families of inputs that random keys from a small range never produce:
  * hash structure: the join hash mix64(SEED ^ key) is a bijection of 64-bit words, so inv_mix64 gives the key of ANY hash word and a
    builder can decide which bucket, Bloom word, head slice, radix bin, radix bucket and tag every key falls into;
  * key values at the edges of the int32 / int64 domains, packed pairs that differ in one half only, dense ranges that end at a
    domain edge.
The references work on the key VALUES only (sort, unique and searchsorted over int64 are exact): nothing here hashes to find a match."""
import numpy as np

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
M64 = 2 ** 64 - 1

# ------------------------------------------------------------------ the hash (device_util.h mix64: the splitmix64 finaliser)
SEED = 0x9E3779B97F4A7C15            # load_keys / big_hash: h = mix64(SEED ^ key)
MUL1, MUL2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
INV1, INV2 = pow(MUL1, -1, 2 ** 64), pow(MUL2, -1, 2 ** 64)


def mix64_int(x):
    x ^= x >> 30
    x = x * MUL1 & M64
    x ^= x >> 27
    x = x * MUL2 & M64
    return x ^ (x >> 31)


def inv_mix64_int(h):
    h ^= (h >> 31) ^ (h >> 62)        # undoes x ^= x >> 31
    h = h * INV2 & M64
    h ^= (h >> 27) ^ (h >> 54)
    h = h * INV1 & M64
    return h ^ (h >> 30) ^ (h >> 60)


def key_hash_int(k):
    """hash of one key value (a Python int in the int64 domain; int32 / DATE values are sign-extended by taking them as they are)"""
    return mix64_int(SEED ^ (k & M64))


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def mix64(x):
    x = _u64(x).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= np.uint64(MUL1)
        x ^= x >> np.uint64(27)
        x *= np.uint64(MUL2)
        x ^= x >> np.uint64(31)
    return x


def inv_mix64(h):
    h = _u64(h).copy()
    with np.errstate(over="ignore"):
        h ^= (h >> np.uint64(31)) ^ (h >> np.uint64(62))
        h *= np.uint64(INV2)
        h ^= (h >> np.uint64(27)) ^ (h >> np.uint64(54))
        h *= np.uint64(INV1)
        h ^= (h >> np.uint64(30)) ^ (h >> np.uint64(60))
    return h


def as_u64(k):
    """a key column as the 64-bit word the kernels hash: 4-byte keys sign-extended (jkey, load_kw), CODE8 zero-extended"""
    k = np.asarray(k)
    return k.astype(np.uint64) if k.dtype == np.uint8 else k.astype(np.int64).view(np.uint64)


def key_hash(k):
    return mix64(np.uint64(SEED) ^ as_u64(k))


def hash2(k0, k1):
    """two key columns through load_keys / part_hashes: the running hash is mixed once per column"""
    return mix64(mix64(np.uint64(SEED) ^ as_u64(k0)) ^ as_u64(k1))


def pack(a, b):
    """big_pack<4, 2>: (a << 32) | (b & 0xffffffff) — what the node table and the radix form hash and compare for two 4-byte keys"""
    return (as_u64(a) << np.uint64(32)) | (as_u64(b) & np.uint64(0xFFFFFFFF))


def pack_hash(a, b):
    return mix64(np.uint64(SEED) ^ pack(a, b))


def keys_with_hash(h, packed=False):
    """the int64 keys whose hash is h; packed: the (a, b) int32 columns whose packed pair has hash h"""
    k = (inv_mix64(h) ^ np.uint64(SEED)).view(np.int64)
    if not packed:
        return k
    return (k >> 32).astype(np.int32), (k & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


# ------------------------------------------------------------------ the bit layout (ops_join.hip), restated
def chained_cap(n):
    """join_build_impl: cap = max(nextpow2(2n), 1024); bucket = h & (cap - 1)"""
    cap = 1024
    while cap < 2 * n:
        cap <<= 1
    return cap


PB_SLICE_LOG = 14                     # part_build_kernel: head slice of the partitioned chained build = bucket >> 14
BG_SLICE_LOG = 15                     # big_build_kernel: head slice of the node table = bucket >> 15
BLOOM_WORD_SHIFT = 34                 # bloom_word: (h >> 34) & inner_mask (+ the slice's bits in front for the partitioned build)
BLOOM_MASK_SHIFT = 24                 # bloom_mask(h >> 24): bits (b & 31) and ((b >> 5) & 31)
COARSE_SHIFT, COARSE_BITS = 40, 20    # coarse_bit: (h >> 40) & (2^20 - 1)
LOOKALIKE_SHIFT = 60                  # bits 0..59 hold everything above for every table size the bitmaps exist for (<= 4 M rows)
RJ_SHIFT = 36                         # rj_count_kernel: bin = (h >> 36) & (bins - 1)
RJ_SLOTS = 8192
RJ_BUCKETS = RJ_SLOTS // 16           # rj_bucket: h & 511
RJ_TAG_SHIFT, RJ_TAG_MASK = 24, 0x7F  # rj_tag: 0x80 | ((h >> 24) & 0x7f)
RJ_BIN_LIMIT = RJ_SLOTS - RJ_SLOTS // 8   # rj_tables_kernel: a bin of more rows than this gives the form up
RJ_STAGE = 8192                       # rj_emit: pairs staged per chunk of RJ_CH probe rows
RJ_CH = 4096


def rj_log_bins(n):
    """build_radix: 64 bins, doubled while the average bin would hold more than 9/16 of a table image"""
    lb = 6
    while (1 << lb) * (RJ_SLOTS * 9 // 16) < n and lb < 13:
        lb += 1
    return lb


def bucket_of(h, cap):
    return h & np.uint64(cap - 1)


def bloom_bits_of(n):
    bits = 1 << 16
    while bits < 16 * n:
        bits <<= 1
    return bits


def bloom_word_of(h, n):
    """word of the atomic build's bitmap (the partitioned build puts the slice's bits, which are bucket bits, in front of fewer of these)"""
    return (h >> np.uint64(BLOOM_WORD_SHIFT)) & np.uint64(bloom_bits_of(n) // 32 - 1)


def bloom_mask_of(h):
    b = h >> np.uint64(BLOOM_MASK_SHIFT)
    return (np.uint64(1) << (b & np.uint64(31))) | (np.uint64(1) << ((b >> np.uint64(5)) & np.uint64(31)))


def coarse_of(h):
    return (h >> np.uint64(COARSE_SHIFT)) & np.uint64((1 << COARSE_BITS) - 1)


def rj_bin_of(h, log_bins):
    return (h >> np.uint64(RJ_SHIFT)) & np.uint64((1 << log_bins) - 1)


def rj_bucket_of(h):
    return h & np.uint64(RJ_BUCKETS - 1)


def rj_tag_of(h):
    return (h >> np.uint64(RJ_TAG_SHIFT)) & np.uint64(RJ_TAG_MASK)


# ------------------------------------------------------------------ hash-structure builders
def _rand_u64(rng, n):
    return rng.integers(0, 2 ** 64, n, dtype=np.uint64)


def _distinct(h):
    assert len(np.unique(h)) == len(h), "constructed hash words collide (reseed)"
    return h


def _set_bits(h, shift, width, value):
    """h with bits [shift, shift + width) replaced by value (a scalar or an array)"""
    mask = np.uint64(((1 << width) - 1) << shift)
    return (h & ~mask) | ((np.asarray(value, dtype=np.uint64) << np.uint64(shift)) & mask)


def _cols(h, packed):
    k = keys_with_hash(h, packed)
    return list(k) if packed else [k]


def _finish(rng, hb, hp, packed, info):
    """shuffle both sides; info keeps the hash words and, per probe row, the class it was built as"""
    ob, op = rng.permutation(len(hb)), rng.permutation(len(hp))
    info.update(build_hash=hb[ob], probe_hash=hp[op], probe_class=info.pop("classes")[op], packed=packed)
    return _cols(hb[ob], packed), _cols(hp[op], packed), info


def one_bucket(n_build, L, seed=1, packed=False):
    """L distinct build keys in ONE bucket of the chained / node table of n_build rows, the other rows spread over other buckets.
    Probe classes: 0 = the L keys (each matches once); 1 = L absent look-alikes: the hash of a present key with only bits 60..63
    changed — same bucket, Bloom word, Bloom mask and coarse bit, so that only the key compare can reject them; 2 = absent keys in
    buckets no build key uses; 3 = some of the other build keys."""
    rng = np.random.default_rng(seed)
    cap = chained_cap(n_build)
    lc = cap.bit_length() - 1
    b0 = int(rng.integers(0, cap))
    hot = _set_bits(_rand_u64(rng, L), 0, lc, b0)
    low60 = np.uint64((1 << LOOKALIKE_SHIFT) - 1)
    assert len(np.unique(hot & low60)) == L, "reseed"
    other_b = rng.integers(0, cap - 1, n_build - L)
    other_b += other_b >= b0
    rest = _set_bits(_rand_u64(rng, n_build - L), 0, lc, other_b)
    hb = _distinct(np.concatenate([hot, rest]))
    look = hot ^ (rng.integers(1, 16, L).astype(np.uint64) << np.uint64(LOOKALIKE_SHIFT))
    free = np.setdiff1d(np.arange(cap), np.append(other_b, b0))
    n_empty = min(L, 512)
    empty = _set_bits(_rand_u64(rng, n_empty), 0, lc, rng.choice(free, n_empty))
    some = rest[: min(len(rest), 256)]
    hp = np.concatenate([hot, look, empty, some])
    classes = np.concatenate([np.full(len(x), c) for c, x in enumerate((hot, look, empty, some))])
    return _finish(rng, hb, hp, packed, dict(cap=cap, bucket=b0, L=L, classes=classes, present=(0, 3)))


def one_slice(n_build, slice_log, seed=2, packed=False, n_probe=4096):
    """every build key in ONE head slice (bucket >> slice_log) of a table of n_build rows, buckets inside the slice spread.
    Probe classes: 0 = present keys; 1 = absent keys of the same slice; 2 = absent keys of other slices."""
    rng = np.random.default_rng(seed)
    cap = chained_cap(n_build)
    lc = cap.bit_length() - 1
    nslices = cap >> slice_log
    assert nslices >= 2
    s0 = int(rng.integers(0, nslices))
    hb = _distinct(_set_bits(_rand_u64(rng, n_build), slice_log, lc - slice_log, s0))
    same = _set_bits(_rand_u64(rng, n_probe), slice_log, lc - slice_log, s0)
    same = same[~np.isin(same, hb)]
    o = rng.integers(0, nslices - 1, n_probe)
    o += o >= s0
    away = _set_bits(_rand_u64(rng, n_probe), slice_log, lc - slice_log, o)
    present = hb[rng.choice(n_build, n_probe)]
    hp = np.concatenate([present, same, away])
    classes = np.concatenate([np.full(len(x), c) for c, x in enumerate((present, same, away))])
    return _finish(rng, hb, hp, packed, dict(cap=cap, slice=s0, slice_log=slice_log, classes=classes, present=(0,)))


def one_radix_bin(n_build, m, same_bucket=False, same_tag=False, seed=3, packed=False, n_absent=1024):
    """exactly m build rows (distinct keys) in ONE bin of the radix form of n_build rows, every other row in another bin.
    same_bucket: the m keys share rj_bucket, so insertion spills over m / 16 consecutive buckets and a probe walks them;
    same_tag: they share the 7 tag bits too, so every slot of those buckets is a candidate.
    Probe classes: 0 = every one of the m keys; 1 = absent keys of the same bin (and bucket / tag where those are shared);
    2 = some of the other build keys."""
    rng = np.random.default_rng(seed)
    lb = rj_log_bins(n_build)
    bins = 1 << lb
    bin0, bk0, tag0 = int(rng.integers(0, bins)), int(rng.integers(0, RJ_BUCKETS)), int(rng.integers(0, 128))

    def in_bin(n):
        h = _set_bits(_rand_u64(rng, n), RJ_SHIFT, lb, bin0)
        if same_bucket:
            h = _set_bits(h, 0, 9, bk0)
        if same_tag:
            h = _set_bits(h, RJ_TAG_SHIFT, 7, tag0)
        return h
    hot = in_bin(m)
    ob = rng.integers(0, bins - 1, n_build - m)
    ob += ob >= bin0
    rest = _set_bits(_rand_u64(rng, n_build - m), RJ_SHIFT, lb, ob)
    hb = _distinct(np.concatenate([hot, rest]))
    absent = in_bin(n_absent)
    absent = absent[~np.isin(absent, hb)]
    some = rest[: min(len(rest), 1024)]
    hp = np.concatenate([hot, absent, some])
    classes = np.concatenate([np.full(len(x), c) for c, x in enumerate((hot, absent, some))])
    return _finish(rng, hb, hp, packed, dict(log_bins=lb, bin=bin0, m=m, bucket=bk0 if same_bucket else None,
                                             tag=tag0 if same_tag else None, classes=classes, present=(0, 2)))


def half_twins(n_build, half, n_twins=32, seed=5):
    """n_twins pairs (build key A, absent probe key A') of int64 keys that agree in one half — half = "low": the low 32 bits are equal,
    "high": the high 32 bits — and fall into the SAME bucket of the chained / node table of n_build rows (found by search: 2^17
    candidates per pair). For every A' the build side also holds a helper key in the neighbouring bucket whose hash equals A''s
    everywhere above the bucket bits, so the Bloom word and mask and the coarse bit of A' are set and A' reaches A's chain: only a compare
    of BOTH halves tells them apart. Probe classes: 0 = the keys A; 1 = the keys A'; 2 = some filler build keys."""
    rng = np.random.default_rng(seed)
    cap = chained_cap(n_build)
    A, A2 = [], []
    for _ in range(n_twins):
        fixed = np.uint64(rng.integers(0, 2 ** 32))
        var = np.uint64(rng.integers(0, 2 ** 31)) + np.arange(1 << 17, dtype=np.uint64)
        keys = (var << np.uint64(32)) | fixed if half == "low" else (fixed << np.uint64(32)) | var
        bk = bucket_of(mix64(np.uint64(SEED) ^ keys), cap)
        order = np.argsort(bk, kind="stable")
        i = int(np.flatnonzero(bk[order][1:] == bk[order][:-1])[0])
        A.append(keys[order[i]])
        A2.append(keys[order[i + 1]])
    A, A2 = np.array(A, np.uint64).view(np.int64), np.array(A2, np.uint64).view(np.int64)
    helper = keys_with_hash(key_hash(A2) ^ np.uint64(1))
    rest = keys_with_hash(_rand_u64(rng, n_build - 2 * n_twins))
    b = np.concatenate([A, helper, rest])
    assert len(np.unique(b)) == n_build and not np.isin(A2, b).any(), "reseed"
    p = np.concatenate([A, A2, rest[:256]])
    classes = np.concatenate([np.full(len(x), c) for c, x in enumerate((A, A2, rest[:256]))])
    ob, op = rng.permutation(n_build), rng.permutation(len(p))
    return [b[ob]], [p[op]], dict(cap=cap, half=half, A=A, A2=A2, helper=helper, probe_class=classes[op], present=(0, 2))


def fan_out(n_build, dup, seed=4, n_probe=8192):
    """every build key dup times, every probe row matching: dup pairs per probe row, so a chunk of RJ_CH probe rows of the radix
    probe produces dup x 4096 pairs (> RJ_STAGE for dup >= 3); the dup equal keys also share one bucket and one tag"""
    rng = np.random.default_rng(seed)
    assert n_build % dup == 0
    keys = np.unique(rng.integers(I64_MIN, I64_MAX, n_build // dup, endpoint=True, dtype=np.int64))
    assert len(keys) == n_build // dup
    b = rng.permutation(np.repeat(keys, dup))
    p = keys[rng.integers(0, len(keys), n_probe)]
    return [b], [p], dict(dup=dup, pairs=n_probe * dup)


# ------------------------------------------------------------------ key-domain edge tables
I64_EDGES = [I64_MIN, I64_MIN + 1, -2 ** 32 - 1, -2 ** 32, -2 ** 31 - 1, -2 ** 31, -1, 0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32,
             I64_MAX - 1, I64_MAX]
# pairs of int64 keys that differ in the high 32 bits only / in the low 32 bits only: the first of each pair is a build key,
# the second is probed and absent
I64_HIGH_ONLY = [(5, 5 + 2 ** 32), (-1, 0xABCD_FFFF_FFFF), (0x1234_5678_0000_0007, 0x1234_5679_0000_0007), (I64_MIN + 2 ** 40 + 9, 2 ** 40 + 9)]
I64_LOW_ONLY = [(7 << 32, (7 << 32) + 1), (-(3 << 32), -(3 << 32) + 2 ** 31), (I64_MAX - 77, I64_MAX - 78)]
I32_EDGES = [I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX]
I32_PAIRS_REQUIRED = [(0, -1), (5, -1), (-1, -1), (-1, 0), (0, 0)]
CODE8_EDGES = [0, 255]


class Case:
    """one join input: key columns of both sides (numpy arrays of their storage type), per-column bool validity (or None),
    sorted selections of both sides (or None), and the key types as names ("i64", "i32", "date", "code8")"""

    def __init__(self, name, types, bcols, pcols, bvalid=None, pvalid=None, bsel=None, psel=None, **info):
        self.name, self.types, self.bcols, self.pcols = name, list(types), list(bcols), list(pcols)
        self.bvalid = list(bvalid) if bvalid is not None else [None] * len(bcols)
        self.pvalid = list(pvalid) if pvalid is not None else [None] * len(pcols)
        self.bsel, self.psel, self.info = bsel, psel, info

    def plain(self):
        """the same columns without NULLs and selections"""
        return Case(self.name + "/plain", self.types, self.bcols, self.pcols, **self.info)

    @property
    def nb(self):
        return len(self.bcols[0])

    @property
    def np_(self):
        return len(self.pcols[0])


_DT = {"i64": np.int64, "i32": np.int32, "date": np.int32, "code8": np.uint8}
_DOMAIN = {"i64": (I64_MIN, I64_MAX), "i32": (I32_MIN, I32_MAX), "date": (I32_MIN, I32_MAX), "code8": (0, 255)}


def _edge_case(name, types, build_rows, probe_rows, nb, npr, seed):
    """build_rows / probe_rows: key tuples that must occur on that side — each is placed three times (duplicates), once in a row
    that is valid and selected. The rest is filler: values from all over the domain, a tenth from a small range around 0, and
    on the probe side rows copied from the build side. NULLs in the first and the last key column, selections on both sides."""
    rng = np.random.default_rng(seed)
    nk = len(types)

    def filler(n):
        cols = []
        for t in types:
            lo, hi = _DOMAIN[t]
            wide = rng.integers(lo, hi, n, endpoint=True, dtype=np.int64)
            w = 40 + nb // 200          # a tenth of the rows from a range that gives ~10 rows per value: duplicates and chance matches
            small = rng.integers(max(lo, -w), min(hi, w), n, endpoint=True, dtype=np.int64)
            cols.append(np.where(rng.random(n) < 0.1, small, wide))
        return cols

    def place(cols, rows, n):
        pos = rng.choice(n, 3 * len(rows), replace=False)
        for c in range(nk):
            cols[c][pos] = np.array([r[c] for r in rows] * 3, dtype=np.int64)
        return pos[: len(rows)]       # one occurrence of every row: kept valid and selected
    b, p = filler(nb), filler(npr)
    take = rng.random(npr) < 0.3
    src = rng.integers(0, nb, npr)
    for c in range(nk):
        p[c] = np.where(take, b[c][src], p[c])
    keep_b, keep_p = place(b, build_rows, nb), place(p, probe_rows, npr)

    def nulls(n, keep):
        out = []
        for c in range(nk):
            if c in (0, nk - 1):
                v = rng.random(n) > 0.1
                v[keep] = True
                out.append(v)
            else:
                out.append(None)
        return out

    def sel(n, keep):
        s = rng.random(n) < 0.6
        s[keep] = True
        return np.flatnonzero(s).astype(np.int32)
    return Case(name, types, [x.astype(_DT[t]) for x, t in zip(b, types)], [x.astype(_DT[t]) for x, t in zip(p, types)],
                nulls(nb, keep_b), nulls(npr, keep_p), sel(nb, keep_b), sel(npr, keep_p),
                build_rows=list(build_rows), probe_rows=list(probe_rows))


def single_key_case(typ, nb=6000, npr=9000, seed=11):
    if typ == "i64":
        build = I64_EDGES + [a for a, _ in I64_HIGH_ONLY + I64_LOW_ONLY]
        probe = build + [b for _, b in I64_HIGH_ONLY + I64_LOW_ONLY]
    elif typ == "code8":
        build, probe = CODE8_EDGES, CODE8_EDGES      # (the filler covers all 256 codes: no code is absent)
    else:
        build, probe = I32_EDGES, I32_EDGES + [I32_MIN + 2, I32_MAX - 2, 2 ** 30 + 1, -2 ** 30 - 1]
    c = _edge_case(f"{typ}-edges", [typ], [(v,) for v in build], [(v,) for v in probe], nb, npr, seed)
    absent = [v for v in probe if v not in build]
    assert not np.isin(np.array(absent, dtype=np.int64), c.bcols[0].astype(np.int64)).any(), "an 'absent' probe value is in the filler (reseed)"
    c.info["absent"] = absent
    return c


def i32_pair_case(nb=6000, npr=9000, seed=12):
    build = sorted(set([(a, b) for a in I32_EDGES for b in I32_EDGES] + I32_PAIRS_REQUIRED))
    absent = [(5, -2 ** 30 - 1), (2 ** 30 + 1, -1), (-1, 2 ** 30 + 1), (I32_MIN, 2 ** 30 + 1), (2 ** 30 + 1, I32_MAX), (0, I32_MAX - 41)]
    c = _edge_case("i32-pair-edges", ["i32", "i32"], build, build + absent, nb, npr, seed)
    bset = set(zip(c.bcols[0].tolist(), c.bcols[1].tolist()))
    assert not any(a in bset for a in absent), "reseed"
    c.info["absent"] = absent
    return c


def multi_key_case(types, nb=5000, npr=7000, seed=13):
    """mixed widths / three and four key columns: the edge values of every column's type against each other (a diagonal walk over
    the value lists rather than their product)"""
    lists = [I64_EDGES if t == "i64" else CODE8_EDGES if t == "code8" else I32_EDGES for t in types]
    m = max(len(x) for x in lists)
    build = sorted({tuple(lists[c][(i + s * c) % len(lists[c])] for c in range(len(types))) for i in range(m) for s in (0, 1, 2)})
    return _edge_case("-".join(types) + "-edges", types, build, build, nb, npr, seed)


DENSE_R = 5000          # R + 1 = 5001 key values: no multiple of 64 (the occupancy bitmap's last word is partial)


def dense_ranges():
    """[(name, type, lo, hi)] of the direct-table cases"""
    R = DENSE_R
    return [("i64-at-min", "i64", I64_MIN, I64_MIN + R), ("i64-at-max", "i64", I64_MAX - R, I64_MAX), ("i64-around-0", "i64", -(R // 2), R - R // 2),
            ("i32-at-min", "i32", I32_MIN, I32_MIN + R), ("i32-at-max", "i32", I32_MAX - R, I32_MAX)]


def dense_case(name, typ, lo, hi, dups, seed=14, npr=9000):
    """build keys in [lo, hi] (lo and hi among them; unique and ascending without dups, shuffled with repeats with dups); probes:
    lo, hi, lo - 1 and hi + 1 where the type holds them, the opposite end of the domain, keys in and around the range"""
    rng = np.random.default_rng(seed)
    dlo, dhi = _DOMAIN[typ]
    span = hi - lo
    off = np.unique(np.concatenate([[0, span], rng.choice(span + 1, (span + 1) * 7 // 8, replace=False)]))
    if dups:
        off = rng.permutation(np.concatenate([off, off[rng.integers(0, len(off), len(off) // 2)], [0, 0, span, span]]))
    b = np.array([lo + int(o) for o in off], dtype=np.int64)
    must = [lo, hi, dlo, dhi, 0] + ([lo - 1] if lo > dlo else []) + ([hi + 1] if hi < dhi else [])
    around = rng.integers(max(dlo, lo - 50), min(dhi, hi + 50), npr, endpoint=True, dtype=np.int64)
    wide = rng.integers(dlo, dhi, npr, endpoint=True, dtype=np.int64)
    p = np.where(rng.random(npr) < 0.8, around, wide)
    pos = rng.choice(npr, 2 * len(must), replace=False)
    p[pos] = np.array(must * 2, dtype=np.int64)
    pv = rng.random(npr) > 0.1
    pv[pos[: len(must)]] = True
    bs = rng.random(len(b)) < 0.7
    bs[[int(np.flatnonzero(b == lo)[0]), int(np.flatnonzero(b == hi)[0])]] = True
    ps = rng.random(npr) < 0.6
    ps[pos[: len(must)]] = True
    return Case(f"{name}{'-dups' if dups else ''}", [typ], [b.astype(_DT[typ])], [p.astype(_DT[typ])], None, [pv],
                np.flatnonzero(bs).astype(np.int32), np.flatnonzero(ps).astype(np.int32), lo=lo, hi=hi, must=must)


# ------------------------------------------------------------------ references: the key values, no hashing
def _codes(bcols, pcols):
    """one int64 code per row of both sides, equal exactly where all key columns are equal (values widened to int64 as the kernels
    widen them: signed columns sign-extended, CODE8 zero-extended)"""
    b = [np.asarray(c).astype(np.int64) for c in bcols]
    p = [np.asarray(c).astype(np.int64) for c in pcols]
    if len(b) == 1:
        return b[0], p[0]
    cols = [np.concatenate([x, y]) for x, y in zip(b, p)]
    order = np.lexsort(cols[::-1])                               # rows in key order: equal rows are neighbours
    new = np.zeros(len(order), bool)
    for c in cols:
        new[1:] |= c[order][1:] != c[order][:-1]
    code = np.empty(len(order), np.int64)
    code[order] = np.cumsum(new)
    return code[: len(b[0])], code[len(b[0]):]


def _live(n, valids, sel):
    """row ids a side offers, in position order, and which of them have no NULL key"""
    rows = np.arange(n, dtype=np.int64) if sel is None else np.asarray(sel, dtype=np.int64)
    ok = np.ones(len(rows), bool)
    for v in valids or []:
        if v is not None:
            ok &= np.asarray(v, bool)[rows]
    return rows, ok


class Ref:
    """the join of one Case-like input restated: build rows ordered by key, one searchsorted per side of every probe key's run"""

    def __init__(self, bcols, pcols, bvalid=None, pvalid=None, bsel=None, psel=None):
        cb, cp = _codes(bcols, pcols)
        self.brows, bok = _live(len(cb), bvalid, bsel)
        self.prows, self.pok = _live(len(cp), pvalid, psel)
        ins = self.brows[bok]                                   # inserted build rows
        self.build_count = len(ins)
        order = np.argsort(cb[ins], kind="stable")
        self.sorted_rows, self.sorted_codes = ins[order], cb[ins][order]
        self.pcode = cp[self.prows]
        self.lo = np.searchsorted(self.sorted_codes, self.pcode, "left")
        self.cnt = np.where(self.pok, np.searchsorted(self.sorted_codes, self.pcode, "right") - self.lo, 0)
        self.row_code = np.full(len(cb), I64_MIN, np.int64)     # code of every inserted build row; others get a value next line
        self.row_in = np.zeros(len(cb), bool)
        self.row_code[ins], self.row_in[ins] = cb[ins], True

    def pairs(self):
        """(probe row id, build row id), sorted by probe row id then build row id — int64[m, 2]"""
        m = int(self.cnt.sum())
        pi = np.repeat(np.arange(len(self.prows)), self.cnt)
        within = np.arange(m) - np.repeat(np.cumsum(self.cnt) - self.cnt, self.cnt)
        out = np.stack([self.prows[pi], self.sorted_rows[self.lo[pi] + within]], 1) if m else np.empty((0, 2), np.int64)
        return out[np.lexsort((out[:, 1], out[:, 0]))]

    def mark(self):
        return (self.cnt > 0).astype(np.uint8)

    def lookup_ok(self, out):
        """per probe position: out is -1 where no build row matches, else ONE of the matching build rows"""
        out = np.asarray(out, dtype=np.int64)
        hit = out >= 0
        safe = np.where(hit & (out < len(self.row_code)), out, 0)
        good = hit & (out < len(self.row_code)) & self.row_in[safe] & (self.row_code[safe] == self.pcode) & self.pok
        return np.where(self.cnt > 0, good, out == -1)

    def lookup_stats(self):
        return [int((self.cnt == 0).sum()), int((self.cnt > 1).sum())]


def ref_pairs(bcols, pcols, bvalid=None, pvalid=None, bsel=None, psel=None):
    return Ref(bcols, pcols, bvalid, pvalid, bsel, psel).pairs()


def ref_mark(bcols, pcols, bvalid=None, pvalid=None, bsel=None, psel=None):
    return Ref(bcols, pcols, bvalid, pvalid, bsel, psel).mark()


def ref_lookup(bcols, pcols, bvalid=None, pvalid=None, bsel=None, psel=None):
    """(allowed: a function of the device's out array giving a bool per probe position, misses, multi)"""
    r = Ref(bcols, pcols, bvalid, pvalid, bsel, psel)
    misses, multi = r.lookup_stats()
    return r.lookup_ok, misses, multi


def ref_counts(child, cvalid, csel, key_min, key_range, parent, pvalid, psel):
    """ph_count_by_key: per parent position the number of child rows (selected, non-NULL, key in [key_min, key_min + key_range))
    with the parent's key; 0 for a NULL parent key. Python ints decide the range test: key_min + key_range may pass 2^63."""
    crow, cok = _live(len(child), [cvalid], csel)
    ck = np.asarray(child).astype(np.int64)[crow][cok]
    inr = np.array([key_min <= int(k) < key_min + key_range for k in ck.tolist()], bool) if len(ck) else np.zeros(0, bool)
    u, c = np.unique(ck[inr], return_counts=True)
    prow, pok = _live(len(parent), [pvalid], psel)
    pk = np.asarray(parent).astype(np.int64)[prow]
    at = np.searchsorted(u, pk)
    at_c = np.minimum(at, max(len(u) - 1, 0))
    hit = pok & (at < len(u)) & (u[at_c] == pk if len(u) else False)
    return np.where(hit, c[at_c] if len(u) else 0, 0).astype(np.int64)


def brute_pairs(bcols, pcols, bvalid=None, pvalid=None, bsel=None, psel=None):
    """the double loop, for the hand-written cases"""
    nb, npr, nk = len(bcols[0]), len(pcols[0]), len(bcols)
    out = []
    for p in (range(npr) if psel is None else psel):
        if any(pvalid and pvalid[c] is not None and not pvalid[c][p] for c in range(nk)):
            continue
        for b in (range(nb) if bsel is None else bsel):
            if any(bvalid and bvalid[c] is not None and not bvalid[c][b] for c in range(nk)):
                continue
            if all(int(bcols[c][b]) == int(pcols[c][p]) for c in range(nk)):
                out.append((int(p), int(b)))
    return sorted(out)


# ------------------------------------------------------------------ the table-less joins (ops_merge.hip)
def sorted_runs_column(typ, runs=(1, 16, 17, 40)):
    """[(run length, ascending build column)]: the type's edge values, each once, except the lowest and the highest value of the type,
    which hold a run of the given length (16 is the longest run the kernel walks, 17 the shortest it finishes with a search)"""
    edges = I64_EDGES if typ == "i64" else I32_EDGES
    out = []
    for r in runs:
        col = [edges[0]] * r + edges[1:-1] + [edges[-1]] * r
        out.append((r, np.array(col, dtype=_DT[typ])))
    return out


def sorted_probe_column(typ, seed=15):
    edges = I64_EDGES if typ == "i64" else I32_EDGES
    lo, hi = _DOMAIN[typ]
    near = sorted({v + d for v in edges for d in (-1, 1) if lo <= v + d <= hi} - set(edges))
    rng = np.random.default_rng(seed)
    p = np.array((edges + near) * 3, dtype=_DT[typ])
    return rng.permutation(p)
