"""Constructed inputs and a plain reference of the aggregate edge tests (test_gpu_agg_edges.py; checked on their own, without a
device, by test_agg_edges_reference.py).

Every sink form of the hash aggregate decides which group a row belongs to from the widened key words, a NULL mask and two hashes:
keys_hash (the global table's slot and the bulk builds' partition) and lds_hash (the slot in a workgroup's LDS table). Two families of
inputs that random small keys never produce:
  * hash structure: keys_hash folds the bijection mix64 over the columns, so inverting its last step gives the trailing key of ANY
    hash word and a builder decides the global slot and the partition of every key; lds_hash is a 32-bit mix, its slot is found by search;
  * key values at the edges of their domains, tuples that differ in one column, one half or their NULL mask only.
The reference groups by the key VALUES (np.unique over int64): nothing in it hashes."""
import numpy as np

from domain_edges import civil_days
from join_edges import I32_MAX, I32_MIN, I64_MAX, I64_MIN, as_u64, inv_mix64, mix64

# ------------------------------------------------------------------ the two hashes (agg_sink.inc)
KH_SEED = 0x9E3779B97F4A7C15                      # keys_hash: h = mix64(nullmask + KH_SEED); h = mix64(h ^ k[c]) per column
LH_NULL_MUL, LH_MUL1, LH_MUL2 = 0x9E3779B1, 0x85EBCA6B, 0xC2B2AE35   # lds_hash
LH_SHIFT_MID, LH_SHIFT_END = 15, 16

_DT = {"i64": np.int64, "dec64": np.int64, "i32": np.int32, "date": np.int32, "code8": np.uint8}
DATE_LO, DATE_HI = civil_days(1, 1, 1), civil_days(9999, 12, 31)


def _words(cols, nullmask):
    """the key words the kernels hash and compare: every column widened to 64 bits (as_u64), zero where the column is NULL"""
    nm = np.asarray(nullmask, dtype=np.uint64)
    return [np.where((nm >> np.uint64(c)) & np.uint64(1), np.uint64(0), as_u64(k)) for c, k in enumerate(cols)], nm


def keys_hash(cols, nullmask=0):
    """keys_hash of agg_sink.inc over key columns (arrays of their storage type) and a NULL mask (bit c: column c is NULL; a scalar
    or one per row)"""
    k, nm = _words(cols, nullmask)
    with np.errstate(over="ignore"):
        h = mix64(nm + np.uint64(KH_SEED))
    for w in k:
        h = mix64(h ^ w)
    return h


def lds_hash(cols, nullmask=0):
    """lds_hash<NK> of agg_sink.inc: a 32-bit mix over the two halves of every key word, as uint32"""
    k, nm = _words(cols, nullmask)
    u32 = np.uint64(0xFFFFFFFF)
    h = (nm * np.uint64(LH_NULL_MUL)) & u32            # (all arithmetic in uint64, reduced to 32 bits after every step)
    for w in k:
        h = h ^ (w & u32)
        h = (h * np.uint64(LH_MUL1)) & u32
        h = h ^ (((w >> np.uint64(32)) + (h >> np.uint64(LH_SHIFT_MID))) & u32)
        h = (h * np.uint64(LH_MUL2)) & u32
    return (h ^ (h >> np.uint64(LH_SHIFT_END))).astype(np.uint32)


def solve_last_key(prefix_cols, nullmask, wanted_hash):
    """the int64 values of a trailing, non-NULL 8-byte key column that make the tuple (prefix..., value) hash to wanted_hash:
    the last step h = mix64(h_prefix ^ k) inverted"""
    assert not (np.asarray(nullmask) >> len(prefix_cols)).any(), "the solved column is not NULL"
    wanted = np.atleast_1d(np.asarray(wanted_hash, dtype=np.uint64))
    return np.ascontiguousarray(inv_mix64(wanted) ^ keys_hash(prefix_cols, nullmask)).view(np.int64)


# ------------------------------------------------------------------ the layout (ops_agg.hip, agg_sink.inc), restated
PART_SHIFT = 40               # B.shift: partition of a row = (keys_hash >> 40) & (nparts - 1); the two-level form cuts the same bits twice
PART_MAX_BITS = 13            # at most 8192 bins (the second bulk build) / 4096 partitions (the first)
PART_FIXED = (40, 53)         # a builder that fixes hash bits 40..53 fixes the partition at every level of every form
PROBE_WINDOW = 32             # bulk_build_kernel, bulk_lds_find_insert and the sliced bulk2_partial_body give up after 32 probes
SINK_PROBE_WINDOW = 16        # agg_sink_body: probes in the LDS table before a row goes to the global table
DIRECT_PROBE_WINDOW = 256     # bulk2_partial_body<DIRECT>
CHUNK_GUARD = 255             # find_or_create looks at the error flag when (guard & 255) == 255
GLOBAL_SLOT_BITS = 24         # one_global_slot: equal low 24 hash bits = one home slot in every table of up to 2^24 slots
MIN_TABLE = 4096              # smallest global table


def closes_at(T):
    """an LDS table takes no new key once it holds this many"""
    return T - T // 4


def bulk_per_entry(nkeys, naggs):
    return 4 + 8 * nkeys + 8 + 20 * naggs


def bulk_T(nkeys, naggs):
    """LDS entries of a build workgroup of both bulk forms (the two-level form's second level uses half of it)"""
    per, T = bulk_per_entry(nkeys, naggs), 256
    while T * 2 * per <= 120 * 1024 and T < 4096:
        T *= 2
    return T


def bulk1_parts(n, hint, T):
    want, nparts = (hint + T // 4 - 1) // (T // 4), 512 if n >= (4 << 20) else 8
    while nparts < want and nparts < 4096:
        nparts *= 2
    return nparts


def bulk2_bins(hint, T):
    """(bins, two_level) of the second form"""
    want, nparts = (hint + T // 4 - 1) // (T // 4), 16
    while nparts < want:
        nparts *= 2
    return nparts, nparts > 512


BUILD_THREADS = 1024          # a build workgroup takes 1024 records of its partition per step, in record order
BULK2_CHUNK_MAX = 256 * 16    # most rows the second form's scatter stages at once (bu <= 16)


def _round_up(x, m):
    return -(-x // m) * m


def bulk1_scatter_range(n):
    """rows of one scatter workgroup of the first form: the records of a partition are ordered by these ranges, not inside them"""
    return max(1024, _round_up((n + 511) // 512, 256))


def bulk2_scatter_range(n, ch=BULK2_CHUNK_MAX):
    """the same of the second form, for its largest chunk"""
    return max(ch, _round_up((n + 511) // 512, ch))


def replay_lds_inserts(home, T, window=PROBE_WINDOW):
    """the insert rule of the build tables (bulk_build_kernel phase 0, bulk_lds_find_insert, the sliced bulk2_partial_body) replayed
    over distinct keys in the order given, home[j] = lds_hash of key j: linear probing from home & (T - 1), at most `window` occupied
    entries passed, no new key once closes_at(T) are in. Per key ("in", probes), ("window", probes) or ("closed", probes)."""
    taken, nent, out = np.zeros(T, bool), 0, []
    for h in np.asarray(home).tolist():
        idx, probes, res = h & (T - 1), 0, None
        while probes < window:
            if not taken[idx]:
                if nent >= closes_at(T):
                    res = ("closed", probes)
                else:
                    taken[idx], nent, res = True, nent + 1, ("in", probes)
                break
            idx, probes = (idx + 1) & (T - 1), probes + 1
        out.append(res or ("window", probes))
    return out


def sink_per_entry(nkeys, naggs):
    return 12 + 8 * nkeys + 12 * naggs


def sink_slots(nkeys, naggs):
    """LDS slots of the generic pre-aggregating sink"""
    per, slots = sink_per_entry(nkeys, naggs), 64
    while slots * 2 * per <= 32 * 1024 and slots < 1024:
        slots *= 2
    return slots


def spec_per_entry(nkeys, naggs, need_cnt):
    return 12 + 8 * nkeys + 8 * naggs + (4 * naggs if need_cnt else 0)


def spec_slots(nkeys, naggs, need_cnt, hint):
    """LDS slots of the specialised sink: the smallest table (32 KiB .. 144 KiB) the hint fills to 70 % at most, else 32 KiB"""
    per = spec_per_entry(nkeys, naggs, need_cnt)

    def fit(b):
        t = 64
        while t * 2 * per <= b and t < 8192:
            t *= 2
        return t
    b = 32 * 1024
    while b <= 144 * 1024:
        if fit(b) * 7 // 10 >= hint:
            return fit(b)
        b = b * 2 if b < 128 * 1024 else b + 16 * 1024
    return fit(32 * 1024)


def partition_of(h, nparts=1 << (PART_FIXED[1] - PART_FIXED[0] + 1)):
    return (h >> np.uint64(PART_SHIFT)) & np.uint64(nparts - 1)


# ------------------------------------------------------------------ key-domain edge tables
VALUES = [I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX, 12_345, -987_654_321, 10 ** 17]   # the argument of a row is one of these
HALF_X = (1, 7, 0x12345678, 0x7FFFFFFF)       # x, x + 2^32 and x << 32 share their low or their high half only
I64_EDGES = [I64_MIN, I64_MIN + 1, -2 ** 32 - 1, -2 ** 32, -2 ** 31 - 1, -2 ** 31, -1, 0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32,
             2 ** 32 + 1, I64_MAX - 1, I64_MAX]
I32_EDGES = [I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX]
CODE8_EDGES = [0, 1, 127, 128, 254, 255]


def edge_table(typ):
    """the values of one key type every form must keep apart, as Python ints, each once"""
    if typ in ("i64", "dec64"):
        v = I64_EDGES + [y for x in HALF_X for y in (x, x + 2 ** 32, x << 32)]
    elif typ == "i32":
        v = list(I32_EDGES)
    elif typ == "date":
        v = I32_EDGES + [DATE_LO, DATE_HI]
    else:
        v = list(CODE8_EDGES)
    return list(dict.fromkeys(v))


def _lowest(typ):
    return {"i64": I64_MIN, "dec64": I64_MIN, "i32": I32_MIN, "date": I32_MIN, "code8": 128}[typ]


def _minus_one(typ):
    return 255 if typ == "code8" else -1


class Groups:
    """key rows: cols[c][i] is the value of key column c in row i (arrays of the column's storage type) and valid[c][i] says that it is
    not NULL (bytes under a NULL are payload: they must not matter). Several rows may be the same group."""

    def __init__(self, types, cols, valid=None, **info):
        self.types = list(types)
        self.cols = [np.asarray(c, dtype=_DT[t]) for c, t in zip(cols, types)]
        n = len(self.cols[0])
        self.valid = [np.ones(n, bool) if valid is None or v is None else np.asarray(v, bool) for v in (valid or [None] * len(types))]
        self.info = info

    def __len__(self):
        return len(self.cols[0])

    def nullmask(self):
        return sum((~v).astype(np.uint64) << np.uint64(c) for c, v in enumerate(self.valid))

    def hash(self):
        return keys_hash(self.cols, self.nullmask())

    def lds(self):
        return lds_hash(self.cols, self.nullmask())

    def tuples(self):
        """the key tuple of every row, None for NULL"""
        cols = [c.tolist() for c in self.cols]
        val = [v.tolist() for v in self.valid]
        return [tuple(cols[c][i] if val[c][i] else None for c in range(len(cols))) for i in range(len(self))]

    def keep_validity(self, which):
        """the same rows with validity on the columns `which` only: the bytes under the other columns' NULLs become their values"""
        return Groups(self.types, self.cols, [v if c in which else None for c, v in enumerate(self.valid)])

    def concat(self, other):
        assert self.types == other.types
        return Groups(self.types, [np.concatenate([a, b]) for a, b in zip(self.cols, other.cols)],
                      [np.concatenate([a, b]) for a, b in zip(self.valid, other.valid)])


def single_key(typ, values):
    return Groups([typ], [np.array(values, dtype=np.int64).astype(_DT[typ])])


TUPLE_TYPES = [("i32", "i64"), ("i64", "i32"), ("i32", "date", "i64"), ("i64", "code8", "i32", "date"), ("i32", "i32", "i32", "i32")]


def tuple_edges(types, seed=21):
    """key rows of 2 to 4 columns that hold
      * base tuples (a diagonal walk over the columns' edge tables) and, for every column position, tuples that differ from a base
        tuple in exactly that column (another edge value; for an 8-byte column also the base value + 2^32: the high half only);
      * for every pair of positions (i, j) the transposed tuples (.. a .. b ..) and (.. b .. a ..), with (a, b) = (1, 2) and, where
        neither column is CODE8, (-1, 0);
      * all 2^nk NULL patterns over the all-zero tuple and over one base tuple, the all-zero tuple itself included, every pattern in
        three rows whose bytes under the NULLs differ: the type's lowest value, -1 (255), a random value."""
    rng = np.random.default_rng(seed)
    nk = len(types)
    tabs = [edge_table(t) for t in types]
    m = max(len(t) for t in tabs)
    base = list(dict.fromkeys(tuple(tabs[c][(i + s * c) % len(tabs[c])] for c in range(nk)) for i in range(m) for s in (0, 1, 3)))
    rows, valid = [], []

    def put(t, mask=0, payload=None):
        t = list(t)
        for c in range(nk):
            if (mask >> c) & 1:
                t[c] = payload[c]
        rows.append(tuple(t))
        valid.append(tuple(not ((mask >> c) & 1) for c in range(nk)))
    one_col = []
    for t in base:
        put(t)
        for c in range(nk):
            other = tabs[c][(tabs[c].index(t[c]) + 1 + len(one_col) % 3) % len(tabs[c])]
            variants = [other] + ([t[c] + 2 ** 32] if types[c] in ("i64", "dec64") and t[c] + 2 ** 32 <= I64_MAX else [])
            for v in variants:
                u = t[:c] + (v,) + t[c + 1:]
                put(u)
                one_col.append((t, u, c))
    transposed = []
    for i in range(nk):
        for j in range(i + 1, nk):
            for a, b in [(1, 2)] + ([(-1, 0)] if "code8" not in (types[i], types[j]) else []):
                t, u = [0] * nk, [0] * nk
                t[i], t[j], u[i], u[j] = a, b, b, a
                put(t)
                put(u)
                transposed.append((tuple(t), tuple(u)))
    null_base = [tuple([0] * nk), base[len(base) // 2]]
    for t in null_base:
        for mask in range(1 << nk):
            for kind in range(3):
                lo = [np.iinfo(_DT[ty]).min if ty != "code8" else 0 for ty in types]
                hi = [np.iinfo(_DT[ty]).max for ty in types]
                payload = [(_lowest(ty), _minus_one(ty), int(rng.integers(lo[c], hi[c], endpoint=True)))[kind] for c, ty in enumerate(types)]
                put(t, mask, payload)
    cols = [np.array([r[c] for r in rows], dtype=np.int64) for c in range(nk)]
    return Groups(types, cols, [np.array([v[c] for v in valid]) for c in range(nk)],
                  base=base, one_col=one_col, transposed=transposed, null_base=null_base)


# ------------------------------------------------------------------ hash-structure builders
def _rand_u64(rng, n):
    return rng.integers(0, 2 ** 64, n, dtype=np.uint64)


def _set_bits(h, shift, width, value):
    mask = np.uint64(((1 << width) - 1) << shift)
    return (h & ~mask) | ((np.asarray(value, dtype=np.uint64) << np.uint64(shift)) & mask)


def _keys_of(h, two_key, rng):
    """the groups whose keys_hash is h: one PH_I64 key, or (i32 drawn at random over its domain, i64 solved)"""
    if not two_key:
        return Groups(["i64"], [solve_last_key([], 0, h)])
    a = rng.integers(I32_MIN, I32_MAX, len(h), endpoint=True, dtype=np.int64).astype(np.int32)
    a[:4] = [I32_MIN, -1, 0, I32_MAX][: len(a[:4])]
    return Groups(["i32", "i64"], [a, solve_last_key([a], 0, h)])


def one_global_slot(m, victims, seed=31, two_key=False):
    """m distinct keys whose keys_hash agrees in its low 24 bits — ONE home slot, so one probe chain of m slots, in every global table
    of 4096 .. 2^24 slots — followed by `victims` keys whose home slot lies strictly inside that chain (home + 1 .. home + m - 2): they
    walk the rest of it. The home slot is a multiple of 4096 and m < 4096, so neither wraps in any table. info: home (low 24 bits)."""
    assert 2 < m < MIN_TABLE
    rng = np.random.default_rng(seed)
    home = int(rng.integers(0, 1 << (GLOBAL_SLOT_BITS - 12))) << 12
    chain = _set_bits(_rand_u64(rng, m), 0, GLOBAL_SLOT_BITS, home)
    vict = _set_bits(_rand_u64(rng, victims), 0, GLOBAL_SLOT_BITS, home + rng.integers(1, m - 1, victims))
    h = np.concatenate([chain, vict])
    assert len(np.unique(h)) == len(h), "reseed"
    g = _keys_of(h, two_key, rng)
    g.info.update(home=home, m=m, victims=victims)
    return g


def partition_stream(p, n, rng):
    """n hash words of partition p (bits 40..53), every other bit random"""
    return _set_bits(_rand_u64(rng, n), PART_FIXED[0], PART_FIXED[1] - PART_FIXED[0] + 1, p)


def one_partition(m, seed=32, p=None):
    """m distinct PH_I64 keys whose keys_hash bits 40..53 are equal (the partition of both bulk forms, at both levels of the two-level
    form) and whose other hash bits are random. info: partition"""
    rng = np.random.default_rng(seed)
    if p is None:
        p = int(rng.integers(0, 1 << (PART_FIXED[1] - PART_FIXED[0] + 1)))
    h = np.unique(partition_stream(p, m + 16, rng))
    h = rng.permutation(h)[:m]
    assert len(h) == m
    g = _keys_of(h, False, rng)
    g.info.update(partition=p)
    return g


def one_lds_slot(m, bits=13, partition=None, seed=33):
    """m distinct PH_I64 keys whose lds_hash agrees in its low `bits` bits: one slot of every LDS table of up to 2^bits entries. Found
    by search over random int64 keys or, with `partition`, over the keys of that partition (one_partition's stream), so that they
    meet in ONE build workgroup. info: slot, partition"""
    rng = np.random.default_rng(seed)
    per_round = max(1 << 18, int(1.5 * m) << bits)
    if partition is None:
        k = rng.integers(I64_MIN, I64_MAX, per_round, endpoint=True, dtype=np.int64)
    else:
        k = solve_last_key([], 0, partition_stream(partition, per_round, rng))
    k = np.unique(k)
    low = (lds_hash([k]) & np.uint32((1 << bits) - 1)).astype(np.int64)
    slot = int(np.argmax(np.bincount(low, minlength=1 << bits)))
    k = rng.permutation(k[low == slot])[:m]
    assert len(k) == m, "too few candidates (reseed)"
    return Groups(["i64"], [k], slot=slot, partition=partition)


# ------------------------------------------------------------------ rows
class Rows:
    """n rows over the key rows of a Groups object: row i holds key row src[i]; its argument is VALUES[kind[i]], NULL where arg_valid[i]
    is False; bytes under a NULL key change from one row of a key row to its next (the lowest value, -1, a random one)"""

    def __init__(self, groups, src, kind, arg_valid, cols):
        self.groups, self.src, self.kind, self.arg_valid, self.cols = groups, src, kind, arg_valid, cols
        self.valid = [v[src] for v in groups.valid]
        self.types = groups.types
        self.n = len(src)

    def args(self):
        return np.array(VALUES, np.int64)[self.kind]


def rows_of(groups, n, seed=41, dup=3):
    """n rows over the key rows of `groups`: every key row at least dup times, the rest drawn at random, in shuffled order. The first
    key row takes only INT64_MIN, the second only INT64_MAX, the third alternates the two, every argument of the fourth is NULL; the
    others draw from VALUES with a tenth of NULLs."""
    rng = np.random.default_rng(seed)
    g = len(groups)
    assert n >= dup * g
    src = rng.permutation(np.concatenate([np.tile(np.arange(g), dup), rng.integers(0, g, n - dup * g)]))
    kind = rng.integers(0, len(VALUES), n)
    arg_valid = rng.random(n) > 0.1
    kind[src == 0] = 0
    if g > 1:
        kind[src == 1] = 6
    if g > 2:
        at = np.flatnonzero(src == 2)
        kind[at] = np.where(np.arange(len(at)) % 2 == 0, 6, 0)
        arg_valid[at] = True
    if g > 3:
        arg_valid[src == 3] = False
    order = np.argsort(src, kind="stable")       # rank[i]: how many earlier rows hold the same key row
    starts = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=g))[:-1]])
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n) - starts[src[order]]
    cols = []
    for c, t in enumerate(groups.types):
        col = groups.cols[c][src]
        null = ~groups.valid[c][src]
        k = int(null.sum())
        if k:
            lo, hi = (0, 255) if t == "code8" else (np.iinfo(_DT[t]).min, np.iinfo(_DT[t]).max)
            junk = rng.integers(lo, hi, k, endpoint=True, dtype=np.int64)
            junk = np.where(rank[null] % 3 == 0, _lowest(t), np.where(rank[null] % 3 == 1, _minus_one(t), junk))
            col[null] = junk.astype(_DT[t])
        cols.append(col)
    return Rows(groups, src, kind, arg_valid, cols)


def tiled(groups, n, seed=42, dup=3):
    """the big shapes: a block of rows_of(groups, dup x len(groups)) tiled out to n rows with np.tile, the tail cut, then shuffled"""
    rng = np.random.default_rng(seed)
    b = rows_of(groups, dup * len(groups), seed, dup)
    take = rng.permutation(np.tile(np.arange(b.n), -(-n // b.n))[:n])
    return Rows(groups, b.src[take], b.kind[take], b.arg_valid[take], [c[take] for c in b.cols])


TILE_FROM = 1_000_000         # shapes of this many rows or more are a tiled block


def probe_window_rows(m, n, p=1234, dup=50, seed=44):
    """the input of the 32-probe window: m keys of partition p that share ONE slot of the partition's LDS table (key rows 0 .. m - 1) and
    2000 ordinary groups of the same partition, every key at least dup times — LED by a block of rows that cycle through the m same-slot
    keys only. The block is as long as the longest range one scatter workgroup takes at n rows in either bulk form, so whatever order
    the scatter leaves inside a range, the first records of the partition — the first steps of its build workgroup, 1024 records each —
    hold the same-slot keys alone: they meet in an EMPTY table, 32 of them fill the window and the others find it exhausted long
    before 2000 ordinary keys close the table. info: m, lead"""
    g = one_lds_slot(m, partition=p).concat(one_partition(2000, p=p))
    assert len(set(g.tuples())) == m + 2000
    lead = max(bulk1_scatter_range(n), bulk2_scatter_range(n) if n >= (4 << 20) else 0)
    rest = (tiled if n >= TILE_FROM else rows_of)(g, n - lead, seed, dup)
    rng = np.random.default_rng(seed + 1)
    src = np.arange(lead) % m
    rows = Rows(g, np.concatenate([src, rest.src]), np.concatenate([rng.integers(0, len(VALUES), lead), rest.kind]),
                np.concatenate([rng.random(lead) > 0.1, rest.arg_valid]), [np.concatenate([g.cols[0][src], rest.cols[0]])])
    g.info.update(m=m, lead=lead)
    return rows


# ------------------------------------------------------------------ the reference: the key values, no hashing
def widened(col):
    col = np.asarray(col)
    return col.astype(np.int64)          # (uint8 zero-extends, int32 sign-extends)


def _group_ids(key_cols, validities, rows):
    """(unique key matrix [groups, nk + 1] with the NULL mask as last column, group of every row in `rows`)"""
    nk = len(key_cols)
    M = np.zeros((len(rows), nk + 1), np.int64)
    for c in range(nk):
        k = widened(key_cols[c])[rows]
        if validities is not None and validities[c] is not None:
            v = np.asarray(validities[c], bool)[rows]
            k = np.where(v, k, 0)
            M[:, nk] |= (~v).astype(np.int64) << c
        M[:, c] = k
    if nk == 1 and not M[:, 1].any():     # one column without NULLs: the same unique, over a vector
        u, inv = np.unique(M[:, 0], return_inverse=True)
        return np.stack([u, np.zeros(len(u), np.int64)], 1), inv.reshape(-1)
    u, inv = np.unique(M, axis=0, return_inverse=True)
    return u, inv.reshape(-1)


def group_reference(key_cols, validities, kind, valid, sel=None, row_base=0, src=None):
    """{key tuple with None for NULL: (first row, sum, count of non-NULL arguments, min, max, rows)} of the rows sel (all rows; a
    selection must ascend) — the argument of row r is VALUES[kind[r]], NULL where valid[r] is False. Sums are Python integers; numpy
    only counts how often each of VALUES occurs in each group.
    src: a promise that the key tuples of rows i and j are equal where src[i] == src[j] (rows_of / tiled: copies of one key row) —
    then np.unique runs over one row per value of src; it is verified on a sample."""
    n = len(key_cols[0])
    rows = np.arange(n, dtype=np.int64) if sel is None else np.asarray(sel, dtype=np.int64)
    nk = len(key_cols)
    if src is None:
        u, inv = _group_ids(key_cols, validities, rows)
    else:
        s = np.asarray(src)[rows]
        us, at, sinv = np.unique(s, return_index=True, return_inverse=True)
        u, ginv = _group_ids(key_cols, validities, rows[at])
        inv = ginv[sinv.reshape(-1)]
        probe = rows[:: max(1, len(rows) // 20_000)]
        pu, pinv = _group_ids(key_cols, validities, probe)
        uidx = {tuple(r): i for i, r in enumerate(u.tolist())}
        assert np.array_equal(np.array([uidx.get(tuple(r), -1) for r in pu.tolist()])[pinv], inv[:: max(1, len(rows) // 20_000)]), "src lies"
    G, K = len(u), len(VALUES)
    first = np.empty(G, np.int64)
    first[inv[::-1]] = rows[::-1]                      # the last write per group is its earliest row
    kd, ok = np.asarray(kind)[rows], np.asarray(valid, bool)[rows]
    cnt = np.bincount(inv[ok] * K + kd[ok], minlength=G * K).reshape(G, K).tolist()
    nrows = np.bincount(inv, minlength=G).tolist()
    out = {}
    for g, r in enumerate(u.tolist()):
        key = tuple(None if (r[nk] >> c) & 1 else r[c] for c in range(nk))
        seen = [VALUES[j] for j in range(K) if cnt[g][j]]
        out[key] = (int(first[g]) + row_base, sum(c * v for c, v in zip(cnt[g], VALUES)), sum(cnt[g]), min(seen, default=None),
                    max(seen, default=None), nrows[g])
    return out


def loop_reference(key_cols, validities, kind, valid, sel=None, row_base=0):
    """the same by a plain double loop (for a few hundred rows)"""
    n, nk = len(key_cols[0]), len(key_cols)
    rows = list(range(n)) if sel is None else [int(r) for r in sel]
    keys = [tuple(None if validities is not None and validities[c] is not None and not validities[c][r] else int(key_cols[c][r])
                  for c in range(nk)) for r in rows]
    out = {}
    for i, r in enumerate(rows):
        if keys[i] in out:
            continue
        mine = [q for j, q in enumerate(rows) if keys[j] == keys[i]]
        vals = [VALUES[int(kind[q])] for q in mine if valid[q]]
        out[keys[i]] = (r + row_base, sum(vals), len(vals), min(vals, default=None), max(vals, default=None), len(mine))
    return out
