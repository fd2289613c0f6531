"""ORDER BY at the seams of ph_sort_rows' own structure (plan_amd/csrc/ops_sort.hip): the inputs, the exact reference and a model of the
kernel's passes. No device and no plan_amd import here; test_sort_edges_reference.py proves on the CPU that every corpus reaches the edge
it is named for, test_gpu_sort_edges.py sorts them on the device.

`order` is the reference: NULLs first in either direction, DESC reverses values only, ties keep their position in the selection. It is
written twice (one `sorted` over key tuples; a byte-walking comparator) and the CPU test holds the two against each other.

`radix_plan`, `refine_plan` and `word_path` restate what the kernel does (which bytes get a pass, how many candidates and segments a
refinement round has, which load path a word takes). They are used only to assert that a corpus reaches its edge: results are always compared
with `order`.

A numeric column is a NumCol (type name, numpy values, scale, bool validity or None); a VARCHAR column is a StrCol (int32 offsets, uint8
bytes, bool validity or None, and the strings as Python bytes / None)."""
import functools
from collections import namedtuple

import numpy as np

from domain_edges import cents_half_even

SORT_TILE, SORT_CHUNK = 256, 4096      # SORT_TILE and SORT_TILE * SORT_TILES_PER_WG of ops_sort.hip
M64 = (1 << 64) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

NumCol = namedtuple("NumCol", "type values scale valid")
StrCol = namedtuple("StrCol", "off data valid strings")
NP_OF = {"I32": np.int32, "DATE": np.int32, "CODE8": np.uint8, "DEC64": np.int64}


def num(typ, values, scale=0, valid=None):
    return NumCol(typ, np.ascontiguousarray(values, dtype=NP_OF[typ]), scale, None if valid is None else np.asarray(valid, dtype=bool))


def pack(strings):
    """a StrCol laid out like hip.str_column: the strings back to back from offset 0, NULL rows empty"""
    lens = [0 if s is None else len(s) for s in strings]
    off = np.zeros(len(strings) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    data = np.frombuffer(b"".join(s for s in strings if s is not None), np.uint8)
    valid = np.array([s is not None for s in strings], bool)
    return StrCol(off.astype(np.int32), data, None if valid.all() else valid, list(strings))


def pykeys(col):
    """the column as `order` takes it: None, a Python int (DECIMAL: cents, half-even) or bytes per row id"""
    if isinstance(col, StrCol):
        return col.strings
    vals = col.values.tolist()
    if col.type == "DEC64":
        vals = [cents_half_even(v, col.scale) for v in vals]
    if col.valid is None:
        return vals
    return [v if ok else None for v, ok in zip(vals, col.valid.tolist())]


# ------------------------------------------------------------------ the reference

def _sort_value(v, desc):
    if v is None:
        return (0,)
    if isinstance(v, bytes):
        # DESC over bytes: every byte reversed, and a terminator above all of them so that an extension comes before its prefix
        return (1, tuple(255 - b for b in v) + (256,)) if desc else (1, v)
    return (1, -v if desc else v)


def order(rows, keys, desc):
    """rows (the selection, in input order; may repeat, may be unsorted) sorted by keys[c][row] with directions desc[c]: NULLs first in
    either direction, DESC reverses values only, ties by position in `rows`"""
    rows = list(rows)
    return [rows[pos] for pos in order_positions(rows, keys, desc)]


def order_positions(rows, keys, desc):
    """`order` as positions in `rows`"""
    tagged = sorted((tuple(_sort_value(k[r], d) for k, d in zip(keys, desc)), pos) for pos, r in enumerate(rows))
    return [pos for _, pos in tagged]


def _cmp_values(a, b):
    if isinstance(a, bytes):
        for i in range(min(len(a), len(b))):
            x, y = a[i], b[i]          # indexing bytes gives 0..255: unsigned
            if x != y:
                return -1 if x < y else 1
        return (len(a) > len(b)) - (len(a) < len(b))    # a proper prefix first
    return (a > b) - (a < b)


def comparator(rows, keys, desc):
    """the order stated a second time, independently, as a comparator of two positions in `rows`: it walks the keys, and bytes keys byte by
    byte; the position decides last"""
    rows = list(rows)

    def cmp(p, q):
        for k, d in zip(keys, desc):
            a, b = k[rows[p]], k[rows[q]]
            if a is None or b is None:
                c = (b is None) - (a is None)           # NULL first, whatever the direction
            else:
                c = _cmp_values(a, b)
                if d:
                    c = -c
            if c:
                return c
        return (p > q) - (p < q)
    return cmp


def order_by_comparator(rows, keys, desc):
    rows = list(rows)
    return [rows[p] for p in sorted(range(len(rows)), key=functools.cmp_to_key(comparator(rows, keys, desc)))]


# ------------------------------------------------------------------ the structural model

def word_of(s, j):
    """word j of a string: bytes 8j..8j+7 big-endian, zero past the end"""
    return int.from_bytes(s[8 * j:8 * j + 8].ljust(8, b"\0"), "big")


def key_words(col, desc, rows=None):
    """(normalised 64-bit key word, NULL digit) per selected row, as sort_norm_kernel writes them: value XOR sign bit (a VARCHAR's word 0
    as it is), inverted for DESC, 0 for NULL; digit 0 = NULL, 1 = value"""
    n = len(col.off) - 1 if isinstance(col, StrCol) else len(col.values)
    rows = range(n) if rows is None else rows
    if isinstance(col, StrCol):
        raw = [None if s is None else word_of(s, 0) for s in col.strings]
    else:
        vals = col.values.tolist()
        if col.type == "DEC64" and col.scale > 2:
            vals = [cents_half_even(v, col.scale) for v in vals]      # round_cents; at scale <= 2 the value itself is the key
        raw = [((v & M64) ^ (1 << 63)) for v in vals]
        if col.valid is not None:
            raw = [k if ok else None for k, ok in zip(raw, col.valid.tolist())]
    out = []
    for r in rows:
        k = raw[r]
        out.append((0, 0) if k is None else ((~k & M64) if desc else k, 1))
    return out


def radix_plan(col, desc=False, rows=None):
    """the passes of a one-word column (the file header of ops_sort.hip, sort_diff_kernel): (set of key bytes that vary = the byte passes
    that run, whether the NULL flag varies = whether the pass over it runs)"""
    kw = key_words(col, desc, rows)
    k0, f0 = kw[0]
    d = dn = 0
    for k, f in kw:
        d |= k ^ k0
        dn |= f ^ f0
    return {b for b in range(8) if (d >> (8 * b)) & 0xFF}, bool(dn)


def _runs(*arrays):
    """head flags and run sizes (per element) of the runs of equal tuples in parallel arrays"""
    m = len(arrays[0])
    head = np.ones(m, bool)
    if m > 1:
        same = np.ones(m - 1, bool)
        for a in arrays:
            same &= a[1:] == a[:-1]
        head[1:] = ~same
    run = np.cumsum(head) - 1
    return head, np.bincount(run)[run]


def refine_plan(strings, desc=False):
    """The refinement rounds of a VARCHAR column given in position order (the selection applied), restated: one dict per round j = 1, 2, ...
    with m (candidates), segments, word_bytes (the bytes of word j that vary), e_varies, seg_bytes (the bytes of the segment id that vary), skipped (word j and e_j equal everywhere: no pass runs), lone (rows whose string goes on but whose segment
    has no second row: dropped), and rows (the candidates' positions in `strings`, in the order the round receives them). The list ends with
    the last round that has candidates."""
    flag = np.array([s is not None for s in strings], np.uint8)
    w0 = np.array([0 if s is None else word_of(s, 0) for s in strings], np.uint64)
    if desc:
        w0 = np.where(flag == 1, ~w0, w0)
    lens = np.array([0 if s is None else len(s) for s in strings], np.int64)
    cont = 0 if desc else 17
    o = np.lexsort((w0, flag))                        # stable, NULL flag most significant
    head, size = _runs(flag[o], w0[o])
    act = (flag[o] == 1) & (size >= 2)
    cand = o[act]
    seg = np.cumsum(head & act)[act] - 1
    rounds = []
    j = 1
    while len(cand):
        w = np.array([word_of(strings[r], j) for r in cand.tolist()], np.uint64)
        e = np.minimum(lens[cand] - 8 * (j - 1), 17)
        if desc:
            w, e = ~w, 17 - e
        his = (seg.astype(np.uint64) << np.uint64(8)) | e.astype(np.uint64)
        dk = int(np.bitwise_or.reduce(w)) ^ int(np.bitwise_and.reduce(w))
        dh = int(np.bitwise_or.reduce(his)) ^ int(np.bitwise_and.reduce(his))
        top = [b for b in range(4) if (dh >> (8 + 8 * b)) & 0xFF]
        o = np.lexsort((e, w, seg))
        head, size = _runs(seg[o], w[o], e[o])
        goes_on = e[o] == cont
        act = goes_on & (size >= 2)
        rounds.append(dict(m=len(cand), segments=int(seg.max()) + 1, word_bytes={b for b in range(8) if (dk >> (8 * b)) & 0xFF},
                           e_varies=bool(dh & 0xFF), seg_bytes=set(top), skipped=dk == 0 and (dh & 0xFF) == 0,
                           lone=int((goes_on & (size == 1)).sum()), rows=cand.tolist(), words=w.tolist(), e=e.tolist()))
        cand = cand[o][act]
        seg = np.cumsum(head & act)[act] - 1
        j += 1
    return rounds


def word_path(off, nbytes, base_misalign, r, j):
    """how str_word loads word j of row r: (path, sh, rest). path is None when the word lies past the string (no load), "aligned" for the
    two funnel-shifted 8-byte loads (the byte buffer's base 8-byte aligned and both loads inside it), "bytes" for the byte loads; sh is the
    funnel shift in bits, rest the string's bytes from the word's start on (< 8: the aligned path masks)"""
    s = int(off[r])
    rest = int(off[r + 1]) - s - 8 * j
    start = s + 8 * j
    a0 = start & ~7
    sh = (start - a0) * 8
    if rest <= 0:
        return None, sh, rest
    return ("aligned" if base_misalign % 8 == 0 and a0 + 16 <= nbytes else "bytes"), sh, rest


# ------------------------------------------------------------------ selections

SEL_KINDS = ("none", "ascending", "descending", "shuffled", "repeated")


def selections(n, seed=0):
    """{kind: row list or None}: no selection; an ascending half; the same half descending; all rows shuffled; 2 * (n // 3) entries in which
    every chosen row stands twice, never next to itself (left out below 6 rows, where there are no two rows to choose)"""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    half = np.sort(rng.choice(n, max(1, n // 2), replace=False))
    out = {"none": None, "ascending": half.tolist(), "descending": half[::-1].tolist(), "shuffled": rng.permutation(n).tolist()}
    k = n // 3
    if k >= 2:
        chosen = rng.choice(n, k, replace=False)
        a, b = rng.permutation(chosen), rng.permutation(chosen)
        if a[-1] == b[0]:
            b = np.roll(b, 1)
        out["repeated"] = a.tolist() + b.tolist()
    return out


# ------------------------------------------------------------------ numeric corpora

SEAM_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 3 * 4096 + 1)
LAYOUTS = ("a", "b", "c", "d", "e", "f")
E_BASE, E_ODD = 7, (200, 3, 9)      # layout (e): one digit everywhere, three other digits in the last three rows


def layout_min_rows(kind):
    """the smallest seam size that can hold the layout: (a) a whole tile of 256 digits; (b) two waves; (c), (d) two rows; (e) a row besides
    the three; (f) any"""
    return {"a": 256, "b": 65, "c": 2, "d": 2, "e": 4, "f": 1}[kind]


def digit_layout(kind, n):
    """the digits (0..255) of n rows, as int32 values; see the list in the module's corpus table"""
    rng = np.random.default_rng(ord(kind) * 100_003 + n)
    i = np.arange(n)
    if kind == "a":      # every tile holds all 256 digits once, in shuffled order (the last, partial tile: the start of such a tile)
        d = np.concatenate([rng.permutation(256) for _ in range((n + 255) // 256)])[:n]
    elif kind == "b":    # each wave of a tile holds one digit; the four waves of a tile differ, and a digit comes back 7 waves later
        d = ((i // 64) * 3 % 7) * 36 + 2
    elif kind == "c":    # two digits alternating by lane
        d = np.where(i & 1, 3, 200)
    elif kind == "d":    # digits 0x00 and 0xFF only
        d = rng.choice(np.array([0x00, 0xFF]), n)
        d[:2] = (0xFF, 0x00)
    elif kind == "e":    # one digit everywhere but in the last three rows: in the last (partial) tile where it has three rows, else across its seam
        d = np.full(n, E_BASE)
        d[n - 3:] = E_ODD
    else:                # one digit everywhere: no pass runs
        d = np.full(n, 0x5A)
    return np.asarray(d, np.int32)


def tie_key(n, seed, values=(-1, 0, 1)):
    """a tie-heavy key: three distinct values, random"""
    return np.random.default_rng(77 + seed * 131 + n).choice(np.array(values), n).astype(np.int32)


@functools.lru_cache(maxsize=None)
def digit_cases(kind):
    """[(name, columns, directions)] of one digit layout at every seam size that can hold it: alone ASC and DESC, and, (a)-(e), with a
    3-valued key behind it so that stability across the seams decides the result"""
    out = []
    for n in SEAM_SIZES:
        if n < layout_min_rows(kind):
            continue
        first = num("I32", digit_layout(kind, n))
        out.append((f"layout {kind} n={n}", [first], [False]))
        out.append((f"layout {kind} n={n} desc", [first], [True]))
        if kind != "f":
            # the first and the last row of one digit (the last row's where it has a twin) get tie-key values against their positions, so
            # that the tie key, not the position, orders at least this pair; the negated key does the same descending
            t, d = tie_key(n, ord(kind)), first.values.tolist()
            count = np.bincount(d, minlength=256)
            twin = next((v for v in [d[-1]] + d if count[v] >= 2), None)
            if twin is not None:
                t[d.index(twin)], t[n - 1 - d[::-1].index(twin)] = 1, -1
            out.append((f"layout {kind} n={n} + tie key", [first, num("I32", t)], [False, False]))
            out.append((f"layout {kind} n={n} desc + tie key desc", [first, num("I32", -t)], [True, True]))
    return out


N_BYTES = 4097
DEC_BASE = 0x0102030405060708


def varying_byte_column(b, n=N_BYTES):
    """PH_DEC64 scale 0 whose 64-bit value varies in byte b only (b = 7: the sign bit among them)"""
    rng = np.random.default_rng(900 + b)
    v = rng.integers(0, 256, n, dtype=np.uint64)
    v[:2] = (0x00, 0xFF)
    u = (np.uint64(DEC_BASE & ~(0xFF << (8 * b))) | (v << np.uint64(8 * b)))
    return num("DEC64", u.view(np.int64))


def varying_two_bytes_column(n=N_BYTES):
    """PH_DEC64 scale 0 that varies in bytes 0 and 5 only"""
    rng = np.random.default_rng(950)
    lo, hi = rng.integers(0, 4, n, dtype=np.uint64), rng.integers(0, 4, n, dtype=np.uint64)
    u = np.uint64(DEC_BASE & ~0x0000FF00000000FF) | lo | (hi << np.uint64(40))
    return num("DEC64", u.view(np.int64))


def mixed_sign_column(n=N_BYTES):
    """PH_I32 of both signs: the sign extension makes bytes 4..7 of the key word vary as well"""
    rng = np.random.default_rng(960)
    v = rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64)
    v[rng.integers(0, n, n // 4)] = -5          # ties
    v[rng.integers(0, n, n // 4)] = 5
    return num("I32", v)


def null_mask(n, seed, share=0.1):
    valid = np.random.default_rng(seed).random(n) >= share
    valid[1], valid[2] = True, False             # both kinds present; row 0 keeps a value
    valid[0] = True
    return valid


@functools.lru_cache(maxsize=None)
def byte_cases():
    """[(name, columns, directions, expectation)] at n = 4097; expectation = (column index, directions it holds for, varying bytes,
    NULL flag varies) for radix_plan, or None"""
    n = N_BYTES
    tie = num("I32", tie_key(n, 1))
    out = []
    for b in range(8):
        c = varying_byte_column(b)
        out.append((f"byte {b} only", [c], [False], (0, {b}, False)))
        out.append((f"byte {b} only desc + tie key", [c, tie], [True, False], (0, {b}, False)))
    c = varying_two_bytes_column()
    out.append(("bytes 0 and 5", [c], [False], (0, {0, 5}, False)))
    out.append(("bytes 0 and 5 desc + tie key", [c, tie], [True, True], (0, {0, 5}, False)))
    c = mixed_sign_column()
    out.append(("mixed sign", [c], [False], (0, set(range(8)), False)))
    out.append(("mixed sign desc + tie key", [c, tie], [True, False], (0, set(range(8)), False)))
    # constant columns as first, middle and last of three keys. `only the NULL flag varies` needs a value whose key word is 0 like a NULL's:
    # INT64_MIN ascending, INT64_MAX descending (PH_DEC64, scale 0)
    a, bcol = num("I32", tie_key(n, 2, (-7, 0, 7, 1 << 20, -(1 << 20)))), num("CODE8", np.random.default_rng(3).integers(0, 4, n))
    consts = (("constant", num("I32", np.full(n, 1234)), False, (set(), False)),
              ("constant with NULLs", num("I32", np.full(n, 1234), valid=null_mask(n, 4)), False, None),
              ("NULL flag only", num("DEC64", np.full(n, I64_MIN), valid=null_mask(n, 5)), False, (set(), True)),
              ("NULL flag only desc", num("DEC64", np.full(n, I64_MAX), valid=null_mask(n, 6)), True, (set(), True)))
    for name, c, d, exp in consts:
        for where, at, cols, desc in (("first", 0, [c, a, bcol], [d, False, True]), ("middle", 1, [a, c, bcol], [True, d, False]),
                                      ("last", 2, [a, bcol, c], [False, False, d])):
            out.append((f"{name} as {where} key", cols, desc, None if exp is None else (at,) + exp))
    v = np.full(n, 0x00010001)
    v[0] = 0x00020002
    c = num("I32", v)
    out.append(("only row 0 differs", [c], [False], (0, {0, 2}, False)))
    out.append(("only row 0 differs desc + tie key", [c, tie], [True, False], (0, {0, 2}, False)))
    valid = np.ones(n, bool)
    valid[0] = False
    c = num("I32", np.full(n, 0x00010001), valid=valid)   # keys[0] = 0: every non-zero byte of the other rows' word looks varying
    out.append(("row 0 NULL, constant otherwise", [c], [False], (0, {0, 2, 7}, True)))
    out.append(("row 0 NULL, constant otherwise desc + tie key", [c, tie], [True, True], (0, set(range(8)), True)))
    return out


@functools.lru_cache(maxsize=None)
def eight_keys():
    """(columns, directions) at n = 4097: eight keys of 2-4 distinct values each, mixed types and directions; 2304 combinations over 4097 rows,
    so every key breaks ties and ties remain after the last"""
    n = N_BYTES
    rng = np.random.default_rng(8)
    pick = lambda vals: rng.choice(np.array(vals), n)
    s = [(b"ab", b"abc", b"ab\x00", b"b")[i] for i in rng.integers(0, 4, n).tolist()]
    cols = [num("I32", pick([-1, 0, 1])), num("DATE", pick([8000, 9000])), num("CODE8", pick([0, 1, 128, 255])),
            num("DEC64", pick([-5, 5]), 0), num("DEC64", pick([10_000, 1_234_550, 1_234_650, 2_000_000]), 4), pack(s),
            num("I32", pick([-(1 << 31), (1 << 31) - 1])), num("CODE8", pick([3, 4]))]
    return cols, [True, False, True, False, True, True, False, True]


# ------------------------------------------------------------------ VARCHAR corpora

def _nul_free(rng, k):
    return bytes(rng.integers(1, 256, k, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def many_segments(nseg=70_000):
    """nseg distinct 8-byte prefixes with two rows each, a random tail of 1..8 bytes per row, rows shuffled: round 1 has 2 nseg candidates in
    nseg segments. 70 000 segments make bytes 0, 1 and 2 of the segment id vary (shifts 72, 80 and 88), 300 and 1 000 pin the first byte
    boundary. Byte 3 of the segment id (shift 96) needs more than 2^24 segments of two rows, over 33 M rows: out of scope here."""
    rng = np.random.default_rng(nseg)
    pre = np.unique(rng.integers(0, 1 << 64, nseg + nseg // 8, dtype=np.uint64))
    pre = rng.permutation(pre)[:nseg]
    assert len(pre) == nseg
    tails = rng.integers(0, 256, (2 * nseg, 8), dtype=np.uint8)
    tlen = rng.integers(1, 9, 2 * nseg).tolist()
    strings = []
    for r in rng.permutation(2 * nseg).tolist():
        strings.append(int(pre[r // 2]).to_bytes(8, "big") + tails[r].tobytes()[:tlen[r]])
    return pack(strings)


@functools.lru_cache(maxsize=None)
def trailing_nul(base_len=21):
    """a NUL-free base followed by t NUL bytes, t = 0..40, each string twice, shuffled. The zero-padded words of all rows are equal: only
    e_j, the length, orders them. base_len = 21: several rounds deep; base_len = 5: the family ties inside the first word"""
    rng = np.random.default_rng(2100 + base_len)
    base = _nul_free(rng, base_len)
    strings = [base + b"\x00" * t for t in range(41) for _ in range(2)]
    return pack([strings[i] for i in rng.permutation(len(strings)).tolist()])


@functools.lru_cache(maxsize=None)
def deep_prefix():
    """600 rows sharing a 256-byte prefix, tails of 0..19 random bytes: rounds 1..30 are skipped, round 31 has only e_j varying (the rows
    that end with the prefix), round 32 compares the tails"""
    rng = np.random.default_rng(256)
    pre = _nul_free(rng, 256)
    tl = rng.integers(0, 20, 600)
    tl[:4] = (0, 0, 19, 1)
    return pack([pre + bytes(rng.integers(0, 256, int(k), dtype=np.uint8)) for k in tl.tolist()])


@functools.lru_cache(maxsize=None)
def deep_prefix_two_groups():
    """(StrCol, rows of the equal group): two 100-byte prefixes that share their first 8 bytes; 300 identical strings on one, 300 strings on
    the other that vary from byte 64 on: round 8 has equal candidates in one segment and varying ones in the other"""
    rng = np.random.default_rng(257)
    first = _nul_free(rng, 8)
    pa, pb = first + _nul_free(rng, 92), first + _nul_free(rng, 92)
    if pa[8] == pb[8]:
        pb = pb[:8] + bytes([pb[8] ^ 0x55 or 1]) + pb[9:]
    strings = [pa] * 300 + [pb[:64] + bytes(rng.integers(0, 256, int(k), dtype=np.uint8)) for k in rng.integers(1, 30, 300).tolist()]
    p = rng.permutation(600).tolist()
    return pack([strings[i] for i in p]), [pos for pos, i in enumerate(p) if i < 300]


ROUND_M = (2, 255, 256, 257, 4096, 4097)


@functools.lru_cache(maxsize=None)
def round_sizes(m):
    """6 000 rows with distinct first words plus exactly m planted rows that share one first word and word 1 and differ in word 2 only,
    shuffled: rounds 1 and 2 have m candidates inside a larger n (the compaction and the pass grid at their seams)"""
    rng = np.random.default_rng(6000 + m)
    firsts = np.unique(rng.integers(1, 1 << 62, 6100, dtype=np.int64))[:6001]
    assert len(firsts) == 6001
    firsts = rng.permutation(firsts)
    w2 = np.unique(rng.integers(0, 1 << 62, m + 64, dtype=np.int64))
    assert len(w2) >= m
    w2 = rng.permutation(w2)[:m]
    planted = int(firsts[6000]).to_bytes(8, "big") + b"word one"
    strings = [int(f).to_bytes(8, "big") + _nul_free(rng, int(k)) for f, k in zip(firsts[:6000].tolist(), rng.integers(0, 12, 6000).tolist())]
    strings += [planted + int(x).to_bytes(8, "big") for x in w2.tolist()]
    return pack([strings[i] for i in rng.permutation(len(strings)).tolist()])


@functools.lru_cache(maxsize=None)
def lone_survivor():
    """Five segments of one 40-byte string and its proper prefixes cut at 8j-1, 8j, 8j+1 (j = 1..4); four segments of a 40-byte string and
    one prefix cut at 8j, where from round j on the long string goes on alone and is dropped; whole strings of length 0, 1, 8, 16, 17 and 24
    five times each, which must keep their earlier order. Shuffled."""
    rng = np.random.default_rng(40)
    strings = []
    for _ in range(5):
        s = _nul_free(rng, 40)
        strings += [s] + [s[:8 * j + d] for j in range(1, 5) for d in (-1, 0, 1)]
    for j in range(1, 5):
        s = _nul_free(rng, 40)
        strings += [s, s[:8 * j]]
    for k in (0, 1, 8, 16, 17, 24):
        strings += [_nul_free(rng, k)] * 5
    return pack([strings[i] for i in rng.permutation(len(strings)).tolist()])


@functools.lru_cache(maxsize=None)
def null_neighbours():
    """NULLs next to the strings whose key word is 0 like a NULL's: empty and NUL strings ascending, 0xFF strings descending; 20 of each"""
    rng = np.random.default_rng(20)
    kinds = [None, b"", b"\x00", b"\x00" * 8, b"\xff" * 8, b"\xff" * 9, b"\xff" * 16]
    strings = [k for k in kinds for _ in range(20)]
    return pack([strings[i] for i in rng.permutation(len(strings)).tolist()])


SWEEP_PARTS = ((0, 8), (9, 17))


@functools.lru_cache(maxsize=None)
def alignment_sweep(part):
    """(StrCol, [(a, L, row x, row y)]): for every start alignment a in 0..7 and length L of the part, two strings that share all but their
    last byte (L = 0: two empty strings), each starting at an offset = a (mod 8) behind a filler row of the length that needs (1..8 bytes).
    A filler's first byte is its own (0x01..0x92), so it never ties; the pairs start with 0xA0 + a. 288 fillers would need more first bytes
    than there are, so the sweep comes in two parts of 72 pairs: L = 0..8 and L = 9..17. One pair stands a second time at the end of each
    part: (a = 3, L = 4) in part 0, both of whose strings then lie in the last 16 bytes of the buffer and take the byte path, and
    (a = 7, L = 9) in part 1, whose deciding last byte is the buffer's last."""
    lo, hi = SWEEP_PARTS[part]
    rng = np.random.default_rng(300 + part)
    todo = [(a, L) for a in range(8) for L in range(lo, hi + 1)]
    final = (3, 4) if part == 0 else (7, 9)
    todo.append(final)      # once more at the end: the first time it takes the aligned path like the others
    strings, pairs, pos, fill = [], [], 0, 0
    for a, L in todo:
        body = bytes([0xA0 + a]) + bytes([L]) + _nul_free(rng, 16)
        x = body[:L]
        y = x[:-1] + bytes([x[-1] ^ 0x08]) if L else x
        rows = []
        for s in (x, y):
            need = (a - pos) % 8 or 8
            fill += 1
            strings.append(bytes([fill]) + b"\xee" * (need - 1))      # non-zero bytes behind short strings: an unmasked load would read them
            pos += need
            assert pos % 8 == a
            rows.append(len(strings))
            strings.append(s)
            pos += L
        pairs.append((a, L, rows[0], rows[1]))
    assert fill == 2 * len(todo) == 146
    return pack(strings), pairs


TINY_BYTES = (1, 7, 8, 15, 16, 17)


@functools.lru_cache(maxsize=None)
def tiny_buffer(total):
    """a column whose byte buffer has `total` bytes in all: a string, a prefix of it (or its double when they are as long), and empty rows"""
    x = b"tiny buffer bytes"
    hi = total - total // 2
    return pack([b"", x[:hi], b"", x[:total - hi]])


@functools.lru_cache(maxsize=None)
def null_with_bytes():
    """A column built from explicit offsets: off[0] = 5 behind five unused 0xFF bytes, and NULL rows whose offset range holds 0xFF or 0x00
    bytes that would change the order if they were read. Every offset stays inside the buffer."""
    rng = np.random.default_rng(55)
    values = [b"", b"\x00", b"\xff", b"\xff" * 8, b"\x00" * 9, b"mid", b"middle of the range", b"\xff" * 8 + b"z"]
    junk = [b"\xff" * 3, b"\x00" * 4, b"\xff" * 12, b"\x00" * 17, b"\xff"]
    buf, off, strings, valid = [b"\xff" * 5], [5], [], []
    for i in range(240):
        if i % 3 == 1:
            piece, s = junk[int(rng.integers(0, len(junk)))], None
        else:
            piece = s = values[int(rng.integers(0, len(values)))]
        buf.append(piece)
        off.append(off[-1] + len(piece))
        strings.append(s)
        valid.append(s is not None)
    data = np.frombuffer(b"".join(buf), np.uint8)
    assert off[-1] == len(data)
    return StrCol(np.array(off, np.int32), data, np.array(valid, bool), strings)


# every VARCHAR corpus by name; nothing is built until varchar_corpus asks for it (each builder keeps what it built)
_VARCHAR = {f"many_segments {k}": functools.partial(many_segments, k) for k in (300, 1000, 70_000)}
_VARCHAR.update({"trailing_nul 21": functools.partial(trailing_nul, 21), "trailing_nul 5": functools.partial(trailing_nul, 5),
                 "deep_prefix": deep_prefix, "deep_prefix two groups": lambda: deep_prefix_two_groups()[0]})
_VARCHAR.update({f"round_sizes {m}": functools.partial(round_sizes, m) for m in ROUND_M})
_VARCHAR.update({"lone_survivor": lone_survivor, "null_neighbours": null_neighbours})
_VARCHAR.update({f"alignment_sweep part {p}": (lambda p=p: alignment_sweep(p)[0]) for p in (0, 1)})
_VARCHAR.update({f"tiny_buffer {t}": functools.partial(tiny_buffer, t) for t in TINY_BYTES})
_VARCHAR["null_with_bytes"] = null_with_bytes
VARCHAR_NAMES = tuple(_VARCHAR)


def varchar_corpus(name):
    """the StrCol of a VARCHAR corpus of VARCHAR_NAMES"""
    return _VARCHAR[name]()


def varchar_runs(col):
    """the four runs of a VARCHAR corpus: [(label, key columns, directions, selection or None)] — alone, and as the first of two keys with a
    3-valued PH_I32 key behind it and a shuffled selection; each ASC and DESC"""
    n = len(col.strings)
    second = num("I32", tie_key(n, 9))
    shuffled = selections(n, 3)["shuffled"] if n > 1 else None
    out = []
    for d in (False, True):
        out.append((("desc" if d else "asc") + " alone", [col], [d], None))
        out.append((("desc" if d else "asc") + " + tie key, shuffled selection", [col, second], [d, not d], shuffled))
    return out
