"""Inputs and plain references of the VARCHAR (PH_STR) edge tests (test_gpu_str_edges.py; checked on their own, without a device, by
test_str_edges_reference.py).

Every reference here is Python over `bytes`: LIKE is the reference's wildcardMatch walked byte by byte (and, for the literal shapes, `in` /
`find`), substring is substringStartEnd in Python's unbounded `int`s followed by a slice, interning is a partition check. None of them
restates the position-parallel formulation of the kernels (windows, overlap words, row lookup): the corpora below are BUILT around those
positions, the references never look at them."""
import numpy as np

I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
OP_EQ, OP_NE, OP_LIKE, OP_NOTLIKE = 1, 2, 7, 8            # planhip.h's and the oracle's numbering
PATTERN_ROOM = 96                                          # the pattern buffer: a pattern of 95 bytes is the longest accepted
ROWS_PER_GROUP = 2048                                      # rows one workgroup of the position-parallel kernels owns
STRIDE = 4096                                              # bytes between two windows of one thread
STAGE_ROWS, STAGE_BYTES = 256, 24 * 1024                   # the staged matcher's round
TAIL = 19                                                  # a window that starts in the last 19 bytes of a workgroup's range is read byte by byte

# 0x00 and bytes >= 0x80 (a signed char compare would order them differently), and the three bytes that mean something in a PATTERN
ALPHABET = bytes([0x00, 0x01]) + b"pink" + bytes([0x7F, 0x80, 0xFE, 0xFF]) + b"%_\\"


# ------------------------------------------------------------------ references
def like(pattern, s):
    """wildcardMatch over bytes: % is any run, _ is one byte, a mismatch goes back to the last %; a backslash is an ordinary byte"""
    p = t = 0
    after_pct = t_at_pct = -1
    plen, tlen = len(pattern), len(s)
    while t < tlen:
        if p < plen and pattern[p] == 0x25:
            p += 1
            after_pct = p
            if p >= plen:
                return True
            t_at_pct = t
        elif p < plen and (pattern[p] == 0x5F or pattern[p] == s[t]):
            p += 1
            t += 1
        else:
            if after_pct == -1 or t_at_pct == -1:
                return False
            p = after_pct
            t_at_pct += 1
            t = t_at_pct
    while p < plen and pattern[p] == 0x25:
        p += 1
    return p >= plen


def literal_shape(pattern):
    """(A,) for %A%, (A, B) for %A%B% with A and B free of % and _, else None"""
    if len(pattern) < 3 or pattern[:1] != b"%" or pattern[-1:] != b"%" or b"_" in pattern:
        return None
    parts = pattern[1:-1].split(b"%")
    return tuple(parts) if len(parts) in (1, 2) and all(parts) else None


def like_literals(lits, s):
    """the independent check of the literal shapes: `in` for %A%, two `find`s for %A%B%"""
    if len(lits) == 1:
        return lits[0] in s
    i = s.find(lits[0])
    return i >= 0 and s.find(lits[1], i + len(lits[0])) >= 0


def match_rows(op, pattern, strings):
    """one bool per row, NULLs not yet considered: LIKE / NOT LIKE / = / != of the row's bytes against the pattern"""
    if op in (OP_EQ, OP_NE):
        hit = [s == pattern for s in strings]
    else:
        lits = literal_shape(pattern)
        hit = [like_literals(lits, s) for s in strings] if lits else [like(pattern, s) for s in strings]
    hit = np.array(hit, dtype=bool).reshape(len(strings))
    return ~hit if op in (OP_NE, OP_NOTLIKE) else hit


def select_reference(op, pattern, strings, valid, sel=None):
    """rows (of sel, or all) the operator selects: a NULL row selects under no operator, NOT LIKE and != included"""
    rows = np.arange(len(strings), dtype=np.int64) if sel is None else np.asarray(sel, np.int64)
    if len(strings) == 0:
        return rows[:0]
    hit = match_rows(op, pattern, strings) & np.asarray(valid, bool)
    return rows[hit[rows]]


def substring_start_end(slen, offset, length):
    """substringStartEnd in unbounded integers: (start, end), or None where the result is empty. length = INT64_MAX is the two-argument
    form, for which the reference passes 2^32 - 1."""
    if length == I64_MAX:
        length = 2 ** 32 - 1
    if length == 0:
        return None
    if offset > 0:
        start = min(slen, offset - 1)
    elif offset < 0:
        start = max(slen + offset, 0)
    else:
        start = 0
        length -= 1
        if length <= 0:
            return None
    if length > 0:
        end = min(slen, start + length)
    else:
        end = start
        start = max(0, start + length)
    return None if start == end else (start, end)


def substring(s, offset, length):
    r = substring_start_end(len(s), offset, length)
    return b"" if r is None else s[r[0]:r[1]]


def reference_accepts(offset, length):
    """isValidRange: the arguments the reference evaluates instead of panicking"""
    return -(2 ** 32) <= offset <= 2 ** 32 - 1 and -(2 ** 32) <= length <= 2 ** 32 - 1


def check_interning(strings, valid, rows, codes, null_code):
    """The partition check of ph_strdict_build over `rows` of the column: NULL rows get null_code, every other row a code that IS a
    valid row holding the same string, equal strings the same code, different strings different codes. Returns {string: code}."""
    ids = {}
    assert len(rows) == len(codes)
    for r, c in zip(rows, codes):
        r, c = int(r), int(c)
        if not valid[r]:
            assert c == null_code, (r, c)
            continue
        assert 0 <= c < len(strings) and valid[c] and strings[c] == strings[r], (r, c)
        assert ids.setdefault(strings[r], c) == c, (r, c, ids[strings[r]])
    assert len(set(ids.values())) == len(ids)
    return ids


def lookup_reference(ids, strings, valid, rows):
    """ph_strdict_lookup: the build's code of the row's string; -2 for a NULL row and for a string the dictionary does not hold"""
    return np.array([ids.get(strings[int(r)], -2) if valid[int(r)] else -2 for r in rows], dtype=np.int32).reshape(len(rows))


# ------------------------------------------------------------------ corpora
class Corpus:
    """A PH_STR column: int32 offsets (off[0] may be > 0), the byte buffer they index (leading bytes included), boolean validity, and
    the rows as Python bytes (a NULL row keeps its bytes). plants: {class: [{"row", "match", "pos"}]} for the placement corpora."""

    def __init__(self, rows, valid=None, lead=b"", plants=None, name=""):
        self.strings = [bytes(r) for r in rows]
        self.n = len(self.strings)
        self.valid = np.ones(self.n, bool) if valid is None else np.asarray(valid, bool)
        off = np.zeros(self.n + 1, np.int64)
        off[0] = len(lead)
        if self.n:
            off[1:] = len(lead) + np.cumsum([len(r) for r in self.strings])
        assert off[-1] < 2 ** 31
        self.off = off.astype(np.int32)
        self.data = np.frombuffer(bytes(lead) + b"".join(self.strings), dtype=np.uint8)
        self.plants = plants or {}
        self.name = name

    def packed_validity(self):
        return None if self.valid.all() else np.packbits(self.valid, bitorder="little")


def third_rows(n):
    """the selection of the tests: every third row"""
    return np.arange(0, n, 3, dtype=np.int64)


def neutral_bytes(*lits):
    """alphabet bytes that occur in none of the literals: rows built from them and ONE planted occurrence hold no other"""
    out = bytes(b for b in ALPHABET if all(b not in lit for lit in lits))
    assert len(out) >= 2, lits
    return out


def _filler(rng, neutral, k):
    return bytes(neutral[i] for i in rng.integers(0, len(neutral), k))


PLACEMENT_CLASSES = "abcdefghij"
PLACEMENT_OFF0 = (0, 5, 16, 37)
PLACEMENT_ROWS = 2 * ROWS_PER_GROUP + 300
# what stands at the two workgroup boundaries (rows 2047|2048 and 4095|4096) of the corpus of each off0:
#   split: the occurrence is cut by the boundary (neither row matches); whole: one ends row r-1 and one starts row r (both match);
#   behind: one ends row r-1, row r holds none and starts at byte 15 of a window, so its workgroup reads the occurrence BEFORE its range
BOUNDARY_MODES = {0: ("split", "whole"), 5: ("whole", "behind"), 16: ("behind", "split"), 37: ("split", "whole")}


def like_placement_corpus(A, B=None, off0=0, seed=0):
    """Two full workgroups and a partial one of short rows. U, the planted unit, is A (for %A%) or A + one other byte + B (for %A%B%);
    it is planted by byte position and row index, and near-misses of it likewise:
      a  wholly inside a row
      b  ending exactly at the row's end, starting exactly at its start, being the whole row
      c  cut by a row end (no row matches): adjacent rows, across an empty row, across a NULL row without bytes. A one-byte U cannot
         be cut: the rows next to one that starts / ends with it hold none (the hit belongs to ONE row)
      d  starting at byte 13, 14, 15 of a 16-byte window (the window's overlap word decides)
      e  across a multiple of 4096 bytes, counted from the 16-byte floor of the offset of the workgroup's first row (a one-byte U: the
         byte just before the multiple)
      f  in the last 19 bytes before the offset of row 2048 / 4096 / n (a U longer than 19 bytes: reaching into them)
      g  at the workgroup boundaries: BOUNDARY_MODES[off0]
      h  rows 0 and n - 1 (row 0 only where no bytes lie before it in its window, off0 % 16 == 0; else row 0 is the `lead` plant)
      i  a NULL row whose bytes hold U
      j  %A%B% only (else a second (a) plant): B before A only; B overlapping A's tail (where A ends with B's first byte); A twice, then B;
         A ending one row and B starting the next
      lead  off0 % 16 != 0: the bytes before off[0] end with U (or, where U is longer, with its head, which row 0 continues): row 0 has none
    Every other row is random over the whole alphabet, 0..11 bytes, some NULL. Returns a Corpus; plants[class] = [{"row", "match", "pos"}],
    pos = the absolute byte position of U in the buffer (classes d, e, f) or None."""
    assert off0 in BOUNDARY_MODES
    rng = np.random.default_rng([seed, off0, len(A), len(B or b"")])
    neutral = neutral_bytes(A, B or b"")
    nb = neutral.replace(b"\x00", b"")[:1]       # between A and B inside the unit (not NUL: the unit is a pattern too, a C string)
    U = A if B is None else A + nb + B
    L = len(U)
    n = PLACEMENT_ROWS
    k = max(1, min(L // 2, 9))           # where a cut falls
    rows, valid = [], []
    plants = {c: [] for c in PLACEMENT_CLASSES}
    plants["lead"] = []
    pad = lambda m: _filler(rng, neutral, m)

    # the bytes before off[0]
    near = off0 % 16
    if near == 0:
        lead, row0, row0_match = (pad(off0) + U)[-off0:] if off0 else b"", U + pad(2), True
    elif L <= near:
        lead, row0, row0_match = pad(off0 - L) + U, pad(3), False
    else:
        kk = min(L - 1, near)
        lead, row0, row0_match = pad(off0 - kk) + U[:kk], U[kk:] + pad(2), False
    assert len(lead) == off0
    cur = [off0]                         # the absolute position of the next row's first byte

    def emit(b, ok=True):
        rows.append(b)
        valid.append(ok)
        cur[0] += len(b)
        return len(rows) - 1

    def plant(cls, b, match, upos=None, ok=True):
        at = None if upos is None else cur[0] + upos
        r = emit(b, ok)
        plants[cls].append({"row": r, "match": match, "pos": at})
        return r

    def fill_to(r):                      # ordinary rows up to row r
        while len(rows) < r:
            m = int(rng.integers(0, 12))
            emit(bytes(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), m)), ok=rng.random() >= 0.03)

    def cut(cls, middle=None):           # U cut by a row end; `middle`: rows between the halves
        if L == 1:
            plant(cls, pad(2) + U, True)
            plant(cls, pad(2), False)
            plant(cls, U + pad(2), True)
            return
        plant(cls, pad(2) + U[:k], False)
        for b, ok in middle or ():
            plant(cls, b, False, ok=ok)
        plant(cls, U[k:] + pad(2), False)

    def boundary(r, mode):               # rows r-2, r-1, r around the first row r of a workgroup
        fill_to(r - 2)
        if mode == "split":
            if L == 1:
                plant("f", pad(2) + U, True, upos=2)
                plant("g", pad(1), False)
                plant("g", U + pad(2), True)
            else:
                plant("f", pad(2) + U, True, upos=2)
                plant("g", U[:k], False)
                plant("g", U[k:] + pad(2), False)
        elif mode == "whole":
            emit(pad(3))
            plant("g", pad(2) + U, True, upos=2)
            plants["f"].append(dict(plants["g"][-1]))
            plant("g", U + pad(2), True)
        else:
            emit(pad(3))
            m = (15 - (cur[0] + L)) % 16                      # the next row then starts at byte 15 of a window
            plant("g", pad(m) + U, True, upos=m)
            plants["f"].append(dict(plants["g"][-1]))
            plant("g", pad(3), False)
            assert (cur[0] - 3) % 16 == 15

    def across(group_first_off):         # class e: the next multiple of STRIDE counted from the workgroup's 16-byte floor, if it is near
        a0 = group_first_off & ~15
        nxt = a0 + ((cur[0] - a0) // STRIDE + 1) * STRIDE
        j = 1 if L == 1 else k
        m = nxt - j - cur[0]
        if 0 <= m <= 30:
            plant("e", pad(m) + U + pad(2), True, upos=m)

    plant("h" if row0_match else "lead", row0, row0_match)
    fill_to(10)
    plant("a", pad(3) + U + pad(2), True)
    fill_to(12)
    plant("b", pad(2) + U, True)
    emit(pad(2))
    plant("b", U + pad(3), True)
    emit(pad(1))
    plant("b", U, True)
    fill_to(20)
    cut("c")
    fill_to(24)
    cut("c", [(b"", True)])
    fill_to(28)
    cut("c", [(b"", False)])
    fill_to(34)
    plant("i", pad(1) + U + pad(1), False, ok=False)
    fill_to(40)
    for want in (13, 14, 15):
        m = (want - cur[0]) % 16
        plant("d", pad(m) + U + pad(1), True, upos=m)
        emit(pad(int(rng.integers(0, 5))))
    fill_to(50)
    if B is None:
        plant("j", pad(1) + U + pad(4), True)
    else:
        plant("j", pad(1) + B + nb + A + pad(1), False)
        if A[-1] == B[0]:
            plant("j", pad(1) + A[:-1] + B + pad(1), False)
        plant("j", A + nb + A + nb + B, True)
        plant("j", pad(2) + A, False)
        plant("j", B + pad(2), False)
    group_first = off0
    for first, mode in ((ROWS_PER_GROUP, BOUNDARY_MODES[off0][0]), (2 * ROWS_PER_GROUP, BOUNDARY_MODES[off0][1])):
        while len(rows) < first - 2 - 1:
            across(group_first)
            fill_to(len(rows) + 1)
        boundary(first, mode)
        assert len(rows) == first + 1
        group_first = cur[0] - len(rows[-1])
    while len(rows) < n - 1:
        across(group_first)
        if len(rows) < n - 1:
            fill_to(len(rows) + 1)
    plant("h", pad(2) + U, True, upos=2)
    plants["f"].append(dict(plants["h"][-1]))
    assert len(rows) == n
    c = Corpus(rows, valid, lead=lead, plants=plants, name=f"placement({A!r},{B!r},off0={off0})")
    c.unit, c.lits = U, (A,) if B is None else (A, B)
    return c


def placement_pattern(c):
    return b"%" + b"%".join(c.lits) + b"%"


def group_first_offset(c, row):
    """the offset of the first row of the workgroup that owns `row`, and of the first row behind that workgroup"""
    g = row // ROWS_PER_GROUP
    return int(c.off[g * ROWS_PER_GROUP]), int(c.off[min((g + 1) * ROWS_PER_GROUP, c.n)])


def stage_boundary_corpus(A=b"pink"):
    """Rounds of 256 rows for the staged matcher, which copies off[first] & ~3 .. off[first + 256] to its 24 KiB stage when that fits:
    round 0 spans 24575 bytes, round 1 24576 (exactly the stage; it starts at byte 3 of a word), round 2 24577 (too long: the per-row
    matcher), round 3 is ONE row of 30 000 bytes that ends with A among 255 empty rows, round 4 is short. The first row of every round
    starts with A and the last one ends with it: A ends on the last staged byte. Returns (Corpus, [bytes each round spans])."""
    rng = np.random.default_rng(24576)
    neutral = neutral_bytes(A)
    rows = []
    cur = 0
    for span in (STAGE_BYTES - 1, STAGE_BYTES, STAGE_BYTES + 1):
        total = span - (cur - (cur & ~3))
        lens = rng.integers(60, 110, STAGE_ROWS)
        lens[-1] += total - int(lens.sum())
        assert lens[-1] >= 2 * len(A) and lens.sum() == total
        for i, m in enumerate(lens.tolist()):
            b = bytearray(ALPHABET[j] for j in rng.integers(0, len(ALPHABET), m))
            if i == 0:
                b[:len(A)] = A
            if i == STAGE_ROWS - 1:
                b[-len(A):] = A
            if i == 100:                                  # a row that holds no A at all
                b = bytearray(_filler(rng, neutral, m))
            rows.append(bytes(b))
        cur += total
    rows += [b""] * 100 + [_filler(rng, neutral, 30_000 - len(A)) + A] + [b""] * 155
    rows += [A, b"", _filler(rng, neutral, 5), A + _filler(rng, neutral, 3), _filler(rng, neutral, 3) + A[:-1], A[1:]]
    c = Corpus(rows, name=f"stage({A!r})")
    spans = [int(c.off[min(f + STAGE_ROWS, c.n)]) - (int(c.off[f]) & ~3) for f in range(0, c.n, STAGE_ROWS)]
    return c, spans


def random_corpus(n=3000, seed=1):
    """rows of 0..14 bytes over the whole alphabet, one in twenty NULL, and a few longer ones"""
    rng = np.random.default_rng(seed)
    rows = [bytes(ALPHABET[j] for j in rng.integers(0, len(ALPHABET), int(rng.integers(0, 15)))) for _ in range(n)]
    for i in range(0, n, 97):
        rows[i] = rows[i] * 9
    return Corpus(rows, rng.random(n) >= 0.05, name=f"random({n})")


def degenerate_corpora():
    """one row; only empty rows over a byte buffer of length zero; only NULL rows; one row that holds all the bytes"""
    whole = bytes(range(1, 256)) * 3 + b"pink\x80\xff"
    return [Corpus([b"pink\xff"], name="one row"), Corpus([b""] * 700, name="all empty"),
            Corpus([b"pink", b"", b"p\x80"] * 100, np.zeros(300, bool), name="all NULL"),
            Corpus([b""] * 300 + [whole] + [b""] * 299, name="one row holds all")]


# ------------------------------------------------------------------ patterns
def _literal(L):
    """a literal of L bytes with high and low bytes at both ends (no NUL: patterns are C strings; no % or _)"""
    base = b"\xffp\x01\x80k\xfen\x7fi"
    return (base * (L // len(base) + 1))[:L]


LITERALS = [_literal(L) for L in (1, 2, 3, 4, 5, 9, 93)]
# A ends with the byte B starts with, so that B can overlap A's tail (two one-byte literals would be the same byte: they differ instead)
PAIRS = [((b"\x80\x01pi\xff")[-la:] if (la, lb) != (1, 1) else b"\x80", (b"\xffk\xfen\x01")[:lb]) for la in (1, 3, 4, 5) for lb in (1, 3, 4, 5)]
GENERIC_PATTERNS = [b"_", b"%_", b"_%", b"%_%", b"%%", b"%%%", b"p%", b"%p", b"p_%_k", b"%\\%", b"", b"%\xff_\x80%", b"_\xfe%", b"%\x7f"]
LITERAL_PATTERNS = [b"%" + a + b"%" for a in LITERALS[:6]] + [b"%p%", b"%in%", b"%\x80\xfe%", b"%pink%", b"%\\%", b"%\\\\%"]
PAIR_PATTERNS = [b"%" + a + b"%" + b + b"%" for a, b in (PAIRS[0], PAIRS[5], PAIRS[15], (b"p", b"p"), (b"in", b"k"), (b"\xff", b"\x80\x80"))]
assert len(b"%" + LITERALS[-1] + b"%") == PATTERN_ROOM - 1
PATTERN_TOO_LONG = b"%" + _literal(94) + b"%"


def equality_constants(c):
    """= / != constants for a corpus: the empty string, a full row with a high byte, a proper prefix of a row, a row plus one byte"""
    full = next((s for s in c.strings if 2 <= len(s) < PATTERN_ROOM - 1 and max(s) >= 0x80 and 0 not in s), b"\xffp")
    return [b"", full, full[:-1], full + b"\x80"]


# ------------------------------------------------------------------ interning
def strdict_capacity(n):
    """the table ph_strdict_build sizes for n rows: max(1024, the next power of two >= 2 n) — computed as ops_str.hip computes it"""
    cap = 1024
    while cap < 2 * n:
        cap <<= 1
    return cap


def strdict_wrap_corpus(n=480, hash_bytes=None):
    """n rows over ~48 distinct strings whose home slots (hash_bytes & (cap - 1), cap = strdict_capacity(n)) are the last four of the
    table — ten times what fits there, so their probe chains run over the table's end — and the first four, which the wrapped chains then
    collide with. Every string is repeated and the order is shuffled. Returns (Corpus, absent): `absent` are strings of the same home
    slots that the corpus does not hold. Candidates are drawn from a counter; hash_bytes is the host-only ph_hash_bytes."""
    if hash_bytes is None:
        from plan_amd import hip
        hash_bytes = hip.hash_bytes
    cap = strdict_capacity(n)
    assert cap == 1024 == strdict_capacity(n // 3), "a selection of every third row must get the same table"
    tail, head, absent = [], [], []
    i = 0
    while len(tail) < 40 or len(head) < 8 or len(absent) < 12:
        s = b"w\xff%d\x00" % i if i % 2 else b"%dw\x80" % i
        i += 1
        slot = hash_bytes(s) & (cap - 1)
        if slot >= cap - 4:
            (tail if len(tail) < 40 else absent).append(s)
        elif slot < 4 and len(head) < 8:
            head.append(s)
    distinct = tail + head
    rng = np.random.default_rng(1024)
    rows = [distinct[j % len(distinct)] for j in range(n)]
    rng.shuffle(rows)
    valid = rng.random(n) >= 0.04
    return Corpus(rows, valid, name=f"wrap({n})"), absent[:12]


def strdict_corpora(hash_bytes=None):
    """[(Corpus, absent strings)]: the wrap corpus, one string in all rows, two strings of one home slot in all rows, strings equal but
    for the last byte / but for a trailing 0x00 / a prefix of each other, and 65536 / 65537 rows (either side of the head launch) over 25
    distinct strings"""
    if hash_bytes is None:
        from plan_amd import hip
        hash_bytes = hip.hash_bytes
    out = [strdict_wrap_corpus(480, hash_bytes)]
    out.append((Corpus([b"only\xff"] * 300, name="one string"), [b"only", b"only\xff\x00", b""]))
    seen, i, trio = {}, 0, None
    while trio is None:                                  # three strings that share their home slot (cap 1024): two in the column, one absent
        s = b"s%d\xfe" % i
        i += 1
        same = seen.setdefault(hash_bytes(s) & 1023, [])
        same.append(s)
        if len(same) == 3:
            trio = same
    out.append((Corpus([trio[j & 1] for j in range(400)], name="two strings, one slot"), [trio[2], trio[0] + b"\x00"]))
    stem = b"stem\x80" * 6
    near = [stem + b"a", stem + b"b", stem, stem + b"\x00", stem + b"\x00\x00", stem[:-1], b"", b"\x00", b"\x00\x00", b"\xff", b"\xff\xff"]
    rng = np.random.default_rng(7)
    rows = [near[j] for j in rng.integers(0, len(near), 600)]
    out.append((Corpus(rows, rng.random(600) >= 0.05, name="near-equal strings"), [stem + b"c", stem[:-2], stem + b"\x00\x00\x00", b"\xff\x00"]))
    words = [b"%02d-\xfe" % j for j in range(25)]
    for n in (65536, 65537):
        pick = np.random.default_rng(n).integers(0, 25, n)
        pick[-1] = 24
        pick[:-1][pick[:-1] == 24] = 3                 # word 24 only in the LAST row: the head launch never sees it
        v = np.ones(n, bool)
        v[[5, 8191, 8192, n - 2]] = False
        out.append((Corpus([words[j] for j in pick], v, name=f"25 strings in {n} rows"), [b"25-\xfe", b"00-"]))
    return out


def lookup_column(c, absent, seed=3):
    """a second column for ph_strdict_lookup: strings of the corpus, absent ones (the same home slots among them), the empty string,
    NULL rows"""
    rng = np.random.default_rng(seed)
    present = sorted(set(s for s, ok in zip(c.strings, c.valid) if ok))
    pool = present + list(absent) + [b""]
    rows = [pool[j] for j in rng.integers(0, len(pool), 500)] + list(absent) + present[:50]
    return Corpus(rows, rng.random(len(rows)) >= 0.1, name=f"lookup of {c.name}")


# ------------------------------------------------------------------ substring
SUBSTRING_OFFSETS = (I64_MIN, -2 ** 32 - 1, -2 ** 32, -40, -3, -1, 0, 1, 2, 3, 40, 2 ** 32 - 1, 2 ** 32, I64_MAX)
SUBSTRING_LENGTHS = (I64_MIN, I64_MIN + 1, -2 ** 32, -3, -1, 0, 1, 2, 100, 2 ** 32 - 1, 2 ** 62, I64_MAX - 1, I64_MAX)


def substring_args():
    return [(o, ln) for o in SUBSTRING_OFFSETS for ln in SUBSTRING_LENGTHS]


def substring_corpus():
    """rows of every length 0..20 (three of each) over the alphabet, every seventh NULL; and a selection with repeated and descending
    row ids whose rows together are no longer than the column (the result always fits the source's byte count)"""
    rng = np.random.default_rng(20)
    rows = [bytes(ALPHABET[j] for j in rng.integers(0, len(ALPHABET), m)) for m in range(21) for _ in range(3)]
    order = rng.permutation(len(rows))
    rows = [rows[j] for j in order]
    valid = np.arange(len(rows)) % 7 != 3
    c = Corpus(rows, valid, name="substring rows")
    sel = np.array([5, 5, 0, 62, 62, 62, 17, 3, 3, 40, 10, 24, 59, 1, 1, 31, 31, 2], dtype=np.int64)
    assert sum(len(rows[r]) for r in sel) <= len(c.data)
    return c, sel
