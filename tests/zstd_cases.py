"""ZSTD streams built from bits, and Parquet files with ZSTD pages. A writer that models its own output (Frame: every block it appends
also extends Frame.out, what a decoder must produce): frame and block headers, a backward bit writer, Huffman literals from given weights
(described direct or FSE-compressed), an FSE encoder from given normalized counts (the decode table is built as RFC 8878 builds it, then
the symbols are encoded from the last one backwards, each time picking the cell whose range holds the next state), XXH64. The reference for
every stream is libzstd as pyarrow carries it. A plain module: no fixtures, no test."""
import os

import numpy as np

import delta_cases as D
import parquet_cases as P
import snappy_cases as SN

WINDOW = 4096         # plan_amd/csrc/zstd_decompress.h: ZS_TILE, the bytes of each of the kernel's two input windows
RING = 32768          # plan_amd/csrc/zstd_decompress.h: ZS_RING, the output bytes the kernel keeps in LDS
BLOCK_MAX = 128 * 1024
N = P.N

LL_NORM = [4, 3] + [2] * 11 + [1] * 3 + [2] * 9 + [3, 2] + [1] * 5 + [-1] * 4
ML_NORM = [1, 4, 3] + [2] * 6 + [1] * 37 + [-1] * 7
OF_NORM = [1] * 6 + [2] * 3 + [1] * 15 + [-1] * 5
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
assert len(LL_NORM) == len(LL_BASE) == 36 and len(ML_NORM) == len(ML_BASE) == 53 and len(OF_NORM) == 29


# ---------------------------------------------------------------- XXH64
M64 = (1 << 64) - 1
XP1, XP2, XP3, XP4, XP5 = 11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579, 2870177450012600261


def xxh64(data):
    rotl = lambda x, r: ((x << r) | (x >> (64 - r))) & M64
    rnd = lambda a, v: rotl((a + v * XP2) & M64, 31) * XP1 & M64
    n, i = len(data), 0
    if n >= 32:
        v = [(XP1 + XP2) & M64, XP2, 0, (-XP1) & M64]
        for i in range(0, n - 31, 32):
            for k in range(4):
                v[k] = rnd(v[k], int.from_bytes(data[i + 8 * k:i + 8 * k + 8], "little"))
        i += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & M64
        for k in range(4):
            h = ((h ^ rnd(0, v[k])) * XP1 + XP4) & M64
    else:
        h = XP5
    h = (h + n) & M64
    while i + 8 <= n:
        h = (rotl(h ^ rnd(0, int.from_bytes(data[i:i + 8], "little")), 27) * XP1 + XP4) & M64
        i += 8
    if i + 4 <= n:
        h = (rotl(h ^ (int.from_bytes(data[i:i + 4], "little") * XP1 & M64), 23) * XP2 + XP3) & M64
        i += 4
    while i < n:
        h = rotl(h ^ (data[i] * XP5 & M64), 11) * XP1 & M64
        i += 1
    h ^= h >> 33
    h = h * XP2 & M64
    h ^= h >> 29
    h = h * XP3 & M64
    return h ^ (h >> 32)


# ---------------------------------------------------------------- bits
def back_stream(fields, marker=True):
    """fields = [(value, bits)] in the order a decoder READS them -> the backward bitstream's bytes (the final-bit marker on top)"""
    acc, n = 0, 0
    for v, b in reversed(fields):
        assert 0 <= v < (1 << b) or b == 0 and v == 0, (v, b)
        acc |= v << n
        n += b
    if marker:
        acc |= 1 << n
        n += 1
    return acc.to_bytes(max((n + 7) // 8, 1), "little")


def fwd_stream(fields):
    acc, n = 0, 0
    for v, b in fields:
        assert 0 <= v < (1 << b), (v, b)
        acc |= v << n
        n += b
    return acc.to_bytes((n + 7) // 8, "little")


# ---------------------------------------------------------------- FSE
class Fse:
    """the decode table of normalized counts `norm` at accuracy log `log`, as RFC 8878 4.1.1 builds it"""

    def __init__(self, norm, log):
        size = 1 << log
        assert sum(abs(c) for c in norm) == size, (sum(abs(c) for c in norm), size)
        self.norm, self.log = list(norm), log
        sym = [None] * size
        high = size - 1
        for s, c in enumerate(norm):
            if c == -1:
                sym[high] = s
                high -= 1
        pos, step = 0, (size >> 1) + (size >> 3) + 3
        for s, c in enumerate(norm):
            for _ in range(max(c, 0)):
                sym[pos] = s
                pos = (pos + step) & (size - 1)
                while pos > high:
                    pos = (pos + step) & (size - 1)
        assert pos == 0
        nxt = [abs(c) for c in norm]
        self.cells = []                                        # (symbol, bits, base)
        self.of_symbol = {}
        for i, s in enumerate(sym):
            x = nxt[s]
            nxt[s] += 1
            nb = log - (x.bit_length() - 1)
            self.cells.append((s, nb, (x << nb) - size))
            self.of_symbol.setdefault(s, []).append(i)

    def description(self):
        """the table description's bytes (FSE_writeNCount)"""
        f = [(self.log - 5, 4)]
        remaining, threshold, nbits, i, prev0 = (1 << self.log) + 1, 1 << self.log, self.log + 1, 0, False
        while remaining > 1 and i < len(self.norm):
            if prev0:
                z = 0
                while self.norm[i + z] == 0:
                    z += 1
                i += z
                while z >= 3:
                    f.append((3, 2))
                    z -= 3
                f.append((z, 2))
            c = self.norm[i]
            i += 1
            mx = 2 * threshold - 1 - remaining
            v = c + 1
            remaining -= abs(c)
            if v < mx:
                f.append((v, nbits - 1))
            else:
                f.append((v if v < threshold else v + mx, nbits))
            prev0 = c == 0
            while remaining < threshold:
                nbits -= 1
                threshold >>= 1
        return fwd_stream(f)

    def chain(self, symbols):
        """the states that decode `symbols` in order and the bits each step to the next state reads -> (first state, [(bits value, bits)])"""
        state = self.of_symbol[symbols[-1]][0]
        steps = []
        for s in reversed(symbols[:-1]):
            for c in self.of_symbol[s]:
                _s, nb, base = self.cells[c]
                if base <= state < base + (1 << nb):
                    steps.append((state - base, nb))
                    state = c
                    break
            else:
                raise AssertionError("no cell of symbol %d reaches state %d" % (s, state))
        return state, steps[::-1]


class RleTable:
    """a sequence table in RLE mode: one symbol, no bits"""

    def __init__(self, symbol):
        self.symbol, self.log = symbol, 0

    def chain(self, symbols):
        assert all(s == self.symbol for s in symbols)
        return 0, [(0, 0)] * (len(symbols) - 1)


PREDEFINED = {"ll": Fse(LL_NORM, 6), "of": Fse(OF_NORM, 5), "ml": Fse(ML_NORM, 6)}


# ---------------------------------------------------------------- Huffman
def complete_weights(weights):
    """weights of symbols 0..n-1 -> the same with the last one set to what completes the sum to a power of two (it must be possible)"""
    total = sum((1 << w) >> 1 for w in weights[:-1])
    bits = total.bit_length()
    rest = (1 << bits) - total
    assert rest & (rest - 1) == 0, (total, rest)
    return list(weights[:-1]) + [rest.bit_length()]


def huffman_codes(weights):
    """{symbol: (code, bits)} as the decoder's table lays them out: the lowest weights first, symbols in order"""
    total = sum((1 << w) >> 1 for w in weights)
    bits = total.bit_length() - 1
    assert 1 << bits == total, total
    at, codes = 0, {}
    for w in range(1, bits + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                codes[s] = (at >> (w - 1), bits + 1 - w)
                at += 1 << (w - 1)
    return codes, bits


def tree_direct(weights):
    n = len(weights) - 1                                       # the last weight is implied
    assert 1 <= n <= 128
    body = bytearray()
    for i in range(0, n, 2):
        body.append(weights[i] << 4 | (weights[i + 1] if i + 1 < n else 0))
    return bytes([127 + n]) + bytes(body)


def tree_fse(weights, norm, log):
    """the weights but the last through an FSE table of `norm`: two interleaved states"""
    w = list(weights[:-1])
    n = len(w)
    assert n >= 2
    t = Fse(norm, log)
    first, steps = [None, None], [None, None]
    for p in (0, 1):
        first[p], steps[p] = t.chain(w[p::2])
    fields = [(first[0], log), (first[1], log)]
    for i in range(n - 2):                                     # the state of symbol i steps on to symbol i + 2
        fields.append(steps[i % 2][i // 2])
    # (the stream ends when the state of symbol n - 2 asks for bits that are not there: that cell must read at least one)
    last = t.of_symbol[w[n - 2]][0]
    assert t.cells[last][1] > 0
    body = t.description() + back_stream(fields)
    assert len(body) < 128
    return bytes([len(body)]) + body


def huffman_stream(lits, codes):
    return back_stream([codes[b] for b in lits])


# ---------------------------------------------------------------- literals sections
def lits_raw(data, fmt=None):
    n = len(data)
    fmt = fmt if fmt is not None else 0 if n < 32 else 1 if n < 4096 else 3
    return _lits_head(0, fmt, n) + bytes(data)


def lits_rle(byte, n, fmt=None):
    fmt = fmt if fmt is not None else 0 if n < 32 else 1 if n < 4096 else 3
    return _lits_head(1, fmt, n) + bytes([byte])


def _lits_head(kind, fmt, n):
    if fmt in (0, 2):
        assert n < 32
        return bytes([kind | fmt << 2 | n << 3])
    if fmt == 1:
        assert n < 4096
        return (kind | 1 << 2 | n << 4).to_bytes(2, "little")
    assert n < 1 << 20
    return (kind | 3 << 2 | n << 4).to_bytes(3, "little")


def lits_huffman(data, weights, fmt=0, tree=None, treeless=False, sizes=None):
    """data through the code of `weights` (all of them, the implied last one included); fmt 0: one stream, 1..3: four. tree: the tree
    description's bytes (default: direct); treeless: no description. sizes: (regenerated, compressed) to state instead of the true ones"""
    codes, _bits = huffman_codes(weights)
    n = len(data)
    if fmt == 0:
        body = huffman_stream(data, codes)
    else:
        seg = (n + 3) // 4
        parts = [huffman_stream(data[i * seg:(i + 1) * seg] if i < 3 else data[3 * seg:], codes) for i in range(4)]
        body = b"".join(len(p).to_bytes(2, "little") for p in parts[:3]) + b"".join(parts)
    body = (b"" if treeless else tree if tree is not None else tree_direct(weights)) + body
    sb = {0: 10, 1: 10, 2: 14, 3: 18}[fmt]
    rs, cs = sizes if sizes else (n, len(body))
    assert rs < 1 << sb and cs < 1 << sb
    head = (3 if treeless else 2) | fmt << 2 | rs << 4 | cs << (4 + sb)
    return head.to_bytes({0: 3, 1: 3, 2: 4, 3: 5}[fmt], "little") + body


# ---------------------------------------------------------------- sequences sections
def ll_code(v):
    c = max(i for i in range(36) if LL_BASE[i] <= v)
    assert v - LL_BASE[c] < 1 << LL_BITS[c]
    return c


def ml_code(v):
    c = max(i for i in range(53) if ML_BASE[i] <= v)
    assert v - ML_BASE[c] < 1 << ML_BITS[c]
    return c


def seq_count(n):
    if n < 128:
        return bytes([n])
    if n < 0x7f00:
        return bytes([128 + (n >> 8), n & 255])
    return b"\xff" + (n - 0x7f00).to_bytes(2, "little")


def sequences(seqs, tables=None, modes=None, count=None, reserved=0):
    """seqs = [(literal length, match length, offset VALUE)] (offset value 1..3: a repeat offset, else the offset + 3). tables: {"ll" / "of" /
    "ml": Fse or RleTable} (default: the predefined ones); modes: {"ll" / ...: 0 Predefined, 1 RLE, 2 FSE_Compressed, 3 Repeat} (default:
    what the table is) -> the section's bytes"""
    if not seqs:
        return seq_count(0 if count is None else count)
    tables = dict(PREDEFINED, **(tables or {}))
    modes = dict(modes or {})
    head = bytearray(seq_count(len(seqs) if count is None else count))
    mode_byte = reserved
    desc = b""
    for name, shift in (("ll", 6), ("of", 4), ("ml", 2)):
        t = tables[name]
        m = modes.get(name, 0 if t is PREDEFINED[name] else 1 if isinstance(t, RleTable) else 2)
        mode_byte |= m << shift
        if m == 1:
            desc += bytes([t.symbol])
        elif m == 2:
            desc += t.description()
    codes = {"ll": [ll_code(s[0]) for s in seqs], "ml": [ml_code(s[1]) for s in seqs], "of": [s[2].bit_length() - 1 for s in seqs]}
    first, steps = {}, {}
    for name in ("ll", "of", "ml"):
        first[name], steps[name] = tables[name].chain(codes[name])
    fields = [(first["ll"], tables["ll"].log), (first["of"], tables["of"].log), (first["ml"], tables["ml"].log)]
    for i, (ll, ml, ofv) in enumerate(seqs):
        oc, mc, lc = codes["of"][i], codes["ml"][i], codes["ll"][i]
        fields += [(ofv - (1 << oc), oc), (ml - ML_BASE[mc], ML_BITS[mc]), (ll - LL_BASE[lc], LL_BITS[lc])]
        if i + 1 < len(seqs):
            fields += [steps["ll"][i], steps["ml"][i], steps["of"][i]]
    return bytes(head) + bytes([mode_byte]) + desc + back_stream(fields)


# ---------------------------------------------------------------- frames
class Frame:
    """one frame under construction; .out is what it must produce"""

    def __init__(self, single=False, window=0x38, fcs=None, checksum=False, did_bytes=0, did=0, reserved=0):
        """window: the Window_Descriptor byte (0x38: 128 KiB); fcs: the width of the Frame_Content_Size in bytes (None: 1 with single, else
        none)"""
        self.single, self.window, self.checksum, self.did_bytes, self.did, self.reserved = single, window, checksum, did_bytes, did, reserved
        self.fcs = fcs if fcs is not None else (1 if single else 0)
        self.blocks = []
        self.out = bytearray()
        self.rep = [1, 4, 8]
        self.fcs_value = None
        self.checksum_value = None

    def _block(self, kind, size, body, last):
        assert size < 1 << 21
        self.blocks.append(((1 if last else 0) | kind << 1 | size << 3).to_bytes(3, "little") + body)
        return self

    def raw(self, data, last=False):
        self.out += data
        return self._block(0, len(data), bytes(data), last)

    def rle(self, byte, n, last=False):
        self.out += bytes([byte]) * n
        return self._block(1, n, bytes([byte]), last)

    def run(self, lits, seqs):
        """the model: literals and sequences executed on .out with the repeat-offset rules"""
        at = 0
        for ll, ml, ofv in seqs:
            self.out += lits[at:at + ll]
            at += ll
            if ofv > 3:
                off = ofv - 3
                self.rep = [off, self.rep[0], self.rep[1]]
            else:
                idx = ofv + (1 if ll == 0 else 0)
                if idx == 1:
                    off = self.rep[0]
                elif idx == 2:
                    off = self.rep[1]
                    self.rep = [off, self.rep[0], self.rep[2]]
                else:
                    off = self.rep[2] if idx == 3 else self.rep[0] - 1
                    self.rep = [off, self.rep[0], self.rep[1]]
            assert 1 <= off <= len(self.out), (off, len(self.out))
            if off >= ml:
                self.out += self.out[len(self.out) - off:len(self.out) - off + ml]
            else:
                pat = bytes(self.out[-off:])
                self.out += (pat * (ml // off + 1))[:ml]
        self.out += lits[at:]

    def compressed(self, lits, lits_section, seqs, last=False, model=True, **kw):
        """lits: the literal bytes; lits_section: their section's bytes; seqs and kw: sequences()"""
        if model:
            self.run(lits, seqs)
        body = lits_section + sequences(seqs, **kw)
        return self._block(2, len(body), body, last)

    def raw_block_bytes(self, kind, size, body, last=False):
        """a block of any bytes; .out is not extended"""
        return self._block(kind, size, body, last)

    def bytes(self):
        fcs_flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[self.fcs]
        assert self.fcs != 0 or not self.single
        fhd = fcs_flag << 6 | (32 if self.single else 0) | self.reserved | (4 if self.checksum else 0) | {0: 0, 1: 1, 2: 2, 4: 3}[self.did_bytes]
        head = b"\x28\xb5\x2f\xfd" + bytes([fhd]) + (b"" if self.single else bytes([self.window])) + self.did.to_bytes(self.did_bytes, "little")
        if self.fcs:
            v = len(self.out) if self.fcs_value is None else self.fcs_value
            head += (v - 256 if self.fcs == 2 else v).to_bytes(self.fcs, "little")
        tail = b""
        if self.checksum:
            tail = ((xxh64(bytes(self.out)) & 0xffffffff) if self.checksum_value is None else self.checksum_value).to_bytes(4, "little")
        return head + b"".join(self.blocks) + tail


def skippable(n, nibble=0):
    return bytes([0x50 + nibble, 0x2a, 0x4d, 0x18]) + n.to_bytes(4, "little") + b"\x5a" * n


def payload(n, seed=0):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def text(n, seed=0):
    """n bytes over a small alphabet with a skewed distribution: what a Huffman code is for"""
    rng = np.random.default_rng(seed)
    return bytes(rng.choice(np.frombuffer(b"etaoinshr ", np.uint8), n, p=[0.25, 0.2, 0.15, 0.1, 0.1, 0.05, 0.05, 0.04, 0.03, 0.03]).tolist())


def weights_for(alphabet, weights):
    """a weight list over byte values: alphabet[i] gets weights[i]; the largest byte value must be the one whose weight is implied"""
    w = [0] * (max(alphabet) + 1)
    for a, x in zip(alphabet, weights):
        w[a] = x
    done = complete_weights(w)
    assert done == w, (done[-1], w[-1])
    return w


TEXT_ALPHABET = sorted(b"etaoinshr ")                          # ' ' a e h i n o r s t: 10 symbols
# 2 of weight 4, 1 of 3, 2 of 2, 4 of 1 and the last, 't', implied: 8+8+4+2+2+1*4 = 28 -> 't' takes 4 (weight 3): 32, five bits
TEXT_WEIGHTS = weights_for(TEXT_ALPHABET, [4, 4, 3, 2, 2, 1, 1, 1, 1, 3])


def text_lits(n, seed=0):
    return text(n, seed)


def eleven_bit_weights():
    """symbols 0..12: weights 11, 10, ..., 2, 1, 1 give codes of 1 to 11 bits"""
    w = [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 1]
    assert sum((1 << x) >> 1 for x in w) == 1 << 11
    return w


# ---------------------------------------------------------------- the streams
_VALID = []


def one_frame(build, **kw):
    f = Frame(**kw)
    build(f)
    return f.bytes(), bytes(f.out)


def straddling_stream():
    """a compressed block whose literal streams and whose sequence stream each cross an edge of the kernel's input windows -> (name,
    stream, out): four Huffman streams of more than a window each, and a sequence stream of more than a window"""
    f = Frame(checksum=True).raw(payload(256, 2))
    lits = text_lits(14 * WINDOW + 5, seed=3)
    seqs = [(3, 4 + (i % 7), 4 + (i * 37) % 200) for i in range(3 * WINDOW // 4)]
    f.compressed(lits, lits_huffman(lits, TEXT_WEIGHTS, fmt=3), seqs, last=True)
    stream = f.bytes()
    assert len(stream) > 3 * WINDOW
    return "straddle_windows", stream, bytes(f.out)


def valid_streams():
    """[(name, stream, what it must produce)]"""
    if _VALID:
        return _VALID
    out = _VALID

    def add(name, stream, data):
        out.append((name, bytes(stream), bytes(data)))

    def frame(name, build, **kw):
        add(name, *one_frame(build, **kw))
    frame("empty_frame", lambda f: f.raw(b"", last=True))
    for n in (0, 1, BLOCK_MAX):
        frame("raw_%d" % n, lambda f: f.raw(payload(n, n), last=True))
        frame("rle_%d" % n, lambda f: f.rle(0x41, n, last=True))
    frame("raw_then_rle_then_empty", lambda f: f.raw(b"abc").rle(0x7a, 300).raw(b"", last=True))
    # every header field: Single_Segment with each content-size width, a window with and without a content size, a checksum, a zero
    # Dictionary_ID of each width, the smallest and a large window
    body = payload(300, 5)
    for fcs in (1, 2, 4, 8):
        data = body[:200] if fcs == 1 else body
        frame("single_segment_fcs_%d" % fcs, lambda f: f.raw(data, last=True), single=True, fcs=fcs)
        frame("single_segment_fcs_%d_checksum" % fcs, lambda f: f.raw(data, last=True), single=True, fcs=fcs, checksum=True)
    for fcs in (0, 2, 4, 8):
        frame("window_fcs_%d" % fcs, lambda f: f.raw(body, last=True), fcs=fcs)
        frame("window_fcs_%d_checksum" % fcs, lambda f: f.raw(body, last=True), fcs=fcs, checksum=True)
    for did in (1, 2, 4):
        frame("dictionary_id_0_in_%d_bytes" % did, lambda f: f.raw(body, last=True), did_bytes=did)
    frame("window_1_kib", lambda f: f.raw(body).rle(1, 1024, last=True), window=0x00)
    frame("window_2_gib", lambda f: f.raw(body, last=True), window=(21 << 3))
    frame("fcs_2_of_256", lambda f: f.raw(payload(256, 1), last=True), fcs=2)
    for n in (0, 1, 31, 32, 33, 63, 64, 1000, 4096 + 32 + 7):
        frame("checksum_of_%d" % n, lambda f: f.raw(payload(n, 9), last=True), checksum=True)
    # frames back to back
    a, ao = one_frame(lambda f: f.raw(b"first frame, ", last=True), checksum=True)
    b, bo = one_frame(lambda f: f.rle(0x2e, 40, last=True), single=True)
    e, _eo = one_frame(lambda f: f.raw(b"", last=True))
    add("two_frames", a + b, ao + bo)
    add("three_frames_empty_and_skippable_between", a + e + skippable(13) + b + skippable(0, 7) + a, ao + bo + ao)
    add("skippable_first", skippable(5, 15) + a, ao)

    # ---- literals
    t37 = text_lits(37, 1)
    for fmt in (0, 1, 3):
        frame("literals_raw_fmt%d" % fmt, lambda f: f.compressed(t37[:20], lits_raw(t37[:20], fmt), [], last=True))
        frame("literals_rle_fmt%d" % fmt, lambda f: f.compressed(b"q" * 20, lits_rle(0x71, 20, fmt), [], last=True))
    frame("literals_raw_4095", lambda f: f.compressed(payload(4095), lits_raw(payload(4095)), [], last=True))
    frame("literals_raw_100000", lambda f: f.compressed(payload(100000), lits_raw(payload(100000)), [], last=True))
    frame("literals_rle_131072", lambda f: f.compressed(b"r" * BLOCK_MAX, lits_rle(0x72, BLOCK_MAX), [], last=True))
    frame("literals_huffman_one_stream", lambda f: f.compressed(t37, lits_huffman(t37, TEXT_WEIGHTS), [], last=True))
    for fmt, n in ((1, 4 * 9 + 1), (1, 4 * 9 + 2), (1, 4 * 9 + 3), (1, 4 * 9), (1, 6), (1, 9), (2, 1023), (2, 4001), (3, 16383), (3, 100003)):
        lits = text_lits(n, n)
        frame("literals_huffman_four_streams_fmt%d_%d" % (fmt, n), lambda f: f.compressed(lits, lits_huffman(lits, TEXT_WEIGHTS, fmt), [], last=True))
    t500 = text_lits(500, 2)
    frame("literals_treeless_after_compressed",
          lambda f: f.compressed(t37, lits_huffman(t37, TEXT_WEIGHTS), []).compressed(t500, lits_huffman(t500, TEXT_WEIGHTS, 1, treeless=True), [])
          .compressed(t37, lits_raw(t37), []).compressed(t500, lits_huffman(t500, TEXT_WEIGHTS, 0, treeless=True), [], last=True))
    w11 = eleven_bit_weights()
    l11 = bytes([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 11, 10, 0, 0, 5] * 9)
    frame("literals_huffman_11_bit_code", lambda f: f.compressed(l11, lits_huffman(l11, w11), [], last=True))
    frame("literals_huffman_two_symbols", lambda f: f.compressed(b"\0\1\1\0\0\0\1" * 5, lits_huffman(b"\0\1\1\0\0\0\1" * 5, [1, 1]), [], last=True))
    # the weights but the last through FSE: the weights of TEXT_WEIGHTS are 0 (most), 1, 2, 3, 4
    tw = TEXT_WEIGHTS[:-1]
    assert all(tw.count(k) > 0 for k in range(5))
    norm = [36, 7, 7, 7, 7]                                    # log 6
    frame("literals_huffman_fse_weights", lambda f: f.compressed(t500, lits_huffman(t500, TEXT_WEIGHTS, 0, tree=tree_fse(TEXT_WEIGHTS, norm, 6)), [], last=True))
    norm5 = [32 - 4 - 2 - 2 - 1, 4, 2, 2, -1]                  # log 5, a "less than 1" probability
    frame("literals_huffman_fse_weights_log5_low_probability",
          lambda f: f.compressed(t500, lits_huffman(t500, TEXT_WEIGHTS, 1, tree=tree_fse(TEXT_WEIGHTS, norm5, 5)), [], last=True))

    # ---- sequences
    base = text_lits(320, 7)
    B = len(base)

    def seq_frame(name, lits, seqs, **kw):
        frame(name, lambda f: f.raw(base).compressed(lits, lits_raw(lits), seqs, last=True, **kw), checksum=True)
    for n in (1, 127, 128, 0x7eff + 1):
        lits = text_lits(n, n)
        seq_frame("sequences_%d" % n, lits, [(1, 3 + (i % 5 if n < 1000 else 0), 4 + i % 60) for i in range(n)])   # (a block regenerates 128 KiB at most)
    # every LL and ML code's base and top value, a block each (a block regenerates 128 KiB at most: that caps the last code's top value)
    f = Frame(checksum=True).raw(base)
    for c in range(36):
        for v in (LL_BASE[c], min(LL_BASE[c] + (1 << LL_BITS[c]) - 1, BLOCK_MAX - 3)):
            f.compressed(bytes([65 + c]) * v, lits_rle(65 + c, v), [(v, 3, 4 + c)])
    for c in range(53):
        for v in (ML_BASE[c], min(ML_BASE[c] + (1 << ML_BITS[c]) - 1, BLOCK_MAX - 1)):
            f.compressed(b"x", lits_raw(b"x"), [(1, v, 4 + c)])
    f.raw(b"", last=True)
    add("sequences_every_length_code_base_and_top", f.bytes(), f.out)
    # offset codes 0..20: a frame that has produced 2^20 + 8 bytes first (RLE blocks of a counter would not do: random bytes)
    f = Frame(checksum=True)
    big = payload(BLOCK_MAX, 11)
    for k in range(9):
        f.raw(big[k:] + big[:k])
    # code 0 (value 1: the first repeat offset), code 1 at its base (2: the second), codes 2..19 at their top value, 20 inside what is produced
    seqs = [(2, 5, 1), (2, 5, 2)] + [(2, 5, (2 << c) - 1) for c in range(2, 20)] + [(2, 5, (1 << 20) + 12345)]
    lits = text_lits(2 * len(seqs), 4)
    f.compressed(lits, lits_raw(lits), seqs, last=True)
    add("sequences_offset_codes_0_to_20", f.bytes(), f.out)
    # the repeat offsets: every rule, with and without literals in front
    reps = [(4, 5, 13 + 3), (3, 4, 1), (3, 4, 2), (3, 4, 3), (0, 4, 1), (0, 4, 2), (0, 4, 3), (2, 4, 29 + 3), (0, 5, 3), (1, 3, 2), (0, 3, 1), (5, 6, 3), (0, 7, 2)]
    lits = text_lits(sum(s[0] for s in reps) + 3, 5)
    seq_frame("sequences_repeat_offsets", lits, reps)
    # modes: RLE tables, FSE_Compressed tables (a -1 probability, a zero-repeat run), Repeat after FSE_Compressed and after RLE
    ll_t = Fse([20, 10, 0, 0, 0, 0, 0, 0, 1, -1], 5)           # codes 0, 1, 8, 9; six zero probabilities between: flags 3, 2
    of_t = Fse([0, 0, 8, 8, 8, 4, 2, 1, -1], 5)                # codes 2..8
    ml_t = Fse([40, 20, 2, -1, -1], 6)                         # codes 0..4
    fs = [([0, 1, 8, 9][i % 4], 3 + i % 5, (1 << (2 + i % 7)) + i % 3) for i in range(60)]
    lits = text_lits(sum(s[0] for s in fs) + 1, 6)
    seq_frame("sequences_fse_compressed_tables", lits, fs, tables={"ll": ll_t, "of": of_t, "ml": ml_t})
    rl = [(2, 7, 5)] * 9
    seq_frame("sequences_rle_tables", text_lits(18, 8), rl, tables={"ll": RleTable(2), "of": RleTable(2), "ml": RleTable(4)})
    seq_frame("sequences_mixed_modes", lits, [(s[0], 7, s[2]) for s in fs], tables={"ll": ll_t, "ml": RleTable(4)})
    f = Frame(checksum=True).raw(base)
    f.compressed(lits, lits_raw(lits), fs, tables={"ll": ll_t, "of": of_t, "ml": ml_t})
    f.compressed(lits, lits_raw(lits), fs[::-1], tables={"ll": ll_t, "of": of_t, "ml": ml_t}, modes={"ll": 3, "of": 3, "ml": 3})
    f.compressed(text_lits(18, 8), lits_raw(text_lits(18, 8)), rl, tables={"ll": RleTable(2), "of": of_t, "ml": RleTable(4)}, modes={"of": 3})
    f.compressed(text_lits(18, 8), lits_raw(text_lits(18, 8)), rl, tables={"ll": RleTable(2), "of": of_t, "ml": RleTable(4)}, modes={"ll": 3, "of": 3, "ml": 3})
    f.compressed(t37, lits_huffman(t37, TEXT_WEIGHTS), [(5, 9, 44)])
    f.compressed(t37, lits_huffman(t37, TEXT_WEIGHTS, treeless=True), [(5, 9, 1), (0, 3, 1)], tables={"ll": PREDEFINED["ll"], "of": PREDEFINED["of"], "ml": PREDEFINED["ml"]},
                 modes={"ll": 3, "of": 3, "ml": 3}, last=True)
    add("sequences_repeat_mode_after_fse_rle_and_predefined", f.bytes(), f.out)

    # ---- copies
    f = Frame(checksum=True).raw(b"a")
    for _ in range(8):
        f.compressed(b"", lits_raw(b""), [(0, 125000, 1 + 3)])
    f.raw(b"", last=True)
    add("offset_1_times_1000000", f.bytes(), f.out)
    seq_frame("offset_equals_length", b"", [(0, 64, 64 + 3), (0, 128, 128 + 3), (0, 5, 5 + 3)])
    seq_frame("offset_equals_produced", b"zz", [(2, 40, B + 2 + 3), (0, 70, B + 42 + 3)])

    def ring_frame(name, offsets, fill=5 * RING):
        f = Frame(checksum=True)
        data = payload(fill, 21)
        for at in range(0, fill, BLOCK_MAX):
            f.raw(data[at:at + BLOCK_MAX])
        seqs = [(3, 600 + 17 * i, off + 3) for i, off in enumerate(offsets)]
        lits = text_lits(3 * len(seqs) + 2, 9)
        f.compressed(lits, lits_raw(lits), seqs, last=True)
        add(name, f.bytes(), f.out)
    ring_frame("offsets_around_the_ring", [RING - 1, RING, RING + 1, 2 * RING + 5, RING - 600, RING + 600, 3 * RING, 5 * RING, 1, RING + 1])
    # a far match long enough to run into bytes that were not flushed when it began: offset RING + 16, 100000 bytes
    ring_frame("far_match_into_unflushed_bytes", [RING + 16], fill=2 * RING)
    f = Frame(checksum=True)
    data = payload(2 * RING, 22)
    f.raw(data)
    f.compressed(b"", lits_raw(b""), [(0, 100000, RING + 16 + 3), (0, 30000, 2 * RING + 1 + 3)], last=True)
    add("far_match_of_100000", f.bytes(), f.out)
    add(*straddling_stream())
    return out


def pyarrow_inputs():
    rng = np.random.default_rng(5)
    txt = b"".join(b"line %d of the text, value=%d;\n" % (i, i * i % 977) for i in range(12000))
    rnd = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    mix = (txt + rnd + bytes(200000) + txt[::-1] + rnd[:50000] + txt)[:900000]
    return [("text", txt), ("zeros", bytes(300000)), ("random", rnd), ("mix_900k", mix)]


LEVELS = (-5, 1, 3, 9, 19)


def zs(data, level=3):
    import pyarrow as pa
    return pa.Codec("zstd", compression_level=level).compress(data, asbytes=True)


def pyarrow_streams():
    return [("pyarrow_%s_level_%d" % (name, level), zs(data, level), data) for name, data in pyarrow_inputs() for level in LEVELS]


# ---------------------------------------------------------------- corrupt streams
def small_frame():
    """one small frame with a compressed block: Huffman literals in four streams, FSE-compressed tables, a checksum and a content size ->
    (stream, out, {field: position})"""
    f = Frame(fcs=2, checksum=True).raw(b"0123456789" * 6)
    lits = text_lits(300, 12)
    ll_t = Fse([20, 10, 0, 0, 0, 0, 0, 0, 1, -1], 5)
    seqs = [([0, 1, 8, 9][i % 4], 3 + i % 5, 4 + i % 50) for i in range(12)]
    f.compressed(lits, lits_huffman(lits, TEXT_WEIGHTS, 1), seqs, tables={"ll": ll_t}, last=True)
    return f.bytes(), bytes(f.out)


def invalid_streams():
    """[(name, stream, expected length, a word of the sub-case's text)]: each is refused by the twin with that sub-case, and by libzstd"""
    out = []
    good, gout = small_frame()
    n = len(gout)

    def add(name, stream, expected, word):
        out.append((name, bytes(stream), expected, word))

    def frame(name, build, word, expected=None, **kw):
        f = Frame(**kw)
        build(f)
        add(name, f.bytes(), len(f.out) if expected is None else expected, word)
    add("empty_for_one", b"", 1, "empty stream")
    add("impossible", good, 32768 * len(good) + 1, "32768")
    add("too_short", good[:8], 0, "fewer than the 9 bytes")
    add("bad_magic", b"\x28\xb5\x2f\xfc" + good[4:], n, "begins with neither")
    add("bad_magic_second_frame", good + b"\x28\xb5\x2f\xfc" + good[4:], 2 * n, "begins with neither")
    frame("reserved_bit", lambda f: f.raw(b"abc", last=True), "reserved bit", reserved=8)
    frame("dictionary_id", lambda f: f.raw(b"abc", last=True), "dictionary ID", did_bytes=1, did=7)
    frame("dictionary_id_4_bytes", lambda f: f.raw(b"abc", last=True), "dictionary ID", did_bytes=4, did=1 << 24)
    frame("window_above_2_gib", lambda f: f.raw(b"abc", last=True), "window above", window=(22 << 3))
    # The input cut at every byte. Below the 9 bytes of the smallest frame the sizes alone refuse it. From there on the decoder meets the
    # end where it asks for a header's bytes, a block header, a block's Block_Size bytes (asked for BEFORE the block is entered, so a cut
    # inside a compressed block's sections shows here and not as a block that ends inside a section) or the checksum: always "the input
    # ends inside a frame".
    CUT = "the input ends inside a frame"
    for k in range(1, len(good)):
        add("cut_at_%d" % k, good[:k], n, CUT if k >= 9 else "fewer than the 9 bytes")
    # a frame with the longest header (a window, a 4-byte zero Dictionary_ID, an 8-byte content size: 18 bytes), cut inside every field
    f = Frame(did_bytes=4, fcs=8, checksum=True)
    f.raw(b"abcdef", last=True)
    long_frame, lout = f.bytes(), bytes(f.out)
    assert len(long_frame) == 18 + 3 + 6 + 4
    for k in range(1, len(long_frame)):
        add("long_header_cut_at_%d" % k, long_frame[:k], len(lout), CUT if k >= 9 else "fewer than the 9 bytes")
    # ... and as the SECOND frame: fewer than 4 bytes of it cannot be another frame, more are a frame that the input ends in
    for k in range(1, len(long_frame)):
        add("second_frame_cut_at_%d" % k, good + long_frame[:k], n + len(lout), "left over" if k < 4 else CUT)
    add("second_frame_missing", good, n + len(lout), "before the expected length")
    add("extended_by_one", good + b"\0", n, "left over")
    add("extended_by_three", good + b"\x28\xb5\x2f", n, "left over")
    add("expected_one_more", good, n + 1, "before the expected length")
    add("expected_one_less", good, n - 1, "content size")
    nf, nfo = one_frame(lambda f: f.compressed(b"abcd", lits_raw(b"abcd"), [(4, 8, 2 + 3)], last=True))     # no content size: only the blocks say
    add("no_fcs_expected_one_more", nf, len(nfo) + 1, "before the expected length")
    add("no_fcs_expected_one_less", nf, len(nfo) - 1, "past the expected length")
    rf, rfo = one_frame(lambda f: f.raw(b"abcdef", last=True))
    add("raw_block_past_expected", rf, 5, "past the expected length")
    lf, _ = one_frame(lambda f: f.rle(7, 100, last=True))
    add("rle_block_past_expected", lf, 99, "past the expected length")
    for bit in range(32):
        add("checksum_bit_%d" % bit, good[:-4] + (int.from_bytes(good[-4:], "little") ^ 1 << bit).to_bytes(4, "little"), n, "content checksum that does not match")
    for d in (-1, 1):
        f = Frame(fcs=2)
        f.raw(payload(400, 1), last=True)
        f.fcs_value = 400 + d
        add("fcs_lies_by_%+d" % d, f.bytes(), 400, "content size")
    frame("block_type_3", lambda f: f.raw_block_bytes(3, 1, b"\0", last=True), "block type 3", expected=1)
    frame("block_cut_inside_literals", lambda f: f.raw_block_bytes(2, 3, lits_raw(b"abcdef")[:3], last=True), "ends inside one of its sections", expected=6)
    frame("block_without_sequence_count", lambda f: f.raw_block_bytes(2, 4, lits_raw(b"abc"), last=True), "ends inside one of its sections", expected=3)
    frame("literals_above_128_kib", lambda f: f.raw_block_bytes(2, 4, _lits_head(1, 3, BLOCK_MAX + 1) + b"x", last=True), "literals section", expected=BLOCK_MAX + 1)
    t37 = text_lits(37, 1)
    t6 = text_lits(5, 1)
    frame("four_streams_for_5_literals", lambda f: f.compressed(t6, lits_huffman(t6, TEXT_WEIGHTS, 1), [], last=True), "literals section")
    frame("treeless_without_a_tree", lambda f: f.compressed(t37, lits_huffman(t37, TEXT_WEIGHTS, treeless=True), [], last=True), "treeless")
    a, ao = one_frame(lambda f: f.compressed(t37, lits_huffman(t37, TEXT_WEIGHTS), [], last=True))
    b, bo = one_frame(lambda f: f.compressed(t37, lits_huffman(t37, TEXT_WEIGHTS, treeless=True), [], last=True))
    add("treeless_with_the_tree_of_another_frame", a + b, len(ao) + len(bo), "treeless")
    # a jump table that states more than the section holds
    sec = bytearray(lits_huffman(text_lits(100, 3), TEXT_WEIGHTS, 1))
    at = 3 + len(tree_direct(TEXT_WEIGHTS))
    sec[at + 4:at + 6] = (500).to_bytes(2, "little")
    frame("jump_table_beyond_the_section", lambda f: f.raw_block_bytes(2, len(sec) + 1, bytes(sec) + b"\0", last=True), "literals section", expected=100)
    # weights
    frame("weights_sum_not_completable", lambda f: f.compressed(t37, lits_huffman(t37, TEXT_WEIGHTS, tree=tree_direct([3, 1, 0])), [], last=True, model=False), "bad weights", expected=37)
    frame("weights_all_zero", lambda f: f.compressed(t37, lits_huffman(t37, TEXT_WEIGHTS, tree=tree_direct([0, 0, 0])), [], last=True, model=False), "bad weights", expected=37)
    frame("weights_odd_number_of_ones", lambda f: f.compressed(t37, lits_huffman(t37, TEXT_WEIGHTS, tree=tree_direct([2, 1, 0])[:1] + bytes([0x31, 0x10])), [], last=True, model=False),
          "bad weights", expected=37)
    frame("weight_13", lambda f: f.compressed(t37, lits_huffman(t37, TEXT_WEIGHTS, tree=bytes([128, 0xd0])), [], last=True, model=False), "bad weights", expected=37)
    # Huffman streams
    sec = bytearray(lits_huffman(t37, TEXT_WEIGHTS))
    sec[-1] = 0
    frame("huffman_stream_without_marker", lambda f: f.raw_block_bytes(2, len(sec) + 1, bytes(sec) + b"\0", last=True), "final-bit marker", expected=37)
    frame("huffman_stream_states_one_literal_more", lambda f: f.compressed(t37, lits_huffman(t37, TEXT_WEIGHTS, sizes=(38, len(lits_huffman(t37, TEXT_WEIGHTS)) - 3)), [], last=True),
          "not consumed exactly", expected=38)
    frame("huffman_stream_states_one_literal_fewer", lambda f: f.compressed(t37, lits_huffman(t37, TEXT_WEIGHTS, sizes=(36, len(lits_huffman(t37, TEXT_WEIGHTS)) - 3)), [], last=True),
          "not consumed exactly", expected=36)
    # sequences
    lits = text_lits(10, 2)
    base = text_lits(64, 7)

    def seq_frame(name, seqs, word, expected=None, lits=lits, **kw):
        f = Frame()
        f.raw(base).compressed(lits, lits_raw(lits), seqs, last=True, model=False, **kw)
        add(name, f.bytes(), 64 + len(lits) + sum(s[1] for s in seqs) if expected is None else expected, word)
    seq_frame("sequence_mode_reserved_bits", [(2, 5, 9)], "sequences section header", reserved=1)
    f = Frame().raw_block_bytes(2, 3, lits_raw(b"") + b"\0\0", last=True)
    add("bytes_behind_a_sequence_count_of_0", f.bytes(), 0, "sequences section header")
    seq_frame("repeat_mode_without_a_table", [(2, 5, 9)], "repeat mode", modes={"of": 3})
    for name, sym in (("ll", 36), ("of", 32), ("ml", 53)):
        f = Frame().raw(base)
        body = lits_raw(lits) + seq_count(1) + bytes([{"ll": 1 << 6, "of": 1 << 4, "ml": 1 << 2}[name], sym]) + b"\x01"
        f.raw_block_bytes(2, len(body), body, last=True)
        add("rle_%s_symbol_above_the_alphabet" % name, f.bytes(), 64 + 10 + 3, "bad FSE table")
    seq_frame("accuracy_log_above_the_limit", [(0, 3, 5)] * 4, "bad FSE table", tables={"of": Fse([0, 0] + [1 << 8, 1 << 7, 1 << 7], 9)}, lits=b"")
    seq_frame("symbol_above_the_alphabet", [(0, 3, 5)] * 4, "bad FSE table", tables={"ll": Fse([32] + [0] * 35 + [32], 6)}, lits=b"")
    over = Fse([29] + [1] * 35, 6)
    over.norm = [1] * 36                                       # described as 36 of 64 cells over the whole alphabet: the sum never lands
    seq_frame("probabilities_do_not_sum", [(0, 3, 5)] * 4, "bad FSE table", tables={"ll": over}, lits=b"")
    f = Frame().raw(base)
    body = bytearray(lits_raw(lits) + sequences([(2, 5, 9), (3, 4, 10)]))
    body[-1] = 0
    f.raw_block_bytes(2, len(body), bytes(body), last=True)
    add("sequence_stream_without_marker", f.bytes(), 64 + 10 + 9, "final-bit marker")
    f = Frame().raw(base)
    body = lits_raw(lits) + sequences([(2, 5, 9), (3, 4, 10)]) + b"\x01"
    f.raw_block_bytes(2, len(body), body, last=True)
    add("sequence_stream_with_a_byte_too_many", f.bytes(), 64 + 10 + 9, "not consumed exactly")
    f = Frame().raw(base)
    body = lits_raw(lits) + seq_count(3) + sequences([(2, 5, 9), (3, 4, 10)])[1:]
    f.raw_block_bytes(2, len(body), body, last=True)
    add("sequence_count_one_too_many", f.bytes(), 64 + 10 + 12, "not consumed exactly")
    seq_frame("sequence_asks_for_more_literals", [(2, 5, 9), (9, 4, 10)], "more literals", expected=64 + 11 + 9)
    seq_frame("offset_one_past_the_produced_bytes", [(2, 5, 67 + 3)], "match offset")
    seq_frame("offset_far_past_the_produced_bytes", [(2, 5, (1 << 28) + 3)], "match offset")
    seq_frame("repeat_offset_1_minus_1_is_0", [(0, 5, 3)], "match offset", lits=b"")
    # in the second frame: the first frame's bytes are no sources (on the device the ring still holds them)
    first, fo = one_frame(lambda f: f.raw(payload(100, 3), last=True))
    f = Frame()
    f.raw(base).compressed(lits, lits_raw(lits), [(2, 5, 67 + 3)], last=True, model=False)
    add("offset_one_past_the_produced_bytes_second_frame", first + f.bytes(), 100 + 64 + 15, "match offset")
    seq_frame("match_past_expected", [(2, 5, 9)], "past the expected length", expected=64 + 10 + 4)
    short, _o = one_frame(lambda f: f.raw(b"abcdef", last=True))
    add("output_short_of_expected", short, 7, "before the expected length")
    return out


def stricter_streams():
    """refused here, read by libzstd: [(name, stream, expected length, word)]"""
    out = []
    # a Huffman code of 12 bits: libzstd's tables take it, RFC 8878 says 11
    w12 = [12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 1]
    lits = bytes(range(13)) * 3
    codes, bits = huffman_codes(w12)
    assert bits == 12
    f = Frame()
    f.compressed(lits, lits_huffman(lits, w12), [], last=True)
    out.append(("huffman_code_of_12_bits", f.bytes(), len(lits), "bad weights"))
    # Block_Maximum_Size (here: a window of 1 KiB): libzstd's one-shot decoder holds no block to it
    for name, build, word in (("block_above_block_maximum", lambda f: f.raw(payload(1025), last=True), "block size above"),
                              ("rle_block_above_block_maximum", lambda f: f.rle(1, 1025, last=True), "block size above"),
                              ("block_regenerates_more_than_block_maximum", lambda f: f.raw(b"x" * 64).compressed(b"", lits_raw(b""), [(0, 1025, 4)], last=True), "regenerates more")):
        f = Frame(window=0x00)
        build(f)
        out.append((name, f.bytes(), len(f.out), word))
    return out


# ---------------------------------------------------------------- Parquet files with ZSTD pages

_CACHE = {}


def generate(dirpath):
    """every well-formed ZSTD case: {name: parquet_cases.Case}. Written once per directory, under names of their own (zs_*)."""
    key = str(dirpath)
    if key in _CACHE:
        return _CACHE[key]
    out = {}

    def add(name, table, **kw):
        out[name] = P._write(dirpath, "zs_" + name, table, compression="ZSTD", **kw)
    m = P.matrix_table(N)
    for ver, v in (("v1", "1.0"), ("v2", "2.0")):
        for dic, d in (("dict", None), ("plain", False)):
            add("matrix_%s_%s_3groups" % (ver, dic), m, data_page_version=v, use_dictionary=d, row_group_size=7000)
        add("matrix_%s_dict_3groups_pages37" % ver, m, data_page_version=v, row_group_size=7000, max_rows_per_page=37)
    nulls = P.null_patterns_table()
    add("nulls_v1", nulls, max_rows_per_page=5000)
    add("nulls_v2_plain", nulls, data_page_version="2.0", use_dictionary=False, max_rows_per_page=5000)
    for kind in ("long", "straddle", "empty"):
        add("varchar_" + kind, P.varchar_table(kind))
        add("varchar_" + kind + "_plain_v2", P.varchar_table(kind), use_dictionary=False, data_page_version="2.0")
    add("zeros_v1", SN.zeros_table(), use_dictionary=False)
    add("random_v2", SN.random_table(), use_dictionary=False, data_page_version="2.0")
    add("text_v1", SN.text_table(), use_dictionary=False, max_rows_per_page=1 << 20, data_page_size=2 << 20)   # ONE page: a section of about 900 KB
    add("text_v2_level_19", SN.text_table(), use_dictionary=False, max_rows_per_page=1 << 20, data_page_size=2 << 20, data_page_version="2.0", compression_level=19)
    add("matrix_level_1", m, compression_level=1, row_group_size=7000)
    add("matrix_level_19", m, compression_level=19, data_page_version="2.0")
    for n in (0, 1, 64, 65):
        add("rows_%d" % n, P.matrix_table(n, seed=100 + n), max_rows_per_page=37 if n > 64 else None)
    _CACHE[key] = out
    return out


CASE_NAMES = ["matrix_%s_%s_3groups" % (v, d) for v in ("v1", "v2") for d in ("dict", "plain")] + ["matrix_v1_dict_3groups_pages37", "matrix_v2_dict_3groups_pages37"] + \
             ["nulls_v1", "nulls_v2_plain"] + ["varchar_" + k + s for k in ("long", "straddle", "empty") for s in ("", "_plain_v2")] + \
             ["zeros_v1", "random_v2", "text_v1", "text_v2_level_19", "matrix_level_1", "matrix_level_19"] + ["rows_%d" % n for n in (0, 1, 64, 65)]

MIXED_CODECS = {"i32_n": "SNAPPY", "i32_r": "GZIP", "i64_n": "NONE", "i64_r": "LZ4_RAW", "date_n": "ZSTD", "date_r": "NONE", "d9_n": "LZ4_RAW", "d9_r": "ZSTD",
                "d15_n": "GZIP", "d15_r": "ZSTD", "s300_n": "ZSTD", "s300_r": "SNAPPY", "s40_n": "NONE", "s40_r": "ZSTD"}

_FLAGGED = {}


def flagged_files(dirpath):
    """{name: (Case, the flags it loads with besides PH_PARQUET_ZSTD)}: one file whose columns are ZSTD, GZIP, SNAPPY, LZ4_RAW and
    UNCOMPRESSED (flags 1 | 16 | 64), and delta-encoded files inside ZSTD pages, v1 and v2 (flags 4)"""
    key = str(dirpath)
    if key not in _FLAGGED:
        m = P.matrix_table(3000, seed=9)
        _FLAGGED[key] = {
            "mixed_codecs": (P._write(dirpath, "zs_mixed", m, compression=MIXED_CODECS, row_group_size=1100, data_page_version="2.0"), 1 | 16 | 64),
            "delta_v1": (D.write_delta(dirpath, "zs_delta_v1", m, compression="ZSTD", row_group_size=1100), 4),
            "delta_v2": (D.write_delta(dirpath, "zs_delta_v2", m, compression="ZSTD", data_page_version="2.0"), 4),
        }
    return _FLAGGED[key]


def patch_sources(dirpath):
    """the small ZSTD files the patches start from: pages of 37 rows, v1, PLAIN"""
    import pyarrow as pa
    n = 100
    period = np.random.default_rng(40).integers(0, 40, 7)[np.arange(n) % 7] * 1000003
    req = pa.Table.from_arrays([pa.array(period)], schema=pa.schema([pa.field("p", pa.int64(), nullable=False)]))
    matches = P._write(dirpath, "zs_patch_matches", req, compression="ZSTD", use_dictionary=False, max_rows_per_page=37, data_page_version="1.0")
    skewed = np.frombuffer(text(8 * n, 42), np.int64)             # bytes of a skewed alphabet: Huffman literals
    huffman = pa.Table.from_arrays([pa.array(skewed)], schema=pa.schema([pa.field("h", pa.int64(), nullable=False)]))
    huffman = P._write(dirpath, "zs_patch_huffman", huffman, compression="ZSTD", use_dictionary=False, max_rows_per_page=37, data_page_version="1.0")
    rnd = np.random.default_rng(41).integers(-2**63, 2**63 - 1, n)
    mask = np.arange(n) % 5 == 2
    levels = P._write(dirpath, "zs_patch_levels", pa.table({"a": pa.array(rnd, mask=mask)}), compression="ZSTD", use_dictionary=False, max_rows_per_page=37,
                      data_page_version="1.0")
    zeros = pa.Table.from_arrays([pa.array(np.zeros(600000, np.int64))], schema=pa.schema([pa.field("z", pa.int64(), nullable=False)]))
    zeros = P._write(dirpath, "zs_patch_zeros", zeros, compression="ZSTD", use_dictionary=False, max_rows_per_page=200000, data_page_size=4 << 20, data_page_version="1.0")
    return {"matches": matches, "huffman": huffman, "levels": levels, "zeros": zeros}


def layout(stream):
    """where the parts of a frame's FIRST block lie: {block, block_type, block_end, last, lits_type, lits_end}"""
    assert stream[:4] == b"\x28\xb5\x2f\xfd"
    fhd = stream[4]
    single, fcs_flag = fhd >> 5 & 1, fhd >> 6
    pos = 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3] + ((1 if single else 0), 2, 4, 8)[fcs_flag]
    bh = int.from_bytes(stream[pos:pos + 3], "little")
    block = pos + 3
    out = {"block": block, "block_type": bh >> 1 & 3, "block_end": block + (bh >> 3 if bh >> 1 & 3 != 1 else 1), "last": bh & 1}
    if out["block_type"] == 2:
        b0 = stream[block]
        kind, fmt = b0 & 3, b0 >> 2 & 3
        if kind < 2:
            hl = 1 if fmt in (0, 2) else 2 if fmt == 1 else 3
            n = int.from_bytes(stream[block:block + hl], "little") >> (3 if hl == 1 else 4)
            out["lits_end"] = block + hl + (n if kind == 0 else 1)
        else:
            hl, sb = (3, 3, 4, 5)[fmt], (10, 10, 14, 18)[fmt]
            out["lits_end"] = block + hl + (int.from_bytes(stream[block:block + hl], "little") >> (4 + sb) & ((1 << sb) - 1))
        out["lits_type"] = kind
    return out


def patched(dirpath, pages_of):
    """{name: (original bytes, patched bytes, column, the page the message must name, a word of the message)}: a ZSTD file with a byte or
    two changed, located through the page directory (pages_of(data, column) -> ph_parquet_pages_ex entries) and the format's layout. Each
    must give PH_EINVAL."""
    src = patch_sources(dirpath)
    out = {}

    def put(name, data, at, new, page, word, column=0):
        new = bytes([new]) if isinstance(new, int) else new
        assert data[at:at + len(new)] != new, (name, at, new)
        out[name] = (data, data[:at] + new + data[at + len(new):], column, page, word)
    d = src["matches"].data
    pages = pages_of(d, 0)
    assert [p["kind"] for p in pages] == [0, 0, 0] and all(p["compressed"] == 1 and p["codec"] == 6 for p in pages)
    top = lambda byte: byte ^ 1 << (byte.bit_length() - 1)       # a stream's last byte without its final-bit marker: every bit behind it moves
    for k, p in enumerate(pages):
        stream = d[p["data_pos"]:p["data_pos"] + p["data_bytes"]]
        lay = layout(stream)                                       # libzstd's frame for a small input: ONE compressed last block, sequences in it
        assert lay["last"] and lay["block_type"] == 2 and lay["block_end"] == len(stream) and stream[lay["lits_end"]] > 0 and p["uncompressed_bytes"] == p["num_values"] * 8
        put("sequence_bit_page%d" % k, d, p["data_pos"] + len(stream) - 1, top(stream[-1]), k, "corrupt ZSTD stream")
    h = src["huffman"].data
    for k, p in enumerate(pages_of(h, 0)):
        stream = h[p["data_pos"]:p["data_pos"] + p["data_bytes"]]
        lay = layout(stream)
        assert p["codec"] == 6 and lay["block_type"] == 2 and lay["lits_type"] == 2                  # Huffman literals
        at = lay["lits_end"] - 1
        # (a flipped code bit may give another literal of the same length, which no frame without a checksum notices: the marker it is)
        put("huffman_marker_page%d" % k, h, p["data_pos"] + at, 0, k, "corrupt ZSTD stream")
    put("magic_page1", d, pages[1]["data_pos"] + 3, 0xfc, 1, "begins with neither")
    put("reserved_bit_page2", d, pages[2]["data_pos"] + 4, d[pages[2]["data_pos"] + 4] | 8, 2, "corrupt ZSTD stream")
    lv = src["levels"].data
    p = pages_of(lv, 0)[1]
    at = p["header_pos"] + 3
    assert lv[at - 1] == 0x15 and lv[at] & 0x80 and lv[at + 1] < 0x80 and lv[at + 2] == 0x15
    assert ((lv[at] & 0x7f) | lv[at + 1] << 7) >> 1 == p["uncompressed_bytes"] and 2 <= (lv[at] & 0x7f) <= 0x7d
    put("uncompressed_size_plus_1", lv, at, lv[at] + 2, 1, "corrupt ZSTD stream")    # (zigzag: the value's bit 0 is the varint's bit 1)
    put("uncompressed_size_minus_1", lv, at, lv[at] - 2, 1, "corrupt ZSTD stream")
    # pages of 200000 zeros are a few dozen bytes each: the size's varint with its top byte raised asks for more than 32768 times that
    z = src["zeros"].data
    p = pages_of(z, 0)[1]
    at = p["header_pos"] + 3
    assert z[at - 1] == 0x15 and z[at] & 0x80 and z[at + 1] & 0x80 and z[at + 2] & 0x80 and z[at + 3] < 0x80 and z[at + 4] == 0x15
    assert ((z[at] & 0x7f) | (z[at + 1] & 0x7f) << 7 | (z[at + 2] & 0x7f) << 14 | z[at + 3] << 21) >> 1 == p["uncompressed_bytes"] == 200000 * 8
    assert (0x7f << 21) >> 1 > 32768 * p["data_bytes"] and p["codec"] == 6 and p["compressed"] == 1
    put("uncompressed_size_impossible", z, at + 3, 0x7f, 1, "32768")
    # a nullable column, v1: [4-byte length n][levels, n bytes][values] is ONE stream. Random values do not compress, so libzstd stores them
    # in a raw block: the length's top byte lies open behind the frame header and the block header
    d = src["levels"].data
    pages = pages_of(d, 0)
    for k in (0, 2):
        p = pages[k]
        stream = d[p["data_pos"]:p["data_pos"] + p["data_bytes"]]
        lay = layout(stream)
        assert p["compressed"] == 1 and p["codec"] == 6 and lay["last"] and lay["block_type"] == 0 and lay["block_end"] == len(stream)   # one raw block
        assert lay["block_end"] - lay["block"] == p["uncompressed_bytes"] and 0 < int.from_bytes(stream[lay["block"]:lay["block"] + 4], "little") < 16
        put("level_prefix_page%d" % k, d, p["data_pos"] + lay["block"] + 3, 0x7f, k, "a level section of")
    return out


def two_bad_pages(dirpath, pages_of):
    """pages 1 and 2 of one column both carry a Huffman stream without its marker -> (bytes, column)"""
    cases = patched(dirpath, pages_of)
    orig, one = cases["huffman_marker_page1"][:2]
    two = cases["huffman_marker_page2"][1]
    both = bytearray(one)
    for i, (a, b) in enumerate(zip(orig, two)):
        if a != b:
            both[i] = b
    return bytes(both), 0


def write_patched(dirpath, pages_of):
    """the patched files on disk, for the stand-alone sanitizer program -> [path]"""
    paths = []
    for name, case in patched(dirpath, pages_of).items():
        path = os.path.join(str(dirpath), "zs_bad_" + name + ".parquet")
        with open(path, "wb") as f:
            f.write(case[1])
        paths.append(path)
    return paths
