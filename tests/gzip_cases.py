"""Inputs of the GZIP tests, shared by the CPU tests (tests/test_gzip_reference.py: the host twin) and the GPU tests
(tests/test_gpu_parquet_gzip.py): GZIP streams built bit by bit with a writer that models its own output — stored, fixed and dynamic blocks
at the edges of every field, members and header fields, codes that straddle the inflate kernel's input window, an output that wraps its ring
— zlib's own output, the corrupt streams with the sub-case each must be refused for, the lists on which this decoder and pyarrow's codec
differ on purpose, and Parquet files written with compression="GZIP" and the writer knobs of tests/parquet_cases.py, plus patches of such
files.

A stream (RFC 1952): members of [1f 8b 08 FLG MTIME(4) XFL OS][FEXTRA][FNAME][FCOMMENT][FHCRC][DEFLATE blocks][CRC32][ISIZE]. DEFLATE
(RFC 1951) packs bits from bit 0 of each byte upwards; Huffman codes go in most significant bit first, everything else least."""
import functools
import os
import zlib

import numpy as np

import delta_cases as D
import parquet_cases as P
import snappy_cases as SN

WINDOW = 4096         # plan_amd/csrc/gzip_decompress.h: GZ_TILE, the bytes of a stream the kernel stages in LDS at a time
RING = 32768          # plan_amd/csrc/gzip_decompress.h: GZ_RING, the output bytes the kernel keeps in LDS
N = P.N
payload = SN.payload

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_LENS = [4] * 13 + [5] * 6                                    # a complete code over the 19 code length symbols: 13/16 + 6/32
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def canonical(lens):
    """{symbol: (code, length)} of the canonical Huffman code with these lengths"""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    code, first = 0, [0] * 16
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        first[n] = code
    out = {}
    for sym, n in enumerate(lens):
        if n:
            out[sym] = (first[n], n)
            first[n] += 1
    return out


def complete_lens(k):
    """lengths of a complete code over k symbols (k = 1: one code of 1 bit, the incomplete set zlib accepts)"""
    if k == 1:
        return [1]
    top = (k - 1).bit_length()
    short = (1 << top) - k
    return [top - 1] * short + [top] * (k - short)


def length_symbol(n):
    s = max(i for i in range(29) if LBASE[i] <= n) if n < 258 else 28
    return 257 + s, n - LBASE[s], LEXTRA[s]


def distance_symbol(d):
    s = max(i for i in range(30) if DBASE[i] <= d)
    return s, d - DBASE[s], DEXTRA[s]


class Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, n):
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):                                    # a Huffman code: its most significant bit first
        self.put(int(format(code, "0%db" % n)[::-1], 2), n)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def pos(self):                                              # in bits
        return 8 * len(self.out) + self.n


class Deflate:
    """one member's DEFLATE stream and what it inflates to"""
    def __init__(self):
        self.w, self.out = Bits(), bytearray()
        self.lit = self.dist = None

    def stored(self, data, final=False, nlen=None, pad=0):
        self.w.put(int(final), 1)
        self.w.put(0, 2)
        if self.w.n:
            self.w.put(pad, 8 - self.w.n)
        self.w.put(len(data), 16)
        self.w.put(~len(data) & 0xffff if nlen is None else nlen, 16)
        self.w.out += data
        self.out += data
        return self

    def fixed(self, final=False):
        self.w.put(int(final), 1)
        self.w.put(1, 2)
        self.lit, self.dist = canonical(FIXED_LIT), canonical(FIXED_DIST)
        return self

    def dynamic(self, lit_lens, dist_lens, final=False, tokens=None, hclen=19, cl_lens=None, hlit=None, hdist=None):
        """the header of a dynamic block. tokens: the code length symbols (symbol, extra value) to write; default: one plain symbol a length"""
        cl_lens = CL_LENS if cl_lens is None else cl_lens
        hlit = len(lit_lens) if hlit is None else hlit
        hdist = len(dist_lens) if hdist is None else hdist
        self.w.put(int(final), 1)
        self.w.put(2, 2)
        self.w.put(hlit - 257, 5)
        self.w.put(hdist - 1, 5)
        self.w.put(hclen - 4, 4)
        for k in range(hclen):
            self.w.put(cl_lens[CL_ORDER[k]], 3)
        cl = canonical(cl_lens)
        if tokens is None:
            tokens = [(n, 0) for n in list(lit_lens) + list(dist_lens)]
        for sym, extra in tokens:
            self.w.code(*cl[sym])
            if sym >= 16:
                self.w.put(extra, {16: 2, 17: 3, 18: 7}[sym])
        self.lit, self.dist = canonical(lit_lens), canonical(dist_lens)
        return self

    def literal(self, data):
        for b in data:
            self.w.code(*self.lit[b])
        self.out += data
        return self

    def symbol(self, sym):                                      # a bare literal/length symbol (the corrupt streams)
        self.w.code(*self.lit[sym])
        return self

    def match(self, dist, n, model=True, length_code=None, dist_code=None):
        sym, ev, eb = length_symbol(n) if length_code is None else length_code
        self.w.code(*self.lit[sym])
        self.w.put(ev, eb)
        sym, ev, eb = distance_symbol(dist) if dist_code is None else dist_code
        self.w.code(*self.dist[sym])
        self.w.put(ev, eb)
        if model:
            assert 1 <= dist <= len(self.out) and 3 <= n <= 258, (dist, n, len(self.out))
            pattern = bytes(self.out[len(self.out) - dist:])
            self.out += (pattern * (n // dist + 1))[:n]
        return self

    def end(self):
        self.w.code(*self.lit[256])
        return self

    def bytes(self):
        w = Bits()
        w.out, w.acc, w.n = bytearray(self.w.out), self.w.acc, self.w.n
        w.align()
        return bytes(w.out)


def header(extra=None, name=None, comment=None, hcrc=False, flg_more=0, cm=8, magic=b"\x1f\x8b", bad_hcrc=False):
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0) | flg_more
    h = magic + bytes([cm, flg]) + b"\x12\x34\x56\x78" + b"\x02\x03"
    if extra is not None:
        h += len(extra).to_bytes(2, "little") + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += ((zlib.crc32(h) & 0xffff) ^ (1 if bad_hcrc else 0)).to_bytes(2, "little")
    return h


def member(deflate, out=None, head=None, crc=None, isize=None):
    """a member around a Deflate (or raw DEFLATE bytes with the output they make)"""
    body = deflate.bytes() if isinstance(deflate, Deflate) else deflate
    out = bytes(deflate.out) if out is None else out
    crc = zlib.crc32(out) if crc is None else crc
    isize = len(out) & 0xffffffff if isize is None else isize
    return (header() if head is None else head) + body + crc.to_bytes(4, "little") + isize.to_bytes(4, "little")


def gz(data, level=6, strategy=0):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, 9, strategy)
    return c.compress(data) + c.flush()


def raw(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


EVERY_LENGTH = sorted(set(LBASE) | {min(LBASE[i] + (1 << LEXTRA[i]) - 1, 257) for i in range(28)})   # every length code's base and top value (284 tops at 257: 258 has a code of its own)
EVERY_DISTANCE = [1, 2, 3, 4, 63, 64, 65, 32767, 32768]


def big_dynamic():
    """HLIT 286 / HDIST 30: every literal/length and distance symbol has a code and is used"""
    lit_lens, dist_lens = [8] * 226 + [9] * 60, [4] * 2 + [5] * 28
    d = Deflate().dynamic(lit_lens, dist_lens, final=True)
    d.literal(bytes(range(256)) * 130)                          # 33 280 bytes: room for distance 32768
    for s in range(29):
        for top in (0, 1):
            n = LBASE[s] + ((1 << LEXTRA[s]) - 1) * top
            d.match(1 + (n * 7) % 300, n)
    for s in range(30):
        for top in (0, 1):
            d.match(DBASE[s] + ((1 << DEXTRA[s]) - 1) * top, 3 + s)
    return d.end()


def fifteen_bit_code():
    lens = [0] * 257
    syms = list(b"abcdefghijklmno") + [256]
    for k, s in enumerate(syms):                                # lengths 1, 2, ..., 14, 15, 15
        lens[s] = min(k + 1, 15)
    d = Deflate().dynamic(lens, [1], final=True)
    return d.literal(b"onmlkjihgfedcbaabcdefghijklmno" * 3).end()           # (HLIT 257: no length symbol, the distance code goes unused)


def one_distance_code():
    """a distance set whose only code has 1 bit (incomplete; zlib accepts it), used by matches"""
    lens = [0] * 260
    for s, n in zip(list(b"ab") + [256, 257, 259], complete_lens(5)):
        lens[s] = n
    return Deflate().dynamic(lens, [1], final=True).literal(b"abba").match(1, 3).match(1, 5).literal(b"b").match(1, 3).end()


def rle_tokens():
    """code lengths written with every repeat code at its smallest and largest count, and with runs that cross from the literal/length
    lengths into the distance lengths -> (Deflate, the tokens)"""
    # symbols 0..161 without a code (runs of 3, 10, 11 and 138 zeros), 162..174 of 6 bits, 175..251 of 7 bits, 252..255 without, 256..280 of
    # 7 bits, 281..285 without: 13 codes of 6 bits and 102 of 7 bits, 26/128 + 102/128 = 1
    lit_lens = [0] * 162 + [6] * 13 + [7] * 77 + [0] * 4 + [7] * 25 + [0] * 5
    assert len(lit_lens) == 286
    dist_lens = [0] * 6 + complete_lens(24)                     # the zero run 281..285 goes on through distance symbols 0..5
    tokens = [(17, 0), (17, 7), (18, 0), (18, 127)]            # 3 + 10 + 11 + 138 zeros
    tokens += [(6, 0), (16, 0)] + [(6, 0)] * 9                  # 13 x 6: one plain, a 16 of 3, nine plain
    tokens += [(7, 0), (16, 3), (16, 3), (16, 3)] + [(7, 0)] * 58   # 77 x 7 (symbols 175..251): one plain, three 16 of 6, 58 plain
    tokens += [(17, 1)]                                         # 252..255
    tokens += [(7, 0), (16, 3), (16, 3), (16, 3), (16, 3)]      # 256..280: 25 x 7
    tokens += [(18, 0)]                                         # 281..285 and distance 0..5: 11 zeros across the boundary
    seq = lit_lens + dist_lens
    tokens += [(n, 0) for n in seq[292:]]
    d = Deflate().dynamic(lit_lens, dist_lens, final=True, tokens=tokens)
    d.literal(bytes(range(162, 252)) * 2).match(DBASE[6], 10).match(90, 19)
    return d.end(), tokens, seq


def expand_tokens(tokens):
    out = []
    for sym, extra in tokens:
        if sym < 16:
            out.append(sym)
        elif sym == 16:
            out += [out[-1]] * (3 + extra)
        else:
            out += [0] * ((3 if sym == 17 else 11) + extra)
    return out


def repeat_across_boundary():
    """a 16 that repeats the last literal/length length into the first distance lengths"""
    lit_lens = [9] * 4 + [8] * 254                              # 4/512 + 254/256 = 1: symbols 0..3 of 9 bits, the rest of 8, HLIT 258
    dist_lens = [8] * 2 + [1, 2, 3, 4, 5, 6, 7]                 # 2/256 + 1/2 + ... + 1/128 = 1
    seq = lit_lens + dist_lens
    tokens = [(n, 0) for n in seq[:255]] + [(16, 2)] + [(n, 0) for n in seq[260:]]   # 255..259: three literal/length lengths and two distance lengths
    assert expand_tokens(tokens) == seq
    d = Deflate().dynamic(lit_lens, dist_lens, final=True, tokens=tokens)
    return d.literal(b"\x00\x01\x02\x03hello, hello").match(1, 3).match(2, 3).match(5, 3).match(13, 3).end()


@functools.lru_cache(maxsize=None)
def straddling_stream():
    """one member of more than four windows whose fields lie across the window edges (for a stream that begins on a 16-byte boundary; the
    GPU test places it at all sixteen) -> ((name, stream, out), {what: byte position in the stream})"""
    W, H = WINDOW, 10
    d = Deflate()
    marks = {}

    def fill_to(target):                                        # a stored block that ends at byte `target` of the stream
        at = (d.w.pos() + 3 + 7) // 8 + 4 + H
        d.stored(payload(target - at, seed=target))
        assert d.w.n == 0 and len(d.w.out) + H == target
    fill_to(W - 11)
    d.fixed().literal(b"a" * 10)                                # 3 + 80 bits: the next code begins at bit 3 of byte W - 1
    marks["code"] = d.w.pos() // 8 + H
    d.literal(b"\xf0")                                          # 9 bits, across the edge
    d.literal(b"bc").match(3, 20).end()
    fill_to(2 * W - 2)
    marks["stored_len"] = 2 * W - 1                             # the header bits in byte 2 W - 2, LEN in 2 W - 1 and 2 W
    d.stored(payload(300, seed=5))
    fill_to(3 * W - 5)
    marks["dynamic_header"] = 3 * W - 5
    d.dynamic([8] * 226 + [9] * 60, [4] * 2 + [5] * 28)
    d.literal(payload(3000, seed=6)).match(2900, 258).match(1, 258).end()
    fill_to(4 * W - 3 - 5)
    d.stored(b"", final=True)                                   # ends at 4 W - 3: the trailer lies across the edge
    marks["trailer"] = 4 * W - 3
    s = member(d) + member(Deflate().fixed(final=True).literal(b"second member").end())
    assert len(d.bytes()) + H == 4 * W - 3 and len(s) > 4 * W
    return ("straddle_windows", s, bytes(d.out) + b"second member"), marks


@functools.lru_cache(maxsize=None)
def valid_streams():
    """[(name, stream, what it inflates to)]"""
    out = []

    def add(name, stream, data):
        out.append((name, bytes(stream), bytes(data)))

    def one(name, d, **kw):
        add(name, member(d, **kw), d.out)
    one("empty_fixed", Deflate().fixed(final=True).end())
    one("empty_stored", Deflate().stored(b"", final=True))
    one("stored_1", Deflate().stored(b"x", final=True))
    one("stored_65535", Deflate().stored(payload(65535, seed=1), final=True))
    for bits in range(1, 8):                                    # a stored block whose header ends `bits` bits into a byte, padding (all ones) behind it
        d = Deflate().fixed().literal(b"\xff" * ((bits - 5) % 8)).end()   # 3 + 9 k + 7 bits, then the stored block's own 3
        assert (d.w.pos() + 3) % 8 == bits
        d.stored(b"behind %d bits" % bits, final=True, pad=(1 << (8 - bits)) - 1)
        one("stored_behind_%d_bits" % bits, d)
    d = Deflate().fixed(final=True).literal(payload(40000, seed=2))
    for n in EVERY_LENGTH:
        d.match(1 + n % 7, n)
    for dist in EVERY_DISTANCE:
        d.match(dist, 11)
    one("fixed_every_length_and_distance", d.end())
    d = Deflate().fixed(final=True).literal(b"z")
    for _ in range(1000000 // 250):
        d.match(1, 250)
    one("distance_1_times_1000000", d.end())
    one("distance_equals_length", Deflate().fixed(final=True).literal(b"abcdefgh").match(8, 8).match(16, 16).end())
    one("distance_equals_produced", Deflate().fixed(final=True).literal(b"abc").match(3, 3).match(6, 100).match(106, 106).end())
    d = Deflate().fixed(final=True).literal(payload(RING, seed=3))
    for k in range(300):                                        # far matches until the output is more than twice the ring
        d.match(RING - (k % 3), 258)
    assert len(d.out) > 2 * RING + 10000
    one("ring_wraps_far_matches", d.end())
    one("dynamic_15_bit_code_hlit_257_hdist_1", fifteen_bit_code())
    one("dynamic_hlit_286_hdist_30", big_dynamic())
    one("dynamic_one_distance_code_of_1_bit", one_distance_code())
    lens = [0] * 257
    for s, n in zip(list(b"0123456") + [256], complete_lens(8)):
        lens[s] = n
    one("dynamic_no_distance_code", Deflate().dynamic(lens, [0], final=True).literal(b"0123456654321000").end())
    d, tokens, seq = rle_tokens()
    assert expand_tokens(tokens) == seq, (len(expand_tokens(tokens)), len(seq))
    one("dynamic_repeat_codes_min_max", d)
    one("dynamic_repeat_across_boundary", repeat_across_boundary())
    d = Deflate().stored(b"stored, ").fixed().literal(b"fixed, fixed, ").match(7, 7).end()
    lens = [0] * 260
    for s, n in zip(sorted(set(b"dynamic. ")) + [256, 259], complete_lens(len(set(b"dynamic. ")) + 2)):
        lens[s] = n
    d.dynamic(lens, [1]).literal(b"dynamic. ").match(1, 5).end().fixed(final=True).literal(b"and fixed again").end()
    one("three_block_types", d)
    a, b, c = Deflate().fixed(final=True).literal(b"first ").match(6, 12).end(), Deflate().fixed(final=True).end(), Deflate().stored(b"third", final=True)
    add("two_members", member(a) + member(c), a.out + c.out)
    add("three_members_empty_middle", member(a) + member(b) + member(c), a.out + c.out)
    add("empty_member_last", member(a) + member(b), a.out)
    x = Deflate().fixed(final=True).literal(b"headers").end()
    for name, kw in (("fextra", dict(extra=b"\x41\x70\x04\x00abcd")), ("fextra_empty", dict(extra=b"")), ("fname", dict(name=b"file.bin")), ("fcomment", dict(comment=b"a comment")),
                     ("fhcrc", dict(hcrc=True)), ("all_fields", dict(extra=b"xy" * 300, name=b"n", comment=b"", hcrc=True))):
        one("header_" + name, x, head=header(**kw))
    add(*straddling_stream()[0])
    for name, data in roundtrip_inputs():
        for level in (1, 6, 9):
            add("zlib_%s_level_%d" % (name, level), gz(data, level), data)
    add("zlib_fixed_strategy", gz(payload(5000, seed=8) * 3, 6, zlib.Z_FIXED), payload(5000, seed=8) * 3)
    add("zlib_stored_level_0", gz(payload(70000, seed=9), 0), payload(70000, seed=9))
    add("zlib_two_members", gz(b"one " * 1000, 9) + gz(b"two " * 1000, 1), b"one " * 1000 + b"two " * 1000)
    return out


@functools.lru_cache(maxsize=None)
def roundtrip_inputs():
    rng = np.random.default_rng(77)
    words = [b"the ", b"quick ", b"brown ", b"fox ", b"jumps ", b"over ", b"a ", b"lazy ", b"dog.\n", b"0123456789"]
    text = b"".join(words[i] for i in rng.integers(0, len(words), 30000))
    rand = rng.integers(0, 256, 100000, dtype=np.uint8).tobytes()
    return [("text", text), ("zeros", bytes(300000)), ("random", rand), ("mix_900k", (text[:250000] + rand + bytes(200000) + text[:350000])[:900000])]


@functools.lru_cache(maxsize=None)
def invalid_streams():
    """[(name, stream, expected length, the sub-case's word in ph_gzip_decompress_host's message)]; zlib refuses every one too"""
    out = []

    def add(name, stream, n, word):
        out.append((name, bytes(stream), n, word))
    good = Deflate().fixed(final=True).literal(b"hello, hello, ").match(7, 21).end()
    n = len(good.out)
    s = member(good)
    add("magic", member(good, head=header(magic=b"\x1f\x8c")), n, "does not begin 1f 8b 08")
    add("method_7", member(good, head=header(cm=7)), n, "does not begin 1f 8b 08")
    for bit in (0x20, 0x40, 0x80):
        add("reserved_flag_%02x" % bit, member(good, head=header(flg_more=bit)), n, "reserved FLG bit")
    add("header_crc", member(good, head=header(name=b"n", hcrc=True, bad_hcrc=True)), n, "header's CRC16")
    for k in range(1, len(s)):                                  # the input cut at every byte: inside the header, the block and the trailer
        if k >= 20:
            add("cut_at_%d" % k, s[:k], n, "input ends inside a member")
    long_head = member(good, head=header(extra=b"e" * 40, name=b"name", comment=b"comment", hcrc=True))
    for k in (21, 30, 52, 55, 57, 60, 63, 65, 66):              # inside FEXTRA, at its end, inside FNAME, FCOMMENT, FHCRC
        add("cut_in_header_fields_at_%d" % k, long_head[:k], n, "input ends inside a member")
    add("extended_by_one_byte", s + b"\0", n, "input is left over")
    add("extended_by_19_bytes", s + s[:19], n, "input is left over")
    add("second_member_bad_magic", s + b"\0" * 20, n, "does not begin 1f 8b 08")
    bad = Deflate().fixed().literal(b"abc").end()
    bad.w.put(1 | 3 << 1, 3)
    bad.w.put(0, 64)
    add("block_type_3", member(bad, out=b"abc"), 3, "block type 3")
    add("stored_nlen", member(Deflate().stored(b"abcdefgh", final=True, nlen=0xfff6), out=b"abcdefgh"), 8, "LEN is not the complement")
    add("stored_runs_past_input", (member(Deflate().stored(b"abcdefgh" * 4, final=True)))[:-8 - 20] + b"\0" * 7, 32, "input ends inside a member")
    add("expected_plus_1", s, n + 1, "ends before the expected length")
    add("expected_minus_1", s, n - 1, "past the expected length")
    add("literal_past_expected", member(Deflate().fixed(final=True).literal(b"abcd").end()), 3, "past the expected length")
    add("stored_past_expected", member(Deflate().stored(b"abcd", final=True)), 3, "past the expected length")
    add("second_member_past_expected", s + s, n, "past the expected length")
    add("expected_above_1032_to_one", s, 1032 * len(s) + 1, "1032")
    add("short_stream", s[:19], 1, "fewer than the 20 bytes")
    add("empty_stream", b"", 1, "empty stream")
    for k in range(32):
        t = bytearray(s)
        t[len(s) - 8 + k // 8] ^= 1 << (k % 8)
        add("crc_bit_%d" % k, t, n, "CRC-32 does not match")
        t = bytearray(s)
        t[len(s) - 4 + k // 8] ^= 1 << (k % 8)
        add("isize_bit_%d" % k, t, n, "ISIZE does not match")
    # distances
    far = Deflate().fixed(final=True).literal(b"abcde").match(6, 3, model=False).end()
    add("distance_one_past_produced", member(far, out=b"abcde" + b"???"), 8, "distance beyond")
    second = Deflate().fixed(final=True).literal(b"ab").match(3, 3, model=False).end()
    add("distance_into_first_member", s + member(second, out=b"ab???"), n + 5, "distance beyond")
    add("distance_before_any_byte", member(Deflate().fixed(final=True).match(1, 3, model=False).end(), out=b"???"), 3, "distance beyond")
    # symbols outside the alphabets (they have codes in the fixed set)
    for sym in (286, 287):
        add("fixed_length_symbol_%d" % sym, member(Deflate().fixed(final=True).literal(b"abc").symbol(sym).end(), out=b"abc"), 3, "outside the alphabet")
    for sym in (30, 31):
        bad = Deflate().fixed(final=True).literal(b"abc").match(1, 3, model=False, dist_code=(sym, 0, 0)).end()
        add("fixed_distance_symbol_%d" % sym, member(bad, out=b"abc???"), 6, "outside the alphabet")
    # dynamic headers
    lens8 = [0] * 257
    for sym, ln in zip(list(b"0123456") + [256], complete_lens(8)):
        lens8[sym] = ln

    def dyn(name, word, **kw):
        lit, dist = kw.pop("lit", lens8), kw.pop("dist", [1])
        d = Deflate().dynamic(lit, dist, final=True, **kw)
        try:
            d.literal(b"0123").end()
        except KeyError:
            pass
        add(name, member(d, out=b"0123"), 4, word)
    dyn("dynamic_hlit_287", "bad code lengths", lit=lens8 + [0] * 30, hlit=287, tokens=[(n, 0) for n in lens8 + [0] * 30 + [1]])
    dyn("dynamic_hdist_31", "bad code lengths", dist=[5] * 31 + [0], hdist=31, tokens=[(n, 0) for n in lens8 + [5] * 31])
    dyn("dynamic_repeat_first", "bad code lengths", tokens=[(16, 0)] + [(n, 0) for n in lens8[3:] + [1]])
    dyn("dynamic_repeat_past_the_end", "bad code lengths", tokens=[(n, 0) for n in lens8] + [(17, 0)])
    dyn("dynamic_zeros_past_the_end", "bad code lengths", tokens=[(n, 0) for n in lens8[:250]] + [(18, 127)])
    over = list(lens8)
    over[ord("9")] = 1
    dyn("dynamic_oversubscribed_literals", "bad code lengths", lit=over)
    under = list(lens8)
    under[ord("6")] = 0
    dyn("dynamic_incomplete_literals", "bad code lengths", lit=under)
    dyn("dynamic_oversubscribed_distances", "bad code lengths", dist=[1, 1, 1])
    dyn("dynamic_incomplete_distances", "bad code lengths", dist=[2, 2, 2])
    dyn("dynamic_one_distance_code_of_2_bits", "bad code lengths", dist=[2])
    no_end = list(lens8)
    no_end[256], no_end[ord("7")] = 0, lens8[256]
    dyn("dynamic_no_end_of_block_code", "bad code lengths", lit=no_end)
    dyn("dynamic_code_length_code_oversubscribed", "bad code lengths", cl_lens=[3] * 19)
    dyn("dynamic_code_length_code_incomplete", "bad code lengths", cl_lens=[5] * 19)
    # a match where the block has no distance code; the code that a one-code distance set leaves unused
    lens9 = [0] * 258
    for sym, ln in zip(list(b"012345") + [256, 257], complete_lens(8)):
        lens9[sym] = ln
    d = Deflate().dynamic(lens9, [0], final=True).literal(b"0123")
    d.dist = {0: (0, 1)}
    add("dynamic_distance_code_without_symbol", member(d.match(1, 3, model=False).literal(b"0" * 8).end(), out=b"0123"), 7, "code without a symbol")
    d = Deflate().dynamic(lens9, [1], final=True).literal(b"0123")
    d.dist = {0: (1, 1)}                                        # the code 1, which the one-code set leaves unused
    add("dynamic_unused_distance_code", member(d.match(1, 3, model=False).literal(b"0" * 8).end(), out=b"0123"), 7, "code without a symbol")
    return out


@functools.lru_cache(maxsize=None)
def stricter_streams():
    """[(name, stream, expected length, word)]: refused here, read by pyarrow's gzip codec"""
    data = b"a Parquet page is a gzip member, not a zlib stream " * 20
    good = gz(data)
    return [("zlib_framing", zlib.compress(data), len(data), "does not begin 1f 8b 08"),
            ("output_short_of_expected", good, len(data) + 100, "ends before the expected length")]


@functools.lru_cache(maxsize=None)
def lenient_streams():
    """[(name, stream, out)]: oddities zlib accepts, accepted here too"""
    d = Deflate().fixed(final=True).literal(b"ab").match(1, 258, length_code=(284, 31, 5)).end()
    lens = [0] * 257
    lens[256] = 1                                               # a literal/length set whose only code is the end of the block
    e = Deflate().dynamic(lens, [0], final=True).end()
    return [("length_symbol_284_extra_31_is_258", member(d), bytes(d.out)), ("only_the_end_code", member(e), b"")]


RAW_DEFLATE = ("raw_deflate", raw(b"raw DEFLATE has no header at all " * 30), 33 * 30, "does not begin 1f 8b 08")   # refused here AND by pyarrow's gzip codec


# ---------------------------------------------------------------- Parquet files with GZIP pages

_CACHE = {}


def generate(dirpath):
    """every well-formed GZIP case: {name: parquet_cases.Case}. Written once per directory, under names of their own (gz_*)."""
    key = str(dirpath)
    if key in _CACHE:
        return _CACHE[key]
    out = {}

    def add(name, table, **kw):
        out[name] = P._write(dirpath, "gz_" + name, table, compression="GZIP", **kw)
    m = P.matrix_table(N)
    for ver, v in (("v1", "1.0"), ("v2", "2.0")):
        for dic, d in (("dict", None), ("plain", False)):
            add("matrix_%s_%s_3groups" % (ver, dic), m, data_page_version=v, use_dictionary=d, row_group_size=7000)
        add("matrix_%s_dict_3groups_pages37" % ver, m, data_page_version=v, row_group_size=7000, max_rows_per_page=37)
    add("matrix_fallback_v2", m, dictionary_pagesize_limit=2048, data_page_version="2.0")
    nulls = P.null_patterns_table()
    add("nulls_v1", nulls, max_rows_per_page=5000)
    add("nulls_v1_plain", nulls, max_rows_per_page=5000, use_dictionary=False)
    add("nulls_v2", nulls, data_page_version="2.0", max_rows_per_page=5000)
    add("nulls_v2_plain", nulls, data_page_version="2.0", use_dictionary=False, max_rows_per_page=5000)
    add("dict_widths_pages37_v2", P.dict_width_table(N, (1, 2, 3, 5, 17, 257)), max_rows_per_page=37, data_page_version="2.0")
    for kind in ("257", "long", "straddle", "empty"):
        add("varchar_" + kind, P.varchar_table(kind))
        add("varchar_" + kind + "_plain_v2", P.varchar_table(kind), use_dictionary=False, data_page_version="2.0")
    add("zeros_v1", SN.zeros_table(), use_dictionary=False)
    add("zeros_v2", SN.zeros_table(), use_dictionary=False, data_page_version="2.0")
    add("random_v1", SN.random_table(), use_dictionary=False)
    add("random_v2", SN.random_table(), use_dictionary=False, data_page_version="2.0")
    add("text_v1", SN.text_table(), use_dictionary=False, max_rows_per_page=1 << 20, data_page_size=2 << 20)   # ONE page: a section of about 900 KB
    add("text_v2", SN.text_table(), use_dictionary=False, max_rows_per_page=1 << 20, data_page_size=2 << 20, data_page_version="2.0")
    add("matrix_level_1", m, compression_level=1, row_group_size=7000)
    add("matrix_level_9", m, compression_level=9, data_page_version="2.0")
    for n in (0, 1, 64, 65):
        add("rows_%d" % n, P.matrix_table(n, seed=100 + n), max_rows_per_page=37 if n > 64 else None)
    _CACHE[key] = out
    return out


CASE_NAMES = ["matrix_%s_%s_3groups" % (v, d) for v in ("v1", "v2") for d in ("dict", "plain")] + ["matrix_v1_dict_3groups_pages37", "matrix_v2_dict_3groups_pages37"] + \
             ["matrix_fallback_v2", "nulls_v1", "nulls_v1_plain", "nulls_v2", "nulls_v2_plain", "dict_widths_pages37_v2"] + \
             ["varchar_" + k + s for k in ("257", "long", "straddle", "empty") for s in ("", "_plain_v2")] + \
             ["zeros_v1", "zeros_v2", "random_v1", "random_v2", "text_v1", "text_v2", "matrix_level_1", "matrix_level_9"] + ["rows_%d" % n for n in (0, 1, 64, 65)]

MIXED_CODECS = {"i32_n": "SNAPPY", "i32_r": "GZIP", "i64_n": "NONE", "i64_r": "LZ4_RAW", "date_n": "GZIP", "date_r": "NONE", "d9_n": "LZ4_RAW", "d9_r": "SNAPPY",
                "d15_n": "GZIP", "d15_r": "LZ4_RAW", "s300_n": "GZIP", "s300_r": "SNAPPY", "s40_n": "NONE", "s40_r": "GZIP"}

_FLAGGED = {}


def flagged_files(dirpath):
    """{name: (Case, the flags it loads with besides PH_PARQUET_GZIP)}: one file whose columns are GZIP, SNAPPY, LZ4_RAW and UNCOMPRESSED
    (flags 1 | 16), and delta-encoded files inside GZIP pages, v1 and v2 (flags 4)"""
    key = str(dirpath)
    if key not in _FLAGGED:
        m = P.matrix_table(3000, seed=9)
        _FLAGGED[key] = {
            "mixed_codecs": (P._write(dirpath, "gz_mixed", m, compression=MIXED_CODECS, row_group_size=1100, data_page_version="2.0"), 1 | 16),
            "delta_v1": (D.write_delta(dirpath, "gz_delta_v1", m, compression="GZIP", row_group_size=1100), 4),
            "delta_v2": (D.write_delta(dirpath, "gz_delta_v2", m, compression="GZIP", data_page_version="2.0"), 4),
        }
    return _FLAGGED[key]


def patch_sources(dirpath):
    """the small GZIP files the patches start from: pages of 37 rows, v1, PLAIN"""
    import pyarrow as pa
    n = 100
    period = np.random.default_rng(40).integers(-2**63, 2**63 - 1, 7)[np.arange(n) % 7]
    req = pa.Table.from_arrays([pa.array(period)], schema=pa.schema([pa.field("p", pa.int64(), nullable=False)]))
    matches = P._write(dirpath, "gz_patch_matches", req, compression="GZIP", use_dictionary=False, max_rows_per_page=37, data_page_version="1.0")
    rnd = np.random.default_rng(41).integers(-2**63, 2**63 - 1, n)
    mask = np.arange(n) % 5 == 2
    levels = P._write(dirpath, "gz_patch_levels", pa.table({"a": pa.array(rnd, mask=mask)}), compression="GZIP", use_dictionary=False, max_rows_per_page=37,
                      data_page_version="1.0")
    zeros = pa.Table.from_arrays([pa.array(np.zeros(5000, np.int64))], schema=pa.schema([pa.field("z", pa.int64(), nullable=False)]))
    zeros = P._write(dirpath, "gz_patch_zeros", zeros, compression="GZIP", use_dictionary=False, max_rows_per_page=2048, data_page_version="1.0")
    return {"matches": matches, "levels": levels, "zeros": zeros}


def patched(dirpath, pages_of):
    """{name: (original bytes, patched bytes, column, the page the message must name, a word of the message)}: a GZIP file with ONE byte
    changed (level_prefix_*: one byte of the page's content, and the member's CRC-32 that covers it), located through the page directory
    (pages_of(data, column) -> ph_parquet_pages_ex entries) and the formats' layout. Each must give PH_EINVAL."""
    src = patch_sources(dirpath)
    out = {}

    def put(name, data, at, new, page, word, column=0):
        new = bytes([new]) if isinstance(new, int) else new
        assert data[at:at + len(new)] != new, (name, at, new)
        out[name] = (data, data[:at] + new + data[at + len(new):], column, page, word)
    d = src["matches"].data
    pages = pages_of(d, 0)
    assert [p["kind"] for p in pages] == [0, 0, 0] and all(p["compressed"] == 1 and p["codec"] == 2 for p in pages)
    for k, p in enumerate(pages):
        stream = d[p["data_pos"]:p["data_pos"] + p["data_bytes"]]
        assert stream[:3] == b"\x1f\x8b\x08" and stream[3] == 0 and len(zlib.decompress(stream, 31)) == p["uncompressed_bytes"]
        assert p["uncompressed_bytes"] == p["num_values"] * 8 and (stream[10] >> 1) & 3 != 0      # a Huffman block
        # one bit of a Huffman code in the middle of the block
        put("huffman_bit_page%d" % k, d, p["data_pos"] + 10 + (len(stream) - 18) // 2, stream[10 + (len(stream) - 18) // 2] ^ 0x08, k, "corrupt GZIP stream")
        put("crc_byte_page%d" % k, d, p["data_pos"] + len(stream) - 7, stream[-7] ^ 0x40, k, "corrupt GZIP stream")
        put("isize_byte_page%d" % k, d, p["data_pos"] + len(stream) - 4, stream[-4] ^ 0x01, k, "corrupt GZIP stream")
    put("magic_page1", d, pages[1]["data_pos"] + 1, 0x8c, 1, "does not begin 1f 8b 08")
    put("reserved_flag_page2", d, pages[2]["data_pos"] + 3, 0x80, 2, "reserved FLG bit")
    # the header of page 1 of the nullable column, whose size the host cannot check against the row count: 0x15 <type> 0x15
    # <uncompressed_page_size, a two-byte zigzag varint> 0x15 <compressed_page_size> ... Only the decoder's exact-length rule sees the lie.
    lv = src["levels"].data
    p = pages_of(lv, 0)[1]
    at = p["header_pos"] + 3
    assert lv[at - 1] == 0x15 and lv[at] & 0x80 and lv[at + 1] < 0x80 and lv[at + 2] == 0x15
    assert ((lv[at] & 0x7f) | lv[at + 1] << 7) >> 1 == p["uncompressed_bytes"] and 2 <= (lv[at] & 0x7f) <= 0x7d
    put("uncompressed_size_plus_1", lv, at, lv[at] + 2, 1, "corrupt GZIP stream")    # (zigzag: the value's bit 0 is the varint's bit 1)
    put("uncompressed_size_minus_1", lv, at, lv[at] - 2, 1, "corrupt GZIP stream")
    # pages of 2048 zeros are a few dozen bytes each: the size's three-byte varint with its top byte raised asks for more than 1032 times that
    z = src["zeros"].data
    p = pages_of(z, 0)[1]
    at = p["header_pos"] + 3
    assert z[at - 1] == 0x15 and z[at] & 0x80 and z[at + 1] & 0x80 and z[at + 2] < 0x80 and z[at + 3] == 0x15
    assert ((z[at] & 0x7f) | (z[at + 1] & 0x7f) << 7 | z[at + 2] << 14) >> 1 == p["uncompressed_bytes"] == 2048 * 8
    assert (0x7f << 14) >> 1 > 1032 * p["data_bytes"] and p["codec"] == 2 and p["compressed"] == 1
    put("uncompressed_size_impossible", z, at + 2, 0x7f, 1, "1032")
    # a nullable column, v1: [4-byte length n][levels, n bytes][values] is ONE stream. Random values do not compress, so zlib stores them:
    # the length's top byte lies open at byte 18 of the stream, and the member's CRC-32 is rewritten for it
    d = src["levels"].data
    pages = pages_of(d, 0)
    for k in (0, 2):
        p = pages[k]
        stream = d[p["data_pos"]:p["data_pos"] + p["data_bytes"]]
        assert p["compressed"] == 1 and p["codec"] == 2 and stream[10] == 1 and len(stream) == 10 + 5 + p["uncompressed_bytes"] + 8   # one stored block
        content = bytearray(stream[15:-8])
        assert 0 < int.from_bytes(content[:4], "little") < 16
        content[3] = 0x7f
        put("level_prefix_page%d" % k, d, p["data_pos"] + 18, bytes([0x7f]) + stream[19:-8] + zlib.crc32(bytes(content)).to_bytes(4, "little"), k, "a level section of")
    return out


def two_bad_pages(dirpath, pages_of):
    """pages 1 and 2 of one column both carry a flipped Huffman bit -> (bytes, column)"""
    cases = patched(dirpath, pages_of)
    orig, one = cases["huffman_bit_page1"][:2]
    two = cases["huffman_bit_page2"][1]
    both = bytearray(one)
    for i, (a, b) in enumerate(zip(orig, two)):
        if a != b:
            both[i] = b
    return bytes(both), 0


def write_patched(dirpath, pages_of):
    """the patched files on disk, for the stand-alone sanitizer program -> [path]"""
    paths = []
    for name, case in patched(dirpath, pages_of).items():
        path = os.path.join(str(dirpath), "gz_bad_" + name + ".parquet")
        with open(path, "wb") as f:
            f.write(case[1])
        paths.append(path)
    return paths
