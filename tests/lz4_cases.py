"""Inputs of the LZ4_RAW tests, shared by the CPU tests (tests/test_lz4_reference.py: the host twin) and the GPU tests
(tests/test_gpu_parquet_lz4.py): bare LZ4 blocks built from bytes — every length form at its edges, overlapping and far matches, sequence
headers that straddle the decompression kernel's input window, an output that wraps its ring — the corrupt ones, the ones on which this
decoder and liblz4 (inside pyarrow) differ on purpose, and Parquet files written with compression="LZ4_RAW" and the writer knobs of
tests/parquet_cases.py, plus one-byte patches of such files.

A block: sequences of [token: literal length << 4 | match length - 4][extension bytes of the literal length when its nibble is 15: added
until one is below 255][literals][offset, 2 bytes little-endian][extension bytes of the match length]; the last sequence ends behind its
literals. Nothing in a block says how long its output is."""
import functools
import os

import numpy as np

import delta_cases as D
import parquet_cases as P
import snappy_cases as SN

WINDOW = 8192         # plan_amd/csrc/lz4_decompress.h: LZ_TILE, the bytes of a block the kernel stages in LDS at a time
RING = 65536          # plan_amd/csrc/lz4_decompress.h: LZ_RING, the output bytes the kernel keeps in LDS
N = P.N
payload = SN.payload


def extension(n):
    """the bytes behind a nibble of 15 for a length field of n >= 15"""
    n -= 15
    return b"\xff" * (n // 255) + bytes([n % 255])


def sequence(lit, offset=None, mlen=None):
    """one sequence's bytes (no check: the corrupt streams use it too); offset None: the last one, literals only"""
    ln = len(lit)
    mn = 0 if offset is None else mlen - 4
    assert mn >= 0
    out = bytes([min(ln, 15) << 4 | min(mn, 15)])
    if ln >= 15:
        out += extension(ln)
    out += lit
    if offset is not None:
        out += int(offset).to_bytes(2, "little")
        if mn >= 15:
            out += extension(mn)
    return out


class Stream:
    """builds a block and what it decodes to"""
    def __init__(self):
        self.body, self.out = bytearray(), bytearray()

    def seq(self, lit, offset, mlen):
        self.out += lit
        assert 1 <= offset <= len(self.out) and mlen >= 4
        self.body += sequence(lit, offset, mlen)
        pattern = bytes(self.out[len(self.out) - offset:])      # an overlapping match repeats the last `offset` bytes
        self.out += (pattern * (mlen // offset + 1))[:mlen]
        return self

    def end(self, lit=b""):
        self.body += sequence(lit)
        self.out += lit
        return self

    def pad_to(self, target, seed):
        """one sequence (incompressible literals, then a 4-byte match) so that the next sequence's token lies at stream position `target`"""
        room = target - len(self.body)
        for n in range(max(0, room - 50), room - 2):
            if len(sequence(bytes(n), 1, 4)) == room:
                return self.seq(payload(n, seed), 5, 4)
        raise AssertionError(room)

    def case(self, name):
        return name, bytes(self.body), bytes(self.out)


TAIL = b"the end."    # liblz4 wants the last 5 bytes of a block to be literals; the valid streams end in 8


def straddling_stream():
    """more than three input windows -> (case, marks). marks: a token that is the last byte of window 0; a token whose literal length's
    extension bytes lie on both sides of the end of window 1; a sequence whose offset bytes lie on both sides of the end of window 2; a
    match whose extension run is longer than a whole window; a literal run that begins in one window and ends two later"""
    s = Stream()
    s.pad_to(WINDOW - 1, 1)
    marks = [len(s.body)]
    s.seq(payload(20, 2), 7, 10)                               # token at WINDOW - 1
    s.pad_to(2 * WINDOW - 3, 3)
    marks.append(len(s.body))
    s.seq(payload(15 + 3 * 255 + 9, 4), 100, 6)                # token at 2 WINDOW - 3, extension ff ff ff 09 at 2 WINDOW - 2 .. 2 WINDOW + 1
    s.pad_to(3 * WINDOW - 12, 5)
    marks.append(len(s.body))
    s.seq(payload(10, 6), 0x1234, 8)                           # token at 3 WINDOW - 12, offset bytes at 3 WINDOW - 1 and 3 WINDOW
    marks.append(len(s.body))
    s.seq(b"q", 1, 4 + 15 + 255 * (WINDOW + 40) + 17)          # WINDOW + 41 extension bytes: more than 2 MB of 'q'
    marks.append(len(s.body))
    s.seq(payload(2 * WINDOW + 100, 7), 3, 5)                  # literals over three windows
    s.end(TAIL)
    assert len(s.body) > 3 * WINDOW
    return s.case("straddle_windows"), marks


@functools.lru_cache(maxsize=None)
def valid_streams():
    """[(name, stream, what it decodes to)]"""
    out = [("empty", b"\0", b""), Stream().end(b"x").case("literal_1")]
    for n in (14, 15, 16, 269, 270, 65536):
        out.append(Stream().end(payload(n, n)).case("literal_%d" % n))
    for m in (4, 18, 19, 20, 273, 274):
        out.append(Stream().seq(payload(5, m), 3, m).end(TAIL).case("match_%d" % m))
    out.append(Stream().seq(b"z", 1, 1000000).end(TAIL).case("offset_1_times_1000000"))
    out.append(Stream().seq(payload(64, 4), 64, 64).seq(payload(5, 5), 5, 5).end(TAIL).case("offset_equals_length"))
    out.append(Stream().seq(payload(10, 6), 10, 30).seq(b"", 40, 40).end(TAIL).case("offset_equals_produced"))
    for off in (2, 3, 63, 64, 65):                             # the overlap forms around the lane count
        out.append(Stream().seq(payload(off, off), off, 700).seq(payload(3, off + 1), off, 70).seq(b"", off + 1, 1300).end(TAIL).case("overlap_offset_%d" % off))
    for k in (RING - 64, RING - 63, RING - 1):                 # what a 16-bit offset can reach, behind more literals than that
        out.append(Stream().seq(payload(70000, k % 1000), k, 300).seq(b"", k, 2000).seq(payload(40, 9), k, 64).seq(b"", k, 33).end(TAIL).case("offset_%d" % k))
    far = Stream().seq(payload(70000, 13), 65535, 64)
    for i in range(300):                                       # far matches in a row, over several flushes
        far.seq(b"", 65535 - i % 60, 4 + i % 70)
    out.append(far.end(TAIL).case("far_matches_300"))
    out.append(straddling_stream()[0])
    wrap = Stream().seq(payload(3000, 20), 2999, 1500)
    for i, off in enumerate([1, 4000, 65535, 33000, 60000, 65534, 17, 65000] * 5):   # > 2 x RING of output: the ring wraps under the matches
        wrap.seq(payload(3000 + i, 21 + i), min(off, len(wrap.out) + 3000 + i), 1500 + i)
    assert len(wrap.out) > 2 * RING
    out.append(wrap.end(TAIL).case("ring_wraps"))
    return out


@functools.lru_cache(maxsize=None)
def roundtrip_inputs():
    """[(name, bytes)]: what Codec.compress gets"""
    rng = np.random.default_rng(77)
    words = ["furiously", "regular", "deposits", "sleep", "carefully", "among", "the", "final", "packages", "blithely", "ironic", "requests", "haggle", "quickly"]
    text = " ".join(words[i] for i in rng.integers(0, len(words), 120000)).encode()
    out = []
    for n in (0, 1, 12, 13, 65535, 65536, 65537, 300000):
        out.append(("zeros_%d" % n, bytes(n)))
        out.append(("random_%d" % n, payload(n, n % 1000)))
        out.append(("text_%d" % n, text[:n]))
        assert len(text) >= n
    mix = b"".join((text[i * 1000:i * 1000 + 30000], payload(20000, i), bytes(40000))[i % 3] for i in range(30))
    assert 850000 < len(mix) < 950000
    out.append(("mix_900k", mix))
    return out


def invalid_streams():
    """[(name, stream, the length it is expected to produce, a word of the sub-case's text)]: each refused here and by pyarrow"""
    lit4 = b"wxyz"
    good = Stream().seq(b"wxyzwxyz", 4, 10).end(TAIL)          # 8 + 10 + 8 = 26 bytes
    assert len(good.out) == 26
    return [
        ("offset_one_beyond_produced", sequence(lit4, 5, 4) + sequence(TAIL), 16, "beyond the bytes produced"),
        ("offset_far_beyond_produced", sequence(lit4, 0xffff, 4) + sequence(TAIL), 16, "beyond the bytes produced"),
        ("literals_past_the_input", sequence(payload(10))[:-1], 10, "ends inside a sequence"),
        ("long_literals_past_the_input", sequence(payload(300))[:-1], 300, "ends inside a sequence"),
        ("input_ends_inside_an_offset", sequence(lit4, 4, 4)[:-1], 8, "ends inside a sequence"),
        ("input_ends_inside_a_literal_extension", b"\xf0\xff\xff", 700, "ends inside a sequence"),
        ("input_ends_inside_a_match_extension", sequence(lit4, 4, 600)[:-1], 604, "ends inside a sequence"),
        ("match_one_byte_past_expected", bytes(good.body), 8 + 9, "past the expected length"),
        ("long_match_past_expected", sequence(lit4, 4, 5000) + sequence(TAIL), 3000, "past the expected length"),
        ("literals_one_byte_past_expected", bytes(good.body), 25, "past the expected length"),
        ("input_left_over", bytes(good.body) + b"\0", 26, "left over"),
        ("a_sequence_left_over", bytes(good.body) + sequence(b"!"), 26, "left over"),
        ("no_final_token", sequence(b"wxyzwxyz", 4, 10), 18, "without a final token"),
        ("ff_run_100000_literal", b"\xf0" + b"\xff" * 100000, 1000, "past the expected length"),
        ("ff_run_100000_literal_large", b"\xf0" + b"\xff" * 100000, 20000000, "ends inside a sequence"),
        ("ff_run_100000_match", sequence(lit4, 1, 19)[:-1] + b"\xff" * 100000, 2000, "past the expected length"),
    ]


def stricter_streams():
    """[(name, stream, expected length, word)]: refused here, read by pyarrow. liblz4 copies a match at offset 0 from the byte it is about to
    write (zeros in a fresh buffer), and decompress(stream, decompressed_size=n) takes n as the room of the buffer, so a block that stops
    short of it is fine there; a Parquet page must produce exactly its header's size"""
    good = Stream().seq(b"wxyzwxyz", 4, 10).end(TAIL)
    return [("offset_0", sequence(b"wxyz", 0, 4) + sequence(TAIL), 16, "offset 0"),
            ("fewer_bytes_than_expected", bytes(good.body), 27, "before the expected length"),
            ("empty_block_for_one_byte", b"\0", 1, "before the expected length")]


def lenient_streams():
    """[(name, stream, what it decodes to)]: read here, refused by pyarrow. liblz4 enforces the end-of-block restrictions that bind
    compressors (the last 5 bytes are literals); a block that breaks them still says exactly one thing"""
    return [Stream().seq(payload(20, 1), 7, 9).end(payload(k, 2)).case("final_run_of_%d" % k) for k in (0, 1, 4)]


def sequences(stream):
    """the sequences of a block: [(token position, literal length, literals' position, offset position or None, offset, match length)]"""
    pos, out = 0, []
    while pos < len(stream):
        tpos, token = pos, stream[pos]
        pos += 1
        ln = token >> 4
        if ln == 15:
            while True:
                b = stream[pos]
                pos += 1
                ln += b
                if b != 255:
                    break
        lpos = pos
        pos += ln
        if pos >= len(stream):
            out.append((tpos, ln, lpos, None, 0, 0))
            break
        opos, off = pos, stream[pos] | stream[pos + 1] << 8
        pos += 2
        mn = token & 15
        if mn == 15:
            while True:
                b = stream[pos]
                pos += 1
                mn += b
                if b != 255:
                    break
        out.append((tpos, ln, lpos, opos, off, mn + 4))
    return out


# ---------------------------------------------------------------- Parquet files with LZ4_RAW pages

_CACHE = {}


def generate(dirpath):
    """every well-formed LZ4_RAW case: {name: parquet_cases.Case}. Written once per directory, under names of their own (lz_*)."""
    key = str(dirpath)
    if key in _CACHE:
        return _CACHE[key]
    out = {}

    def add(name, table, **kw):
        out[name] = P._write(dirpath, "lz_" + name, table, compression="LZ4_RAW", **kw)
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
    for n in (0, 1, 64, 65):
        add("rows_%d" % n, P.matrix_table(n, seed=100 + n), max_rows_per_page=37 if n > 64 else None)
    _CACHE[key] = out
    return out


CASE_NAMES = ["matrix_%s_%s_3groups" % (v, d) for v in ("v1", "v2") for d in ("dict", "plain")] + ["matrix_v1_dict_3groups_pages37", "matrix_v2_dict_3groups_pages37"] + \
             ["matrix_fallback_v2", "nulls_v1", "nulls_v1_plain", "nulls_v2", "nulls_v2_plain", "dict_widths_pages37_v2"] + \
             ["varchar_" + k + s for k in ("257", "long", "straddle", "empty") for s in ("", "_plain_v2")] + \
             ["zeros_v1", "zeros_v2", "random_v1", "random_v2", "text_v1", "text_v2"] + ["rows_%d" % n for n in (0, 1, 64, 65)]

MIXED_CODECS = {"i32_n": "SNAPPY", "i32_r": "LZ4_RAW", "i64_n": "NONE", "i64_r": "LZ4_RAW", "date_n": "SNAPPY", "date_r": "NONE", "d9_n": "LZ4_RAW", "d9_r": "SNAPPY",
                "d15_n": "NONE", "d15_r": "LZ4_RAW", "s300_n": "LZ4_RAW", "s300_r": "SNAPPY", "s40_n": "NONE", "s40_r": "LZ4_RAW"}

_FLAGGED = {}


def flagged_files(dirpath):
    """{name: (Case, the flags it loads with besides PH_PARQUET_LZ4_RAW)}: one file whose columns are SNAPPY, LZ4_RAW and UNCOMPRESSED
    (flags 1), and delta-encoded files inside LZ4_RAW pages, v1 and v2 (flags 4)"""
    key = str(dirpath)
    if key not in _FLAGGED:
        m = P.matrix_table(3000, seed=9)
        _FLAGGED[key] = {
            "mixed_codecs": (P._write(dirpath, "lz_mixed", m, compression=MIXED_CODECS, row_group_size=1100, data_page_version="2.0"), 1),
            "delta_v1": (D.write_delta(dirpath, "lz_delta_v1", m, compression="LZ4_RAW", row_group_size=1100), 4),
            "delta_v2": (D.write_delta(dirpath, "lz_delta_v2", m, compression="LZ4_RAW", data_page_version="2.0"), 4),
        }
    return _FLAGGED[key]


def patch_sources(dirpath):
    """the small LZ4_RAW files the one-byte patches start from: 100 rows in pages of 37, v1, PLAIN"""
    import pyarrow as pa
    n = 100
    period = np.random.default_rng(40).integers(-2**63, 2**63 - 1, 7)[np.arange(n) % 7]   # 56 bytes of literals, then one long match at offset 56
    req = pa.Table.from_arrays([pa.array(period)], schema=pa.schema([pa.field("p", pa.int64(), nullable=False)]))
    matches = P._write(dirpath, "lz_patch_matches", req, compression="LZ4_RAW", use_dictionary=False, max_rows_per_page=37, data_page_version="1.0")
    rnd = np.random.default_rng(41).integers(-2**63, 2**63 - 1, n)
    mask = np.arange(n) % 5 == 2
    levels = P._write(dirpath, "lz_patch_levels", pa.table({"a": pa.array(rnd, mask=mask)}), compression="LZ4_RAW", use_dictionary=False, max_rows_per_page=37,
                      data_page_version="1.0")
    zeros = pa.Table.from_arrays([pa.array(np.zeros(n, np.int64))], schema=pa.schema([pa.field("z", pa.int64(), nullable=False)]))
    zeros = P._write(dirpath, "lz_patch_zeros", zeros, compression="LZ4_RAW", use_dictionary=False, max_rows_per_page=37, data_page_version="1.0")
    return {"matches": matches, "levels": levels, "zeros": zeros}


def patched(dirpath, pages_of):
    """{name: (original bytes, patched bytes, column, the page the message must name, a word of the message)}: ONE byte changed in an
    LZ4_RAW file, located through the page directory (pages_of(data, column) -> ph_parquet_pages_ex entries) and the formats' layout.
    Each must give PH_EINVAL."""
    src = patch_sources(dirpath)
    out = {}

    def put(name, data, at, new, page, word, column=0):
        assert data[at] != new and 0 <= new < 256, (name, at, new)
        out[name] = (data, data[:at] + bytes([new]) + data[at + 1:], column, page, word)
    d = src["matches"].data
    pages = pages_of(d, 0)
    assert [p["kind"] for p in pages] == [0, 0, 0] and all(p["compressed"] == 1 and p["codec"] == 7 for p in pages)
    for k, p in enumerate(pages):
        stream = d[p["data_pos"]:p["data_pos"] + p["data_bytes"]]
        assert p["uncompressed_bytes"] == p["num_values"] * 8
        seqs = sequences(stream)
        first = seqs[0]
        assert first[3] is not None and first[4] == 56 and first[1] == 56, seqs
        # the first match's offset: its high byte set, far beyond the 56 bytes produced
        put("match_offset_page%d" % k, d, p["data_pos"] + first[3] + 1, 0xff, k, "corrupt LZ4_RAW stream")
        # the first token's literal length nibble, 15 -> 14: every later byte of the block is read as something else
        put("token_nibble_page%d" % k, d, p["data_pos"] + first[0], stream[first[0]] ^ 0x10, k, "corrupt LZ4_RAW stream")
    # the header of page 1 of the nullable column, whose size the host cannot check against the row count: 0x15 <type> 0x15
    # <uncompressed_page_size, a two-byte zigzag varint> 0x15 <compressed_page_size> ... Only the decoder's exact-length rule sees the lie.
    lv = src["levels"].data
    p = pages_of(lv, 0)[1]
    at = p["header_pos"] + 3
    assert lv[at - 1] == 0x15 and lv[at] & 0x80 and lv[at + 1] < 0x80 and lv[at + 2] == 0x15
    assert ((lv[at] & 0x7f) | lv[at + 1] << 7) >> 1 == p["uncompressed_bytes"] and 2 <= (lv[at] & 0x7f) <= 0x7d
    put("uncompressed_size_plus_1", lv, at, lv[at] + 2, 1, "corrupt LZ4_RAW stream")    # (zigzag: the value's bit 0 is the varint's bit 1)
    put("uncompressed_size_minus_1", lv, at, lv[at] - 2, 1, "corrupt LZ4_RAW stream")
    # pages of zeros are a dozen bytes each: the same varint's second byte raised asks for more than 255 times that
    z = src["zeros"].data
    p = pages_of(z, 0)[1]
    at = p["header_pos"] + 3
    assert z[at - 1] == 0x15 and z[at] & 0x80 and z[at + 1] < 0x80 and z[at + 2] == 0x15 and ((z[at] & 0x7f) | z[at + 1] << 7) >> 1 == p["uncompressed_bytes"]
    assert ((z[at] & 0x7f) | 0x7f << 7) >> 1 > 255 * p["data_bytes"] and p["codec"] == 7 and p["compressed"] == 1
    put("uncompressed_size_impossible", z, at + 1, 0x7f, 1, "255")
    # a nullable column, v1: [4-byte length n][levels, n bytes][values] is ONE block; random values keep its head inside the first literal
    # run, so the length's top byte can be patched in place
    d = src["levels"].data
    pages = pages_of(d, 0)
    for k in (0, 2):
        p = pages[k]
        stream = d[p["data_pos"]:p["data_pos"] + p["data_bytes"]]
        first = sequences(stream)[0]
        assert first[1] >= 8 and p["compressed"] == 1 and p["codec"] == 7
        n = int.from_bytes(stream[first[2]:first[2] + 4], "little")
        assert 0 < n < 16
        put("level_prefix_page%d" % k, d, p["data_pos"] + first[2] + 3, 0x7f, k, "a level section of")
    return out


def two_bad_pages(dirpath, pages_of):
    """pages 1 and 2 of one column both carry a match that reaches in front of the block -> (bytes, column)"""
    cases = patched(dirpath, pages_of)
    orig, one = cases["match_offset_page1"][:2]
    two = cases["match_offset_page2"][1]
    both = bytearray(one)
    for i, (a, b) in enumerate(zip(orig, two)):
        if a != b:
            both[i] = b
    return bytes(both), 0


def write_patched(dirpath, pages_of):
    """the patched files on disk, for the stand-alone sanitizer program -> [path]"""
    paths = []
    for name, case in patched(dirpath, pages_of).items():
        path = os.path.join(str(dirpath), "lz_bad_" + name + ".parquet")
        with open(path, "wb") as f:
            f.write(case[1])
        paths.append(path)
    return paths
