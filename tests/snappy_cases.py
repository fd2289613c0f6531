"""Inputs of the SNAPPY tests, shared by the CPU tests (tests/test_snappy_reference.py: the host twin) and the GPU tests
(tests/test_gpu_parquet_snappy.py): raw Snappy streams built from bytes — every element form, the overlapping and far copies, elements that
straddle the decompression kernel's input tile, and the corrupt ones — and Parquet files written with compression="SNAPPY" and the writer
knobs of tests/parquet_cases.py, plus one-byte patches of such files.

A raw stream: a varint length, then elements. Tag low bits 00: a literal (upper 6 bits = len - 1 up to 59; 60..63 = 1..4 bytes of len - 1
follow); 01: a copy of 4..11 bytes, 11-bit offset; 10 / 11: a copy of 1..64 bytes, 2- / 4-byte offset."""
import os

import numpy as np

import parquet_cases as P

TILE = 8192           # plan_amd/csrc/snappy_decompress.h: SN_TILE, the bytes of a stream the kernel stages in LDS at a time
RING = 65536          # plan_amd/csrc/snappy_decompress.h: SN_RING, the output bytes the kernel keeps in LDS
N = P.N


def varint(n):
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7f) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def payload(n, seed=0):
    """n bytes that no compressor would call a pattern"""
    return np.random.default_rng(1000 + seed).integers(0, 256, n).astype(np.uint8).tobytes()


def literal_tag(n, form=None):
    """the tag and length bytes of a literal of n bytes; form: the number of length bytes (0: in the tag), default the shortest"""
    if form is None:
        form = 0 if n <= 60 else 1 if n <= 256 else 2 if n <= 65536 else 3 if n <= 1 << 24 else 4
    if form == 0:
        assert 1 <= n <= 60
        return bytes([(n - 1) << 2])
    return bytes([(59 + form) << 2]) + (n - 1).to_bytes(form, "little")


def copy_bytes(offset, length, kind):
    """a copy element's bytes; kind 1, 2 or 4 = the bytes of its offset (no check: the corrupt streams use it too)"""
    if kind == 1:
        assert 4 <= length <= 11 and offset < 2048
        return bytes([1 | (length - 4) << 2 | (offset >> 8) << 5, offset & 0xff])
    assert 1 <= length <= 64
    return bytes([(2 if kind == 2 else 3) | (length - 1) << 2]) + offset.to_bytes(kind, "little")


class Stream:
    """builds a stream and what it decodes to"""
    def __init__(self):
        self.body, self.out = bytearray(), bytearray()

    def lit(self, data, form=None):
        self.body += literal_tag(len(data), form) + data
        self.out += data
        return self

    def copy(self, offset, length, kind):
        assert 1 <= offset <= len(self.out)
        self.body += copy_bytes(offset, length, kind)
        for _ in range(length):
            self.out.append(self.out[-offset])
        return self

    def at(self, preamble_bytes):
        """the stream position of the next element"""
        return preamble_bytes + len(self.body)

    def pad_to(self, target, preamble_bytes, seed):
        """a literal with a 2-byte length so that the next element begins at stream position `target`"""
        n = target - self.at(preamble_bytes) - 3
        assert 257 <= n <= 65536, n
        return self.lit(payload(n, seed), 2)

    def stream(self):
        return varint(len(self.out)) + bytes(self.body)

    def case(self, name):
        return name, self.stream(), bytes(self.out)


def straddling_stream():
    """more than three input tiles; a copy's tag is the last byte of tile 0, a literal's two length bytes lie on both sides of the end of
    tile 1, and a 4-byte copy operand on both sides of the end of tile 2. Returns (case, [the three element positions])"""
    s = Stream()
    pre = 3                                                    # the preamble of 16384 .. 2097151 bytes
    s.pad_to(TILE - 1, pre, 1)
    marks = [s.at(pre)]
    s.copy(300, 64, 2)                                         # tag at TILE - 1, operand in the next tile
    s.pad_to(2 * TILE - 2, pre, 2)
    marks.append(s.at(pre))
    s.lit(payload(700, 3), 2)                                  # tag at 2 TILE - 2, length bytes at 2 TILE - 1 and 2 TILE
    s.pad_to(3 * TILE - 3, pre, 4)
    marks.append(s.at(pre))
    s.copy(20000, 64, 4)                                       # tag at 3 TILE - 3, operand bytes 3 TILE - 2 .. 3 TILE + 1
    s.lit(payload(500, 5))
    assert len(varint(len(s.out))) == pre and len(s.stream()) > 3 * TILE
    return s.case("straddle_tiles"), marks


def valid_streams():
    """[(name, stream, what it decodes to)]"""
    out = [("empty", b"\0", b"")]
    for n in (1, 60, 61, 256, 257, 65536, 65537):
        out.append(Stream().lit(payload(n, n)).case("literal_%d" % n))
    out.append(Stream().lit(payload(10, 10), 4).case("literal_4_byte_length"))
    out.append(Stream().lit(payload(9, 11), 3).lit(payload(70, 12), 2).case("literal_long_forms_of_short_lengths"))
    out.append(Stream().lit(payload(2047, 1)).copy(1, 4, 1).copy(2047, 11, 1).copy(2047, 4, 1).copy(1, 11, 1).case("copy_1_byte_offset_min_max"))
    out.append(Stream().lit(payload(65535, 2)).copy(1, 1, 2).copy(65535, 64, 2).copy(65535, 1, 2).copy(1, 64, 2).case("copy_2_byte_offset_min_max"))
    out.append(Stream().lit(payload(70000, 3)).copy(1, 1, 4).copy(70000, 64, 4).copy(70000, 1, 4).copy(1, 64, 4).case("copy_4_byte_offset_min_max"))
    out.append(Stream().lit(b"x").copy(1, 64, 2).case("offset_1_length_64"))
    for off in (2, 3, 7):
        out.append(Stream().lit(payload(off, off)).copy(off, 64, 2).copy(off, 64, 4).case("overlap_offset_%d" % off))
    out.append(Stream().lit(b"ab").copy(2, 64, 2).case("ab_times_33"))
    out.append(Stream().lit(payload(64, 4)).copy(64, 64, 2).lit(payload(5, 5)).copy(5, 5, 1).case("offset_equals_length"))
    out.append(Stream().lit(payload(10, 6)).copy(10, 30, 2).copy(40, 40, 4).case("offset_equals_produced"))
    out.append(Stream().lit(payload(65535, 7)).copy(65535, 64, 2).lit(payload(3, 8)).copy(65535, 64, 4).case("offset_65535"))
    for k in (RING - 70, RING - 65, RING - 64, RING - 63, RING - 1, RING, RING + 1, RING + 2):   # around what the ring can hold
        out.append(Stream().lit(payload(k + 9, k)).copy(k, 64, 4).copy(k + 64, 64, 4).lit(payload(40, 9)).copy(k, 33, 4).case("offset_%d" % k))
    far = Stream().lit(payload(70000, 13)).copy(70000, 64, 4).lit(payload(4097, 14))
    for i in range(300):                                       # far copies between near ones, over several flushes
        far.copy(70000 + i, 1 + i % 64, 4).copy(1 + i % 50, 64, 2)
    out.append(far.copy(70001, 64, 4).case("offset_70000_behind_the_ring"))
    out.append(straddling_stream()[0])
    return out


def roundtrip_inputs():
    """[(name, bytes)]: what Codec.compress gets"""
    rng = np.random.default_rng(77)
    words = ["furiously", "regular", "deposits", "sleep", "carefully", "among", "the", "final", "packages", "blithely", "ironic", "requests", "haggle", "quickly"]
    text = " ".join(words[i] for i in rng.integers(0, len(words), 260000)).encode()
    out = []
    for n in (0, 1, 15, 16, 17, 65535, 65536, 65537, (1 << 20) + 3):
        out.append(("zeros_%d" % n, bytes(n)))
        out.append(("random_%d" % n, payload(n, n % 1000)))
        out.append(("text_%d" % n, text[:n]))
        assert len(text) >= n
    return out


def invalid_streams():
    """[(name, stream, the length it is expected to produce)]: each a valid stream with one thing wrong"""
    lit4 = literal_tag(4) + b"wxyz"
    good = Stream().lit(b"wxyz").copy(4, 4, 2).stream()           # 8 bytes
    assert good == varint(8) + lit4 + copy_bytes(4, 4, 2)
    return [
        ("offset_0", varint(8) + lit4 + copy_bytes(0, 4, 2), 8),
        ("offset_0_one_byte", varint(8) + lit4 + copy_bytes(0, 4, 1), 8),
        ("offset_0_four_bytes", varint(8) + lit4 + copy_bytes(0, 4, 4), 8),
        ("offset_one_beyond_produced", varint(8) + lit4 + copy_bytes(5, 4, 2), 8),
        ("offset_far_beyond_produced", varint(8) + lit4 + copy_bytes(0xfffffff0, 4, 4), 8),
        ("literal_cut", varint(10) + literal_tag(10) + payload(9), 10),
        ("literal_length_bytes_cut", varint(300) + literal_tag(300)[:2], 300),
        ("literal_4_byte_length_cut", varint(8) + lit4 + bytes([63 << 2, 3, 0, 0]), 8),
        ("copy_operand_cut", varint(8) + lit4 + copy_bytes(4, 4, 2)[:2], 8),
        ("copy_4_byte_operand_cut", varint(8) + lit4 + copy_bytes(4, 4, 4)[:4], 8),
        ("copy_tag_alone", varint(8) + lit4 + copy_bytes(4, 4, 1)[:1], 8),
        ("copy_one_byte_past_expected", varint(7) + lit4 + copy_bytes(4, 4, 2), 7),
        ("literal_one_byte_past_expected", varint(7) + lit4 + lit4, 7),
        ("huge_literal_past_expected", varint(8) + lit4 + bytes([63 << 2, 0xff, 0xff, 0xff, 0xff]) + b"abcd", 8),
        ("input_one_byte_short", varint(9) + lit4 + copy_bytes(4, 4, 2), 9),
        ("only_a_preamble", varint(5), 5),
        ("one_element_too_many", good + literal_tag(1) + b"!", 8),
        ("one_byte_left_over", good + b"\0", 8),
        ("preamble_6_bytes", b"\x88\x80\x80\x80\x80\x00" + lit4 + copy_bytes(4, 4, 2), 8),
        ("preamble_above_32_bits", b"\x88\x80\x80\x80\x10" + lit4 + copy_bytes(4, 4, 2), 8),
        ("preamble_cut", b"\x88", 8),
        ("preamble_disagrees_smaller", good, 7),
    ]


def stricter_streams():
    """[(name, stream, expected length)]: refused here, read by pyarrow. Its decompress(stream, decompressed_size=n) takes n as the room
    of the buffer and reads a stream whose preamble says LESS; a Parquet page must produce exactly its header's uncompressed size, so the
    decoder here refuses every disagreement"""
    good = Stream().lit(b"wxyz").copy(4, 4, 2).stream()
    return [("preamble_disagrees_larger", good, 9), ("preamble_disagrees_empty", b"\0", 1)]


def elements(stream):
    """the elements of a stream: [(position of the tag, kind 0 literal / 1, 2, 4 copy by offset bytes, length, offset or the literal's first byte)]"""
    pos = 0
    while stream[pos] & 0x80:
        pos += 1
    pos += 1
    out = []
    while pos < len(stream):
        tag = stream[pos]
        kind, up = tag & 3, tag >> 2
        if kind == 0:
            nb = max(0, up - 59)
            n = (int.from_bytes(stream[pos + 1:pos + 1 + nb], "little") if nb else up) + 1
            out.append((pos, 0, n, pos + 1 + nb))
            pos += 1 + nb + n
        elif kind == 1:
            out.append((pos, 1, 4 + (up & 7), (up >> 3) << 8 | stream[pos + 1]))
            pos += 2
        else:
            nb = 2 if kind == 2 else 4
            out.append((pos, nb, 1 + up, int.from_bytes(stream[pos + 1:pos + 1 + nb], "little")))
            pos += 1 + nb
    return out


# ---------------------------------------------------------------- Parquet files with SNAPPY pages

def text_table(n=100000):
    """short words, required and with NULLs: PLAIN in ONE default-size page of about 900 KB, a section far above the tile and the ring"""
    import pyarrow as pa
    rng = np.random.default_rng(21)
    words = np.array(["quick", "final", "ideas", "deps", "slyly", "even", "bold", "pinto", "beans", "nag", "doze", "cajol"])
    vals = words[rng.integers(0, len(words), n)].tolist()
    return pa.Table.from_arrays([pa.array(vals, pa.string()), pa.array(vals, pa.string(), mask=rng.random(n) < 0.1)],
                                schema=pa.schema([pa.field("t_r", pa.string(), nullable=False), pa.field("t_n", pa.string(), nullable=True)]))


def zeros_table(n=100000):
    import pyarrow as pa
    z = np.zeros(n, np.int64)
    mask = np.zeros(n, bool)
    mask[::1000] = True
    return pa.Table.from_arrays([pa.array(z), pa.array(z, mask=mask), pa.array(np.zeros(n, np.int32))],
                                schema=pa.schema([pa.field("z_r", pa.int64(), nullable=False), pa.field("z_n", pa.int64()), pa.field("z32_r", pa.int32(), nullable=False)]))


def random_table(n=30000):
    """INT64 that no compressor shrinks: a v1 page then grows by Snappy's framing, a v2 page is stored raw (is_compressed = false)"""
    import pyarrow as pa
    v = np.random.default_rng(31).integers(-2**63, 2**63 - 1, n)
    mask = np.random.default_rng(32).random(n) < 0.2
    return pa.Table.from_arrays([pa.array(v), pa.array(v, mask=mask)], schema=pa.schema([pa.field("r_r", pa.int64(), nullable=False), pa.field("r_n", pa.int64())]))


_CACHE = {}


def generate(dirpath):
    """every well-formed SNAPPY case: {name: parquet_cases.Case}. Written once per directory, under names of their own (sn_*)."""
    key = str(dirpath)
    if key in _CACHE:
        return _CACHE[key]
    out = {}

    def add(name, table, **kw):
        out[name] = P._write(dirpath, "sn_" + name, table, compression="SNAPPY", **kw)
    m = P.matrix_table(N)
    for ver, v in (("v1", "1.0"), ("v2", "2.0")):
        for dic, d in (("dict", None), ("plain", False)):
            add("matrix_%s_%s_3groups" % (ver, dic), m, data_page_version=v, use_dictionary=d, row_group_size=7000)
            add("matrix_%s_%s_3groups_pages37" % (ver, dic), m, data_page_version=v, use_dictionary=d, row_group_size=7000, max_rows_per_page=37)
    add("matrix_fallback_v2", m, dictionary_pagesize_limit=2048, data_page_version="2.0")
    add("matrix_decint", m, store_decimal_as_integer=True)
    nulls = P.null_patterns_table()
    add("nulls_v1", nulls, max_rows_per_page=5000)
    add("nulls_v1_plain", nulls, max_rows_per_page=5000, use_dictionary=False)
    add("nulls_v2", nulls, data_page_version="2.0", max_rows_per_page=5000)
    add("nulls_v2_plain", nulls, data_page_version="2.0", use_dictionary=False, max_rows_per_page=5000)
    add("dict_widths", P.dict_width_table(N, (1, 2, 3, 5, 17, 257)))
    add("dict_widths_pages37_v2", P.dict_width_table(N, (1, 2, 3, 5, 17, 257)), max_rows_per_page=37, data_page_version="2.0")
    for kind in ("257", "long", "straddle", "empty"):
        add("varchar_" + kind, P.varchar_table(kind))
        add("varchar_" + kind + "_plain_v2", P.varchar_table(kind), use_dictionary=False, data_page_version="2.0")
    add("zeros_v1", zeros_table(), use_dictionary=False)
    add("zeros_v2", zeros_table(), use_dictionary=False, data_page_version="2.0")
    add("random_v1", random_table(), use_dictionary=False)
    add("random_v2", random_table(), use_dictionary=False, data_page_version="2.0")
    add("text_v1", text_table(), use_dictionary=False)
    add("text_v2", text_table(), use_dictionary=False, data_page_version="2.0")
    for n in (0, 1, 64, 65):
        add("rows_%d" % n, P.matrix_table(n, seed=100 + n), max_rows_per_page=37 if n > 64 else None)
    _CACHE[key] = out
    return out


CASE_NAMES = ["matrix_%s_%s_3groups%s" % (v, d, p) for v in ("v1", "v2") for d in ("dict", "plain") for p in ("", "_pages37")] + \
             ["matrix_fallback_v2", "matrix_decint", "nulls_v1", "nulls_v1_plain", "nulls_v2", "nulls_v2_plain", "dict_widths", "dict_widths_pages37_v2"] + \
             ["varchar_" + k + s for k in ("257", "long", "straddle", "empty") for s in ("", "_plain_v2")] + \
             ["zeros_v1", "zeros_v2", "random_v1", "random_v2", "text_v1", "text_v2"] + ["rows_%d" % n for n in (0, 1, 64, 65)]


def patch_sources(dirpath):
    """the small SNAPPY files the one-byte patches start from: 100 rows in pages of 37, v1, PLAIN"""
    import pyarrow as pa
    n = 100
    period = (np.arange(n, dtype=np.int64) % 7) * 1000003           # repeats every 56 bytes: a literal, then 64-byte copies at offset 56
    req = pa.Table.from_arrays([pa.array(period)], schema=pa.schema([pa.field("p", pa.int64(), nullable=False)]))
    copies = P._write(dirpath, "sn_patch_copies", req, compression="SNAPPY", use_dictionary=False, max_rows_per_page=37, data_page_version="1.0")
    rnd = np.random.default_rng(41).integers(-2**63, 2**63 - 1, n)
    mask = np.arange(n) % 5 == 2
    levels = P._write(dirpath, "sn_patch_levels", pa.table({"a": pa.array(rnd, mask=mask)}), compression="SNAPPY", use_dictionary=False, max_rows_per_page=37,
                      data_page_version="1.0")
    # dictionary-coded, required: a fixed-width dictionary (8-byte values that differ in one byte) and a BYTE_ARRAY one, both compressible
    dic = pa.Table.from_arrays([pa.array((np.arange(n, dtype=np.int64) % 40) << 32), pa.array(["value %03d" % (i % 40) for i in range(n)], pa.string())],
                               schema=pa.schema([pa.field("k", pa.int64(), nullable=False), pa.field("s", pa.string(), nullable=False)]))
    dicts = P._write(dirpath, "sn_patch_dicts", dic, compression="SNAPPY", max_rows_per_page=37, data_page_version="1.0")
    return {"copies": copies, "levels": levels, "dicts": dicts}


def corrupt_in_place(stream):
    """(position in the stream, new byte): one byte that only decompression can find wrong — a copy's offset (below 256, one- or two-byte
    form) set to 0, or, in a stream without such a copy, the last literal made one byte longer than the input and the expected length"""
    els = elements(stream)
    near = [e for e in els if e[1] in (1, 2) and 0 < e[3] < 256]
    if near:
        return near[0][0] + 1, 0
    pos, kind, n, _first = els[-1]
    assert kind == 0 and n < 60, els
    return pos, stream[pos] + 4


def patched(dirpath, pages_of):
    """{name: (original bytes, patched bytes, column, the page the message must name)}: ONE byte changed in a SNAPPY file, located through
    the page directory (pages_of(data, column) -> ph_parquet_pages_ex entries) and the formats' layout. Each must give PH_EINVAL."""
    src = patch_sources(dirpath)
    out = {}

    def put(name, data, at, new, page, column=0):
        assert data[at] != new, (name, at)
        out[name] = (data, data[:at] + bytes([new]) + data[at + 1:], column, page)
    d = src["copies"].data
    pages = pages_of(d, 0)
    assert [p["kind"] for p in pages] == [0, 0, 0] and all(p["compressed"] == 1 and p["codec"] == 1 for p in pages)
    for k, p in enumerate(pages):
        stream = d[p["data_pos"]:p["data_pos"] + p["data_bytes"]]
        assert p["uncompressed_bytes"] == p["num_values"] * 8 and stream[:len(varint(p["uncompressed_bytes"]))] == varint(p["uncompressed_bytes"])
        # the stream's own length preamble: one more byte than the header says
        put("preamble_page%d" % k, d, p["data_pos"], stream[0] ^ 1, k)
        # a copy with a 2-byte offset below 256: its low byte becomes 0
        near = [e for e in elements(stream) if e[1] == 2 and 0 < e[3] < 256]
        assert near, elements(stream)
        put("copy_offset_0_page%d" % k, d, p["data_pos"] + near[0][0] + 1, 0, k)
    # the header of page 1: 0x15 <type> 0x15 <uncompressed_page_size, a two-byte zigzag varint> 0x15 <compressed_page_size> ...
    p = pages[1]
    at = p["header_pos"] + 3
    assert d[at - 1] == 0x15 and d[at] & 0x80 and d[at + 1] < 0x80 and d[at + 2] == 0x15
    assert ((d[at] & 0x7f) | d[at + 1] << 7) >> 1 == p["uncompressed_bytes"]
    assert ((d[at] & 0x7f) | 0x7f << 7) >> 1 > 22 * p["data_bytes"]
    put("uncompressed_size_impossible", d, at + 1, 0x7f, 1)
    # a nullable column, v1: [4-byte length n][levels, n bytes][values] is ONE stream; random values keep it a single literal, so the
    # length's top byte can be patched in place
    d = src["levels"].data
    pages = pages_of(d, 0)
    for k in (0, 2):
        p = pages[k]
        stream = d[p["data_pos"]:p["data_pos"] + p["data_bytes"]]
        first = elements(stream)[0]
        assert first[1] == 0 and first[2] >= 8 and p["compressed"] == 1
        n = int.from_bytes(stream[first[3]:first[3] + 4], "little")
        assert 0 < n < 16
        put("level_prefix_page%d" % k, d, p["data_pos"] + first[3] + 3, 0x7f, k)
    # a compressed dictionary page's stream, fixed-width (column 0) and BYTE_ARRAY (column 1): page 0 of the column's directory
    d = src["dicts"].data
    for column, name in ((0, "dictionary_stream_int"), (1, "dictionary_stream_str")):
        pages = pages_of(d, column)
        assert [p["kind"] for p in pages] == [2, 0, 0, 0] and all(p["compressed"] == 1 for p in pages)
        p = pages[0]
        at, new = corrupt_in_place(d[p["data_pos"]:p["data_pos"] + p["data_bytes"]])
        put(name, d, p["data_pos"] + at, new, 0, column)
    return out


def bad_dictionary_and_data_page(dirpath, pages_of, column):
    """the dictionary page (page 0) AND data page 2 of one column of the dictionary file corrupt -> bytes. planhip.h's order of pages names
    page 0 for a BYTE_ARRAY column (1) and page 2 for a fixed-width one (0), whose dictionary streams are judged last."""
    d = bytearray(patch_sources(dirpath)["dicts"].data)
    pages = pages_of(bytes(d), column)
    for k in (0, 2):
        p = pages[k]
        at, new = corrupt_in_place(bytes(d[p["data_pos"]:p["data_pos"] + p["data_bytes"]]))
        d[p["data_pos"] + at] = new
    return bytes(d)


def two_bad_pages(dirpath, pages_of):
    """pages 1 and 2 of one column both carry a copy with offset 0 -> (bytes, column)"""
    cases = patched(dirpath, pages_of)
    orig, one, column, _page = cases["copy_offset_0_page1"]
    _orig, two, _column, _page = cases["copy_offset_0_page2"]
    both = bytearray(one)
    for i, (a, b) in enumerate(zip(orig, two)):
        if a != b:
            both[i] = b
    return bytes(both), column


def write_gzip(dirpath):
    import pyarrow as pa
    return P._write(dirpath, "sn_refuse_gzip", pa.table({"i": pa.array(np.arange(100, dtype=np.int32))}), compression="GZIP").path


def write_patched(dirpath, pages_of):
    """the patched files on disk, for the stand-alone sanitizer program -> [path]"""
    paths = []
    for name, (_orig, bad, _column, _page) in patched(dirpath, pages_of).items():
        path = os.path.join(str(dirpath), "sn_bad_" + name + ".parquet")
        with open(path, "wb") as f:
            f.write(bad)
        paths.append(path)
    return paths
