"""Delta-encoded Parquet pages for the load-path tests (PH_PARQUET_DELTA), shared by the CPU tests (tests/test_delta_reference.py: the host
twin and the raw host decoder) and the GPU tests (tests/test_gpu_parquet_delta.py).

Raw DELTA_BINARY_PACKED streams come from the small encoder below, and `decode` restates the format description (parquet-format's
Encodings.md and the rules of include/planhip.h) in Python: it is the reference for raw streams, written from the description and not from
the product's code. Files are written with pyarrow (use_dictionary=False, column_encoding=...), and pq.read_table is their reference.

Sizes sit at the edges of a miniblock (32 / 64 values), a block (128 / 256) and a 256-lane step of the kernel; every file is a few
thousand rows at most."""
import os

import numpy as np

import parquet_cases as C

M64 = (1 << 64) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
MAX_BLOCK, MAX_MINIBLOCKS = 65536, 512          # plan_amd/csrc/parquet_decode.h: DELTA_MAX_BLOCK, DELTA_MAX_MINIBLOCKS
COUNTS = (0, 1, 2, 32, 33, 64, 65, 128, 129, 130, 256, 257, 258, 513)
E_DELTA_BINARY_PACKED, E_DELTA_LENGTH_BYTE_ARRAY = 5, 6


# ---------------------------------------------------------------- the format, restated

class Refused(Exception):
    """what the format (with this build's limits) refuses; .sub names the rule, .unsupported = a limit of this build, not of the format"""
    def __init__(self, sub, unsupported=False):
        super().__init__(sub)
        self.sub, self.unsupported = sub, unsupported


def uleb(n, pad=0):
    """ULEB128 of n >= 0; pad: extra continuation bytes (a longer spelling of the same number)"""
    out = bytearray()
    while True:
        b = n & 0x7f
        n >>= 7
        if n or pad:
            out.append(b | 0x80)
            if not n:
                out += bytes([0x80] * (pad - 1)) + b"\0"
                return bytes(out)
        else:
            out.append(b)
            return bytes(out)


def zigzag(v):
    """a signed 64-bit value as the unsigned number its zigzag ULEB128 spells"""
    return ((v << 1) ^ (v >> 63)) & M64


def signed(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def decode(stream, bits, expected=None, exact=False):
    """one DELTA_BINARY_PACKED stream -> ([values as signed `bits`-bit integers], bytes consumed, {miniblock widths met}); raises Refused"""
    pos = 0

    def varint():
        nonlocal pos
        v = 0
        for k in range(10):
            if pos >= len(stream):
                raise Refused("varint")
            b = stream[pos]
            pos += 1
            if k == 9 and b > 1:
                raise Refused("varint")           # more than 64 bits, or an eleventh byte
            v |= (b & 0x7f) << (7 * k)
            if not b & 0x80:
                return v
        raise Refused("varint")

    def unzig(u):
        return (u >> 1) ^ -(u & 1)
    block, mini, total, first = varint(), varint(), varint(), unzig(varint())
    if block == 0 or block % 128:
        raise Refused("block size")
    if mini == 0:
        raise Refused("0 miniblocks")
    if block > MAX_BLOCK or mini > MAX_MINIBLOCKS:
        raise Refused("limit", unsupported=True)
    if block % mini or (block // mini) % 32:
        raise Refused("multiple of 32")
    if expected is not None and total != expected:
        raise Refused("count")
    per = block // mini
    values, widths = [], set()
    if total:
        v = first & M64
        values.append(signed(v, bits))
        while len(values) < total:
            need = total - len(values)
            min_delta = unzig(varint())
            if pos + mini > len(stream):
                raise Refused("width bytes")
            wbytes = stream[pos:pos + mini]
            pos += mini
            for m in range(mini):
                if m * per >= need:
                    break                          # no bytes, and the width byte means nothing
                w = wbytes[m]
                if w > bits:
                    raise Refused("width")
                nbytes = per * w // 8
                if pos + nbytes > len(stream):
                    raise Refused("miniblock")
                widths.add(w)
                word = int.from_bytes(stream[pos:pos + nbytes], "little")
                pos += nbytes
                for j in range(min(per, need - m * per)):
                    v = (v + min_delta + ((word >> (j * w)) & ((1 << w) - 1))) & M64
                    values.append(signed(v, bits))
    if exact and pos != len(stream):
        raise Refused("left over")
    return values, pos, widths


def header(block, mini, total, first, pad=0):
    return uleb(block) + uleb(mini) + uleb(total) + uleb(zigzag(first), pad)


def pack(rel, w):
    word = 0
    for j, r in enumerate(rel):
        word |= r << (j * w)
    return word.to_bytes(len(rel) * w // 8, "little")


def encode(values, bits=64, block=128, mini=4, junk_width=0, min_width=0, pad=0):
    """the stream a writer emits for `values`: per block the smallest delta, per miniblock the widest remainder. junk_width: the width byte
    of the miniblocks of the last block that hold no value; min_width: no miniblock narrower than this; pad: longer varints"""
    per = block // mini
    mask = (1 << bits) - 1
    out = bytearray(header(block, mini, len(values), values[0] if values else 0, pad))
    deltas = [signed(values[i] - values[i - 1], bits) for i in range(1, len(values))]
    for b in range(0, len(deltas), block):
        d = deltas[b:b + block]
        lo = min(d)
        rel = [(x - lo) & mask for x in d]
        out += uleb(zigzag(lo), pad)
        widths, body = bytearray(), bytearray()
        for m in range(mini):
            r = rel[m * per:(m + 1) * per]
            if not r:
                widths.append(junk_width)
                continue
            w = max(min_width, max(x.bit_length() for x in r))
            widths.append(w)
            body += pack(r + [0] * (per - len(r)), w)
        out += widths + body
    return bytes(out)


def valid_streams():
    """[(name, stream, bits)]: what no writer here produces, and the edges in raw form"""
    rng = np.random.default_rng(3)
    out = []
    ramp = [3 * i - 7 for i in range(300)]
    out.append(("block128_1_miniblock", encode(ramp, block=128, mini=1), 64))
    out.append(("block256_8_miniblocks", encode([int(v) for v in rng.integers(-10**6, 10**6, 700)], block=256, mini=8), 64))
    out.append(("block384_4_miniblocks_of_96", encode([int(v) for v in rng.integers(-50, 50, 1000)], block=384, mini=4), 64))
    out.append(("block65536_512_miniblocks", encode([int(v) for v in rng.integers(0, 9, 600)], block=65536, mini=512), 32))
    out.append(("junk_width_bytes_on_unneeded_miniblocks", encode(ramp[:130], junk_width=0xff), 64))
    out.append(("junk_width_bytes_int32", encode(ramp[:34], bits=32, junk_width=0xff), 32))
    out.append(("width_64_random", encode([int(v) for v in rng.integers(I64_MIN, I64_MAX, 515, endpoint=True)], min_width=64), 64))
    out.append(("width_32_random_int32", encode([int(v) for v in rng.integers(I32_MIN, I32_MAX, 515, endpoint=True)], bits=32, min_width=32), 32))
    out.append(("first_value_and_min_delta_of_10_bytes", encode([I64_MIN, 0, I64_MIN, 0, I64_MIN + 5]), 64))
    out.append(("padded_varints_of_10_bytes", encode(ramp[:140], pad=8), 64))
    out.append(("alternating_int64_extremes", encode([I64_MIN, I64_MAX] * 200), 64))
    out.append(("alternating_int32_extremes", encode([I32_MIN, I32_MAX] * 200, bits=32), 32))
    out.append(("int32_stream_wraps_through_64_bit_sums", header(128, 4, 3, I32_MAX) + uleb(zigzag(1)) + bytes([0, 0, 0, 0]), 32))
    for n in COUNTS:
        vals = [int(v) for v in rng.integers(-10**12, 10**12, n)]
        out.append(("count_%d" % n, encode(vals) if n else header(128, 4, 0, 0), 64))
    return out


def invalid_streams():
    """[(name, stream, bits, expected count or None, the word the message must hold, unsupported)]; all are decoded with exact=True"""
    ramp = [5 * i + i * i % 7 for i in range(200)]
    good = encode(ramp)
    one_block = encode(ramp[:129])                # header, min_delta, 4 width bytes, 4 miniblocks
    hdr = len(header(128, 4, 129, 0))
    out = [
        ("block_size_0", header(0, 4, 5, 0) + bytes(40), 64, None, "block size", False),
        ("block_size_127", header(127, 1, 5, 0) + bytes(40), 64, None, "block size", False),
        ("block_192_of_4_miniblocks", header(192, 4, 5, 0) + bytes(40), 64, None, "block size", False),
        ("block_384_of_8_miniblocks_of_48", header(384, 8, 5, 0) + bytes(40), 64, None, "multiple of 32", False),
        ("miniblocks_0", header(128, 0, 5, 0) + bytes(40), 64, None, "0 miniblocks", False),
        ("block_size_131072", header(131072, 4, 5, 0) + bytes(40), 64, None, "65536", True),
        ("miniblocks_1024", header(32768, 1024, 5, 0) + bytes(1100), 64, None, "512", True),
        ("count_one_more", good, 64, len(ramp) - 1, "count", False),
        ("count_one_less", good, 64, len(ramp) + 1, "count", False),
        ("width_65", one_block[:hdr + 1] + bytes([65]) + one_block[hdr + 2:] + bytes(300), 64, None, "width", False),
        ("width_33_int32", header(128, 4, 129, 0) + b"\0" + bytes([33, 0, 0, 0]) + bytes(200), 32, None, "width", False),
        ("miniblock_cut_by_one_byte", one_block[:-1], 64, None, "runs off", False),
        ("width_bytes_cut", one_block[:hdr + 3], 64, None, "run off", False),
        ("varint_of_11_bytes", uleb(128, pad=9) + uleb(4) + uleb(1) + uleb(0), 64, None, "varint", False),
        ("varint_above_64_bits", uleb(128) + uleb(4) + uleb(1) + bytes([0xff] * 9 + [0x02]), 64, None, "varint", False),
        ("varint_off_the_end", uleb(128) + uleb(4) + b"\x80", 64, None, "varint", False),
        ("min_delta_off_the_end", header(128, 4, 2, 0) + b"\x80\x80", 64, None, "varint", False),
        ("empty_stream", b"", 64, None, "varint", False),
        ("one_trailing_byte", good + b"\0", 64, None, "left over", False),
    ]
    assert one_block[hdr] < 0x80 and all(0 < w <= 8 for w in one_block[hdr + 1:hdr + 5])       # a one-byte min_delta, then the four widths
    return out


# ---------------------------------------------------------------- files

def encodings_for(table, strings=True):
    import pyarrow as pa
    enc = {}
    for f in table.schema:
        if pa.types.is_string(f.type) or pa.types.is_binary(f.type):
            if strings:
                enc[f.name] = "DELTA_LENGTH_BYTE_ARRAY"
        else:
            enc[f.name] = "DELTA_BINARY_PACKED"
    return enc


def write_delta(dirpath, name, table, **kw):
    kw.setdefault("use_dictionary", False)
    kw.setdefault("column_encoding", encodings_for(table))
    kw.setdefault("store_decimal_as_integer", True)
    return C._write(dirpath, name, table, **kw)


def count_table(n, nullable, seed):
    """n VALUES per column: required columns of n rows, or nullable ones with about 30 % NULL rows around the n values"""
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    rows = n if not nullable else n + max(7, int(round(n * 0.43)))
    mask = None
    if nullable:
        mask = np.ones(rows, bool)
        mask[rng.permutation(rows)[:n]] = False
    i32 = rng.integers(I32_MIN, I32_MAX, rows, endpoint=True).astype(np.int32)
    i64 = rng.integers(-2**40, 2**40, rows)
    strs = ["s%d" % v * int(v % 4) for v in rng.integers(0, 1000, rows)]
    fields = [pa.field("i32", pa.int32(), nullable), pa.field("i64", pa.int64(), nullable), pa.field("s", pa.string(), nullable)]
    arrays = [pa.array(i32, pa.int32(), mask=mask), pa.array(i64, pa.int64(), mask=mask), pa.array(strs, pa.string(), mask=mask)]
    return pa.Table.from_arrays(arrays, schema=pa.schema(fields))


def widths_table(n=1000, seed=21):
    """int64 columns whose deltas need 0, 1, 7, 8, 9, 31, 32, 33, 63 and 64 bits, the wraps, a negative min_delta and a block whose
    miniblocks differ in width; the int32 ones beside them. Required and, with suffix _n, about 30 % NULL."""
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    cols = {"stride": np.arange(n, dtype=np.int64) * 12345 - 99, "steps01": np.cumsum(rng.integers(0, 2, n)).astype(np.int64)}
    for w in (7, 8, 9, 31, 32, 33, 63):
        d = rng.integers(0, 1 << w, n, dtype=np.uint64)
        d[1::32] = 0
        d[2::32] = (1 << w) - 1
        cols["w%d" % w] = np.cumsum(d, dtype=np.uint64).view(np.int64)
    cols["w64"] = rng.integers(I64_MIN, I64_MAX, n, endpoint=True)
    cols["alt64"] = np.where(np.arange(n) % 2 == 0, I64_MIN, I64_MAX).astype(np.int64)
    cols["falling"] = -np.cumsum(rng.integers(1000, 5000, n)).astype(np.int64)
    mixed = np.concatenate([rng.integers(0, 3, 70), rng.integers(0, 1 << 50, n - 70)])
    cols["mixed_widths"] = np.cumsum(mixed).astype(np.int64)
    cols["alt32"] = np.where(np.arange(n) % 2 == 0, I32_MIN, I32_MAX).astype(np.int32)
    cols["w32_i32"] = rng.integers(I32_MIN, I32_MAX, n, endpoint=True).astype(np.int32)
    cols["stride_i32"] = (np.arange(n, dtype=np.int64) * 7 - 3).astype(np.int32)
    cols["w9_i32"] = np.cumsum(rng.integers(0, 512, n)).astype(np.int32)
    arrays, fields = [], []
    for name, v in cols.items():
        typ = pa.int32() if v.dtype == np.int32 else pa.int64()
        arrays += [pa.array(v, typ), pa.array(v, typ, mask=C._mask(rng, n))]
        fields += [pa.field(name, typ, False), pa.field(name + "_n", typ, True)]
    return pa.Table.from_arrays(arrays, schema=pa.schema(fields))


def overrides_table(n=700):
    import pyarrow as pa
    rng = np.random.default_rng(31)
    small = rng.integers(I32_MIN, I32_MAX, n, endpoint=True)
    big = small.copy()
    big[n // 2] = I32_MAX + 1
    return pa.table({"i32": pa.array(small.astype(np.int32)), "small64": pa.array(small), "big64": pa.array(big),
                     "small64_n": pa.array(small, mask=C._mask(rng, n))})


def strings_table(kind):
    import pyarrow as pa
    if kind == "all_null":
        return pa.table({"s": pa.array([None] * 300, pa.string()), "i": pa.array([None] * 300, pa.int64())})
    if kind == "one_value":
        return pa.table({"s": pa.array(["only"], pa.string()), "n": pa.array(["x"], pa.string())})
    return C.varchar_table(kind)


MATRIX_ROWS = 3000
STRING_KINDS = ("256_nulls", "256_empty_nulls", "257", "nul_byte", "empty", "long", "all_null", "one_value")
_CACHE = {}


def case_specs():
    """[(name, table builder, SNAPPY?, writer knobs)] of every well-formed file"""
    out = []

    def add(name, build, snappy=False, **kw):
        out.append((name, build, snappy, kw))
    for n in COUNTS:
        add("count_%d_nullable" % n, lambda n=n: count_table(n, True, 200 + n), data_page_version="2.0" if n % 2 else "1.0")
        if n:
            add("count_%d_required" % n, lambda n=n: count_table(n, False, 300 + n), data_page_version="1.0" if n % 2 else "2.0")

    def m():
        return C.matrix_table(MATRIX_ROWS)
    for snappy in (False, True):
        tail = "_snappy" if snappy else ""
        add("matrix_v1" + tail, m, snappy, data_page_version="1.0")
        add("matrix_v2" + tail, m, snappy, data_page_version="2.0")
        add("matrix_pages37_v1" + tail, m, snappy, max_rows_per_page=37, data_page_version="1.0")
        add("matrix_pages37_v2" + tail, m, snappy, max_rows_per_page=37, data_page_version="2.0")
        add("matrix_3groups" + tail, m, snappy, row_group_size=1100)
    add("widths_v1", widths_table, data_page_version="1.0")
    add("widths_v2_pages37", widths_table, data_page_version="2.0", max_rows_per_page=37)
    add("widths_v2_snappy", widths_table, True, data_page_version="2.0")
    add("overrides", overrides_table)
    for kind in STRING_KINDS:
        add("strings_" + kind, lambda kind=kind: strings_table(kind), data_page_version="2.0" if kind in ("257", "long") else "1.0")
    add("strings_long_snappy", lambda: strings_table("long"), True)
    # dictionary pages in two columns, delta pages in the others of the same file
    add("dictionary_beside_delta", m, use_dictionary=["s40_n", "s40_r"], column_encoding="not s40")
    return out


CASE_NAMES = [spec[0] for spec in case_specs()]


def generate(dirpath):
    """every well-formed file, written once per directory: {name: (Case, the flag it needs beside PH_PARQUET_DELTA: 0 or PH_PARQUET_SNAPPY)}.
    Without a Snappy codec in pyarrow the SNAPPY files are left out."""
    import pyarrow as pa
    key = str(dirpath)
    if key in _CACHE:
        return _CACHE[key]
    out, tables = {}, {}
    for name, build, snappy, kw in case_specs():
        if snappy and not pa.Codec.is_available("snappy"):
            continue
        if build not in tables:
            tables[build] = build()
        table = tables[build]
        kw = dict(kw)
        if snappy:
            kw["compression"] = "SNAPPY"
        if kw.get("column_encoding") == "not s40":
            kw["column_encoding"] = {k: v for k, v in encodings_for(table).items() if not k.startswith("s40")}
        out[name] = (write_delta(dirpath, name, table, **kw), 1 if snappy else 0)
    _CACHE[key] = out
    return out


def plain_twin(dirpath, name, table):
    """the same rows written PLAIN (no dictionary), for the cross-encoding comparison at flags 0"""
    return C._write(dirpath, name + "_plain", table, use_dictionary=False, store_decimal_as_integer=True)


def unsupported_files(dirpath):
    """{name: (path, the encoding its refusal names)}: outside the subset with the flag too"""
    import pyarrow as pa
    n = 100
    t = pa.table({"s": pa.array(["v%d" % i for i in range(n)]), "i": pa.array(np.arange(n, dtype=np.int32))})
    return {
        "delta_byte_array": (C._write(dirpath, "un_dba", t, use_dictionary=False, column_encoding={"s": "DELTA_BYTE_ARRAY", "i": "PLAIN"}).path, "s", "DELTA_BYTE_ARRAY"),
        "byte_stream_split": (C._write(dirpath, "un_bss", t, use_dictionary=False, column_encoding={"s": "PLAIN", "i": "BYTE_STREAM_SPLIT"}).path, "i", "BYTE_STREAM_SPLIT"),
    }


def delta_length_file(dirpath):
    import pyarrow as pa
    t = pa.table({"s": pa.array(["v%d" % i for i in range(100)])})
    return C._write(dirpath, "refuse_delta_length", t, use_dictionary=False, column_encoding={"s": "DELTA_LENGTH_BYTE_ARRAY"}).path


# ---------------------------------------------------------------- one-byte patches of pyarrow-written files

def patch_sources(dirpath):
    import pyarrow as pa
    ints = pa.Table.from_arrays([pa.array(np.arange(300, dtype=np.int64) * 1000 + np.arange(300) % 7)], schema=pa.schema([pa.field("v", pa.int64(), False)]))
    strs = pa.Table.from_arrays([pa.array(["alpha", "be", "gamma"] * 20, pa.string())], schema=pa.schema([pa.field("s", pa.string(), False)]))
    return {"ints": write_delta(dirpath, "patch_delta_ints", ints, max_rows_per_page=100, data_page_version="1.0"),
            "strs": write_delta(dirpath, "patch_delta_strs", strs, data_page_version="1.0")}


def patched(dirpath, pages_of):
    """{name: (original bytes, patched bytes, column, page)}: ONE byte changed inside a delta page, located through the page directory
    (encoding 5 / 6) and the stream's layout. A name that begins with tolerated_ is a file pyarrow still reads."""
    src = patch_sources(dirpath)
    out = {}

    def put(name, data, at, old, new, page, column=0):
        assert data[at] == old, (name, at, data[at], old)
        out[name] = (data, data[:at] + bytes([new]) + data[at + 1:], column, page)
    # a required INT64 column, 100 rows a page: [block 256 = 80 02][4 miniblocks][total 100][first][min_delta][4 widths][miniblocks]
    d = src["ints"].data
    pages = [p for p in pages_of(d, 0)]
    assert [p["encoding"] for p in pages] == [E_DELTA_BINARY_PACKED] * 3 and all(p["num_values"] == 100 for p in pages)
    at = pages[1]["data_pos"]
    assert d[at:at + 4] == bytes([0x80, 0x02, 4, 100])
    put("tolerated_header_count_more", d, at + 3, 100, 101, 1)
    put("header_count_fewer", d, at + 3, 100, 99, 1)
    vals, used, _w = decode(d[at:at + pages[1]["data_bytes"]], 64, 100, exact=True)
    assert vals == [1000 * i + i % 7 for i in range(100, 200)] and used == pages[1]["data_bytes"]
    first_len = len(uleb(zigzag(vals[0])))
    min_len = len(uleb(zigzag(min(vals[i + 1] - vals[i] for i in range(99)))))
    widths_at = at + 4 + first_len + min_len
    assert 0 < d[widths_at] <= 64 and d[widths_at + 1] == d[widths_at]
    put("width_65", d, widths_at + 1, d[widths_at + 1], 65, 1)
    put("block_size_384", d, at + 1, 0x02, 0x03, 1)          # 80 03 = 384, of 4 miniblocks of 96: well-formed so far; the stream then ends early
    # a required DELTA_LENGTH_BYTE_ARRAY column: lengths 5, 2, 5, ... then 240 bytes of values
    d = src["strs"].data
    p0 = [p for p in pages_of(d, 0)][0]
    assert p0["encoding"] == E_DELTA_LENGTH_BYTE_ARRAY and p0["num_values"] == 60
    at = p0["data_pos"]
    lens, used, _w = decode(d[at:at + p0["data_bytes"]], 32, 60)
    assert lens == [5, 2, 5] * 20 and p0["data_bytes"] - used == 240 and d[at:at + 4] == bytes([0x80, 0x01, 4, 60]) and d[at + 4] == zigzag(5)
    put("length_negative", d, at + 4, zigzag(5), zigzag(-5), 0)                    # the first length, and every third after it less by 10
    put("lengths_sum_past_the_page", d, at + 4, zigzag(5), zigzag(6), 0)
    put("tolerated_lengths_sum_short", d, at + 4, zigzag(5), zigzag(4), 0)
    return out


def two_bad_pages(dirpath, pages_of):
    """pages 1 and 2 of one column patched: page 1 must be named"""
    src = patch_sources(dirpath)
    d = bytearray(src["ints"].data)
    pages = [p for p in pages_of(bytes(d), 0)]
    for p in pages[1:]:
        assert d[p["data_pos"] + 3] == 100
        d[p["data_pos"] + 3] = 99
    return bytes(d), 0


def write_all(dirpath, pages_of):
    """every generated, patched and unsupported file as paths (for the sanitizer's program) -> (paths, columns that decode, columns refused)"""
    paths, good, bad = [], 0, 0
    for case, _f in generate(dirpath).values():
        paths.append(case.path)
        good += case.table.num_columns
    for name, (_orig, data, _c, _p) in patched(dirpath, pages_of).items():
        p = os.path.join(str(dirpath), "bad_" + name + ".parquet")
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p)
        bad += 1
    both, _c = two_bad_pages(dirpath, pages_of)
    p = os.path.join(str(dirpath), "bad_two_pages.parquet")
    with open(p, "wb") as f:
        f.write(both)
    paths.append(p)
    bad += 1
    for path, _col, _enc in unsupported_files(dirpath).values():
        paths.append(path)
        good += 1
        bad += 1
    return paths, good, bad
