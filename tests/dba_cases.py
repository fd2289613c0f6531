"""Front-coded Parquet pages (DELTA_BYTE_ARRAY) for the load-path tests (PH_PARQUET_DELTA_BYTE_ARRAY), shared by the CPU tests
(tests/test_dba_reference.py: the host twin and the raw host decoder) and the GPU tests (tests/test_gpu_parquet_dba.py).

Raw values sections come from the small encoder below (over tests/delta_cases.py's DELTA_BINARY_PACKED encoder), and `decode` restates the
format description (parquet-format's Encodings.md and the rules of include/planhip.h) in Python: it is the reference for raw sections, written
from the description and not from the product's code, and the CPU tests pin it against the values sections pyarrow writes. Files are written
with pyarrow (use_dictionary=False, column_encoding=DELTA_BYTE_ARRAY), and pq.read_table is their reference.

Counts sit at the edges of a lane group (64 values), a workgroup step (256) and a delta block (128); string shapes at the edges of the
one-byte-a-lane copy (64), a copy step (1024 bytes) and the reconstruction kernel's ring (RING). Every file is a few thousand rows at most."""
import os

import numpy as np

import delta_cases as D
import parquet_cases as C

RING = 16384                                     # plan_amd/csrc/dba_decode.h: DBA_RING
COUNTS = (0, 1, 2, 32, 33, 64, 65, 128, 129, 256, 257, 513)
E_DELTA_BYTE_ARRAY = 7
Refused = D.Refused


# ---------------------------------------------------------------- the format, restated

def front_code(values):
    """[bytes] -> (prefix lengths, suffixes): the longest prefix each value shares with the one in front of it"""
    pre, suf, last = [], [], b""
    for v in values:
        n = 0
        while n < len(v) and n < len(last) and v[n] == last[n]:
            n += 1
        pre.append(n)
        suf.append(v[n:])
        last = v
    return pre, suf


def section(prefixes, suffix_lens, suffix_bytes, prefix_total=None, suffix_total=None):
    """a values section from its parts, which need not agree with each other"""
    def stream(vals, total):
        s = D.encode(vals, bits=32) if vals else D.header(128, 4, 0, 0)
        if total is not None:
            head = D.header(128, 4, len(vals), vals[0] if vals else 0)
            assert s.startswith(head)
            s = D.header(128, 4, total, vals[0] if vals else 0) + s[len(head):]
        return s
    return stream(prefixes, prefix_total) + stream(suffix_lens, suffix_total) + bytes(suffix_bytes)


def encode(values, shared=True):
    """the section a writer emits for `values`; shared=False: no front coding at all (every prefix 0), which is as valid"""
    pre, suf = front_code(values) if shared else ([0] * len(values), list(values))
    return section(pre, [len(s) for s in suf], b"".join(suf))


def decode(data, expected=None):
    """one values section -> [values]; raises Refused. The section ends where its suffix bytes end."""
    pre, used, _w = D.decode(data, 32, expected)
    if any(p < 0 for p in pre):
        raise Refused("prefix")
    try:
        suf, used2, _w = D.decode(data[used:], 32, len(pre))
    except Refused as r:
        raise Refused("suffix stream: " + r.sub, r.unsupported)
    if any(s < 0 for s in suf):
        raise Refused("negative suffix")
    before = 0
    for p, s in zip(pre, suf):
        if p > before:
            raise Refused("prefix")
        before = p + s
    at = used + used2
    if sum(suf) > len(data) - at:
        raise Refused("suffix past")
    if sum(suf) < len(data) - at:
        raise Refused("suffix short")
    if sum(p + s for p, s in zip(pre, suf)) >= 1 << 31:
        raise Refused("2^31")
    out, last = [], b""
    for p, s in zip(pre, suf):
        last = last[:p] + data[at:at + s]
        at += s
        out.append(last)
    return out


def shapes():
    """{name: [bytes]}: each the smallest at which the chain can go wrong"""
    rng = np.random.default_rng(9)
    out = {
        "identical": [b"the same value"] * 70,
        "nothing_shared": [bytes([65 + i % 26]) + b"tail%d" % i for i in range(70)],
        "sorted_keys": [b"key/%08d" % (i * 37) for i in range(300)],
        "empty_between_long": [b"x" * 300, b"", b"x" * 300, b"", b"", b"x" * 301, b""],
        "nul_byte": [b"a\0b", b"a\0bc", b"a\0", b"\0", b"\0\0"],
        "one_value": [b"only"],
        "random_text": [bytes(rng.integers(97, 123, int(n), dtype=np.uint8)) for n in rng.integers(0, 40, 200)],
    }
    for n in (63, 64, 65, 255, 256, 257, 1023, 1024, 1025):
        out["prefix_%d" % n] = [b"p" * n + b"first", b"p" * n + b"second", b"p" * n, b"p" * n + b"x" * n]
    for n in (RING - 1, RING, RING + 1):
        big = bytes(rng.integers(97, 123, n, dtype=np.uint8))
        out["ring_%d" % n] = [b"head", big, big, big + b"+tail", big[:n // 2], b"", big]
    for n in COUNTS:
        out["count_%d" % n] = [b"k%05d" % (i * 7 // 3) for i in range(n)]
    return out


def valid_sections():
    """[(name, section, values)]"""
    out = [(name, encode(vals), vals) for name, vals in shapes().items()]
    vals = shapes()["sorted_keys"]
    out.append(("no_front_coding", encode(vals, shared=False), vals))
    return out


def bomb():
    """prefix = 0, 1, 2, ... with one-byte suffixes: all deltas are 1, both streams together take 5 KB, the values 2.45 GB"""
    n = 70000
    return section(list(range(n)), [1] * n, b"z" * n)


def invalid_sections():
    """[(name, section, expected count or None, the word the message must hold, status name)]"""
    vals = shapes()["sorted_keys"][:40]
    pre, suf = front_code(vals)
    lens, byts = [len(s) for s in suf], b"".join(suf)
    assert pre[1] == 10 and len(vals[0]) == 12

    def with_(i, p):
        q = list(pre)
        q[i] = p
        return q
    bad_lens = list(lens)
    bad_lens[5] = -1
    return [
        ("prefix_0_not_0", section(with_(0, 1), lens, byts), None, "prefix longer", "EINVAL"),
        ("prefix_one_above_the_value_in_front", section(with_(1, 13), lens, byts), None, "prefix longer", "EINVAL"),
        ("prefix_negative", section(with_(7, -1), lens, byts), None, "prefix longer", "EINVAL"),
        ("suffix_length_negative", section(pre, bad_lens, byts), None, "negative suffix", "EINVAL"),
        ("suffix_bytes_one_short", section(pre, lens, byts[:-1]), None, "past the end", "EINVAL"),
        ("suffix_bytes_one_over", section(pre, lens, byts + b"!"), None, "left over", "EINVAL"),
        ("counts_differ", section(pre, lens[:-1], byts[:-lens[-1]]), None, "suffix-length stream: a header count", "EINVAL"),
        ("count_other_than_expected", section(pre, lens, byts), len(vals) + 1, "prefix-length stream: a header count", "EINVAL"),
        ("prefix_stream_malformed", D.header(127, 1, 5, 0) + bytes(40), None, "prefix-length stream: a block size", "EINVAL"),
        ("suffix_stream_over_the_limit", D.encode(pre, bits=32) + D.header(131072, 4, len(pre), 0) + bytes(40), None, "suffix-length stream: a block of more", "EUNSUPPORTED"),
        ("empty_section", b"", None, "varint", "EINVAL"),
        ("expansion_bomb", bomb(), None, "2^31", "EINVAL"),
    ]


# ---------------------------------------------------------------- files

def write_dba(dirpath, name, table, front=None, **kw):
    """front: the columns written DELTA_BYTE_ARRAY (default: every string / binary column); the others keep pyarrow's defaults unless
    column_encoding names them"""
    import pyarrow as pa
    cols = front if front is not None else [f.name for f in table.schema if pa.types.is_string(f.type) or pa.types.is_binary(f.type)]
    enc = dict(kw.pop("column_encoding", {}))
    enc.update({c: "DELTA_BYTE_ARRAY" for c in cols})
    if "use_dictionary" not in kw:
        kw["use_dictionary"] = False
    return C._write(dirpath, name, table, column_encoding=enc, store_decimal_as_integer=True, **kw)


def count_table(n, nullable, seed):
    """n VALUES per column: required columns of n rows, or nullable ones with about 30 % NULL rows around the n values"""
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    rows = n if not nullable else n + max(7, int(round(n * 0.43)))
    mask = None
    if nullable:
        mask = np.ones(rows, bool)
        mask[rng.permutation(rows)[:n]] = False
    keys = ["key/%06d" % (i * 3) for i in range(rows)]
    text = ["".join(chr(c) for c in rng.integers(97, 100, int(k))) for k in rng.integers(0, 12, rows)]
    fields = [pa.field("sorted", pa.string(), nullable), pa.field("text", pa.string(), nullable)]
    return pa.Table.from_arrays([pa.array(keys, pa.string(), mask=mask), pa.array(text, pa.string(), mask=mask)], schema=pa.schema(fields))


MATRIX_ROWS = 3000


def matrix_table(n=MATRIX_ROWS, seed=13):
    """the string shapes side by side, each required (_r) and with about 30 % NULLs (_n), and an integer and a low-cardinality column"""
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    cols = {
        "same": ["one and the same"] * n,
        "none": [chr(65 + i % 26) + "x%d" % i for i in range(n)],
        "sorted": ["customer#%09d" % (i * 11) for i in range(n)],
        "text": ["".join(chr(c) for c in rng.integers(97, 101, int(k))) for k in rng.integers(0, 30, n)],
        "gaps": [("y" * 200 + str(i % 7)) if i % 3 == 0 else "" for i in range(n)],
        "s40": ["k%d" % v for v in rng.integers(0, 40, n)],
    }
    arrays, fields = [], []
    for name, v in cols.items():
        arrays += [pa.array(v, pa.string(), mask=C._mask(rng, n)), pa.array(v, pa.string())]
        fields += [pa.field(name + "_n", pa.string(), True), pa.field(name + "_r", pa.string(), False)]
    arrays.append(pa.array(np.arange(n, dtype=np.int64) * 5))
    fields.append(pa.field("i64", pa.int64(), False))
    return pa.Table.from_arrays(arrays, schema=pa.schema(fields))


def shape_table(kind):
    import pyarrow as pa
    if kind == "all_null":
        return pa.table({"s": pa.array([None] * 300, pa.string()), "t": pa.array([None] * 300, pa.binary())})
    if kind == "long":
        return C.varchar_table("long")
    if kind in ("256", "257"):
        d = ["str %05d" % (i * 7919 % 100000) for i in range(int(kind))]
        return pa.table({"s": pa.array(sorted(d * 3), pa.string()), "u": pa.array(d * 3, pa.string())})
    vals = shapes()[kind]
    t = {"s": pa.array(vals, pa.binary()), "n": pa.array([None if i % 4 == 1 else v for i, v in enumerate(vals)], pa.binary())}
    return pa.table(t)


FILE_SHAPES = ("identical", "nothing_shared", "empty_between_long", "nul_byte", "one_value", "prefix_63", "prefix_64", "prefix_65", "prefix_255", "prefix_256", "prefix_257",
               "prefix_1024", "ring_%d" % (RING - 1), "ring_%d" % RING, "ring_%d" % (RING + 1), "long", "256", "257", "all_null")
CODECS = (("snappy", "SNAPPY", 1), ("lz4", "LZ4", 16), ("gzip", "GZIP", 64), ("zstd", "ZSTD", 256))      # pyarrow's name, the writer's, the load's flag
_CACHE = {}


def case_specs():
    """[(name, table builder, codec row or None, PH_PARQUET_DELTA needed too, writer knobs)] of every well-formed file"""
    out = []

    def add(name, build, codec=None, delta=False, **kw):
        out.append((name, build, codec, delta, kw))
    for n in COUNTS:
        add("count_%d_nullable" % n, lambda n=n: count_table(n, True, 200 + n), data_page_version="2.0" if n % 2 else "1.0")
        if n:
            add("count_%d_required" % n, lambda n=n: count_table(n, False, 300 + n), data_page_version="1.0" if n % 2 else "2.0")
    add("matrix_v1", matrix_table, data_page_version="1.0")
    add("matrix_v2", matrix_table, data_page_version="2.0")
    add("matrix_pages37_v1", matrix_table, max_rows_per_page=37, data_page_version="1.0")
    add("matrix_pages37_v2", matrix_table, max_rows_per_page=37, data_page_version="2.0")
    add("matrix_3groups", matrix_table, row_group_size=1100)
    for kind in FILE_SHAPES:
        add("shape_" + kind, lambda kind=kind: shape_table(kind), data_page_version="2.0" if kind in ("257", "long", "prefix_64") else "1.0")
    # a dictionary column and a DELTA_LENGTH_BYTE_ARRAY column beside the front-coded ones; the integers DELTA_BINARY_PACKED
    add("beside_dictionary_and_delta_length", matrix_table, delta=True, front="mixed", max_rows_per_page=500)
    for codec in CODECS:
        add("matrix_pages37_v2_" + codec[0], matrix_table, codec, max_rows_per_page=37, data_page_version="2.0")
        add("matrix_v1_" + codec[0], matrix_table, codec, data_page_version="1.0")
        add("shape_ring_%d_%s" % (RING + 1, codec[0]), lambda: shape_table("ring_%d" % (RING + 1)), codec)
        add("shape_long_" + codec[0], lambda: shape_table("long"), codec, data_page_version="2.0")
    return out


CASE_NAMES = [spec[0] for spec in case_specs()]


def generate(dirpath):
    """every well-formed file, written once per directory: {name: (Case, the flags it needs beside PH_PARQUET_DELTA_BYTE_ARRAY)}. A codec
    this pyarrow cannot write is left out."""
    import pyarrow as pa
    key = str(dirpath)
    if key in _CACHE:
        return _CACHE[key]
    out, tables = {}, {}
    for name, build, codec, delta, kw in case_specs():
        if codec and not pa.Codec.is_available(codec[0]):
            continue
        if build not in tables:
            tables[build] = build()
        table = tables[build]
        kw = dict(kw)
        if codec:
            kw["compression"] = codec[1]
        if kw.get("front") == "mixed":
            kw["front"] = [c for c in table.column_names if c[:4] in ("same", "sort", "gaps")]
            kw["use_dictionary"] = ["s40_n", "s40_r"]
            kw["column_encoding"] = {"text_n": "DELTA_LENGTH_BYTE_ARRAY", "text_r": "DELTA_LENGTH_BYTE_ARRAY", "none_n": "PLAIN", "none_r": "PLAIN", "i64": "DELTA_BINARY_PACKED"}
        out[name] = (write_dba(dirpath, name, table, **kw), (codec[2] if codec else 0) | (4 if delta else 0))
    _CACHE[key] = out
    return out


def plain_twin(dirpath, name, table):
    """the same rows written PLAIN (no dictionary), for the cross-encoding comparison at flags 0"""
    return C._write(dirpath, name + "_plain", table, use_dictionary=False, store_decimal_as_integer=True)


def unsupported_files(dirpath):
    """{name: (path, column, the encoding its refusal names, the physical type it names or None)}: outside the subset with the flag too"""
    import pyarrow as pa
    n = 100
    import decimal
    t = pa.table({"f": pa.array([decimal.Decimal(i * 1000003) for i in range(n)], pa.decimal128(20, 0)), "s": pa.array(["v%d" % i for i in range(n)]), "i": pa.array(np.arange(n, dtype=np.int32))})
    return {
        "flba": (C._write(dirpath, "un_dba_flba", t, use_dictionary=False, column_encoding={"f": "DELTA_BYTE_ARRAY", "s": "DELTA_BYTE_ARRAY", "i": "PLAIN"}).path, "f",
                 "DELTA_BYTE_ARRAY", "FIXED_LEN_BYTE_ARRAY"),
        "byte_stream_split": (C._write(dirpath, "un_dba_bss", t, use_dictionary=False, column_encoding={"f": "PLAIN", "s": "DELTA_BYTE_ARRAY", "i": "BYTE_STREAM_SPLIT"}).path, "i",
                              "BYTE_STREAM_SPLIT", None),
    }


# ---------------------------------------------------------------- one-byte patches of pyarrow-written files

PATCH_VALUES = ["alpha", "alpine", "beta"] * 20          # prefixes 0, 3, 0, ...; suffixes of 5, 3 and 4 bytes


def patch_sources(dirpath):
    import pyarrow as pa
    strs = pa.Table.from_arrays([pa.array(PATCH_VALUES, pa.string())], schema=pa.schema([pa.field("s", pa.string(), False)]))
    pages = pa.Table.from_arrays([pa.array(PATCH_VALUES * 5, pa.string())], schema=pa.schema([pa.field("s", pa.string(), False)]))
    return {"strs": write_dba(dirpath, "patch_dba_strs", strs, data_page_version="1.0"),
            "pages": write_dba(dirpath, "patch_dba_pages", pages, data_page_version="1.0", max_rows_per_page=60)}


def layout(d, page):
    """a page of PATCH_VALUES, 60 values: (where the section begins, where the suffix-length stream begins), the layout asserted"""
    at = page["data_pos"]
    assert page["encoding"] == E_DELTA_BYTE_ARRAY and page["num_values"] == 60
    pre, used, _w = D.decode(d[at:at + page["data_bytes"]], 32, 60)
    assert pre == [0, 3, 0] * 20 and d[at:at + 5] == bytes([0x80, 0x01, 4, 60, 0])
    suf, _u, _w = D.decode(d[at + used:at + page["data_bytes"]], 32, 60)
    assert suf == [5, 3, 4] * 20 and d[at + used:at + used + 5] == bytes([0x80, 0x01, 4, 60, D.zigzag(5)])
    return at, at + used


def patched(dirpath, pages_of):
    """{name: (original bytes, patched bytes, column, page, the words the message must hold)}: ONE byte changed inside a front-coded page,
    located through the page directory (encoding 7) and the streams' layout. A name that begins with tolerated_ is a file pyarrow still
    reads (recorded from pyarrow 25)."""
    d = patch_sources(dirpath)["strs"].data
    (p0,) = pages_of(d, 0)
    at, suffix_at = layout(d, p0)
    out = {}

    def put(name, pos, old, new, what):
        assert d[pos] == old, (name, pos, d[pos], old)
        out[name] = (d, d[:pos] + bytes([new]) + d[pos + 1:], 0, 0, what)
    put("tolerated_prefix_count_more", at + 3, 60, 61, "fewer or more values")
    put("prefix_count_fewer", at + 3, 60, 59, "fewer or more values")
    put("prefix_0_is_1", at + 4, 0, D.zigzag(1), "prefix longer than the value in front")      # every third prefix is 1, the value in front of the page empty
    # [min_delta: 1 byte][4 width bytes]: the first miniblock's width
    assert d[at + 5] < 0x80 and 0 < d[at + 6] <= 8
    put("prefix_width_33", at + 6, d[at + 6], 33, "malformed DELTA_BINARY_PACKED")
    put("suffix_length_negative", suffix_at + 4, D.zigzag(5), D.zigzag(-5), "BYTE_ARRAY length")
    put("suffix_lengths_sum_past_the_page", suffix_at + 4, D.zigzag(5), D.zigzag(6), "BYTE_ARRAY length")
    put("tolerated_suffix_lengths_sum_short", suffix_at + 4, D.zigzag(5), D.zigzag(4), "fewer or more values")
    return out


def two_bad_pages(dirpath, pages_of):
    """pages 1 and 3 of one column patched: page 1 must be named"""
    d = bytearray(patch_sources(dirpath)["pages"].data)
    pages = pages_of(bytes(d), 0)
    assert len(pages) == 5
    for p in (pages[1], pages[3]):
        at, _s = layout(bytes(d), p)
        d[at + 3] = 59
    return bytes(d), 0


def front_and_compressed(dirpath, pages_of_ex):
    """one file, a front-coded uncompressed column `s` and a SNAPPY-compressed integer column `z`, one corrupt page in each: page 1 of s
    (its prefix count) and page 0 of z (a byte only decompression can find wrong) -> (bytes, page of s, page of z); None without Snappy"""
    import pyarrow as pa
    import snappy_cases as S
    if not pa.Codec.is_available("snappy"):
        return None
    n = len(PATCH_VALUES) * 5
    period = (np.arange(n, dtype=np.int64) % 7) * 1000003
    t = pa.Table.from_arrays([pa.array(PATCH_VALUES * 5, pa.string()), pa.array(period)], schema=pa.schema([pa.field("s", pa.string(), False), pa.field("z", pa.int64(), False)]))
    c = write_dba(dirpath, "front_and_compressed", t, data_page_version="1.0", max_rows_per_page=60, compression={"s": "NONE", "z": "SNAPPY"})
    d = bytearray(c.data)
    at, _s = layout(bytes(d), pages_of_ex(bytes(d), 0)[1])
    d[at + 3] = 59
    z0 = pages_of_ex(bytes(d), 1)[0]
    stream = bytes(d[z0["data_pos"]:z0["data_pos"] + z0["data_bytes"]])
    pos, new = S.corrupt_in_place(stream)
    d[z0["data_pos"] + pos] = new
    return bytes(d), 1, 0


def write_all(dirpath, pages_of):
    """every generated, patched and unsupported file as paths (for the sanitizer's program) -> (paths, columns that decode, columns refused)"""
    paths, good, bad = [], 0, 0
    for case, _f in generate(dirpath).values():
        paths.append(case.path)
        good += case.table.num_columns
    extra = {name: data for name, (_o, data, _c, _p, _w) in patched(dirpath, pages_of).items()}
    extra["two_pages"] = two_bad_pages(dirpath, pages_of)[0]
    for name, data in extra.items():
        p = os.path.join(str(dirpath), "bad_" + name + ".parquet")
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p)
        bad += 1
    for path, _col, _enc, _phys in unsupported_files(dirpath).values():
        paths.append(path)
        good += 2
        bad += 1
    return paths, good, bad
