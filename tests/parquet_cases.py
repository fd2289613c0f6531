"""Parquet files for the load-path tests, written once with pyarrow (uncompressed) and shared by the CPU tests (the host twin,
tests/test_parquet_reference.py) and the GPU tests (tests/test_gpu_parquet_load.py). The writer knobs give the awkward pages: 13 / 26
and 37 rows a page (page boundaries inside bitmap bytes and words), data pages v1 and v2, several row groups, the mid-chunk
fall-back from RLE_DICTIONARY to PLAIN, decimals as INT32 / INT64 or FIXED_LEN_BYTE_ARRAY, required columns without a level section.

generate(dir) -> {name: Case}; refusals(dir), truncations(data) and patched(dir) build the files that must be refused."""
import decimal
import os

import numpy as np

TILE = 16384          # plan_amd/csrc/parquet_load.hip: PQ_TILE, the bytes of a BYTE_ARRAY page one step stages in LDS
ROW_PAD = 8192        # plan_amd/csrc/common.h: PH_ROW_PAD
N = 20000


class Case:
    def __init__(self, name, path, table):
        self.name, self.path, self.table = name, path, table

    @property
    def data(self):
        with open(self.path, "rb") as f:
            return f.read()


def _mask(rng, n, frac=0.3):
    return rng.random(n) < frac


def matrix_table(n, seed=7):
    """int32, int64, date32, decimal(9,0), decimal(15,2), a string column with 300 distinct values and one with 40; each with
    about 30 % NULLs (suffix _n) and required (suffix _r)"""
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    i32 = rng.integers(-2**31, 2**31, n).astype(np.int32)
    i64 = rng.integers(-2**62, 2**62, n)
    date = rng.integers(-3000, 20000, n).astype(np.int32)
    d9 = [decimal.Decimal(int(v)) for v in rng.integers(-10**9 + 1, 10**9, n)]
    d15 = [decimal.Decimal(int(v)).scaleb(-2) for v in rng.integers(-10**15 + 1, 10**15, n)]
    s300 = ["value %03d" % v for v in rng.integers(0, 300, n)]
    s40 = ["k%d" % v for v in rng.integers(0, 40, n)]
    base = [("i32", pa.array(i32), pa.int32()), ("i64", pa.array(i64), pa.int64()), ("date", pa.array(date, pa.int32()).cast(pa.date32()), pa.date32()),
            ("d9", pa.array(d9, pa.decimal128(9, 0)), pa.decimal128(9, 0)), ("d15", pa.array(d15, pa.decimal128(15, 2)), pa.decimal128(15, 2)),
            ("s300", pa.array(s300, pa.string()), pa.string()), ("s40", pa.array(s40, pa.string()), pa.string())]
    arrays, fields = [], []
    for name, arr, typ in base:
        m = _mask(rng, n)
        arrays.append(pa.array(arr.to_pylist(), typ, mask=m) if n else arr)
        fields.append(pa.field(name + "_n", typ, nullable=True))
        arrays.append(arr)
        fields.append(pa.field(name + "_r", typ, nullable=False))
    return pa.Table.from_arrays(arrays, schema=pa.schema(fields))


def null_patterns_table(n=N):
    import pyarrow as pa
    v = np.arange(n, dtype=np.int64) * 3 - 5
    s = ["s%d" % (i % 50) for i in range(n)]
    all_null = np.ones(n, bool)
    last = np.zeros(n, bool)
    last[n - 20:] = True
    alt = np.zeros(n, bool)
    alt[n // 2:] = np.arange(n - n // 2) % 2 == 1          # a long all-valid stretch, then alternating: RLE and bit-packed level runs
    cols = {"all_null": pa.array(v, mask=all_null), "none_null": pa.array(v), "last_page": pa.array(v, mask=last), "rle_then_alt": pa.array(v, mask=alt),
            "s_all_null": pa.array(s, pa.string(), mask=all_null), "s_none_null": pa.array(s, pa.string()), "s_alt": pa.array(s, pa.string(), mask=alt)}
    return pa.table(cols)


def dict_width_table(n, distinct, seed=11):
    """int64 columns over dictionaries of the given sizes (index widths 1, 2, 3, 5, 9, 17 bits), and one with long constant stretches
    between random ones (both run kinds)"""
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    cols = {}
    for d in distinct:
        pick = np.concatenate([np.arange(d), rng.integers(0, d, n - d)]) if d <= n else np.arange(n)
        rng.shuffle(pick)
        cols["d%d" % d] = pa.array(pick.astype(np.int64) * 1000003 - 17)
    runs = rng.integers(0, 1000, n).astype(np.int64)
    for a in range(0, n, 4000):
        runs[a:a + 2500] = a
    cols["runs"] = pa.array(runs)
    cols["runs_n"] = pa.array(runs, mask=_mask(rng, n))
    return pa.table(cols)


def varchar_table(kind):
    import pyarrow as pa
    rng = np.random.default_rng(5)
    if kind in ("256_nulls", "256_empty_nulls", "257"):
        k = 257 if kind == "257" else 256
        d = ["str %05d" % (i * 7919 % 100000) for i in range(k)]
        if kind == "256_empty_nulls":
            d.append("")
        pick = np.concatenate([np.arange(len(d)), rng.integers(0, len(d), 1500 - len(d))])
        rng.shuffle(pick)
        vals = [d[j] for j in pick]
        mask = _mask(rng, len(vals), 0.2) if kind != "257" else None
        if mask is not None:
            for j in range(len(d)):                      # every distinct value keeps one valid row
                mask[int(np.nonzero(pick == j)[0][0])] = False
        return pa.table({"s": pa.array(vals, pa.string(), mask=mask), "i": pa.array(np.arange(len(vals), dtype=np.int32))})
    if kind == "nul_byte":
        return pa.table({"s": pa.array(["a\0b", "c", None, "", "c"], pa.string()), "t": pa.array(["x", "y", "x", None, ""], pa.string())})
    if kind == "empty":
        return pa.table({"s": pa.array(["", "", None, "", "x", ""] * 50, pa.string()), "e": pa.array([""] * 300, pa.string())})
    if kind == "long":
        big = "L" * (100 * 1024)
        return pa.table({"s": pa.array(["a", big, "b", None, big + "x", ""] + ["t%d" % i for i in range(300)], pa.string())})
    if kind == "straddle":
        vals = []
        for d in (-2, -1, 0, 1, 2):
            vals += ["h", "y" * (TILE + d), "t" * 3, "z" * (TILE - 4 + d), None, "w" * (TILE - 8 + d)]
        return pa.table({"s": pa.array(vals, pa.string()), "r": pa.array([v or "" for v in vals], pa.string())})
    raise KeyError(kind)


def _write(dirpath, name, table, **kw):
    import pyarrow.parquet as pq
    path = os.path.join(str(dirpath), name + ".parquet")
    kw = {k: v for k, v in kw.items() if v is not None}
    kw.setdefault("compression", "NONE")
    pq.write_table(table, path, **kw)
    return Case(name, path, table)


_CACHE = {}


def generate(dirpath):
    """every well-formed case: {name: Case}. Written once per directory."""
    key = str(dirpath)
    if key in _CACHE:
        return _CACHE[key]
    import pyarrow as pa
    out = {}

    def add(name, table, **kw):
        out[name] = _write(dirpath, name, table, **kw)
    m = matrix_table(N)
    add("matrix_v1", m)
    add("matrix_v2", m, data_page_version="2.0")
    add("matrix_pages13", m, write_batch_size=13, data_page_size=64)
    add("matrix_pages37_v2", m, max_rows_per_page=37, data_page_version="2.0")
    add("matrix_pages37_v1_plain", m, max_rows_per_page=37, data_page_version="1.0", use_dictionary=False)
    add("matrix_plain_v2", m, use_dictionary=False, data_page_version="2.0")
    add("matrix_decint_3groups", m, store_decimal_as_integer=True, row_group_size=7000)
    add("matrix_3groups_pages37", m, row_group_size=7000, max_rows_per_page=37)
    add("matrix_fallback", m, dictionary_pagesize_limit=2048)
    add("matrix_fallback_v2_3groups", m, dictionary_pagesize_limit=2048, data_page_version="2.0", row_group_size=7000)
    add("matrix_dict_some", m, use_dictionary=["i64_n", "s300_r", "d15_n"])
    for n in (0, 1, 7, 8, 9, 63, 64, 65, ROW_PAD - 1, ROW_PAD + 1):
        add("rows_%d" % n, matrix_table(n, seed=100 + n), max_rows_per_page=37 if n > 64 else None)
    nulls = null_patterns_table()
    add("nulls_v1", nulls, max_rows_per_page=5000)
    add("nulls_v2_plain", nulls, data_page_version="2.0", use_dictionary=False, max_rows_per_page=5000)
    add("dict_widths", dict_width_table(N, (1, 2, 3, 5, 17, 257)))
    add("dict_widths_pages37_v2", dict_width_table(N, (1, 2, 3, 5, 17, 257)), max_rows_per_page=37, data_page_version="2.0")
    add("dict_width17", dict_width_table(100000, (70000,)), dictionary_pagesize_limit=4 << 20)
    for kind in ("256_nulls", "256_empty_nulls", "257", "nul_byte", "empty", "long", "straddle"):
        add("varchar_" + kind, varchar_table(kind))
        add("varchar_" + kind + "_plain", varchar_table(kind), use_dictionary=False, data_page_version="2.0")
    # an unannotated BYTE_ARRAY (binary) column reads as VARCHAR too
    add("binary", pa.table({"b": pa.array([b"x", b"\xff\xfe", None, b""] * 10, pa.binary())}))
    _CACHE[key] = out
    return out


def expected_column(col):
    """a pyarrow column as the host twin returns one: (values int64 or None, valid bool[n], [bytes] or None)"""
    import pyarrow as pa
    if isinstance(col, pa.ChunkedArray):
        col = col.combine_chunks()
    n = len(col)
    valid = ~np.asarray(col.is_null().to_numpy(zero_copy_only=False), dtype=bool) if n else np.zeros(0, bool)
    t = col.type
    if pa.types.is_string(t) or pa.types.is_binary(t):
        return None, valid, [b"" if v is None else (v if isinstance(v, bytes) else v.encode()) for v in col.to_pylist()]
    if pa.types.is_decimal(t):
        vals = np.array([0 if v is None else int(v.scaleb(t.scale)) for v in col.to_pylist()], dtype=np.int64)
    elif pa.types.is_date32(t):
        vals = col.cast(pa.int32()).fill_null(0).to_numpy(zero_copy_only=False).astype(np.int64)
    else:
        vals = col.fill_null(0).to_numpy(zero_copy_only=False).astype(np.int64)
    return vals.reshape(n), valid, None


# ---------------------------------------------------------------- files that must be refused

def refusals(dirpath):
    """{name: (path, column name, expected code name)}: outside the subset"""
    import pyarrow as pa
    n = 100
    t = pa.table({"i": pa.array(np.arange(n, dtype=np.int32)), "f": pa.array(np.arange(n, dtype=np.float64)),
                  "l": pa.array([[1, 2]] * n, pa.list_(pa.int32())), "s": pa.array(["a"] * n)})
    out = {}
    out["snappy"] = (_write(dirpath, "refuse_snappy", t, compression="SNAPPY").path, "i", "SNAPPY")
    out["zstd"] = (_write(dirpath, "refuse_zstd", t, compression="ZSTD").path, "s", "ZSTD")
    plain = _write(dirpath, "refuse_types", t).path
    out["double"] = (plain, "f", "DOUBLE")
    out["list"] = (plain, "element", "nested or repeated")
    delta = _write(dirpath, "refuse_delta", pa.table({"i": t["i"], "ok": t["i"]}), use_dictionary=False, column_encoding={"i": "DELTA_BINARY_PACKED", "ok": "PLAIN"}).path
    out["delta"] = (delta, "i", "DELTA_BINARY_PACKED")
    return out


def truncations(data):
    """{name: bytes}: what the host checks refuse with PH_EINVAL"""
    flen = int.from_bytes(data[-8:-4], "little")
    return {
        "cut_1": data[:-1], "cut_8": data[:-8], "cut_9": data[:-9], "cut_mid_footer": data[:len(data) - 8 - flen // 2],
        "short_11": data[:11], "empty": b"",
        "head_magic": b"PAR2" + data[4:], "tail_magic": data[:-4] + b"PARX",
        "footer_len_large": data[:-8] + (len(data)).to_bytes(4, "little") + data[-4:],
        "footer_garbage": data[:len(data) - 8 - flen] + bytes([0xff] * flen) + data[-8:],
    }


def patch_sources(dirpath):
    """the small files the one-byte patches start from"""
    import pyarrow as pa
    n = 100
    v = np.arange(n, dtype=np.int64)
    mask = np.zeros(n, bool)
    mask[50:] = np.arange(50) % 3 == 0
    levels = _write(dirpath, "patch_levels", pa.table({"a": pa.array(v, mask=mask)}), use_dictionary=False, max_rows_per_page=37, data_page_version="1.0")
    strs = pa.Table.from_arrays([pa.array(["alpha", "be", "gamma"] * 20, pa.string())], schema=pa.schema([pa.field("s", pa.string(), nullable=False)]))
    plain = _write(dirpath, "patch_bytes", strs, use_dictionary=False, data_page_version="1.0")
    two = pa.Table.from_arrays([pa.array(["A"] * 50 + ["B"] * 50, pa.string()), pa.array([5] * 50 + [9] * 50, pa.int64())],
                               schema=pa.schema([pa.field("s", pa.string(), nullable=False), pa.field("v", pa.int64(), nullable=False)]))
    dic = _write(dirpath, "patch_dict", two, data_page_version="1.0")
    return {"levels": levels, "bytes": plain, "dict": dic}


def patched(dirpath, pages_of):
    """{name: (original bytes, patched bytes, column)}: ONE byte changed, located through the page directory (pages_of(data, column) ->
    ph_parquet_pages entries) and the format's layout. What only decoding can see; each must give PH_EINVAL."""
    src = patch_sources(dirpath)
    out = {}

    def put(name, data, at, old, new, column=0):
        assert data[at] == old, (name, at, data[at], old)
        out[name] = (data, data[:at] + bytes([new]) + data[at + 1:], column)
    # a nullable column, v1, 37 rows a page, no NULL in the first page: [4-byte length = 2][RLE header 37 << 1][value 1]
    d = src["levels"].data
    p0 = [p for p in pages_of(d, 0) if p["kind"] == 0][0]
    assert int.from_bytes(d[p0["data_pos"]:p0["data_pos"] + 4], "little") == 2
    hdr = p0["data_pos"] + 4
    put("level_run_past_section", d, hdr, 37 << 1, 0x7f)          # a bit-packed run of 63 groups in a section of 2 bytes
    put("levels_fewer", d, hdr, 37 << 1, 36 << 1)                 # 36 levels for 37 values
    put("tolerated_levels_more", d, hdr, 37 << 1, 38 << 1)        # an RLE run of 38 in a page of 37 (pyarrow reads 37 of them and goes on)
    # a required PLAIN BYTE_ARRAY column: the first length's top byte
    d = src["bytes"].data
    p0 = [p for p in pages_of(d, 0) if p["kind"] == 0][0]
    assert int.from_bytes(d[p0["data_pos"]:p0["data_pos"] + 4], "little") == 5
    put("byte_array_length_past_page", d, p0["data_pos"] + 3, 0, 0x7f)
    put("byte_array_count", d, p0["data_pos"], 5, 4)              # the chain no longer ends at the page's end
    # required columns over two-entry dictionaries: [bit width 1][RLE header 50 << 1][value 0][RLE header 50 << 1][value 1]
    d = src["dict"].data
    for column, name in ((0, "dict_index_str"), (1, "dict_index_int")):
        p0 = [p for p in pages_of(d, column) if p["kind"] == 0][0]
        at = p0["data_pos"]
        assert d[at] == 1 and d[at + 1] == 50 << 1
        put(name, d, at + 2, 0, 0x7f, column)
    p0 = [p for p in pages_of(d, 1) if p["kind"] == 0][0]
    put("dict_bit_width", d, p0["data_pos"], 1, 33, 1)
    put("dict_run_empty", d, p0["data_pos"] + 1, 50 << 1, 0, 1)   # a run of no values
    return out
