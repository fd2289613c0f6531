"""Column load path: Arrow / parquet columns -> the device encodings, whole columns at a time.

Replaces the reference's COPY FROM parquet + scan materialisation (pkg/compute/executor_scan.go:272-309
readers, :410-466 parquetColToValue + Vector.SetValue, one VALUE at a time into 24-byte Decimal /
12-byte Date / malloc'd String cells) — SURVEY.md §8f rank 3. The parquet physical encodings are
already the narrow ones the device wants (DATE = int32 days, DECIMAL = unscaled integer), so the
columns go straight from Arrow buffers to pinned staging to HBM.

Arrow's validity bitmap has the same convention as pkg/util/bitmap.go (1 bit per row, LSB first,
1 = valid), so it is passed through untouched when the column has NULLs.

table_from_csv is the reference's OTHER load path, COPY FROM ... (format csv, delimiter '|') (executor_scan.go:107-120
encoding/csv reader, :311-408 readCsvTable + fieldToValue, pkg/chunk/vector.go:195-264 SetValue): dbgen's .tbl text, or CSV
with encoding/csv's quoted fields (quoting=True), goes to the device as bytes and is parsed there (ph_table_create_csv_ex), no
Arrow in between.

table_from_parquet_device decodes the Parquet file's column chunks on the device (ph_table_create_parquet): the host reads the footer
and the page headers only, the requested columns' chunks are uploaded as they lie in the file, and kernels decode levels, dictionary
indices and values. Without flags only uncompressed pages are decoded: a compressed file is refused (PH_EUNSUPPORTED). With
flags=hip.PH_PARQUET_SNAPPY (ph_table_create_parquet_ex) SNAPPY pages — what pq.write_table and parquet-go write by default — are uploaded as
stored and decompressed on the device in front of the decoders, with flags=hip.PH_PARQUET_LZ4_RAW LZ4_RAW pages — what pq.write_table
writes for compression="LZ4" — likewise, and with flags=hip.PH_PARQUET_GZIP GZIP pages (inflated there, CRC-32 verified), and with
flags=hip.PH_PARQUET_ZSTD ZSTD pages (every frame's content size and XXH64 checksum verified there); the other
codecs stay refused and go through table_from_parquet. With
flags=hip.PH_PARQUET_DELTA, alone or or-ed with them, DELTA_BINARY_PACKED pages of integer, date and integer-stored decimal columns and
DELTA_LENGTH_BYTE_ARRAY pages of strings (parquet-mr's v2 writer) are decoded on the device too instead of refused. With
flags=hip.PH_PARQUET_DELTA_BYTE_ARRAY, alone or or-ed with any of them, DELTA_BYTE_ARRAY (front-coded) pages of strings are.
"""
import numpy as np

from . import hip


def _validity(arr, n):
    if arr.null_count == 0:
        return None
    buf = arr.buffers()[0]
    bits = np.frombuffer(buf, dtype=np.uint8)
    if arr.offset % 8 == 0:
        return bits[arr.offset // 8: arr.offset // 8 + (n + 7) // 8].copy()
    unpacked = np.unpackbits(bits, bitorder="little")[arr.offset: arr.offset + n]
    return np.packbits(unpacked, bitorder="little")


def arrow_to_spec(arr):
    """pyarrow.Array / ChunkedArray -> (ph type, numpy data, scale, validity, dictionary, aux)
    in plan_amd.hip.host_col's argument order."""
    import pyarrow as pa
    import pyarrow.compute as pc
    if isinstance(arr, pa.ChunkedArray):
        arr = arr.combine_chunks() if arr.num_chunks != 1 else arr.chunk(0)
    n = len(arr)
    t = arr.type
    val = _validity(arr, n)
    if pa.types.is_int32(t):
        return (hip.PH_I32, arr.fill_null(0).to_numpy(zero_copy_only=False).astype(np.int32, copy=False), 0, val, None, None)
    if pa.types.is_int64(t):
        return (hip.PH_I64, arr.fill_null(0).to_numpy(zero_copy_only=False).astype(np.int64, copy=False), 0, val, None, None)
    if pa.types.is_date32(t):
        days = arr.cast(pa.int32()).fill_null(0).to_numpy(zero_copy_only=False)
        return (hip.PH_DATE, days.astype(np.int32, copy=False), 0, val, None, None)
    if pa.types.is_decimal(t):
        if t.precision > 18:
            raise ValueError(f"DECIMAL({t.precision},{t.scale}) does not fit the int64 device encoding")
        # decimal128 values are 16-byte little-endian two's-complement unscaled integers
        raw = np.frombuffer(arr.buffers()[1], dtype=np.int64).reshape(-1, 2)[arr.offset: arr.offset + n]
        lo = raw[:, 0].copy()
        if not np.array_equal(raw[:, 1], lo >> 63):
            raise ValueError("decimal value outside the int64 range")
        if val is not None:
            lo[~np.unpackbits(val, bitorder="little")[:n].astype(bool)] = 0
        return (hip.PH_DEC64, lo, t.scale, val, None, None)
    if pa.types.is_string(t) or pa.types.is_large_string(t):
        enc = pc.dictionary_encode(arr)
        if isinstance(enc, pa.ChunkedArray):
            enc = enc.combine_chunks()
        d = enc.dictionary.to_pylist()
        if len(d) <= 256:   # VARCHAR with few distinct values -> uint8 codes + dictionary
            order = sorted(range(len(d)), key=lambda i: d[i])          # codes in dictionary order
            remap = np.zeros(max(len(d), 1), np.uint8)
            for new, old in enumerate(order):
                remap[old] = new
            codes = remap[enc.indices.fill_null(0).to_numpy(zero_copy_only=False)]
            return (hip.PH_CODE8, codes.astype(np.uint8), 0, val, [d[i] for i in order], None)
        s = arr.cast(pa.string())
        off = np.frombuffer(s.buffers()[1], dtype=np.int32)[s.offset: s.offset + n + 1]
        data = np.frombuffer(s.buffers()[2], dtype=np.uint8)
        base = int(off[0])
        return (hip.PH_STR, (off - base).astype(np.int32), 0, val, None, data[base: int(off[-1])].copy())
    raise ValueError(f"arrow type {t} has no device encoding")


def table_from_arrow(ctx, tbl, columns=None):
    """pyarrow.Table -> resident hip.Table (column order = `columns` or the table's)."""
    names = list(columns) if columns is not None else tbl.column_names
    specs = [arrow_to_spec(tbl.column(c)) for c in names]
    t = hip.Table(ctx, specs, tbl.num_rows)
    t.column_names = names
    return t


def table_from_parquet(ctx, path, columns=None):
    """Reads only the pruned columns (the reference's scan reads the plan's pruned column list,
    executor_scan.go:61-143) and loads them resident."""
    import pyarrow.parquet as pq
    return table_from_arrow(ctx, pq.read_table(path, columns=columns), columns)


# ---------------------------------------------------------------- through the C-ABI (Arrow C data interface)

class _ArrowSchema(__import__("ctypes").Structure):
    pass


class _ArrowArray(__import__("ctypes").Structure):
    pass


def _declare_arrow_structs():
    import ctypes
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    _ArrowSchema._fields_ = [("format", ctypes.c_char_p), ("name", ctypes.c_char_p), ("metadata", vp), ("flags", i64), ("n_children", i64),
                             ("children", vp), ("dictionary", vp), ("release", ctypes.CFUNCTYPE(None, ctypes.POINTER(_ArrowSchema))), ("private_data", vp)]
    _ArrowArray._fields_ = [("length", i64), ("null_count", i64), ("offset", i64), ("n_buffers", i64), ("n_children", i64), ("buffers", vp),
                            ("children", vp), ("dictionary", vp), ("release", ctypes.CFUNCTYPE(None, ctypes.POINTER(_ArrowArray))), ("private_data", vp)]


_declare_arrow_structs()


def table_from_arrow_c(ctx, tbl, columns=None):
    """pyarrow.Table / RecordBatch -> resident table through ph_table_create_arrow: the batch is exported with the Arrow C data
    interface (what Go's arrow/cdata or any parquet reader hands a C library) and the LIBRARY maps the buffers to the device
    encodings — the load path a host without Python uses. Returns a hip.Table (column_names, dictionaries attached)."""
    import ctypes
    import pyarrow as pa
    if isinstance(tbl, pa.Table):
        names = list(columns) if columns is not None else tbl.column_names
        tbl = tbl.select(names).combine_chunks()
        batch = tbl.to_batches()[0] if tbl.num_rows else pa.RecordBatch.from_pylist([], schema=tbl.schema)
    else:
        batch = tbl
    sch, arr = _ArrowSchema(), _ArrowArray()
    batch._export_to_c(ctypes.addressof(arr), ctypes.addressof(sch))
    t = hip.Table.__new__(hip.Table)
    t.ctx, t.h = ctx, hip.vp()
    try:
        hip.check(hip.lib().ph_table_create_arrow(ctx.h, ctypes.byref(sch), ctypes.byref(arr), None, hip.i32(0), ctypes.byref(t.h)))
    finally:
        arr.release(ctypes.byref(arr))      # the consumer releases what it was given (C data interface protocol)
        sch.release(ctypes.byref(sch))
    t.nrows, t.ncols, t.column_names = batch.num_rows, batch.num_columns, batch.schema.names
    _attach_dicts(t)
    return t


# ---------------------------------------------------------------- delimited text (dbgen .tbl / CSV with encoding/csv quoting)

def _attach_dicts(t):
    """t.dicts: per column the dictionary of a PH_CODE8 column as the library holds it (code -> string), [] for any other column"""
    import ctypes
    lib = hip.lib()
    lib.ph_table_dict_entry.restype = ctypes.c_char_p
    t.dicts = [[lib.ph_table_dict_entry(t.h, hip.i32(c), hip.i32(k)).decode("utf-8", "surrogateescape")
                for k in range(max(lib.ph_table_dict_size(t.h, hip.i32(c)), 0))] for c in range(t.ncols)]


def table_from_csv(ctx, source, columns, delimiter="|", quoting=False):
    """Delimited text -> resident table through ph_table_create_csv_ex: records and values are parsed on the device (the rules are in
    include/planhip.h). source: a path (memory-mapped) or bytes; columns: [(name, field, type, scale)] with the 0-based field of
    the record, type PH_I32 / PH_I64 / PH_DATE / PH_DEC64 or PH_STR (VARCHAR: dictionary codes when <= 256 distinct strings,
    else offsets + bytes). Returns a hip.Table with column_names and dicts filled like table_from_arrow_c.
    quoting=False (dbgen's .tbl): a '"' byte in the text raises PlanHipError with PH_EUNSUPPORTED. quoting=True (PH_CSV_QUOTES):
    a field that begins with '"' is a quoted field as Go's encoding/csv reads it, strictly: it may hold the delimiter, line breaks
    ("\\r\\n" becomes "\\n") and "" for one '"'; a bare '"' in an unquoted field and an extraneous or missing '"' raise PH_EINVAL
    naming the row."""
    import mmap
    cols = [(f, t, sc) for _n, f, t, sc in columns]
    flags = hip.PH_CSV_QUOTES if quoting else 0
    delim = ord(delimiter) if isinstance(delimiter, (str, bytes)) and len(delimiter) == 1 else -1
    t = hip.Table.__new__(hip.Table)
    t.ctx = ctx
    if isinstance(source, (bytes, bytearray, memoryview)):
        data = bytes(source)
        t.h = hip.table_create_csv(ctx, data, len(data), delim, cols, flags)
    else:
        with open(source, "rb") as f:
            size = f.seek(0, 2)
            if size == 0:
                t.h = hip.table_create_csv(ctx, b"", 0, delim, cols, flags)
            else:
                with mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as m:
                    view = np.frombuffer(m, dtype=np.uint8)
                    try:
                        t.h = hip.table_create_csv(ctx, int(view.ctypes.data), size, delim, cols, flags)
                    finally:
                        del view
    t.nrows = int(hip.lib().ph_table_rows(t.h))
    t.ncols, t.column_names = len(cols), [n for n, _f, _t, _s in columns]
    _attach_dicts(t)
    return t


# ---------------------------------------------------------------- Parquet column chunks, decoded on the device

def _with_file_bytes(source, f):
    """f(address or bytes, size) over a path (memory-mapped) or bytes"""
    import mmap
    if isinstance(source, (bytes, bytearray, memoryview)):
        data = bytes(source)
        return f(data, len(data))
    with open(source, "rb") as fh:
        size = fh.seek(0, 2)
        if size == 0:
            return f(b"", 0)
        with mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) as m:
            view = np.frombuffer(m, dtype=np.uint8)
            try:
                return f(int(view.ctypes.data), size)
            finally:
                del view


def parquet_schema(source):
    """The leaves of a Parquet file's schema through ph_parquet_schema (host only) -> {"rows", "row_groups", "columns": [{"name",
    "physical_type", "type_length", "type" (the ph type the schema maps to, 0 if none), "scale", "nullable"}]}"""
    def run(data, size):
        rows, groups, info = hip.parquet_schema(data, size)
        import ctypes
        cols = []
        for c in info:
            if isinstance(data, int):
                name = ctypes.string_at(data + c.name_pos, c.name_len)
            else:
                name = data[c.name_pos:c.name_pos + c.name_len]
            cols.append({"name": name.decode("utf-8", "surrogateescape"), "physical_type": c.physical_type, "type_length": c.type_length,
                         "type": c.type, "scale": c.scale, "nullable": bool(c.nullable)})
        return {"rows": rows, "row_groups": groups, "columns": cols}
    return _with_file_bytes(source, run)


def parquet_pages(source, column, codecs=False):
    """The page directory of one column (a name or a leaf index) through ph_parquet_pages (host only) -> [dict of ph_parquet_page's fields].
    codecs=True: through ph_parquet_pages_ex, which lists the pages of a chunk in any codec (data_bytes = the bytes as stored); every dict
    then also holds ph_parquet_page_codec's fields "codec", "compressed" and "uncompressed_bytes"."""
    if isinstance(column, str):
        column = [c["name"] for c in parquet_schema(source)["columns"]].index(column)
    fields = [f for f, _t in hip.ParquetPage._fields_]
    if not codecs:
        return _with_file_bytes(source, lambda data, size: [{f: int(getattr(p, f)) for f in fields} for p in hip.parquet_pages(data, column, size)])
    more = [f for f, _t in hip.ParquetPageCodec._fields_]

    def run(data, size):
        pages, how = hip.parquet_pages_ex(data, column, size)
        return [{**{f: int(getattr(p, f)) for f in fields}, **{f: int(getattr(c, f)) for f in more}} for p, c in zip(pages, how)]
    return _with_file_bytes(source, run)


def table_from_parquet_device(ctx, source, columns=None, types=None, flags=0):
    """Parquet file -> resident table through ph_table_create_parquet_ex: the column chunks are decoded on the device (the subset and the
    rules are in include/planhip.h). flags: 0 = compressed pages are refused with PH_EUNSUPPORTED; hip.PH_PARQUET_SNAPPY = SNAPPY pages are
    decompressed on the device; hip.PH_PARQUET_LZ4_RAW = LZ4_RAW pages are; hip.PH_PARQUET_GZIP = GZIP pages are; hip.PH_PARQUET_ZSTD = ZSTD pages are (every other codec is
    still refused); hip.PH_PARQUET_DELTA =
    DELTA_BINARY_PACKED pages of INT32 / INT64 columns and DELTA_LENGTH_BYTE_ARRAY pages of BYTE_ARRAY columns (what parquet-mr's v2 writer
    emits) are decoded instead of refused; the five may be or-ed. source: a path (memory-mapped) or bytes; columns:
    names in the order wanted (a name may repeat), None = every column; types: {name: (ph type, scale)} overrides of what the schema says
    (PH_I64 over INT32, PH_I32 over INT64, PH_DEC64 + scale over a plain integer). Returns a hip.Table with column_names and dicts filled
    like table_from_csv."""
    names = [c["name"] for c in parquet_schema(source)["columns"]]
    want = list(columns) if columns is not None else names
    types = types or {}
    cols = []
    for n in want:
        if n not in names:
            raise KeyError(f"the file has no column {n!r}")
        typ, scale = types.get(n, (0, 0))
        cols.append((names.index(n), typ, scale))
    t = hip.Table.__new__(hip.Table)
    t.ctx = ctx
    t.h = _with_file_bytes(source, lambda data, size: hip.table_create_parquet(ctx, data, size, cols, flags))
    t.nrows = int(hip.lib().ph_table_rows(t.h))
    t.ncols, t.column_names = len(cols), want
    _attach_dicts(t)
    return t


# ---------------------------------------------------------------- tables that arrive in pieces

def concat_tables(ctx, tables):
    """Resident tables -> ONE new resident table with their rows in that order, through ph_table_concat: built on the device, the
    pieces are only read and stay valid (the rules are in include/planhip.h: same column count, per column the same type and scale,
    except that dictionary-coded and plain VARCHAR columns may mix; dictionaries are merged, statistics and narrowed copies are the
    concatenation's own; declared unique keys, co-located copies and packed scan groups are not carried over). Returns a hip.Table
    with column_names taken from the first table and dicts filled like table_from_csv."""
    tables = list(tables)
    t = hip.Table.__new__(hip.Table)
    t.ctx = ctx
    t.h = hip.table_concat(ctx, tables)
    t.nrows = int(hip.lib().ph_table_rows(t.h))
    t.ncols = int(hip.lib().ph_table_ncols(t.h))
    t.column_names = list(getattr(tables[0], "column_names", None) or [])
    _attach_dicts(t)
    return t


def _load_pieces(ctx, sources, load):
    """load(source) per source, the pieces concatenated on the device and freed, also on error"""
    pieces = []
    try:
        for s in sources:
            pieces.append(load(s))
        return concat_tables(ctx, pieces)
    finally:
        for p in pieces:
            p.free()


def table_from_parquet_files(ctx, sources, columns=None, types=None, flags=0):
    """A table stored as several Parquet files (a directory of them, in the order given) -> one resident table: each file goes
    through table_from_parquet_device (same columns, types and flags for all), the pieces are concatenated on the device
    (concat_tables) and freed. The host never holds more than one file's bytes, and no row crosses PCIe twice."""
    return _load_pieces(ctx, sources, lambda s: table_from_parquet_device(ctx, s, columns, types, flags))


def table_from_csv_files(ctx, sources, columns, delimiter="|", quoting=False):
    """The same for delimited text (dbgen's .tbl chunks): each source through table_from_csv, then concat_tables."""
    return _load_pieces(ctx, sources, lambda s: table_from_csv(ctx, s, columns, delimiter, quoting))
