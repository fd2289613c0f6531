"""ctypes binding of libplanhip.so (include/planhip.h).

There is no CPU fallback: if the library is missing or a call fails, this raises."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

PH_JOIN_KEY_RANGE, PH_JOIN_FK_PROBES, PH_JOIN_KEYS_SORTED_UNIQUE, PH_JOIN_EXISTS_ONLY = 1, 2, 4, 8
PH_OK, PH_EINVAL, PH_EHIP, PH_EUNSUPPORTED, PH_EOVERFLOW, PH_ECAPACITY, PH_ECONSTRAINT = 0, -1, -2, -3, -4, -5, -6
PH_I32, PH_I64, PH_DATE, PH_DEC64, PH_CODE8, PH_F32, PH_F64, PH_STR = range(1, 9)
PH_EQ, PH_NE, PH_LT, PH_LE, PH_GT, PH_GE, PH_LIKE, PH_NOTLIKE = range(1, 9)
PH_X_COL, PH_X_CONST, PH_X_ADD, PH_X_SUB, PH_X_MUL = range(1, 6)
PH_A_SUM, PH_A_AVG, PH_A_COUNT, PH_A_MIN, PH_A_MAX, PH_A_COUNT_STAR, PH_A_COUNT_DISTINCT = range(1, 8)
PH_COMM_ID_BYTES = 128
PH_CSV_QUOTES = 1
PH_PARQUET_SNAPPY = 1
PH_PARQUET_DELTA = 4
PH_PARQUET_LZ4_RAW = 16
PH_PARQUET_GZIP = 64
PH_PARQUET_ZSTD = 256
PH_PARQUET_DELTA_BYTE_ARRAY = 1024
PH_RED_SUM, PH_RED_MAX, PH_RED_MIN = 1, 2, 3

i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p

NP_TYPES = {PH_I32: np.int32, PH_I64: np.int64, PH_DATE: np.int32, PH_DEC64: np.int64,
            PH_CODE8: np.uint8, PH_F32: np.float32, PH_F64: np.float64}


class PlanHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"planhip error {code}: {msg}")
        self.code = code


class Col(ctypes.Structure):
    _fields_ = [("type", i32), ("scale", i32), ("data", vp), ("validity", vp), ("aux", vp),
                ("aux_bytes", i64)]


class CsvCol(ctypes.Structure):
    """ph_csv_col: one column of ph_table_create_csv"""
    _fields_ = [("field", i32), ("type", i32), ("scale", i32)]


class ParquetCol(ctypes.Structure):
    """ph_parquet_col: one column of ph_table_create_parquet"""
    _fields_ = [("column", i32), ("type", i32), ("scale", i32)]


class ParquetColInfo(ctypes.Structure):
    """ph_parquet_colinfo: one leaf of the file's schema"""
    _fields_ = [("name_pos", i64), ("name_len", i32), ("physical_type", i32), ("type_length", i32), ("type", i32), ("scale", i32),
                ("nullable", i32)]


class ParquetPage(ctypes.Structure):
    """ph_parquet_page: one entry of a column's page directory"""
    _fields_ = [("row_group", i32), ("kind", i32), ("encoding", i32), ("num_values", i32), ("first_row", i64), ("header_pos", i64),
                ("data_pos", i64), ("data_bytes", i64), ("rep_levels_bytes", i64), ("def_levels_bytes", i64)]


class ParquetPageCodec(ctypes.Structure):
    """ph_parquet_page_codec: how one page of ph_parquet_pages_ex's directory is stored"""
    _fields_ = [("codec", i32), ("compressed", i32), ("uncompressed_bytes", i64)]


class DeltaStream(ctypes.Structure):
    """ph_delta_stream: one raw DELTA_BINARY_PACKED stream of ph_delta_decode / ph_delta_decode_host"""
    _fields_ = [("src_pos", i64), ("src_bytes", i64), ("bits", i32), ("exact", i32), ("expected", i64), ("dst_pos", i64), ("dst_cap", i64),
                ("count", i64), ("consumed", i64), ("status", i32), ("sub", i32)]


class DbaStream(ctypes.Structure):
    """ph_dba_stream: one raw DELTA_BYTE_ARRAY values section of ph_delta_byte_array_decode / ph_delta_byte_array_decode_host"""
    _fields_ = [("src_pos", i64), ("src_bytes", i64), ("expected", i64), ("len_pos", i64), ("len_cap", i64), ("byte_pos", i64), ("byte_cap", i64),
                ("count", i64), ("total_bytes", i64), ("consumed", i64), ("status", i32), ("sub", i32)]


PH_PARQUET_PAGE_DATA, PH_PARQUET_PAGE_DICTIONARY, PH_PARQUET_PAGE_DATA_V2 = 0, 2, 3


class Const(ctypes.Structure):
    _fields_ = [("type", i32), ("scale", i32), ("i", i64), ("f", ctypes.c_double),
                ("s", ctypes.c_char_p)]


class Pred(ctypes.Structure):
    _fields_ = [("col", i32), ("op", i32), ("k", Const)]


class Rpn(ctypes.Structure):
    _fields_ = [("op", i32), ("col", i32), ("ival", i64), ("scale", i32)]


class AggExpr(ctypes.Structure):
    _fields_ = [("kind", i32), ("nprog", i32), ("prog", Rpn * 12)]


class AggSpec(ctypes.Structure):
    _fields_ = [("kind", i32), ("arg", i32)]


class AggResult(ctypes.Structure):
    _fields_ = [("ngroups", i64), ("first_row", ctypes.POINTER(i64)), ("keys", ctypes.POINTER(i64)),
                ("sum_lo", ctypes.POINTER(ctypes.c_uint64)), ("sum_hi", ctypes.POINTER(i64)),
                ("count", ctypes.POINTER(ctypes.c_uint64)), ("scale", ctypes.POINTER(i32)),
                ("nkeys", i32), ("naggs", i32), ("key_null", ctypes.POINTER(ctypes.c_uint8))]


class RowsResult(ctypes.Structure):
    _fields_ = [("nrows", i64), ("ncols", i32), ("type", ctypes.POINTER(i32)), ("scale", ctypes.POINTER(i32)),
                ("values", ctypes.POINTER(ctypes.POINTER(i64))), ("offsets", ctypes.POINTER(ctypes.POINTER(i32))),
                ("bytes", ctypes.POINTER(ctypes.c_void_p))]


def _preload_torch_hip_runtime():
    """One HIP runtime per process. PyTorch-ROCm bundles its own libamdhip64.so / libhiprtc.so /
    librccl.so (SONAMEs libamdhip64.so.7, libhiprtc.so.7, librccl.so.1 — the ones libplanhip.so
    asks for), and its libraries ask for them by the unversioned names: if ROCm's copies were loaded
    first (through libplanhip.so's NEEDED entries) a later `import torch` would bring in a second
    runtime, whose device discovery then fails ("No HIP GPUs are available").
    So when torch is installed it is imported FIRST, and libplanhip.so then binds to the copies torch
    has loaded, by SONAME. Loading only torch's .so files here and importing torch later was tried:
    the process then aborts at exit ("double free or corruption") because the libraries' static
    destructors run in an order torch never sees (measured on the GPU box, round 2)."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    try:
        import torch  # noqa: F401  (initialises torch's bundled ROCm libraries in torch's own order)
    except Exception:  # noqa: BLE001 - a broken torch install: fall back to its bare libraries
        pass
    for name in ("libamdhip64.so", "libhiprtc.so", "librccl.so"):
        cand = os.path.join(os.path.dirname(spec.origin), "lib", name)
        if os.path.exists(cand):
            try:
                ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
            except OSError:
                pass


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "libplanhip.so")
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} is missing — the HIP extension is required (no CPU fallback). "
                "Build it with `python -c 'import __graft_entry__ as g; g.build()'`.")
        _preload_torch_hip_runtime()
        L = ctypes.CDLL(path)
        for name, rt in (("ph_last_error", ctypes.c_char_p), ("ph_version", ctypes.c_char_p),
                         ("ph_scan_plan_kind", ctypes.c_char_p), ("ph_join_kind", ctypes.c_char_p), ("ph_agg_sink_kind", ctypes.c_char_p), ("ph_table_rows", i64),
                         ("ph_hash_bytes", ctypes.c_uint64), ("ph_join_count", i64),
                         ("ph_comm_nranks", i32), ("ph_comm_rank", i32)):
            getattr(L, name).restype = rt  # a missing symbol raises: the ABI must be complete
        _LIB = L
    return _LIB


def last_error():
    return lib().ph_last_error().decode()


def check(rc):
    if rc != PH_OK:
        raise PlanHipError(rc, lib().ph_last_error().decode())


def const(typ, i=0, f=0.0, s=None, scale=0):
    k = Const()
    k.type, k.scale, k.i, k.f = typ, scale, int(i), float(f)
    k.s = None if s is None else s if isinstance(s, bytes) else s.encode()   # bytes: a pattern with bytes >= 0x80 (no NUL: a C string)
    return k


def pred(col, op, k):
    p = Pred()
    p.col, p.op, p.k = col, op, k
    return p


def aggexpr(kind, prog=()):
    a = AggExpr()
    a.kind = kind
    a.nprog = len(prog)
    for j, (op, col, ival, scale) in enumerate(prog):
        a.prog[j] = Rpn(op, col, ival, scale)
    return a


def X_COL(c):
    return (PH_X_COL, c, 0, 0)


def X_CONST(v, scale=0):
    return (PH_X_CONST, -1, v, scale)


X_ADD = (PH_X_ADD, -1, 0, 0)
X_SUB = (PH_X_SUB, -1, 0, 0)
X_MUL = (PH_X_MUL, -1, 0, 0)


class Ctx:
    """One HIP device + one stream (ph_ctx)."""

    def __init__(self, device=0, stream=None):
        self.h = vp()
        check(lib().ph_ctx_create(i32(device), ctypes.byref(self.h)))
        self.device = device
        if stream is not None:
            check(lib().ph_ctx_set_stream(self.h, vp(stream)))

    def sync(self):
        check(lib().ph_ctx_sync(self.h))

    def set_deferred_errors(self, on=True):
        """flags that would cost a host round trip each (expression overflow) are reported by the next
        call that reads anything back (ph_ctx_set_deferred_errors)"""
        check(lib().ph_ctx_set_deferred_errors(self.h, i32(2 if on == 2 else 1 if on else 0)))   # 2: held until check_deferred()

    def check_deferred(self):
        check(lib().ph_ctx_check_deferred(self.h))

    def set_async_counts(self, on=True):
        """row counts of filter_select / probe_inner* are filled in by wait_counts() (ph_ctx_set_async_counts)"""
        check(lib().ph_ctx_set_async_counts(self.h, i32(1 if on else 0)))

    def wait_counts(self):
        check(lib().ph_ctx_wait_counts(self.h))

    def scan_forms(self):
        """ph_ctx_scan_forms: how often this context's block-count scan took each form so far, as a dict
        (loop, small, lookback, three_pass); a test takes the difference around a call"""
        out = (i64 * 4)()
        check(lib().ph_ctx_scan_forms(self.h, out))
        return dict(zip(("loop", "small", "lookback", "three_pass"), (int(x) for x in out)))

    def close(self):
        if self.h:
            lib().ph_ctx_destroy(self.h)
            self.h = None

    # -- plain device buffers
    def alloc(self, nbytes):
        p = vp()
        check(lib().ph_dev_alloc(self.h, i64(nbytes), ctypes.byref(p)))
        return p

    def free(self, p):
        check(lib().ph_dev_free(self.h, p))

    def free_many(self, ptrs):
        ptrs = [p for p in ptrs if p]
        if ptrs:
            arr = (vp * len(ptrs))(*[vp(p.value) if isinstance(p, vp) else vp(p) for p in ptrs])
            check(lib().ph_dev_free_many(self.h, arr, i64(len(ptrs))))

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        check(lib().ph_dev_upload(self.h, p, vp(arr.ctypes.data), i64(arr.nbytes)))
        return p

    def download(self, p, dtype, n):
        out = np.empty(n, dtype=dtype)
        check(lib().ph_dev_download(self.h, vp(out.ctypes.data), p, i64(out.nbytes)))
        return out


def host_col(typ, arr, scale=0, validity=None, dictionary=None, aux=None):
    """ph_col over host numpy memory (for ph_table_create). Returns (Col, keepalive)."""
    c = Col()
    c.type, c.scale = typ, scale
    arr = np.ascontiguousarray(arr)
    c.data = arr.ctypes.data
    keep = [arr]
    if validity is not None:
        validity = np.ascontiguousarray(validity, dtype=np.uint8)
        c.validity = validity.ctypes.data
        keep.append(validity)
    if dictionary is not None:
        blob = b"".join(s.encode() + b"\0" for s in dictionary)
        buf = ctypes.create_string_buffer(blob, len(blob))
        c.aux = ctypes.cast(buf, vp)
        c.aux_bytes = len(blob)
        keep.append(buf)
    if aux is not None:
        aux = np.ascontiguousarray(aux)
        c.aux = aux.ctypes.data
        c.aux_bytes = aux.nbytes
        keep.append(aux)
    return c, keep


class Table:
    """Device-resident table (ph_table). cols: list of (type, array, scale, dictionary|None)."""

    def __init__(self, ctx, cols, nrows):
        self.ctx = ctx
        arr = (Col * len(cols))()
        keep = []
        for j, spec in enumerate(cols):
            c, k = host_col(*spec) if not isinstance(spec, dict) else host_col(**spec)
            arr[j] = c
            keep.append(k)
        self.h = vp()
        check(lib().ph_table_create(ctx.h, i32(len(cols)), arr, i64(nrows), ctypes.byref(self.h)))
        self.nrows = nrows
        self.ncols = len(cols)

    def col(self, c):
        out = Col()
        check(lib().ph_table_col(self.h, i32(c), ctypes.byref(out)))
        return out

    def col_run_len(self, c):
        """ph_table_col_run_len: > 0 = the column is stored in runs of that one length over consecutive values"""
        lib().ph_table_col_run_len.restype = ctypes.c_int32
        return int(lib().ph_table_col_run_len(self.h, i32(c)))

    def col_range(self, c):
        mn, mx = i64(), i64()
        check(lib().ph_table_col_range(self.h, i32(c), ctypes.byref(mn), ctypes.byref(mx)))
        return mn.value, mx.value

    def col_narrow(self, c):
        """ph_table_col_narrow: (width, base) of the column's narrowed copy (code = value - base in width bytes), None when it has none"""
        w, base = i32(), i64()
        rc = lib().ph_table_col_narrow(self.h, i32(c), ctypes.byref(w), ctypes.byref(base))
        if rc < 0:
            check(rc)
        return (w.value, base.value) if rc == 1 else None

    def narrow_bytes(self):
        """ph_table_narrow_bytes: device bytes held by the table's narrowed column copies"""
        lib().ph_table_narrow_bytes.restype = i64
        return int(lib().ph_table_narrow_bytes(self.h))

    def colocate(self, cols):
        """ph_table_colocate: a co-located (row-major) copy of these columns beside the column arrays; ph_gather_multi over
        views of them then reads one sector per row id"""
        check(lib().ph_table_colocate(self.h, i32(len(cols)), (i32 * len(cols))(*cols)))

    def colocated(self, cols):
        return bool(lib().ph_table_colocated(self.h, i32(len(cols)), (i32 * len(cols))(*cols)))

    def set_replicated(self, on=True):
        """multi-rank plans: this rank holds ALL rows of the table (default: a shard)"""
        check(lib().ph_table_set_replicated(self.h, i32(1 if on else 0)))

    def set_colocate_budget(self, nbytes):
        """bytes of HBM the library may spend on its own on co-located copies of this table (0 = never; default 4 GiB)"""
        check(lib().ph_table_set_colocate_budget(self.h, i64(nbytes)))

    def colocate_bytes(self):
        lib().ph_table_colocate_bytes.restype = i64
        return int(lib().ph_table_colocate_bytes(self.h))

    def pack_scan_group(self, cols):
        """ph_table_pack_scan_group: one bit-packed 64-bit word a row for the seven columns a lowcard_chain plan reads (the
        predicate column, q, e, d, t, the two group columns); lean plans over them then load 8 bytes a row ("packed64")"""
        check(lib().ph_table_pack_scan_group(self.h, i32(len(cols)), (i32 * len(cols))(*cols)))

    def pack_scan_group_ex(self, cols, form):
        """ph_table_pack_scan_group_ex: the same with the form named: 0 the 64-bit word, 1 the 7-byte split blocks (lineitem's
        layout only; lean plans over them then load 7 bytes a row, "split56")"""
        check(lib().ph_table_pack_scan_group_ex(self.h, i32(len(cols)), (i32 * len(cols))(*cols), i32(form)))

    def scan_group_bytes(self):
        """ph_table_scan_group_bytes: device bytes held by the table's packed scan groups"""
        lib().ph_table_scan_group_bytes.restype = i64
        return int(lib().ph_table_scan_group_bytes(self.h))

    def free(self):
        if self.h:
            lib().ph_table_free(self.h)
            self.h = None


def csv_parse_field(typ, scale, field):
    """ph_csv_parse_field (host only, no device): one field of delimited text as the device parser reads it ->
    (return code, value, is_null); field: bytes"""
    field = bytes(field)
    value, null = i64(0), i32(0)
    rc = lib().ph_csv_parse_field(i32(typ), i32(scale), ctypes.c_char_p(field), i64(len(field)), ctypes.byref(value), ctypes.byref(null))
    return int(rc), int(value.value), bool(null.value)


def csv_split_record(text, pos=0, delimiter="|", flags=0, cap=64):
    """ph_csv_split_record (host only, no device): the record that starts at text[pos] (empty lines skipped first), walked by the
    function the field kernel runs -> (return code, [(begin, end, field flags)], fields seen, next); field flags: bit 0 quoted,
    bit 1 the content holds "" or "\\r\\n" that the value drops. text: bytes; flags: 0 or PH_CSV_QUOTES"""
    text = bytes(text)
    begin, end, ff = (i64 * cap)(), (i64 * cap)(), (i32 * cap)()
    nf, nxt = i32(0), i64(0)
    delim = ord(delimiter) if isinstance(delimiter, (str, bytes)) and len(delimiter) == 1 else -1
    rc = lib().ph_csv_split_record(ctypes.c_char_p(text), i64(len(text)), i32(delim), ctypes.c_uint32(flags), i64(pos), begin, end, ff,
                                   i32(cap), ctypes.byref(nf), ctypes.byref(nxt))
    n = min(int(nf.value), cap)
    return int(rc), [(int(begin[i]), int(end[i]), int(ff[i])) for i in range(n)], int(nf.value), int(nxt.value)


def _file_arg(data):
    """the file's bytes for a ph_parquet_* call: an address (int) or bytes -> (argument, keep-alive)"""
    if isinstance(data, int):
        return vp(data), None
    data = bytes(data)
    return ctypes.c_char_p(data), data


def parquet_schema(data, nbytes=None):
    """ph_parquet_schema (host only, no device) -> (rows, row groups, [ParquetColInfo]); data: bytes, or an address with nbytes"""
    src, keep = _file_arg(data)
    nbytes = len(keep) if nbytes is None else nbytes
    nrows, ngroups, ncols = i64(0), i32(0), i32(0)
    check(lib().ph_parquet_schema(src, i64(nbytes), ctypes.byref(nrows), ctypes.byref(ngroups), None, i32(0), ctypes.byref(ncols)))
    info = (ParquetColInfo * max(ncols.value, 1))()
    check(lib().ph_parquet_schema(src, i64(nbytes), ctypes.byref(nrows), ctypes.byref(ngroups), info, i32(ncols.value), ctypes.byref(ncols)))
    return int(nrows.value), int(ngroups.value), [info[i] for i in range(ncols.value)]


def parquet_pages(data, column, nbytes=None):
    """ph_parquet_pages (host only, no device): the page directory of one leaf column -> [ParquetPage]"""
    src, keep = _file_arg(data)
    nbytes = len(keep) if nbytes is None else nbytes
    n = i32(0)
    check(lib().ph_parquet_pages(src, i64(nbytes), i32(column), None, i32(0), ctypes.byref(n)))
    pages = (ParquetPage * max(n.value, 1))()
    check(lib().ph_parquet_pages(src, i64(nbytes), i32(column), pages, i32(n.value), ctypes.byref(n)))
    return [pages[i] for i in range(n.value)]


def parquet_pages_ex(data, column, nbytes=None):
    """ph_parquet_pages_ex (host only, no device): the page directory of one leaf column, whatever the chunks' codec ->
    ([ParquetPage], [ParquetPageCodec]); data_bytes are the bytes as stored"""
    src, keep = _file_arg(data)
    nbytes = len(keep) if nbytes is None else nbytes
    n = i32(0)
    check(lib().ph_parquet_pages_ex(src, i64(nbytes), i32(column), None, None, i32(0), ctypes.byref(n)))
    pages, codecs = (ParquetPage * max(n.value, 1))(), (ParquetPageCodec * max(n.value, 1))()
    check(lib().ph_parquet_pages_ex(src, i64(nbytes), i32(column), pages, codecs, i32(n.value), ctypes.byref(n)))
    return [pages[i] for i in range(n.value)], [codecs[i] for i in range(n.value)]


def snappy_decompress_host(data, expected=None):
    """ph_snappy_decompress_host (host only, no device): one raw Snappy stream, decoded by the host twin of the device decoder -> bytes.
    expected: the length the stream must produce; None: what its preamble says. The C entry point has no such parameter (it reports the
    preamble's length), so a disagreement is found HERE, by comparing the two, and raised as PH_EINVAL — the code the device call gives
    such a stream, where the decoder's own check (snappy_decode.h, read_preamble) finds it"""
    data = bytes(data)
    n = i64(0)
    check(lib().ph_snappy_decompress_host(ctypes.c_char_p(data), i64(len(data)), None, i64(0), ctypes.byref(n)))
    if expected is not None and n.value != expected:
        raise PlanHipError(PH_EINVAL, f"ph_snappy_decompress_host: a corrupt Snappy stream: its preamble says {n.value} bytes, {expected} are expected")
    buf = np.zeros(max(n.value, 1), np.uint8)
    check(lib().ph_snappy_decompress_host(ctypes.c_char_p(data), i64(len(data)), vp(buf.ctypes.data), i64(n.value), ctypes.byref(n)))
    return buf[:n.value].tobytes()


def snappy_decompress(ctx, streams, expected_sizes, canary=0):
    """ph_snappy_decompress: the streams (bytes each) are packed into one device buffer and decompressed by the kernel of the Parquet load
    in ONE call -> ([bytes or None per stream: None = refused (PH_EINVAL)], the whole destination buffer as a numpy array, [destination
    position per stream]). canary: bytes left between the destinations (they start on odd positions when it is odd) and filled with 0xA5
    before the call, for callers that check nothing else is written"""
    return _decompress_streams(lib().ph_snappy_decompress, ctx, streams, expected_sizes, canary)


def _decompress_streams(entry, ctx, streams, expected_sizes, canary):
    n = len(streams)
    assert n == len(expected_sizes)
    src_pos, dst_pos = np.zeros(n, np.int64), np.zeros(n, np.int64)
    src_len = np.array([len(s) for s in streams], np.int64).reshape(n)
    dst_len = np.array(expected_sizes, np.int64).reshape(n)
    at_s, at_d = 0, canary
    for k in range(n):
        src_pos[k], dst_pos[k] = at_s, at_d
        at_s += int(src_len[k])
        at_d += int(dst_len[k]) + canary
    src = np.frombuffer(b"".join(bytes(s) for s in streams) + b"\0", np.uint8)
    dst = np.full(at_d + 1, 0xA5, np.uint8)
    src_dev, dst_dev = ctx.upload(src), ctx.upload(dst)
    status = np.zeros(max(n, 1), np.int32)
    try:
        check(entry(ctx.h, src_dev, vp(src_pos.ctypes.data), vp(src_len.ctypes.data), dst_dev, vp(dst_pos.ctypes.data), vp(dst_len.ctypes.data), i32(n),
                    vp(status.ctypes.data)))
        out = ctx.download(dst_dev, np.uint8, len(dst))
    finally:
        ctx.free(src_dev)
        ctx.free(dst_dev)
    res = [out[int(dst_pos[k]):int(dst_pos[k] + dst_len[k])].tobytes() if status[k] == PH_OK else None for k in range(n)]
    return res, out, [int(p) for p in dst_pos]


def lz4_decompress_host(data, expected):
    """ph_lz4_decompress_host (host only, no device): one bare LZ4 block (Parquet's LZ4_RAW), decoded by the host twin of the device decoder
    -> bytes. expected: the length the block must produce (the format has no preamble that says). A refused block raises PlanHipError
    (PH_EINVAL) naming the sub-case."""
    data = bytes(data)
    n = i64(0)
    buf = np.zeros(max(int(expected), 1), np.uint8)
    check(lib().ph_lz4_decompress_host(ctypes.c_char_p(data), i64(len(data)), vp(buf.ctypes.data), i64(int(expected)), ctypes.byref(n)))
    return buf[:n.value].tobytes()


def lz4_decompress(ctx, streams, expected_sizes, canary=0):
    """ph_lz4_decompress: the blocks (bytes each) are packed into one device buffer and decompressed by the kernel of the Parquet load in
    ONE call -> what snappy_decompress returns: ([bytes or None per block: None = refused (PH_EINVAL)], the whole destination buffer as a
    numpy array, [destination position per block]). canary: as there"""
    return _decompress_streams(lib().ph_lz4_decompress, ctx, streams, expected_sizes, canary)


def gzip_decompress_host(data, expected):
    """ph_gzip_decompress_host (host only, no device): one GZIP stream (RFC 1952, one or more members), decoded by the host twin of the
    device decoder -> bytes. expected: the length all members together must produce. A refused stream raises PlanHipError (PH_EINVAL)
    naming the sub-case."""
    data = bytes(data)
    n = i64(0)
    buf = np.zeros(max(int(expected), 1), np.uint8)
    check(lib().ph_gzip_decompress_host(ctypes.c_char_p(data), i64(len(data)), vp(buf.ctypes.data), i64(int(expected)), ctypes.byref(n)))
    return buf[:n.value].tobytes()


def gzip_decompress(ctx, streams, expected_sizes, canary=0):
    """ph_gzip_decompress: the streams (bytes each) are packed into one device buffer and inflated by the kernel of the Parquet load in
    ONE call -> what snappy_decompress returns: ([bytes or None per stream: None = refused (PH_EINVAL)], the whole destination buffer as a
    numpy array, [destination position per stream]). canary: as there"""
    return _decompress_streams(lib().ph_gzip_decompress, ctx, streams, expected_sizes, canary)


def zstd_decompress_host(data, expected):
    """ph_zstd_decompress_host (host only, no device): one ZSTD stream (RFC 8878, one or more frames), decoded by the host twin of the
    device decoder -> bytes. expected: the length all frames together must produce. A refused stream raises PlanHipError (PH_EINVAL)
    naming the sub-case."""
    data = bytes(data)
    n = i64(0)
    buf = np.zeros(max(int(expected), 1), np.uint8)
    check(lib().ph_zstd_decompress_host(ctypes.c_char_p(data), i64(len(data)), vp(buf.ctypes.data), i64(int(expected)), ctypes.byref(n)))
    return buf[:n.value].tobytes()


def zstd_stream_stats_host(data, expected, far_limit=32768):
    """ph_zstd_stream_stats_host (host only): what one ZSTD stream is made of -> (literal bytes, sequences, match bytes, match bytes whose
    offset is above far_limit)"""
    data = bytes(data)
    st = (i64 * 4)()
    check(lib().ph_zstd_stream_stats_host(ctypes.c_char_p(data), i64(len(data)), i64(int(expected)), i64(int(far_limit)), st))
    return tuple(int(v) for v in st)


def zstd_decompress(ctx, streams, expected_sizes, canary=0):
    """ph_zstd_decompress: the streams (bytes each) are packed into one device buffer and decompressed by the kernel of the Parquet load
    in ONE call -> what snappy_decompress returns: ([bytes or None per stream: None = refused (PH_EINVAL)], the whole destination buffer
    as a numpy array, [destination position per stream]). canary: as there"""
    return _decompress_streams(lib().ph_zstd_decompress, ctx, streams, expected_sizes, canary)


DELTA_HOST_MAX = 1 << 24   # values delta_decode_host allocates for on a header's word alone
DELTA_CANARY = -0x5a5a5a5a5a5a5a5b   # what delta_decode fills its destination with before the call


def delta_decode_host(data, bits, expected=-1, exact=False):
    """ph_delta_decode_host (host only, no device): one raw DELTA_BINARY_PACKED stream, decoded by the host twin of the device decoder ->
    (values int64, bytes consumed). bits: 32 or 64; expected: the count the header must state (-1: whatever it states, up to
    DELTA_HOST_MAX); exact: the stream must end where `data` ends. A refused stream raises PlanHipError naming the sub-case."""
    data = bytes(data)
    s = DeltaStream(0, len(data), int(bits), int(bool(exact)), int(expected), 0, 0, 0, 0, 0, 0)
    rc = lib().ph_delta_decode_host(ctypes.c_char_p(data), None, ctypes.byref(s))
    if rc == PH_ECAPACITY and s.count <= DELTA_HOST_MAX:      # (the header is readable: room for what it states)
        out = np.zeros(int(s.count), np.int64)
        s.dst_cap = int(s.count)
        rc = lib().ph_delta_decode_host(ctypes.c_char_p(data), vp(out.ctypes.data), ctypes.byref(s))
    else:
        out = np.zeros(0, np.int64)
    check(rc)
    return out[:int(s.count)], int(s.consumed)


def delta_decode(ctx, streams, canary=0):
    """ph_delta_decode: streams = [(bytes, bits, expected count or -1, exact, room in values)], packed into one device buffer and decoded by
    the device function of the Parquet load in ONE call -> ([(status, values int64 or None, count, consumed)], the whole destination as a
    numpy array, [destination position per stream, in values]). canary: values left between the destinations, filled with a pattern
    before the call, for callers that check nothing else is written"""
    n = len(streams)
    arr = (DeltaStream * max(n, 1))()
    at_s, at_d = 0, canary
    for k, (byts, bits, expected, exact, room) in enumerate(streams):
        arr[k] = DeltaStream(at_s, len(byts), int(bits), int(bool(exact)), int(expected), at_d, int(room), 0, 0, 0, 0)
        at_s += len(byts)
        at_d += int(room) + canary
    src = np.frombuffer(b"".join(bytes(s[0]) for s in streams) + b"\0", np.uint8)
    dst = np.full(at_d + 1, DELTA_CANARY, np.int64)
    src_dev, dst_dev = ctx.upload(src), ctx.upload(dst)
    try:
        check(lib().ph_delta_decode(ctx.h, src_dev, dst_dev, arr, i32(n)))
        out = ctx.download(dst_dev, np.int64, len(dst))
    finally:
        ctx.free(src_dev)
        ctx.free(dst_dev)
    res = []
    for k in range(n):
        s = arr[k]
        vals = out[int(s.dst_pos):int(s.dst_pos + s.count)].copy() if s.status == PH_OK else None
        res.append((int(s.status), vals, int(s.count), int(s.consumed)))
    return res, out, [int(arr[k].dst_pos) for k in range(n)]


DBA_CANARY = 0x5a   # the byte delta_byte_array_decode fills both destinations with before the call


def delta_byte_array_decode_host(data, expected=-1, len_room=None, byte_room=None):
    """ph_delta_byte_array_decode_host (host only, no device): one raw DELTA_BYTE_ARRAY values section, decoded by the host twin of the device
    decoder -> (lengths int32, the values' bytes back to back, the DbaStream record). len_room / byte_room None: learned from the section
    by calls that state too little room (up to DELTA_HOST_MAX values). A refused section raises PlanHipError with .record = the record."""
    data = bytes(data)

    def call(lr, br):
        s = DbaStream(0, len(data), int(expected), 0, int(lr), 0, int(br), 0, 0, 0, 0, 0)
        lens, byts = np.zeros(max(int(lr), 1), np.int32), np.zeros(max(int(br), 1), np.uint8)
        rc = lib().ph_delta_byte_array_decode_host(ctypes.c_char_p(data), vp(lens.ctypes.data), vp(byts.ctypes.data), ctypes.byref(s))
        return rc, s, lens, byts
    lr, br = 0 if len_room is None else len_room, 0 if byte_room is None else byte_room
    rc, s, lens, byts = call(lr, br)
    if rc == PH_ECAPACITY and len_room is None and s.count > lr and s.count <= DELTA_HOST_MAX:
        lr = s.count
        rc, s, lens, byts = call(lr, br)
    if rc == PH_ECAPACITY and byte_room is None and s.total_bytes > br:
        rc, s, lens, byts = call(lr, s.total_bytes)
    if rc != PH_OK:
        try:
            check(rc)
        except PlanHipError as e:
            e.record = s
            raise
    return lens[:int(s.count)], byts[:int(s.total_bytes)].tobytes(), s


def delta_byte_array_decode(ctx, streams, canary=0):
    """ph_delta_byte_array_decode: streams = [(bytes, expected count or -1, room in values, room in bytes)], packed into one device buffer
    and decoded by the device functions of the Parquet load in ONE call -> ([DbaStream record per stream], the whole lengths destination
    (int32), the whole bytes destination (uint8)). canary: values / bytes left between the destinations; both are filled with DBA_CANARY
    bytes before the call, for callers that check nothing else is written"""
    n = len(streams)
    arr = (DbaStream * max(n, 1))()
    at_s, at_l, at_b = 0, canary, canary
    for k, (byts, expected, lroom, broom) in enumerate(streams):
        arr[k] = DbaStream(at_s, len(byts), int(expected), at_l, int(lroom), at_b, int(broom), 0, 0, 0, 0, 0)
        at_s += len(byts)
        at_l += int(lroom) + canary
        at_b += int(broom) + canary
    src = np.frombuffer(b"".join(bytes(s[0]) for s in streams) + b"\0", np.uint8)
    lens = np.full(at_l + 1, DBA_CANARY * 0x01010101, np.int32)
    byts = np.full(at_b + 1, DBA_CANARY, np.uint8)
    src_dev, lens_dev, byts_dev = ctx.upload(src), ctx.upload(lens), ctx.upload(byts)
    try:
        check(lib().ph_delta_byte_array_decode(ctx.h, src_dev, lens_dev, byts_dev, arr, i32(n)))
        lens_out = ctx.download(lens_dev, np.int32, len(lens))
        byts_out = ctx.download(byts_dev, np.uint8, len(byts))
    finally:
        ctx.free(src_dev)
        ctx.free(lens_dev)
        ctx.free(byts_dev)
    return [arr[k] for k in range(n)], lens_out, byts_out


def parquet_read_column_host(data, column, typ=0, scale=0, nbytes=None, flags=0):
    """ph_parquet_read_column_host_ex (host only, no device): one column decoded by the functions the kernels run ->
    (values int64 or None, valid bool[nrows], offsets int32[nrows + 1] or None, string bytes or None); flags: PH_PARQUET_SNAPPY | PH_PARQUET_DELTA | PH_PARQUET_DELTA_BYTE_ARRAY | PH_PARQUET_LZ4_RAW | PH_PARQUET_GZIP | PH_PARQUET_ZSTD"""
    src, keep = _file_arg(data)
    nbytes = len(keep) if nbytes is None else nbytes
    nrows, _g, info = parquet_schema(data, nbytes)
    col = ParquetCol(int(column), int(typ), int(scale))
    valid = np.zeros(max(nrows, 1), np.uint8)
    is_str = 0 <= column < len(info) and info[column].type == PH_STR
    L = lib()
    fl = ctypes.c_uint32(flags)
    if not is_str:
        values = np.zeros(max(nrows, 1), np.int64)
        check(L.ph_parquet_read_column_host_ex(src, i64(nbytes), ctypes.byref(col), fl, vp(values.ctypes.data), vp(valid.ctypes.data), None, None, i64(0), None))
        return values[:nrows], valid[:nrows].astype(bool), None, None
    off = np.zeros(nrows + 1, np.int32)
    total = i64(0)
    check(L.ph_parquet_read_column_host_ex(src, i64(nbytes), ctypes.byref(col), fl, None, vp(valid.ctypes.data), vp(off.ctypes.data), None, i64(0), ctypes.byref(total)))
    buf = np.zeros(max(total.value, 1), np.uint8)
    check(L.ph_parquet_read_column_host_ex(src, i64(nbytes), ctypes.byref(col), fl, None, vp(valid.ctypes.data), vp(off.ctypes.data), vp(buf.ctypes.data), i64(total.value),
                                        ctypes.byref(total)))
    return None, valid[:nrows].astype(bool), off, buf[:total.value].tobytes()


def table_create_parquet(ctx, data, nbytes, cols=None, flags=0):
    """ph_table_create_parquet_ex: data = an address (int) or bytes; cols = [(leaf column, type or 0, scale)] or None for every column;
    flags: PH_PARQUET_SNAPPY | PH_PARQUET_DELTA | PH_PARQUET_DELTA_BYTE_ARRAY | PH_PARQUET_LZ4_RAW | PH_PARQUET_GZIP | PH_PARQUET_ZSTD -> ph_table handle"""
    src, _keep = _file_arg(data)
    h = vp()
    if cols:
        arr = (ParquetCol * len(cols))(*[ParquetCol(int(c), int(t), int(sc)) for c, t, sc in cols])
        check(lib().ph_table_create_parquet_ex(ctx.h, src, i64(nbytes), arr, i32(len(cols)), ctypes.c_uint32(flags), ctypes.byref(h)))
    else:
        check(lib().ph_table_create_parquet_ex(ctx.h, src, i64(nbytes), None, i32(0), ctypes.c_uint32(flags), ctypes.byref(h)))
    return h


def table_create_csv(ctx, text, nbytes, delimiter, cols, flags=0):
    """ph_table_create_csv_ex: text = an address (int) or bytes; cols = [(field, type, scale)]; flags: 0 or PH_CSV_QUOTES
    -> ph_table handle"""
    arr = (CsvCol * len(cols))(*[CsvCol(int(f), int(t), int(sc)) for f, t, sc in cols])
    h = vp()
    src = ctypes.c_char_p(text) if isinstance(text, bytes) else vp(text)
    check(lib().ph_table_create_csv_ex(ctx.h, src, i64(nbytes), i32(delimiter), arr, i32(len(cols)), ctypes.c_uint32(flags), ctypes.byref(h)))
    return h


def table_concat(ctx, tables):
    """ph_table_concat: one new resident table from the rows of `tables` (Table objects or ph_table handles; None = a NULL part) in
    that order, built on the device; the parts are only read -> ph_table handle"""
    hs = [t.h if isinstance(t, Table) else t for t in tables]
    arr = (vp * max(len(hs), 1))(*[h if isinstance(h, vp) else vp(h) for h in hs])
    h = vp()
    check(lib().ph_table_concat(ctx.h, arr, i32(len(hs)), ctypes.byref(h)))
    return h


def validity_concat_host(bitmaps, rows, out_bytes=None):
    """ph_validity_concat_host (host only, no device): bitmaps = per part a uint8 array or None (all valid), rows = per part its row
    count -> the concatenated bitmap as a uint8 array of out_bytes bytes (default: (total + 7) // 8)"""
    n = len(rows)
    keep = [None if b is None else np.ascontiguousarray(b, dtype=np.uint8) for b in bitmaps]
    ptrs = (vp * max(n, 1))(*[vp(None) if b is None else vp(b.ctypes.data) for b in keep])
    if out_bytes is None:
        out_bytes = (int(sum(rows)) + 7) // 8
    out = np.full(max(out_bytes, 1), 0xAA, np.uint8)
    check(lib().ph_validity_concat_host(i32(n), ptrs, (i64 * max(n, 1))(*[int(r) for r in rows]), vp(out.ctypes.data), i64(out_bytes)))
    return out[:out_bytes]


def dict_merge_host(dicts, cap=None):
    """ph_dict_merge_host (host only): dicts = per part a list of bytes entries -> (merged entries as a list of bytes, remap as a
    uint8 array [nparts, 256], identical); cap = room for the merged blob (default: enough)"""
    n = len(dicts)
    blobs = [b"".join(bytes(e) + b"\0" for e in d) for d in dicts]
    keep = [ctypes.create_string_buffer(b, max(len(b), 1)) for b in blobs]
    ptrs = (vp * max(n, 1))(*[ctypes.cast(k, vp) for k in keep])
    sizes = (i64 * max(n, 1))(*[len(b) for b in blobs])
    if cap is None:
        cap = sum(len(b) for b in blobs) + 1
    merged = ctypes.create_string_buffer(max(cap, 1))
    nbytes, nmerged, identical = i64(), i32(), i32()
    remap = np.full((max(n, 1), 256), 0xAA, np.uint8)
    check(lib().ph_dict_merge_host(i32(n), ptrs, sizes, merged, i64(cap), ctypes.byref(nbytes), ctypes.byref(nmerged), vp(remap.ctypes.data),
                                   ctypes.byref(identical)))
    entries = merged.raw[:nbytes.value].split(b"\0")[:-1] if nbytes.value else []
    assert len(entries) == nmerged.value
    return entries, remap[:n], bool(identical.value)


def _result(rp):
    r = rp.contents
    ng, nk, na = r.ngroups, r.nkeys, r.naggs
    out = {
        "ngroups": ng,
        "first_row": np.array([r.first_row[g] for g in range(ng)], dtype=np.int64),
        "keys": np.array([r.keys[i] for i in range(ng * nk)], dtype=np.int64).reshape(ng, nk),
        "scale": [r.scale[a] for a in range(na)],
        # python ints: exact 128-bit sums
        "sum": [[(int(r.sum_hi[g * na + a]) << 64) + int(r.sum_lo[g * na + a]) for a in range(na)]
                for g in range(ng)],
        "count": [[int(r.count[g * na + a]) for a in range(na)] for g in range(ng)],
        # 1 = the group's key is NULL (None when the result has no NULL-able key)
        "key_null": np.array([r.key_null[i] for i in range(ng * nk)], dtype=np.uint8).reshape(ng, nk) if r.key_null else None,
    }
    lib().ph_agg_result_free(rp)
    return out


class ScanPlan:
    """Fused Agg <- Scan(filter) over a resident table (ph_scan_plan)."""

    def __init__(self, ctx, table, preds, group_cols, aggs):
        self.ctx, self.table = ctx, table
        pa = (Pred * max(len(preds), 1))(*preds)
        ga = (i32 * max(len(group_cols), 1))(*group_cols)
        aa = (AggExpr * len(aggs))(*aggs)
        self.h = vp()
        check(lib().ph_scan_plan_create(ctx.h, table.h, pa, i32(len(preds)), ga,
                                        i32(len(group_cols)), aa, i32(len(aggs)),
                                        ctypes.byref(self.h)))
        self._keep = (pa, ga, aa)

    @property
    def kind(self):
        return lib().ph_scan_plan_kind(self.h).decode()

    @property
    def bytes_per_row(self):
        """ph_scan_plan_bytes_per_row: bytes per row the scan kernel loads (the narrowed copies when it reads them)"""
        lib().ph_scan_plan_bytes_per_row.restype = i32
        return int(lib().ph_scan_plan_bytes_per_row(self.h))

    @property
    def variant(self):
        """ph_scan_plan_variant: the kernel instance the plan launches ("narrow32_lean", "narrow32", "narrow_rt", "narrow64", "wide", ...)"""
        lib().ph_scan_plan_variant.restype = ctypes.c_char_p
        return lib().ph_scan_plan_variant(self.h).decode()

    @property
    def row_body(self):
        """ph_scan_plan_row_body: "bins" or "columns", the row body of the plan's next launch (PH_SCAN_HIST=0: always "columns")"""
        lib().ph_scan_plan_row_body.restype = ctypes.c_char_p
        return lib().ph_scan_plan_row_body(self.h).decode()

    def run(self, row_begin=0, row_end=None):
        if row_end is None:
            row_end = self.table.nrows
        check(lib().ph_scan_plan_run(self.h, i64(row_begin), i64(row_end)))

    def fetch(self):
        rp = ctypes.POINTER(AggResult)()
        check(lib().ph_scan_plan_fetch(self.h, ctypes.byref(rp)))
        return _result(rp)

    def partials_dev(self):
        """(device pointer, number of 64-bit words) of the raw partial result of the last run."""
        dev, n = vp(), i32()
        check(lib().ph_scan_plan_partials_dev(self.h, ctypes.byref(dev), ctypes.byref(n)))
        return dev.value, n.value

    def fetch_merged(self, words, nranks):
        """words: uint64 numpy array, the ranks' raw partials concatenated rank-major."""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        rp = ctypes.POINTER(AggResult)()
        check(lib().ph_scan_plan_fetch_merged(self.h, vp(words.ctypes.data), i32(nranks), ctypes.byref(rp)))
        return _result(rp)

    def free(self):
        if self.h:
            lib().ph_scan_plan_free(self.h)
            self.h = None


# ---------------------------------------------------------------- operator-granular API

class DevColumn:
    """A device-resident column built from a numpy array (ph_dev_alloc + ph_dev_upload)."""

    def __init__(self, ctx, typ, arr, scale=0, validity=None, aux=None):
        self.ctx, self.type, self.scale = ctx, typ, scale
        arr = np.ascontiguousarray(arr)
        self.n = len(arr) - 1 if typ == PH_STR else len(arr)
        self.ptrs = []
        self.data = ctx.upload(arr) if arr.nbytes else ctx.alloc(8)
        self.ptrs.append(self.data)
        self.validity = None
        if validity is not None:
            self.validity = ctx.upload(np.ascontiguousarray(validity, dtype=np.uint8))
            self.ptrs.append(self.validity)
        self.aux, self.aux_bytes = None, 0
        if aux is not None:
            aux = np.ascontiguousarray(aux)
            self.aux = ctx.upload(aux) if aux.nbytes else ctx.alloc(8)
            self.aux_bytes = aux.nbytes
            self.ptrs.append(self.aux)

    def col(self):
        c = Col()
        c.type, c.scale = self.type, self.scale
        c.data = self.data
        c.validity = self.validity
        c.aux = self.aux
        c.aux_bytes = self.aux_bytes
        return c

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)
        self.ptrs = []


def str_column(ctx, values):
    """A PH_STR DevColumn from a list of bytes (None = NULL): int32 offsets[n+1], the bytes, and a validity bitmap when a value is NULL."""
    lens = np.fromiter((0 if v is None else len(v) for v in values), dtype=np.int64, count=len(values))
    off = np.zeros(len(values) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    if off[-1] >= 2**31:
        raise ValueError("PH_STR column: 2^31 bytes or more (int32 offsets)")
    data = np.frombuffer(b"".join(v for v in values if v is not None), dtype=np.uint8)
    valid = np.fromiter((v is not None for v in values), dtype=bool, count=len(values))
    validity = None if valid.all() else np.packbits(valid, bitorder="little")
    return DevColumn(ctx, PH_STR, off.astype(np.int32), validity=validity, aux=data)


class TableColumn(DevColumn):
    """Column c of a resident Table, usable wherever a DevColumn is (col(), data, type, scale, n); freed with its table."""

    def __init__(self, table, c):
        self.table, self.index = table, c
        v = table.col(c)
        self.ctx, self.type, self.scale, self.data, self.validity, self.n = table.ctx, v.type, v.scale, v.data, v.validity, table.nrows
        self.aux, self.aux_bytes = v.aux, v.aux_bytes
        self.ptrs = []

    def col(self):
        return self.table.col(self.index)

    def free(self):
        pass


def _cols(cols):
    return (Col * max(len(cols), 1))(*[c.col() if isinstance(c, DevColumn) else c for c in cols])


def filter_select(ctx, col, n, op, k, sel_in=None, n_in=None, defer=False):
    """Returns (sel_out_dev, count). sel_in: device pointer or None. defer (with Ctx.set_async_counts):
    the count comes back as the ctypes int64 itself, valid after Ctx.wait_counts()."""
    if n_in is None:
        n_in = n
    out = ctx.alloc(max(n_in, 1) * 4)
    cnt = i64()
    c = col.col() if isinstance(col, DevColumn) else col
    try:
        check(lib().ph_filter_select(ctx.h, ctypes.byref(c), i64(n), i32(op), ctypes.byref(k),
                                     sel_in, i64(n_in), out, ctypes.byref(cnt)))
    except PlanHipError:
        ctx.free(out)
        raise
    return (out, cnt) if defer else (out, cnt.value)


def filter_select_and(ctx, col, n, op1, k1, op2, k2, sel_in=None, n_in=None):
    """ph_filter_select_and: two conjuncts over one column in one pass; (sel_out_dev, count). PH_EUNSUPPORTED when they are not two value ranges."""
    if n_in is None:
        n_in = n
    out = ctx.alloc(max(n_in, 1) * 4)
    cnt = i64()
    c = col.col() if isinstance(col, DevColumn) else col
    try:
        check(lib().ph_filter_select_and(ctx.h, ctypes.byref(c), i64(n), i32(op1), ctypes.byref(k1), i32(op2), ctypes.byref(k2), sel_in, i64(n_in), out, ctypes.byref(cnt)))
    except PlanHipError:
        ctx.free(out)
        raise
    return out, cnt.value


def filter_select_in(ctx, col, n, values, sel_in=None, n_in=None):
    """ph_filter_select_in: col IN (values) in one pass over an INTEGER or dictionary-code column; (sel_out_dev, count)"""
    if n_in is None:
        n_in = n
    out = ctx.alloc(max(n_in, 1) * 4)
    cnt = i64()
    c = col.col() if isinstance(col, DevColumn) else col
    vals = (ctypes.c_int64 * max(len(values), 1))(*values)
    try:
        check(lib().ph_filter_select_in(ctx.h, ctypes.byref(c), i64(n), vals, i32(len(values)), sel_in, i64(n_in), out, ctypes.byref(cnt)))
    except PlanHipError:
        ctx.free(out)
        raise
    return out, cnt.value


def filter_select_cols(ctx, a, b, n, op, sel_in=None, n_in=None):
    """ph_filter_select_cols: column OP column over the same rows; (sel_out_dev, count)"""
    if n_in is None:
        n_in = n
    out = ctx.alloc(max(n_in, 1) * 4)
    cnt = i64()
    ca = a.col() if isinstance(a, DevColumn) else a
    cb = b.col() if isinstance(b, DevColumn) else b
    try:
        check(lib().ph_filter_select_cols(ctx.h, ctypes.byref(ca), ctypes.byref(cb), i64(n), i32(op), sel_in, i64(n_in), out, ctypes.byref(cnt)))
    except PlanHipError:
        ctx.free(out)
        raise
    return out, cnt.value


def dev_exclusive_scan_i32(ctx, dev, n):
    """ph_dev_exclusive_scan_i32: the operators' exclusive scan over device int32[n], in place; returns the total"""
    total = ctx.alloc(8)
    try:
        check(lib().ph_dev_exclusive_scan_i32(ctx.h, dev, i64(n), total))
        return int(ctx.download(total, np.int64, 1)[0])
    finally:
        ctx.free(total)


def dev_iota(ctx, n):
    """ph_dev_iota: device int32[n] = 0 .. n-1"""
    out = ctx.alloc(max(n, 1) * 4)
    check(lib().ph_dev_iota(ctx.h, out, i64(n)))
    return out


def sel_mark(ctx, sel_dev, n, marks_dev):
    """ph_sel_mark: marks_dev[sel_dev[i]] = 1 for i < n (bytes the caller has cleared)"""
    check(lib().ph_sel_mark(ctx.h, sel_dev, i64(n), marks_dev))


def rowid_validity(ctx, ids_dev, n):
    """ph_rowid_validity: device bitmap of (n + 7) / 8 bytes, bit i = ids_dev[i] >= 0"""
    out = ctx.alloc((n + 7) // 8 + 8)
    check(lib().ph_rowid_validity(ctx.h, ids_dev, i64(n), out))
    return out


def widen_codes(ctx, col, sel, n):
    """ph_widen_codes: the dictionary codes of rows sel[0..n) / 0..n as device int32[n]"""
    c = col.col() if isinstance(col, DevColumn) else col
    out = ctx.alloc(max(n, 1) * 4)
    check(lib().ph_widen_codes(ctx.h, ctypes.byref(c), sel, i64(n), out))
    return out


def sel_union(ctx, sels, counts, n_rows):
    """OR of predicates: ascending union of the children's selections (device pointers).
    Returns (sel_out_dev, count)."""
    k = len(sels)
    arr = (vp * max(k, 1))(*sels)
    cnts = (i64 * max(k, 1))(*[int(c) for c in counts])
    out = ctx.alloc(max(min(n_rows, sum(int(c) for c in counts)), 1) * 4)
    n = i64()
    check(lib().ph_sel_union(ctx.h, arr, cnts, i32(k), i64(n_rows), out, ctypes.byref(n)))
    return out, n.value


def sel_difference(ctx, parent, n_parent, child, n_child, n_rows):
    """falseSel: rows of parent (None = identity over n_rows) not in child. Returns (sel_dev, count)."""
    out = ctx.alloc(max(n_parent, 1) * 4)
    n = i64()
    check(lib().ph_sel_difference(ctx.h, parent, i64(n_parent), child, i64(n_child), i64(n_rows), out, ctypes.byref(n)))
    return out, n.value


def scatter(ctx, values, sel, n, out_data, out_validity=None):
    """FillSwitch: out[sel[i]] = values[i] (values: positional ph_col / DevColumn)"""
    c = values.col() if isinstance(values, DevColumn) else values
    check(lib().ph_scatter(ctx.h, ctypes.byref(c), sel, i64(n), out_data, out_validity))


def sort_rows(ctx, keys, descending, sel, n):
    """ORDER BY: device array of the n row ids (sel[i] or i) in sorted order."""
    out = ctx.alloc(max(n, 1) * 4)
    desc = (i32 * len(keys))(*[1 if d else 0 for d in descending])
    check(lib().ph_sort_rows(ctx.h, _cols(keys), desc, i32(len(keys)), sel, i64(n), out))
    return out


def hash_cols(ctx, cols, n, dict_hashes=None):
    out = ctx.alloc(max(n, 1) * 8)
    dh = None
    if dict_hashes is not None:
        dh = (vp * len(cols))(*[d if d is not None else None for d in dict_hashes])
    check(lib().ph_hash(ctx.h, _cols(cols), dh, i32(len(cols)), i64(n), out))
    return out


def hash_bytes(b):
    return int(lib().ph_hash_bytes(ctypes.c_char_p(b), ctypes.c_uint64(len(b))))


def expr_scale(cols, prog):
    p = (Rpn * len(prog))(*[Rpn(*x) for x in prog])
    s = i32()
    check(lib().ph_expr_scale(_cols(cols), p, i32(len(prog)), ctypes.byref(s)))
    return s.value


def expr_eval(ctx, cols, prog, sel, n, want_validity=False):
    p = (Rpn * len(prog))(*[Rpn(*x) for x in prog])
    out = ctx.alloc(max(n, 1) * 8)
    val = ctx.alloc((n + 7) // 8 + 8) if want_validity else None
    check(lib().ph_expr_eval(ctx.h, _cols(cols), i32(len(cols)), p, i32(len(prog)), sel, i64(n),
                             out, val))
    return out, val


def float_eval_validity_bytes(n):
    """the size ph_float_eval documents for its validity bitmap: one 64-bit word per 64 rows"""
    return (n + 63) // 64 * 8


def float_eval(ctx, cols, prog, sel, n, truth=True, wide=False, want_validity=False):
    """ph_float_eval: FLOAT / DOUBLE program over device columns -> device pointer of int32 truth values (truth=True) or of the values
    (float32, or float64 for a DOUBLE program). want_validity: returns (out, validity) — validity a device bitmap of the documented size
    (float_eval_validity_bytes(n), 8-byte aligned as every allocation is), or a device pointer the caller allocated that way"""
    arr = (Col * len(cols))(*_cols(cols))
    pr = (Rpn * len(prog))(*[Rpn(*x) for x in prog])
    out = ctx.alloc(max(n, 1) * (8 if wide and not truth else 4))
    out_type = PH_I32 if truth else PH_F64 if wide else PH_F32
    val = None
    if want_validity:
        val = want_validity if isinstance(want_validity, vp) else ctx.alloc(max(float_eval_validity_bytes(n), 8))
    check(lib().ph_float_eval(ctx.h, arr, i32(len(cols)), pr, i32(len(prog)), i32(1 if wide else 0), sel, i64(n), i32(out_type), out, val))
    return (out, val) if want_validity else out


AGG_SIZING = ("T", "nparts", "bins", "shift", "slices", "bu", "tpb", "lds_scatter", "lds_build", "rows_per_wg", "slots", "threads")


def agg_sink_choice(rows, expected_groups, nkeys=1, naggs=1, used_args=1, rows_sunk=0, any_nulls=False, need_cnt=False):
    """ph_agg_sink_choice: (kind, sizing by the names of AGG_SIZING) a sink of this shape would choose; needs no device"""
    kind, sizing = ctypes.c_char_p(), (i64 * len(AGG_SIZING))()
    check(lib().ph_agg_sink_choice(i64(rows), i64(rows_sunk), i64(expected_groups), i32(nkeys), i32(naggs), i32(used_args),
                                   i32(1 if any_nulls else 0), i32(1 if need_cnt else 0), ctypes.byref(kind), sizing))
    return kind.value.decode(), dict(zip(AGG_SIZING, sizing))


class Agg:
    def __init__(self, ctx, key_types, aggs, expected_groups=1024):
        self.ctx = ctx
        self.nkeys, self.naggs = len(key_types), len(aggs)
        kt = (i32 * len(key_types))(*key_types)
        sp = (AggSpec * max(len(aggs), 1))(*[AggSpec(k, a) for k, a in aggs])
        self.h = vp()
        check(lib().ph_agg_create(ctx.h, i32(len(key_types)), kt, i32(len(aggs)), sp,
                                  i64(expected_groups), ctypes.byref(self.h)))

    @property
    def sink_kind(self):
        """ph_agg_sink_kind: the form that sank the most recent rows ("" before any sink)"""
        return lib().ph_agg_sink_kind(self.h).decode()

    def sink_sorted(self, keys, args, n, row_base=0):
        """ph_agg_sink_sorted: streaming aggregate over rows ordered by the group key (first sink only);
        False when the shape is not supported (the caller sinks with sink())"""
        rc = lib().ph_agg_sink_sorted(self.h, _cols(keys), _cols(args), i32(len(args)), i64(n), i64(row_base))
        if rc == PH_EUNSUPPORTED:
            return False
        check(rc)
        return True

    def sink(self, keys, args, sel, n, positional=False, row_base=0, mask=None):
        """mask: bit a set = aggregate a is updated (AddChunk's filter); None = all"""
        if mask is None:
            check(lib().ph_agg_sink(self.h, _cols(keys), _cols(args), i32(len(args)), sel, i64(n),
                                    i32(1 if positional else 0), i64(row_base)))
        else:
            check(lib().ph_agg_sink_masked(self.h, _cols(keys), _cols(args), i32(len(args)), sel, i64(n),
                                           i32(1 if positional else 0), i64(row_base), ctypes.c_uint32(mask)))

    def key_column(self, c, key_type, scale=0):
        """key column c of all groups as a device column (data ptr, validity ptr, ngroups, ph_col)"""
        ng = self.group_count()
        w = 4 if key_type in (PH_I32, PH_DATE) else 1 if key_type == PH_CODE8 else 8
        data = self.ctx.alloc(max(ng, 1) * w)
        valid = self.ctx.alloc((max(ng, 1) + 7) // 8 + 8)
        n = i64()
        check(lib().ph_agg_keys_dev(self.h, i32(c), data, valid, i64(ng), ctypes.byref(n)))
        col = Col()
        col.type, col.scale, col.data, col.validity = key_type, scale, data, valid
        return data, valid, n.value, col

    def value_column(self, a):
        """aggregate a of all groups as a device int64 column (data ptr, validity ptr, ngroups); ph_agg_values_dev"""
        ng = self.group_count()
        data = self.ctx.alloc(max(ng, 1) * 8)
        valid = self.ctx.alloc((max(ng, 1) + 7) // 8 + 8)
        n = i64()
        rc = lib().ph_agg_values_dev(self.h, i32(a), data, valid, i64(ng), ctypes.byref(n))
        if rc != PH_OK:
            self.ctx.free_many([data, valid])
            check(rc)
        return data, valid, n.value

    def group_count(self):
        n = i64()
        check(lib().ph_agg_group_count(self.h, ctypes.byref(n)))
        return n.value

    def finalize(self, python_ints=True, room=1024, where=None):
        """ph_agg_fetch with room for `room` groups first (one host round trip when they fit), again
        with the reported count when there are more. where = [(agg_index, op, Const, value_scale), ...]: ph_agg_fetch_where — only the
        groups whose aggregates satisfy every conjunct (HAVING on the device)"""
        na = max(self.naggs, 1)
        P = lambda a: vp(a.ctypes.data)
        m = max(room, 1)
        if where:
            wi = (i32 * len(where))(*[w[0] for w in where])
            wo = (i32 * len(where))(*[w[1] for w in where])
            wk = (Const * len(where))(*[w[2] for w in where])
            ws = (i32 * len(where))(*[w[3] for w in where])
        while True:
            first = np.zeros(m, np.int64)
            keys = np.zeros(m * self.nkeys, np.int64)
            knull = np.zeros(m * self.nkeys, np.uint8)
            lo = np.zeros(m * na, np.uint64)
            hi = np.zeros(m * na, np.int64)
            cnt = np.zeros(m * na, np.uint64)
            n = i64()
            if where:
                rc = lib().ph_agg_fetch_where(self.h, i32(len(where)), wi, wo, wk, ws, i64(m), ctypes.byref(n), P(first), P(keys), P(knull), P(lo), P(hi), P(cnt))
            else:
                rc = lib().ph_agg_fetch(self.h, i64(m), ctypes.byref(n), P(first), P(keys), P(knull), P(lo), P(hi), P(cnt))
            if rc == PH_ECAPACITY and n.value > m:
                m = n.value
                continue
            check(rc)
            break
        ng = n.value
        out = dict(ngroups=ng, first_row=first[:ng], keys=keys.reshape(m, self.nkeys)[:ng],
                   key_null=knull.reshape(m, self.nkeys)[:ng],
                   sum_lo=lo.reshape(m, na)[:ng, :self.naggs], sum_hi=hi.reshape(m, na)[:ng, :self.naggs],
                   count=cnt.reshape(m, na)[:ng, :self.naggs].astype(np.int64))
        if python_ints:  # exact 128-bit python ints (one C-level tolist per word array, then plain int arithmetic)
            hl, ll = hi[:ng * na].tolist(), lo[:ng * na].tolist()
            nag = self.naggs
            out["sum"] = [[(hl[g * na + a] << 64) + ll[g * na + a] for a in range(nag)] for g in range(ng)]
        return out

    def topk(self, agg_index, k, descending=True, cap=4096):
        """Groups whose aggregate `agg_index` is at least as good as the k-th best (>= k with ties)."""
        first = np.zeros(cap, np.int64)
        keys = np.zeros(cap * self.nkeys, np.int64)
        knull = np.zeros(cap * self.nkeys, np.uint8)
        na = max(self.naggs, 1)
        lo = np.zeros(cap * na, np.uint64)
        hi = np.zeros(cap * na, np.int64)
        cnt = np.zeros(cap * na, np.uint64)
        n = i64()
        P = lambda a: vp(a.ctypes.data)
        check(lib().ph_agg_topk(self.h, i32(agg_index), i32(1 if descending else 0), i64(k), i64(cap),
                                ctypes.byref(n), P(first), P(keys), P(knull), P(lo), P(hi), P(cnt)))
        m = n.value
        return dict(ngroups=m, first_row=first[:m], keys=keys.reshape(cap, self.nkeys)[:m],
                    key_null=knull.reshape(cap, self.nkeys)[:m], sum_lo=lo.reshape(cap, na)[:m, :self.naggs],
                    sum_hi=hi.reshape(cap, na)[:m, :self.naggs],
                    count=cnt.reshape(cap, na)[:m, :self.naggs].astype(np.int64))

    def free(self):
        if self.h:
            lib().ph_agg_free(self.h)
            self.h = None


class Join:
    def __init__(self, ctx, keys, sel, n, key_range=None, fk_probes=False, sorted_unique=False, exists_only=False):
        """key_range = (lo, hi) of the single key column from column statistics (Table.col_range): a
        direct table for dense keys; fk_probes: the probe side is a foreign key into these keys (node
        table, no Bloom bitmap) — ph_join_build_ex"""
        self.ctx = ctx
        self.h = vp()
        if key_range is None and not fk_probes and not sorted_unique and not exists_only:
            check(lib().ph_join_build(ctx.h, _cols(keys), i32(len(keys)), sel, i64(n), ctypes.byref(self.h)))
        else:
            flags = ((PH_JOIN_KEY_RANGE if key_range is not None else 0) | (PH_JOIN_FK_PROBES if fk_probes else 0) |
                     (PH_JOIN_KEYS_SORTED_UNIQUE if sorted_unique else 0) | (PH_JOIN_EXISTS_ONLY if exists_only else 0))
            lo, hi = key_range if key_range is not None else (0, 0)
            check(lib().ph_join_build_ex(ctx.h, _cols(keys), i32(len(keys)), sel, i64(n), i32(flags), i64(lo), i64(hi),
                                         ctypes.byref(self.h)))

    @classmethod
    def build_where(cls, ctx, keys, where_col, where_op, where_k, sel, n, key_range, sorted_unique=False):
        """ph_join_build_where_ex (Filter -> build fused, direct tables only); None when the shape is not fused.
        sorted_unique: PH_JOIN_KEYS_SORTED_UNIQUE (the gated sorted fill + occupancy bitmap)"""
        self = cls.__new__(cls)
        self.ctx, self.h = ctx, vp()
        w = where_col.col() if isinstance(where_col, DevColumn) else where_col
        rc = lib().ph_join_build_where_ex(ctx.h, _cols(keys), i32(len(keys)), ctypes.byref(w), i32(where_op), ctypes.byref(where_k),
                                          sel, i64(n), i32(PH_JOIN_KEYS_SORTED_UNIQUE if sorted_unique else 0),
                                          i64(key_range[0]), i64(key_range[1]), ctypes.byref(self.h))
        if rc == PH_EUNSUPPORTED:
            return None
        check(rc)
        return self

    @property
    def kind(self):
        return lib().ph_join_kind(self.h).decode()

    def pairs_ordered(self):
        """ph_join_pairs_ordered: inner probes emit their pairs in probe-row order (every form except 'radix')"""
        return bool(lib().ph_join_pairs_ordered(self.h))

    def count(self):
        return int(lib().ph_join_count(self.h))

    def probe_inner(self, keys, sel, n, cap, defer=False):
        """defer (with Ctx.set_async_counts): the pair count comes back as the ctypes int64 itself, valid
        after Ctx.wait_counts()"""
        op = self.ctx.alloc(max(cap, 1) * 4)
        ob = self.ctx.alloc(max(cap, 1) * 4)
        m = i64()
        check(lib().ph_join_probe_inner(self.h, _cols(keys), sel, i64(n), op, ob, i64(cap), ctypes.byref(m)))
        return (m if defer else m.value), op, ob

    def probe_inner_where(self, keys, where_col, where_op, where_k, sel, n, cap):
        """Filter -> probe in one pass; returns None when the shape is not fused (caller runs
        filter_select + probe_inner)"""
        op = self.ctx.alloc(max(cap, 1) * 4)
        ob = self.ctx.alloc(max(cap, 1) * 4)
        m = i64()
        w = where_col.col() if isinstance(where_col, DevColumn) else where_col
        rc = lib().ph_join_probe_inner_where(self.h, _cols(keys), ctypes.byref(w), i32(where_op), ctypes.byref(where_k),
                                             sel, i64(n), op, ob, i64(cap), ctypes.byref(m))
        if rc == PH_EUNSUPPORTED:
            self.ctx.free(op)
            self.ctx.free(ob)
            return None
        check(rc)
        return m.value, op, ob

    def probe_inner_residual(self, keys, where_col, where_op, where_k, build_flags, sel, n, cap):
        """ph_join_probe_inner_residual: pairs whose build row has build_flags[row] != 0; where_col may be
        None. Returns None when the shape is not supported (direct tables only)."""
        op = self.ctx.alloc(max(cap, 1) * 4)
        ob = self.ctx.alloc(max(cap, 1) * 4)
        m = i64()
        w = None
        if where_col is not None:
            w = ctypes.byref(where_col.col() if isinstance(where_col, DevColumn) else where_col)
        rc = lib().ph_join_probe_inner_residual(self.h, _cols(keys), w, i32(where_op), ctypes.byref(where_k) if where_k is not None else None,
                                                build_flags, sel, i64(n), op, ob, i64(cap), ctypes.byref(m))
        if rc == PH_EUNSUPPORTED:
            self.ctx.free(op)
            self.ctx.free(ob)
            return None
        check(rc)
        return m.value, op, ob

    def probe_mark_where(self, keys, where_col, where_op, where_k, n):
        """ph_join_probe_mark_where: byte flags (filter && key present) or None when not supported"""
        f = self.ctx.alloc(max(n, 1) + 16)
        w = where_col.col() if isinstance(where_col, DevColumn) else where_col
        rc = lib().ph_join_probe_mark_where(self.h, _cols(keys), ctypes.byref(w), i32(where_op), ctypes.byref(where_k), i64(n), f)
        if rc == PH_EUNSUPPORTED:
            self.ctx.free(f)
            return None
        check(rc)
        return f

    def lookup(self, keys, sel, n, stats=None):
        """N:1 lookup probe: device int32[n] of matching build rows (-1 = none); stats: optional
        device int32[2] (misses, multi-matches), zeroed by the caller"""
        out = self.ctx.alloc(max(n, 1) * 4)
        check(lib().ph_join_lookup(self.h, _cols(keys), sel, i64(n), out, stats))
        return out

    def lookup_strict(self, keys, sel, n):
        """ph_join_lookup_strict: a miss / multi-match is a deferred PH_ECONSTRAINT error of the ctx"""
        out = self.ctx.alloc(max(n, 1) * 4)
        check(lib().ph_join_lookup_strict(self.h, _cols(keys), sel, i64(n), out))
        return out

    def probe_mark(self, keys, sel, n):
        f = self.ctx.alloc(max(n, 1))
        check(lib().ph_join_probe_mark(self.h, _cols(keys), sel, i64(n), f))
        return f

    def free(self):
        if self.h:
            lib().ph_join_free(self.h)
            self.h = None


def merge_lookup(ctx, build_key, n_build, probe_key, sel, n, strict=False):
    """ph_merge_lookup: N:1 lookup of probe keys that arrive in key order into a unique, ascending key column;
    device int32[n] of build rows (-1 = none)"""
    out = ctx.alloc(max(n, 1) * 4)
    b = build_key.col() if isinstance(build_key, DevColumn) else build_key
    p = probe_key.col() if isinstance(probe_key, DevColumn) else probe_key
    check(lib().ph_merge_lookup(ctx.h, ctypes.byref(b), i64(n_build), ctypes.byref(p), sel, i64(n), i32(1 if strict else 0), out))
    return out


def join_sorted_pairs(ctx, build_key, n_build, probe_key, sel, n, cap):
    """ph_join_sorted_pairs: inner pairs against a key column stored in ascending order with duplicates, no table; (probe rows, build rows, count)"""
    op, ob = ctx.alloc(max(cap, 1) * 4), ctx.alloc(max(cap, 1) * 4)
    b = build_key.col() if isinstance(build_key, DevColumn) else build_key
    p = probe_key.col() if isinstance(probe_key, DevColumn) else probe_key
    m = ctypes.c_int64(0)
    check(lib().ph_join_sorted_pairs(ctx.h, ctypes.byref(b), i64(n_build), ctypes.byref(p), sel, i64(n), op, ob, i64(cap), ctypes.byref(m)))
    return op, ob, m.value


def join_run_lookup(ctx, build_key2, n_build, key1_min, run_len, probe_keys, sel, n, strict=False):
    """ph_join_run_lookup: N:1 lookup on (first key, second key) into a table stored in runs of run_len by the first key; device int32[n] (-1 = none)"""
    out = ctx.alloc(max(n, 1) * 4)
    b = build_key2.col() if isinstance(build_key2, DevColumn) else build_key2
    arr = (Col * 2)(*[k.col() if isinstance(k, DevColumn) else k for k in probe_keys])
    check(lib().ph_join_run_lookup(ctx.h, ctypes.byref(b), i64(n_build), i64(key1_min), i32(run_len), arr, sel, i64(n), i32(1 if strict else 0), out))
    return out


def count_by_key(ctx, child_key, child_sel, n_child, key_min, key_range, parent_key, parent_sel, n_parent):
    """ph_count_by_key: child rows counted by key, every parent row reads its count; (device int64[n_parent], device validity bits: count > 0)"""
    out, val = ctx.alloc(max(n_parent, 1) * 8), ctx.alloc((n_parent + 63) // 64 * 8 + 64)
    c = child_key.col() if isinstance(child_key, DevColumn) else child_key
    p = parent_key.col() if isinstance(parent_key, DevColumn) else parent_key
    check(lib().ph_count_by_key(ctx.h, ctypes.byref(c), child_sel, i64(n_child), i64(key_min), i64(key_range), ctypes.byref(p), parent_sel, i64(n_parent), out, val))
    return out, val


def gather(ctx, col, idx_dev, n):
    c = col.col() if isinstance(col, DevColumn) else col
    w = {PH_CODE8: 1, PH_I32: 4, PH_DATE: 4, PH_F32: 4}.get(c.type, 8)
    out = ctx.alloc(max(n, 1) * w)
    check(lib().ph_gather(ctx.h, ctypes.byref(c), idx_dev, i64(n), out))
    return out


def gather_multi(ctx, cols, idx_dev, n):
    """ph_gather_multi: several columns through one row-id array in one pass -> list of device pointers"""
    cs = [c.col() if isinstance(c, DevColumn) else c for c in cols]
    w = [{PH_CODE8: 1, PH_I32: 4, PH_DATE: 4, PH_F32: 4}.get(c.type, 8) for c in cs]
    outs = [ctx.alloc(max(n, 1) * wi) for wi in w]
    arr = (Col * len(cs))(*cs)
    po = (vp * len(cs))(*[vp(o.value) for o in outs])
    check(lib().ph_gather_multi(ctx.h, i32(len(cs)), arr, idx_dev, i64(n), po))
    return outs


def partition(ctx, key, sel, n, nparts):
    c = key.col() if isinstance(key, DevColumn) else key
    counts = (i64 * nparts)()
    perm = ctx.alloc(max(n, 1) * 4)
    check(lib().ph_partition(ctx.h, ctypes.byref(c), sel, i64(n), i32(nparts), counts, perm))
    return [counts[p] for p in range(nparts)], perm


def partition_dev(ctx, key, sel, n, nparts):
    """ph_partition_dev: (device int64[nparts] counts, device permutation); no host round trip."""
    c = key.col() if isinstance(key, DevColumn) else key
    counts = ctx.alloc(max(nparts, 1) * 8)
    perm = ctx.alloc(max(n, 1) * 4)
    check(lib().ph_partition_dev(ctx.h, ctypes.byref(c), sel, i64(n), i32(nparts), counts, perm))
    return counts, perm


def read_reduce(ctx, dev, nbytes, out_words_dev, grid=256):
    check(lib().ph_dev_read_reduce(ctx.h, dev, i64(nbytes), out_words_dev, i32(grid)))


PH_PART_YEAR, PH_PART_MONTH, PH_PART_DAY = 1, 2, 3


def date_extract(ctx, part, col, sel, n):
    c = col.col() if isinstance(col, DevColumn) else col
    out = ctx.alloc(max(n, 1) * 4)
    check(lib().ph_date_extract(ctx.h, i32(part), ctypes.byref(c), sel, i64(n), out))
    return out


def substring(ctx, col, offset, length, sel, n):
    """ph_substring: (offsets dev int32[n+1], bytes dev, nbytes) of substring(col FROM offset FOR length)"""
    c = col.col() if isinstance(col, DevColumn) else col
    cap = max(int(c.aux_bytes), 1) + 64
    off = ctx.alloc((max(n, 0) + 1) * 4)
    out = ctx.alloc(cap)
    nb = i64()
    check(lib().ph_substring(ctx.h, ctypes.byref(c), i64(offset), i64(length), sel, i64(n), off, out, i64(cap), ctypes.byref(nb)))
    return off, out, nb.value


def substring_range(slen, offset, length):
    """ph_substring_range (host only): the (start, end) ph_substring takes from a row of slen bytes, or None when it takes nothing"""
    s, e = i64(), i64()
    some = lib().ph_substring_range(i64(slen), i64(offset), i64(length), ctypes.byref(s), ctypes.byref(e))
    return (s.value, e.value) if some else None


def cross_pairs(ctx, n_left, n_right):
    tot = max(n_left * n_right, 1)
    ol, orr = ctx.alloc(tot * 4), ctx.alloc(tot * 4)
    check(lib().ph_cross_pairs(ctx.h, i64(n_left), i64(n_right), ol, orr))
    return ol, orr


# ---------------------------------------------------------------- resident plans (ph_plan_*)

PH_PN_SCAN, PH_PN_FILTER, PH_PN_JOIN, PH_PN_PROJECT, PH_PN_AGG = range(1, 6)
PH_JT_INNER, PH_JT_SEMI, PH_JT_ANTI, PH_JT_LEFT = 1, 2, 3, 4
PH_PE_COL, PH_PE_DECIMAL, PH_PE_YEAR = 1, 2, 3
PH_STAT_ASCENDING, PH_STAT_STRICT, PH_STAT_DECLARED_UNIQUE = 1, 2, 4


PH_PE_CASE = 4
PH_PE_SUBSTR = 5
PH_PE_FLOAT = 6
PH_X_DIV, PH_X_LT, PH_X_LE, PH_X_GT, PH_X_GE = 6, 7, 8, 9, 10
PH_B_CMP, PH_B_AND, PH_B_OR = 1, 2, 3
PH_COLREF = 9


class Bool(ctypes.Structure):
    _fields_ = [("kind", i32), ("col", i32), ("op", i32), ("k", Const), ("first_child", i32), ("nchildren", i32)]


class PlanExpr(ctypes.Structure):
    _fields_ = [("kind", i32), ("col", i32), ("nprog", i32), ("prog", Rpn * 12), ("nwhen", i32), ("when", ctypes.POINTER(Bool)),
                ("nelse", i32), ("else_prog", Rpn * 12), ("result_int", i32), ("sub_offset", i64), ("sub_length", i64), ("float_wide", i32)]


def bool_tree(expr):
    """Nested tuples -> a flat ph_bool array (node 0 = root, children of a node contiguous):
         ("cmp", col, op, Const) | ("colcmp", col, op, other_col) | ("and", child, ...) | ("or", child, ...)
         ("in", col, [Const, ...])  =  OR of '=' comparisons, as the reference binds IN lists"""
    nodes = []

    def norm(e):
        if e[0] == "in":
            return ("or",) + tuple(("cmp", e[1], PH_EQ, k) for k in e[2])
        return e

    def emit(e, at):
        e = norm(e)
        b = Bool()
        if e[0] == "cmp":
            b.kind, b.col, b.op, b.k = PH_B_CMP, e[1], e[2], e[3]
        elif e[0] == "colcmp":
            b.kind, b.col, b.op = PH_B_CMP, e[1], e[2]
            b.k = const(PH_COLREF, i=e[3])
        else:
            kids = e[1:]
            b.kind = PH_B_AND if e[0] == "and" else PH_B_OR
            b.first_child, b.nchildren = len(nodes), len(kids)
            base = len(nodes)
            nodes.extend([None] * len(kids))
            for j, kid in enumerate(kids):
                emit(kid, base + j)
        nodes[at] = b

    nodes.append(None)
    emit(expr, 0)
    return (Bool * len(nodes))(*nodes)


class PlanAgg(ctypes.Structure):
    _fields_ = [("kind", i32), ("arg", PlanExpr)]


class PlanNode(ctypes.Structure):
    _fields_ = [("kind", i32), ("child", i32 * 2), ("table", vp), ("ncols", i32), ("cols", ctypes.POINTER(i32)),
                ("npreds", i32), ("preds", ctypes.POINTER(Pred)), ("nbools", i32), ("bools", ctypes.POINTER(Bool)),
                ("join_type", i32), ("nkeys", i32),
                ("probe_keys", ctypes.POINTER(i32)), ("build_keys", ctypes.POINTER(i32)), ("nout", i32), ("out", ctypes.POINTER(i32)),
                ("nexprs", i32), ("exprs", ctypes.POINTER(PlanExpr)), ("ngroups", i32), ("groups", ctypes.POINTER(PlanExpr)),
                ("naggs", i32), ("aggs", ctypes.POINTER(PlanAgg))]


def pe_col(c):
    e = PlanExpr()
    e.kind, e.col = PH_PE_COL, c
    return e


def pe_year(c):
    e = PlanExpr()
    e.kind, e.col = PH_PE_YEAR, c
    return e


def X_F32(v):
    """a FLOAT literal of a PH_PE_FLOAT program (its float32 bits)"""
    return (PH_X_CONST, -1, int(np.float32(v).view(np.uint32)), 0)


def X_OP(op):
    return (op, -1, 0, 0)


def pe_float(prog, truth=True, wide=False):
    """FLOAT (wide=False) / DOUBLE arithmetic ending — truth=True — in a comparison whose 1 / 0 a Filter above tests (ph_float_eval)"""
    e = PlanExpr()
    e.kind, e.col, e.nprog, e.result_int, e.float_wide = PH_PE_FLOAT, -1, len(prog), 1 if truth else 0, 1 if wide else 0
    for i, r in enumerate(prog):
        e.prog[i] = Rpn(*r)
    return e


def pe_substr(c, offset, length):
    """substring(<VARCHAR column c> FROM offset FOR length): a VARCHAR computed in the plan (filter by = / <> / IN, group key)"""
    e = PlanExpr()
    e.kind, e.col, e.sub_offset, e.sub_length = PH_PE_SUBSTR, c, offset, length
    return e


def pe_dec(prog):
    e = PlanExpr()
    e.kind, e.col, e.nprog = PH_PE_DECIMAL, -1, len(prog)
    for j, x in enumerate(prog):
        e.prog[j] = Rpn(*x)
    return e


def pe_case(when, then_prog, else_prog, result_int=False, keep=None):
    """CASE WHEN <when: bool_tree()> THEN <then_prog> ELSE <else_prog> END; keep: a list the WHEN array is appended to
    (it must outlive Plan.create)"""
    e = PlanExpr()
    e.kind, e.col, e.nprog, e.nelse, e.result_int = PH_PE_CASE, -1, len(then_prog), len(else_prog), 1 if result_int else 0
    for j, x in enumerate(then_prog):
        e.prog[j] = Rpn(*x)
    for j, x in enumerate(else_prog):
        e.else_prog[j] = Rpn(*x)
    e.nwhen, e.when = len(when), when
    if keep is not None:
        keep.append(when)
    return e


def _i32arr(v):
    return (i32 * max(len(v), 1))(*v)


class Plan:
    """ph_plan: an operator subtree Agg <- [Project] <- Join* <- Scan over resident tables, described node by node
    (children first, the aggregate last) and lowered inside the library from the tables' statistics."""

    def __init__(self, ctx):
        self.ctx, self.nodes, self._keep, self.h = ctx, [], [], None

    def _add(self, n):
        self.nodes.append(n)
        return len(self.nodes) - 1

    def scan(self, table, cols, preds=(), bools=None):
        """preds: simple conjuncts over TABLE columns; bools: one more conjunct of any shape (bool_tree())"""
        n = PlanNode()
        n.kind, n.child[0], n.child[1] = PH_PN_SCAN, -1, -1
        n.table = table.h
        ca, pa = _i32arr(cols), (Pred * max(len(preds), 1))(*preds)
        self._keep += [ca, pa, table, bools]
        n.ncols, n.cols = len(cols), ca
        n.npreds, n.preds = len(preds), pa
        if bools is not None:
            n.nbools, n.bools = len(bools), bools
        return self._add(n)

    def filter(self, child, preds=(), bools=None):
        n = PlanNode()
        n.kind, n.child[0], n.child[1] = PH_PN_FILTER, child, -1
        pa = (Pred * max(len(preds), 1))(*preds)
        self._keep += [pa, bools]
        n.npreds, n.preds = len(preds), pa
        if bools is not None:
            n.nbools, n.bools = len(bools), bools
        return self._add(n)

    def join(self, probe, build, probe_keys, build_keys, out, join_type=PH_JT_INNER, residual=None):
        """residual: a bool_tree over [probe columns | build columns] — the join's non-equi condition (INNER keeps the pairs that satisfy it,
        SEMI / ANTI the probe rows with / without such a pair)"""
        n = PlanNode()
        n.kind, n.child[0], n.child[1] = PH_PN_JOIN, probe, build
        pk, bk, oa = _i32arr(probe_keys), _i32arr(build_keys), _i32arr(out)
        self._keep += [pk, bk, oa, residual]
        if residual is not None:
            n.nbools, n.bools = len(residual), residual
        n.join_type, n.nkeys, n.probe_keys, n.build_keys = join_type, len(probe_keys), pk, bk
        n.nout, n.out = len(out), oa
        return self._add(n)

    def project(self, child, exprs):
        n = PlanNode()
        n.kind, n.child[0], n.child[1] = PH_PN_PROJECT, child, -1
        ea = (PlanExpr * len(exprs))(*exprs)
        self._keep.append(ea)
        n.nexprs, n.exprs = len(exprs), ea
        return self._add(n)

    def agg(self, child, groups, aggs):
        """aggs: list of (ph_aggkind, PlanExpr or None)"""
        n = PlanNode()
        n.kind, n.child[0], n.child[1] = PH_PN_AGG, child, -1
        ga = (PlanExpr * max(len(groups), 1))(*groups)
        aa = (PlanAgg * len(aggs))()
        for j, (kind, arg) in enumerate(aggs):
            aa[j].kind = kind
            if arg is not None:
                aa[j].arg = arg
        self._keep += [ga, aa]
        n.ngroups, n.groups, n.naggs, n.aggs = len(groups), ga, len(aggs), aa
        return self._add(n)

    def create(self):
        arr = (PlanNode * len(self.nodes))(*self.nodes)
        self.h = vp()
        check(lib().ph_plan_create(self.ctx.h, arr, i32(len(self.nodes)), ctypes.byref(self.h)))
        return self

    def set_having(self, conjuncts):
        """conjuncts: hip.pred(result column, op, const) over the root's aggregate columns; raises PlanHipError(PH_EUNSUPPORTED) when the
        plan cannot apply them on the device (the caller filters the fetched groups)"""
        arr = (Pred * max(len(conjuncts), 1))(*conjuncts)
        self._keep.append(arr)
        check(lib().ph_plan_set_having(self.h, i32(len(conjuncts)), arr))

    def set_comm(self, comm, broadcast_rows=None):
        """multi-rank execution (ph_plan_set_comm): comm = a Comm (RCCL or the in-process transport); every rank creates, runs and fetches the same
        plan over its shard and receives the complete result"""
        check(lib().ph_plan_set_comm(self.h, comm.h if comm is not None else None))
        if broadcast_rows is not None:
            check(lib().ph_plan_set_broadcast_rows(self.h, i64(broadcast_rows)))

    def set_topk(self, agg_index, k, descending=True):
        check(lib().ph_plan_set_topk(self.h, i32(agg_index), i32(1 if descending else 0), i64(k)))

    def set_rows_topk(self, col, k, descending=True):
        """ph_plan_set_rows_topk: a join-rooted plan under ORDER BY <column col> [DESC] LIMIT k returns only the rows that can be among the first k"""
        check(lib().ph_plan_set_rows_topk(self.h, i32(col), i32(1 if descending else 0), i64(k)))

    def run(self):
        check(lib().ph_plan_run(self.h))

    def fetch(self):
        rp = ctypes.POINTER(AggResult)()
        check(lib().ph_plan_fetch(self.h, ctypes.byref(rp)))
        return _result(rp)

    def fetch_rows(self):
        """rows of a plan whose root is a join / filter / project (ph_plan_fetch_rows): {"nrows", "types", "scales", "columns"} — a fixed-width
        column is an int64 numpy array, a VARCHAR column a list of str"""
        rp = ctypes.POINTER(RowsResult)()
        check(lib().ph_plan_fetch_rows(self.h, ctypes.byref(rp)))
        r = rp.contents
        n, cols = r.nrows, []
        for c in range(r.ncols):
            if r.values[c]:
                cols.append(np.ctypeslib.as_array(r.values[c], shape=(max(n, 1),))[:n].copy())
            else:
                off = np.ctypeslib.as_array(r.offsets[c], shape=(n + 1,))
                raw = ctypes.string_at(r.bytes[c], int(off[n])) if n else b""
                cols.append([raw[off[i]:off[i + 1]].decode() for i in range(n)])
        out = dict(nrows=n, types=[r.type[c] for c in range(r.ncols)], scales=[r.scale[c] for c in range(r.ncols)], columns=cols)
        lib().ph_rows_result_free(rp)
        return out

    def explain(self):
        lib().ph_plan_explain.restype = ctypes.c_char_p
        return lib().ph_plan_explain(self.h).decode()

    def free(self):
        if self.h:
            lib().ph_plan_free(self.h)
            self.h = None


def table_col_stats(table, c):
    f = i32()
    check(lib().ph_table_col_stats(table.h, i32(c), ctypes.byref(f)))
    return f.value


def table_declare_unique(table, cols):
    check(lib().ph_table_declare_unique(table.h, i32(len(cols)), _i32arr(cols)))


def table_col_range_of(table, c):
    mn, mx = i64(), i64()
    check(lib().ph_table_col_range(table.h, i32(c), ctypes.byref(mn), ctypes.byref(mx)))
    return mn.value, mx.value


class StrDict:
    """ph_strdict: VARCHAR keys as int32 codes (the representative row of each distinct string)"""

    def __init__(self, ctx, col, sel, n):
        self.ctx, self.h = ctx, vp()
        c = col.col() if isinstance(col, DevColumn) else col
        self.codes = ctx.alloc(max(n, 1) * 4)
        check(lib().ph_strdict_build(ctx.h, ctypes.byref(c), sel, i64(n), self.codes, ctypes.byref(self.h)))
        self._keep = col

    def lookup(self, col, sel, n):
        c = col.col() if isinstance(col, DevColumn) else col
        out = self.ctx.alloc(max(n, 1) * 4)
        check(lib().ph_strdict_lookup(self.h, ctypes.byref(c), sel, i64(n), out))
        return out

    def free(self):
        if self.h:
            lib().ph_strdict_free(self.h)
            self.h = None
            self.ctx.free(self.codes)


def plan_key_info(plan, k):
    """(type, scale, table handle or None, column) of group key k of a ph_plan's last run"""
    t, s, tab, c = i32(), i32(), vp(), i32()
    check(lib().ph_plan_key_info(plan.h, i32(k), ctypes.byref(t), ctypes.byref(s), ctypes.byref(tab), ctypes.byref(c)))
    return t.value, s.value, tab.value, c.value


def table_strings(ctx, table, c, rows):
    """strings of the given rows of PH_STR column c (ph_table_strings); `table` is a Table or the raw handle plan_key_info returned"""
    return [b.decode() for b in table_strings_bytes(ctx, table, c, rows)]


def table_strings_bytes(ctx, table, c, rows):
    """table_strings without the decoding: the rows' raw bytes (a VARCHAR is any byte string)"""
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    n = len(rows)
    off = np.zeros(n + 1, np.int32)
    cap = 1 << 20
    buf = ctypes.create_string_buffer(cap)
    check(lib().ph_table_strings(ctx.h, table.h if hasattr(table, "h") else vp(table), i32(c), vp(rows.ctypes.data), i64(n), vp(off.ctypes.data), buf, i64(cap)))
    raw = buf.raw
    return [raw[off[i]:off[i + 1]] for i in range(n)]


class LocalGroup:
    """the rendezvous object of the in-process transport (ph_local_group): the ranks are threads of this process"""

    def __init__(self, nranks):
        self.h, self.nranks = vp(), nranks
        check(lib().ph_local_group_create(i32(nranks), ctypes.byref(self.h)))

    def free(self):
        if self.h:
            lib().ph_local_group_free(self.h)
            self.h = None


class Comm:
    """ph_comm over the in-process transport (group = LocalGroup) — the RCCL form lives in plan_amd.dist.RcclGroup"""

    def __init__(self, ctx, group, rank):
        self.h, self.ctx, self.rank, self.nranks = vp(), ctx, rank, group.nranks
        check(lib().ph_comm_init_local(ctx.h, group.h, i32(rank), ctypes.byref(self.h)))

    def close(self):
        if self.h:
            lib().ph_comm_destroy(self.h)
            self.h = None
