"""ph_table_concat on the device: every array of the concatenated table against the table ph_table_create builds over the numpy
concatenation of the pieces' host arrays, on the same context — type, scale, dictionary, presence and bytes of the validity bitmap up to
padded / 8, data up to padded, offsets and bytes, range, order statistics, run length, narrowed copies. The whole table's dictionary is
built HERE (the byte-sorted union, or the identical dictionary), so the reference is defined without the code under test. Then part
handling, every refusal (code, a word of the message, the context usable afterwards) and TPC-H lineitem at SF0.01 in three pieces."""
import numpy as np
import pytest

from plan_amd import hip, loader, queries

pytestmark = pytest.mark.gpu

ROW_PAD = 8192
I32, I64, DATE, DEC64, CODE8, F32, F64, STR = (hip.PH_I32, hip.PH_I64, hip.PH_DATE, hip.PH_DEC64, hip.PH_CODE8, hip.PH_F32, hip.PH_F64, hip.PH_STR)
ALIGN_ROWS = [1, 7, 8, 9, 31, 33, 63, 64, 65, 0, 2047, 8192, 8193]


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


def outcome(f, *a):
    """the call's value, or the code it refuses with (a VARCHAR column has no range statistics, in either table)"""
    try:
        return f(*a)
    except hip.PlanHipError as e:
        return ("refused", e.code)


def assert_tables_equal(ctx, t, ref, n):
    """every device array of t against ref's (a local copy of tests/test_gpu_parquet_load.py's)"""
    assert t.nrows == ref.nrows == n and t.ncols == ref.ncols
    padded = (n + ROW_PAD - 1) // ROW_PAD * ROW_PAD
    for k in range(t.ncols):
        a, b = t.col(k), ref.col(k)
        assert (a.type, a.scale) == (b.type, b.scale), k
        assert t.dicts[k] == ref.dicts[k], k
        if n == 0:
            continue
        assert bool(a.validity) == bool(b.validity), k
        if a.validity:
            assert ctx.download(hip.vp(a.validity), np.uint8, padded // 8).tobytes() == ctx.download(hip.vp(b.validity), np.uint8, padded // 8).tobytes(), k
        if a.type == hip.PH_STR:
            oa, ob = ctx.download(hip.vp(a.data), np.int32, n + 1), ctx.download(hip.vp(b.data), np.int32, n + 1)
            assert np.array_equal(oa, ob) and a.aux_bytes == b.aux_bytes == oa[n], k
            if a.aux_bytes:
                assert ctx.download(hip.vp(a.aux), np.uint8, int(a.aux_bytes)).tobytes() == ctx.download(hip.vp(b.aux), np.uint8, int(b.aux_bytes)).tobytes(), k
        else:
            dt = hip.NP_TYPES[a.type]
            assert ctx.download(hip.vp(a.data), dt, padded).tobytes() == ctx.download(hip.vp(b.data), dt, padded).tobytes(), k
        assert outcome(hip.table_col_range_of, t, k) == outcome(hip.table_col_range_of, ref, k), k
        assert outcome(hip.table_col_stats, t, k) == outcome(hip.table_col_stats, ref, k), k
        assert outcome(t.col_run_len, k) == outcome(ref.col_run_len, k), k
        assert outcome(t.col_narrow, k) == outcome(ref.col_narrow, k), k
    assert t.narrow_bytes() == ref.narrow_bytes()


# ---------------------------------------------------------------- host columns and their concatenation (the reference's input)

def col(typ, data=None, scale=0, valid=None, dic=None, off=None, aux=None):
    """one piece's column on the host. valid: bool per row or None. CODE8: dic = list of str. STR: off (int32, n + 1) and aux (uint8)."""
    return dict(typ=typ, data=data, scale=scale, valid=valid, dic=dic, off=off, aux=aux)


def dense_strs(values):
    lens = np.array([len(v) for v in values], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return off, np.frombuffer(b"".join(values) + b"\0", np.uint8)[:int(off[-1])]


def spec_of(c, n):
    val = None if c["valid"] is None else np.packbits(np.asarray(c["valid"], np.uint8), bitorder="little")
    if val is not None and len(val) == 0:
        val = np.zeros(1, np.uint8)
    if c["typ"] == STR:
        return (STR, np.asarray(c["off"], np.int32), 0, val, None, np.ascontiguousarray(c["aux"], np.uint8))
    return (c["typ"], np.ascontiguousarray(c["data"], hip.NP_TYPES[c["typ"]]), c["scale"], val, c["dic"], None)


def rows_as_bytes(c, n):
    """a VARCHAR piece's rows: a code's dictionary entry (a NULL row: the empty string), or the bytes between a row's offsets"""
    if c["typ"] == STR:
        raw = bytes(np.asarray(c["aux"], np.uint8))
        return [raw[c["off"][i]:c["off"][i + 1]] for i in range(n)]
    ok = np.ones(n, bool) if c["valid"] is None else np.asarray(c["valid"], bool)
    return [c["dic"][int(c["data"][i])].encode() if ok[i] else b"" for i in range(n)]


def whole_col(cs, rows):
    """what ph_table_concat's rules make of one column's pieces, as a host column over all rows"""
    total = sum(rows)
    valid = None
    if any(c["valid"] is not None for c in cs):
        valid = np.concatenate([np.ones(n, bool) if c["valid"] is None else np.asarray(c["valid"], bool) for c, n in zip(cs, rows)])
    typ = cs[0]["typ"]
    if typ not in (CODE8, STR):
        dt = hip.NP_TYPES[typ]
        return col(typ, np.concatenate([np.asarray(c["data"], dt)[:n] for c, n in zip(cs, rows)]), cs[0]["scale"], valid)
    if all(c["typ"] == CODE8 for c in cs):
        if all(c["dic"] == cs[0]["dic"] for c in cs):                      # identical: kept, codes untouched
            return col(CODE8, np.concatenate([np.asarray(c["data"], np.uint8)[:n] for c, n in zip(cs, rows)]), 0, valid, list(cs[0]["dic"]))
        merged = sorted(set(e.encode() for c in cs for e in c["dic"]))     # bytes sort as unsigned bytes
        if len(merged) <= 256:
            where = {e: k for k, e in enumerate(merged)}
            codes = []
            for c, n in zip(cs, rows):
                ok = np.ones(n, bool) if c["valid"] is None else np.asarray(c["valid"], bool)
                codes += [where[c["dic"][int(c["data"][i])].encode()] if ok[i] else 0 for i in range(n)]
            return col(CODE8, np.array(codes, np.uint8), 0, valid, [e.decode() for e in merged])
    values = [v for c, n in zip(cs, rows) for v in rows_as_bytes(c, n)]
    assert len(values) == total
    off, aux = dense_strs(values)
    return col(STR, valid=valid, off=off, aux=aux)


def concat_and_compare(ctx, pieces, rows, on=None, keep=False):
    """pieces: per piece a list of columns; -> the expected columns. on: per piece the context it is created on (default ctx)"""
    tables = [hip.Table((on or {}).get(k, ctx), [spec_of(c, n) for c in p], n) for k, (p, n) in enumerate(zip(pieces, rows))]
    total = sum(rows)
    want = [whole_col([p[k] for p in pieces], rows) for k in range(len(pieces[0]))]
    ref = hip.Table(ctx, [spec_of(c, total) for c in want], total)
    ref.ncols = len(want)
    loader._attach_dicts(ref)
    t = None
    try:
        before = [snapshot(ctx, x) for x in tables]
        t = loader.concat_tables(ctx, tables)
        assert_tables_equal(ctx, t, ref, total)
        assert [snapshot(ctx, x) for x in tables] == before               # the parts download unchanged afterwards
        return want
    finally:
        for x in tables + [ref] + ([t] if t is not None and not keep else []):
            x.free()


def snapshot(ctx, t):
    """the bytes of a table's rows: data (offsets and bytes for VARCHAR) and validity, per column"""
    n, out = t.nrows, []
    for k in range(t.ncols):
        c = t.col(k)
        if c.type == STR:
            off = ctx.download(hip.vp(c.data), np.int32, n + 1)
            out.append((off.tobytes(), ctx.download(hip.vp(c.aux), np.uint8, int(c.aux_bytes)).tobytes() if c.aux_bytes else b""))
        else:
            out.append((ctx.download(hip.vp(c.data), hip.NP_TYPES[c.type], max(n, 1)).tobytes(),))
        if c.validity:
            out.append(ctx.download(hip.vp(c.validity), np.uint8, (n + 7) // 8 or 1).tobytes())
    return out


WORDS = ["w%03d" % i for i in range(300)]


def random_piece(rng, n, validity=False, str_values=None, dic=None):
    """one column of every type; CODE8 over `dic`, STR over str_values"""
    dic = dic or WORDS[:40]
    sv = str_values or [w.encode() * 2 for w in WORDS]
    picks = [sv[int(i)] for i in rng.integers(0, len(sv), n)]
    v = (lambda: rng.integers(0, 4, n) > 0) if validity else (lambda: None)
    off, aux = dense_strs(picks)
    return [col(I32, rng.integers(-2**31, 2**31 - 1, n).astype(np.int32), valid=v()),
            col(I64, rng.integers(-2**62, 2**62, n), valid=None),
            col(DATE, rng.integers(0, 20000, n).astype(np.int32)),
            col(DEC64, rng.integers(-10**12, 10**12, n), scale=2),
            col(F32, rng.standard_normal(n).astype(np.float32)),
            col(F64, rng.standard_normal(n)),
            col(CODE8, rng.integers(0, len(dic), n).astype(np.uint8), dic=list(dic), valid=None),
            col(STR, off=off, aux=aux)]


# ---------------------------------------------------------------- alignment, every type, validity

def test_every_type_at_every_alignment(ctx):
    rng = np.random.default_rng(7)
    pieces = [random_piece(rng, n) for n in ALIGN_ROWS]
    want = concat_and_compare(ctx, pieces, ALIGN_ROWS)
    assert [c["typ"] for c in want] == [I32, I64, DATE, DEC64, F32, F64, CODE8, STR]


def null_columns(rng, n, bitmap):
    """a fixed-width, a CODE8 and a STR column; bitmap: the piece has validity bitmaps. NULL rows hold code 0 / the empty string."""
    ok = rng.integers(0, 3, n) > 0 if bitmap else np.ones(n, bool)
    dic = ["zz", "b", "mm"] if n % 2 else ["b", "c"]                    # dictionaries differ: the codes are rewritten; dict[0] is not empty
    codes = np.where(ok, rng.integers(0, len(dic), n), 0).astype(np.uint8)
    off, aux = dense_strs([WORDS[int(i)].encode() if o else b"" for i, o in zip(rng.integers(0, 300, n), ok)])
    v = (lambda: ok.copy()) if bitmap else (lambda: None)
    return [col(I64, rng.integers(-50, 50, n), valid=v()), col(CODE8, codes, dic=dic, valid=v()), col(STR, off=off, aux=aux, valid=v())]


def test_validity_some_pieces_with_a_bitmap_some_without(ctx):
    rng = np.random.default_rng(8)
    rows = [5, 31, 0, 64, 1, 1, 1, 33, 700, 9000, 3]
    with_bitmap = [True, False, True, True, False, True, False, False, True, False, True]
    want = concat_and_compare(ctx, [null_columns(rng, n, b) for n, b in zip(rows, with_bitmap)], rows)
    assert all(c["valid"] is not None for c in want) and want[1]["typ"] == CODE8 and want[1]["dic"] == ["b", "c", "mm", "zz"]


def test_no_piece_with_a_bitmap_gives_none(ctx):
    rng = np.random.default_rng(9)
    rows = [40, 3, 8200]
    want = concat_and_compare(ctx, [null_columns(rng, n, False) for n in rows], rows)
    assert all(c["valid"] is None for c in want)


# ---------------------------------------------------------------- CODE8 forms

def code_piece(rng, n, dic, nulls=False):
    ok = rng.integers(0, 2, n) > 0 if nulls else None
    codes = rng.integers(0, len(dic), n).astype(np.uint8)
    if nulls:
        codes[~ok] = 0
    return [col(CODE8, codes, dic=list(dic), valid=ok)]


def test_identical_unsorted_dictionaries_are_kept(ctx):
    rng = np.random.default_rng(10)
    dic = ["pear", "apple", "zoo", "", "mango"]
    rows = [100, 7, 9000]
    want = concat_and_compare(ctx, [code_piece(rng, n, dic) for n in rows], rows)
    assert want[0]["typ"] == CODE8 and want[0]["dic"] == dic


def test_different_dictionaries_are_merged_in_byte_order(ctx):
    rng = np.random.default_rng(11)
    dics = [["b", "a"], ["a", "c", "b"], ["é", "z", "a"], ["dup", "q", "dup"]]       # bytes >= 0x80 after 'z'; a duplicate inside one part
    rows = [33, 8200, 65, 40]
    want = concat_and_compare(ctx, [code_piece(rng, n, d) for n, d in zip(rows, dics)], rows)
    assert want[0]["typ"] == CODE8 and want[0]["dic"] == ["a", "b", "c", "dup", "q", "z", "é"]


def test_union_of_exactly_256_stays_code8_and_257_becomes_str(ctx):
    rng = np.random.default_rng(12)
    rows = [300, 9000, 77]
    for last, typ in ((256, CODE8), (257, STR)):
        dics = [WORDS[:200], WORDS[100:last][::-1], WORDS[50:60]]
        want = concat_and_compare(ctx, [code_piece(rng, n, d) for n, d in zip(rows, dics)], rows)
        assert want[0]["typ"] == typ
    assert len(want[0]["off"]) == sum(rows) + 1 and want[0]["off"][-1] == 4 * sum(rows)


def test_null_rows_keep_code_0_and_are_empty_in_the_str_fallback(ctx):
    rng = np.random.default_rng(13)
    rows = [50, 8200, 9]
    # stored code 0 under NULL while dict[0] is not empty and is NOT the merged dictionary's first entry
    want = concat_and_compare(ctx, [code_piece(rng, n, d, nulls=True) for n, d in zip(rows, (["m", "a"], ["z", "b"], ["q"]))], rows)
    assert want[0]["typ"] == CODE8 and want[0]["dic"] == ["a", "b", "m", "q", "z"]
    assert np.all(want[0]["data"][~want[0]["valid"]] == 0) and not np.all(want[0]["valid"])
    dics = [WORDS[:200], WORDS[100:257], WORDS[5:6]]
    want = concat_and_compare(ctx, [code_piece(rng, n, d, nulls=True) for n, d in zip(rows, dics)], rows)
    lens = np.diff(want[0]["off"])
    assert want[0]["typ"] == STR and np.all(lens[~want[0]["valid"]] == 0) and np.all(lens[want[0]["valid"]] == 4)


# ---------------------------------------------------------------- STR forms

def test_str_parts_mixed_with_code_parts(ctx):
    rng = np.random.default_rng(14)
    rows = [40, 8200, 0, 300, 5]
    pieces = []
    for k, n in enumerate(rows):
        if k % 2:
            pieces.append(code_piece(rng, n, ["alpha", "", "be"], nulls=(k == 1)))
        else:
            off, aux = dense_strs([WORDS[int(i)].encode() * int(i % 3) for i in rng.integers(0, 300, n)])
            pieces.append([col(STR, off=off, aux=aux)])
    want = concat_and_compare(ctx, pieces, rows)
    assert want[0]["typ"] == STR and want[0]["valid"] is not None


def test_str_part_whose_offsets_start_above_0_with_gaps(ctx):
    rng = np.random.default_rng(15)
    vals = [WORDS[int(i)].encode() for i in rng.integers(0, 300, 70)]
    off = []
    blob, at = bytearray(b"#" * 11), 11                                 # 11 unused bytes in front; rows are dense behind them
    for v in vals:
        off.append(at)
        blob += v
        at += len(v)
    off.append(at)
    shifted = col(STR, off=np.array(off, np.int32), aux=np.frombuffer(bytes(blob) + b"!!!", np.uint8))
    d_off, d_aux = dense_strs([b"x", b"", b"yy"])
    empty_off, _unused = dense_strs([b""] * 9)
    pieces = [[col(STR, off=d_off, aux=d_aux)], [shifted], [col(STR, off=empty_off, aux=np.zeros(1, np.uint8))]]
    want = concat_and_compare(ctx, pieces, [3, 70, 9])
    assert want[0]["off"][0] == 0 and want[0]["off"][-1] == 3 + sum(len(v) for v in vals)


def test_str_part_of_only_empty_strings(ctx):
    off, _aux = dense_strs([b""] * 100)
    want = concat_and_compare(ctx, [[col(STR, off=off, aux=np.zeros(1, np.uint8))], [col(STR, off=off[:8], aux=np.zeros(1, np.uint8))]], [100, 7])
    assert want[0]["off"][-1] == 0


# ---------------------------------------------------------------- statistics

def stats_of(ctx, pieces, rows):
    tables = [hip.Table(ctx, [spec_of(c, n) for c in p], n) for p, n in zip(pieces, rows)]
    t = loader.concat_tables(ctx, tables)
    try:
        return hip.table_col_stats(t, 0), t.col_run_len(0), t.col_narrow(0), t.col_range(0)
    finally:
        for x in tables + [t]:
            x.free()


def test_order_statistics_are_the_concatenations_own(ctx):
    a, b = np.arange(0, 5000, dtype=np.int64), np.arange(5000, 9000, dtype=np.int64)
    for first, second, asc in ((a, b, True), (b, a, False)):
        pieces, rows = [[col(I64, first)], [col(I64, second)]], [len(first), len(second)]
        concat_and_compare(ctx, pieces, rows)
        flags = stats_of(ctx, pieces, rows)[0]
        assert bool(flags & hip.PH_STAT_ASCENDING) == asc and bool(flags & hip.PH_STAT_STRICT) == asc


def test_run_length_column_split_inside_a_run_and_at_a_boundary(ctx):
    v = (np.arange(8800) // 4 + 17).astype(np.int32)
    for cut in (4402, 4400):
        pieces, rows = [[col(I32, v[:cut])], [col(I32, v[cut:])]], [cut, len(v) - cut]
        concat_and_compare(ctx, pieces, rows)
        assert stats_of(ctx, pieces, rows)[1] == 4


def test_pieces_narrow_to_uint8_the_whole_to_uint16(ctx):
    rng = np.random.default_rng(16)
    a, b = rng.integers(0, 200, 500).astype(np.int32), rng.integers(300, 500, 9000).astype(np.int32)
    a[0], b[-1] = 0, 499
    pa_, pb = hip.Table(ctx, [spec_of(col(I32, a), 500)], 500), hip.Table(ctx, [spec_of(col(I32, b), 9000)], 9000)
    try:
        assert pa_.col_narrow(0)[0] == 1 and pb.col_narrow(0)[0] == 1
    finally:
        pa_.free()
        pb.free()
    pieces, rows = [[col(I32, a)], [col(I32, b)]], [500, 9000]
    concat_and_compare(ctx, pieces, rows)
    assert stats_of(ctx, pieces, rows)[2] == (2, 0)


# ---------------------------------------------------------------- part handling

def test_one_part_gives_a_distinct_table(ctx):
    rng = np.random.default_rng(17)
    piece = random_piece(rng, 1000)
    src = hip.Table(ctx, [spec_of(c, 1000) for c in piece], 1000)
    t = loader.concat_tables(ctx, [src])
    try:
        assert t.h.value != src.h.value and all(t.col(k).data != src.col(k).data for k in range(t.ncols))
        src.ncols = len(piece)
        loader._attach_dicts(src)
        assert_tables_equal(ctx, t, src, 1000)
    finally:
        src.free()
    try:                                                                # the copy outlives its source
        assert ctx.download(hip.vp(t.col(0).data), np.int32, 1000).tobytes() == piece[0]["data"].tobytes()
    finally:
        t.free()


def test_the_same_table_named_twice(ctx):
    rng = np.random.default_rng(18)
    piece = random_piece(rng, 777, validity=True)
    src = hip.Table(ctx, [spec_of(c, 777) for c in piece], 777)
    want = [whole_col([c, c], [777, 777]) for c in piece]
    ref = hip.Table(ctx, [spec_of(c, 1554) for c in want], 1554)
    ref.ncols = len(want)
    loader._attach_dicts(ref)
    t = loader.concat_tables(ctx, [src, src])
    try:
        assert_tables_equal(ctx, t, ref, 1554)
    finally:
        for x in (src, ref, t):
            x.free()


def test_a_part_created_on_a_second_context(ctx):
    rng = np.random.default_rng(19)
    other = hip.Ctx(0)
    try:
        rows = [100, 8300, 65]
        concat_and_compare(ctx, [random_piece(rng, n, validity=True) for n in rows], rows, on={1: other})
    finally:
        other.close()


def test_all_parts_empty_gives_an_empty_table(ctx):
    rng = np.random.default_rng(20)
    concat_and_compare(ctx, [random_piece(rng, 0), random_piece(rng, 0)], [0, 0])


# ---------------------------------------------------------------- refusals

def small(ctx, typ=I32, scale=0, n=10, ncols=1, dic=None):
    data = np.arange(n).astype(hip.NP_TYPES[typ]) % (len(dic) if dic else 100)
    return hip.Table(ctx, [(typ, data, scale, None, dic, None)] * ncols, n)


def refused(ctx, tables, word):
    with pytest.raises(hip.PlanHipError) as e:
        hip.table_concat(ctx, tables)
    assert e.value.code == hip.PH_EINVAL and word in str(e.value), str(e.value)
    # the context stays usable: a successful concat on it afterwards
    a = small(ctx)
    t = loader.concat_tables(ctx, [a, a])
    try:
        assert t.nrows == 20 and ctx.download(hip.vp(t.col(0).data), np.int32, 20).tolist() == list(range(10)) * 2
    finally:
        a.free()
        t.free()


def test_refusals(ctx):
    a, b64, two = small(ctx), small(ctx, I64), small(ctx, ncols=2)
    d2, d3 = small(ctx, DEC64, 2), small(ctx, DEC64, 3)
    code = small(ctx, CODE8, dic=["x", "y"])
    try:
        refused(ctx, [], "parts")
        refused(ctx, [a, None], "part 1 is NULL")
        refused(ctx, [a, two], "columns")
        refused(ctx, [a, b64], "column 0: part 1 has type %d, part 0 has type %d" % (I64, I32))
        refused(ctx, [d2, d2, d3], "column 0: part 2 has scale 3, part 0 has scale 2")
        refused(ctx, [code, a], "column 0: part 1 has type %d, part 0 has type %d" % (I32, CODE8))
    finally:
        for t in (a, b64, two, d2, d3, code):
            t.free()


def test_2_to_the_31_rows_are_refused_before_anything_is_allocated(ctx):
    big = hip.Table(ctx, [(I32, np.zeros(524288, np.int32))], 524288)
    try:
        refused(ctx, [big] * 4096, "%d rows exceed the int32 row-id domain" % 2**31)
        t = loader.concat_tables(ctx, [big] * 3)                        # below the limit the same parts concatenate
        assert t.nrows == 3 * 524288
        t.free()
    finally:
        big.free()


# ---------------------------------------------------------------- end to end: TPC-H lineitem in three pieces

CUTS = [0, 20001, 40003]


def lineitem_pieces(L):
    n = len(L["l_shipdate"])
    bounds = CUTS + [n]
    return [{k: v[a:b] for k, v in L.items() if isinstance(v, np.ndarray) and len(v) == n} for a, b in zip(bounds, bounds[1:])]


def test_lineitem_in_three_pieces_is_byte_identical_and_answers_q1_alike(ctx, sf001):
    L = sf001["lineitem"]
    whole = queries.lineitem_table(ctx, L, keys=True)
    parts = [queries.lineitem_table(ctx, P, keys=True) for P in lineitem_pieces(L)]
    t = loader.concat_tables(ctx, parts)
    try:
        assert all(p.nrows % 64 for p in parts) and t.nrows == whole.nrows == len(L["l_shipdate"])
        whole.ncols = t.ncols
        loader._attach_dicts(whole)
        assert_tables_equal(ctx, t, whole, whole.nrows)
        res = []
        for x in (t, whole):
            p = queries.q1_plan(ctx, x)
            p.run()
            r = p.fetch()
            res.append((r["ngroups"], [tuple(k) for k in r["keys"]], [list(s) for s in r["sum"]], [list(c) for c in r["count"]], p.bytes_per_row))
            p.free()
        assert res[0] == res[1] and res[0][0] == 4
    finally:
        for x in parts + [t, whole]:
            x.free()


def test_three_parquet_files_equal_the_one_file_with_all_rows(ctx, sf001, tmp_path):
    pa = pytest.importorskip("pyarrow")
    pq = pytest.importorskip("pyarrow.parquet")
    import decimal
    from plan_amd import tpchgen
    L = sf001["lineitem"]

    def arrow_of(P):
        return pa.Table.from_arrays([
            pa.array(P["l_orderkey"].astype(np.int64)), pa.array(P["l_quantity"].astype(np.int32)),
            pa.array([decimal.Decimal(int(v)).scaleb(-2) for v in P["l_extendedprice"].tolist()], pa.decimal128(15, 2)),
            pa.array(np.array(tpchgen.RETURNFLAG_DICT)[P["l_returnflag"]].tolist(), pa.string()),
            pa.array(P["l_shipdate"].astype(np.int32), pa.int32()).cast(pa.date32())],
            names=["l_orderkey", "l_quantity", "l_extendedprice", "l_returnflag", "l_shipdate"])

    paths = []
    for k, P in enumerate(lineitem_pieces(L) + [{k: v for k, v in L.items() if isinstance(v, np.ndarray)}]):
        paths.append(str(tmp_path / ("piece%d.parquet" % k)))
        pq.write_table(arrow_of(P), paths[-1], compression="NONE", row_group_size=25000)
    t = loader.table_from_parquet_files(ctx, paths[:3])
    ref = loader.table_from_parquet_device(ctx, paths[3])
    try:
        assert t.column_names == ref.column_names == ["l_orderkey", "l_quantity", "l_extendedprice", "l_returnflag", "l_shipdate"]
        assert_tables_equal(ctx, t, ref, len(L["l_shipdate"]))
    finally:
        t.free()
        ref.free()
    with pytest.raises(KeyError):                                       # an error while loading a piece is passed on
        loader.table_from_parquet_files(ctx, paths[:2], columns=["l_orderkey", "no_such_column"])
