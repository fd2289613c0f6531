"""ph_table_create_csv on the device: delimited text -> resident table, compared exactly with the restatement of the reference's CSV
scan (tests/csv_reference.py). Shapes are the smallest at which each piece can go wrong: record boundaries, tile boundaries of the
kernels' 32 KiB text tiles, NULLs / validity, field selection, the lowest failing row of every error, both VARCHAR encodings, and
TPC-H at SF0.01 written out as dbgen's .tbl text."""

import numpy as np
import pytest

import csv_reference as R
import oracle_lib as O
from plan_amd import hip, loader, queries, tpch, tpchgen

pytestmark = pytest.mark.gpu

T = 32768            # plan_amd/csrc/csv_load.hip: CSV_TILE, the bytes of text one workgroup counts / stages in LDS
ROW_PAD = 8192       # plan_amd/csrc/common.h: PH_ROW_PAD
I32, I64, DATE, DEC, STR = hip.PH_I32, hip.PH_I64, hip.PH_DATE, hip.PH_DEC64, hip.PH_STR
OK, EINVAL, EUNSUPPORTED, EOVERFLOW = hip.PH_OK, hip.PH_EINVAL, hip.PH_EUNSUPPORTED, hip.PH_EOVERFLOW
FIVE = [("i", 0, I32, 0), ("b", 1, I64, 0), ("d", 2, DATE, 0), ("m", 3, DEC, 2), ("s", 4, STR, 0)]


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


def rec(i, s=None, eol=b"\n"):
    """one record of the five-column schema (dbgen style: a delimiter after every field)"""
    s = b"s%d" % (i % 7) if s is None else s
    return b"%d|%d|19%02d-%02d-%02d|%d.%02d|%s|" % (i - 3, (i - 5) * 10**10, 60 + i % 40, 1 + i % 12, 1 + i % 28, i % 1000, i % 100, s) + eol


def strings_of(ctx, t, k, n):
    """the strings of VARCHAR column k as bytes, whichever encoding the library chose"""
    col = t.col(k)
    if col.type == hip.PH_CODE8:
        codes = ctx.download(hip.vp(col.data), np.uint8, n)
        return [t.dicts[k][c].encode("utf-8", "surrogateescape") for c in codes]
    assert col.type == hip.PH_STR
    off = ctx.download(hip.vp(col.data), np.int32, n + 1)
    byts = ctx.download(hip.vp(col.aux), np.uint8, int(col.aux_bytes)).tobytes()
    return [byts[off[i]:off[i + 1]] for i in range(n)]


def assert_table_equals(ctx, t, want, columns):
    """every device array of the table against what the restatement computed: values, zeroed NULL slots and padding, the bitmap (only
    where a NULL exists), dictionary / offsets / bytes"""
    n = want.nrows
    assert t.nrows == n
    if n == 0:
        return
    padded = (n + ROW_PAD - 1) // ROW_PAD * ROW_PAD
    for k, (_name, _field, typ, scale) in enumerate(columns):
        col = t.col(k)
        kind = want.columns[k][0]
        if kind == "fixed":
            _kind, vals, nulls = want.columns[k]
            assert (col.type, col.scale) == (typ, scale if typ == DEC else 0)
            got = ctx.download(hip.vp(col.data), hip.NP_TYPES[typ], padded)
            assert np.array_equal(got[:n].astype(np.int64), vals), k
            assert not got[n:].any(), k
            if nulls.any():
                bits = np.unpackbits(ctx.download(hip.vp(col.validity), np.uint8, padded // 8), bitorder="little")
                assert np.array_equal(bits[:n].astype(bool), ~nulls) and not bits[n:].any(), k
                assert t.col_narrow(k) is None
            else:
                assert not col.validity, k
        elif kind == "code8":
            _kind, codes, dic = want.columns[k]
            assert col.type == hip.PH_CODE8 and not col.validity
            assert [s.encode("utf-8", "surrogateescape") for s in t.dicts[k]] == dic, k
            got = ctx.download(hip.vp(col.data), np.uint8, padded)
            assert np.array_equal(got[:n], codes) and not got[n:].any(), k
        else:
            _kind, off, byts = want.columns[k]
            assert col.type == hip.PH_STR and not col.validity and t.dicts[k] == []
            got_off = ctx.download(hip.vp(col.data), np.int32, n + 1)
            assert np.array_equal(got_off, off) and got_off[n] == col.aux_bytes == len(byts), k
            assert ctx.download(hip.vp(col.aux), np.uint8, len(byts)).tobytes() == byts, k


def load_and_compare(ctx, text, columns=FIVE, delimiter="|"):
    want = R.load(text, [(f, t, s) for _n, f, t, s in columns], delimiter.encode())
    assert want.code == OK
    t = loader.table_from_csv(ctx, text, columns, delimiter)
    try:
        assert t.column_names == [c[0] for c in columns]
        assert_table_equals(ctx, t, want, columns)
    finally:
        t.free()
    return want


def padded_to(prefix, newline_at, eol=b"\n", i=900):
    """prefix + one record whose VARCHAR field is padded so that the record's '\\n' is byte `newline_at` of the text"""
    base = rec(i, b"", eol)
    fill = newline_at + 1 - len(prefix) - len(base)
    assert fill > 0
    out = prefix + rec(i, b"p" * fill, eol)
    assert out[newline_at:newline_at + 1] == b"\n" and len(out) == newline_at + 1
    return out


# ---------------------------------------------------------------- record boundaries

BOUNDARY_TEXTS = {
    "empty": b"",
    "only_empty_lines": b"\n\n\r\n",
    "one_record_no_newline": rec(1, eol=b""),
    "one_record_newline": rec(1),
    "lone_cr_at_end": rec(1) + rec(2, eol=b"\r"),
    "only_a_cr": b"\r",
    "crlf_throughout": b"".join(rec(i, eol=b"\r\n") for i in range(12)),
    "empty_lines_start_middle_end": b"\n\r\n" + rec(1) + rec(2) + b"\n\n" + rec(3, eol=b"\r\n") + b"\r\n\r\n" + rec(4) + b"\n\r\n\n",
    "no_trailing_delimiter": b"1|2|1999-01-01|3.5|x\n4|5|1999-01-02|6|y",
    "cr_inside_a_field": b"1|2|1999-01-01|3.5|a\rb|\n4|5|1999-01-02|6|\r|\r\n",
}


@pytest.mark.parametrize("name", sorted(BOUNDARY_TEXTS))
def test_record_boundaries(ctx, name):
    want = load_and_compare(ctx, BOUNDARY_TEXTS[name])
    assert want.nrows == {"empty": 0, "only_empty_lines": 0, "one_record_no_newline": 1, "one_record_newline": 1, "lone_cr_at_end": 2, "only_a_cr": 0,
                          "crlf_throughout": 12, "empty_lines_start_middle_end": 4, "no_trailing_delimiter": 2, "cr_inside_a_field": 2}[name]


# ---------------------------------------------------------------- tile boundaries

@pytest.mark.parametrize("tiles", [1, 2])
@pytest.mark.parametrize("d", [-2, -1, 0, 1, 2])
def test_newline_around_a_tile_boundary(ctx, tiles, d):
    """d = 0: the '\\n' is the last byte of a tile, d = 1: the first byte of the next; the following record starts right behind it"""
    head = rec(1) + rec(2)
    text = padded_to(head, tiles * T - 1 + d) + rec(3) + rec(4, eol=b"")
    assert load_and_compare(ctx, text).nrows == 5


@pytest.mark.parametrize("tiles", [1, 2])
def test_crlf_pair_split_across_two_tiles(ctx, tiles):
    text = padded_to(rec(1, eol=b"\r\n"), tiles * T, eol=b"\r\n") + rec(3, eol=b"\r\n") + rec(4, eol=b"\r\n")
    assert text[tiles * T - 1:tiles * T + 1] == b"\r\n"
    assert load_and_compare(ctx, text).nrows == 4


@pytest.mark.parametrize("empty", [b"\n", b"\r\n"])
def test_empty_line_begins_exactly_at_a_tile_start(ctx, empty):
    text = padded_to(rec(1), T - 1) + empty + rec(2) + rec(3)
    assert text[T:T + len(empty)] == empty
    assert load_and_compare(ctx, text).nrows == 4
    # and an empty "\r\n" line whose '\r' ends one tile and whose '\n' begins the next
    text = padded_to(rec(1), T - 2) + b"\r\n" + rec(2) + rec(3)
    assert text[T - 1:T + 1] == b"\r\n"
    assert load_and_compare(ctx, text).nrows == 4


def test_record_longer_than_whole_tiles_between_short_ones(ctx):
    head = b"".join(rec(i) for i in range(20))
    text = padded_to(head, len(head) + 3 * T - 1) + b"".join(rec(i) for i in range(20, 40))
    want = load_and_compare(ctx, text)
    assert want.nrows == 41 and max(len(s) for s in want.columns[4][2]) > 3 * T - 100


def test_record_counts_place_rows_through_every_scan_form(ctx):
    """1, 255, 256, 257 rows: the one-workgroup loop; 5 000: the one-step form; 70 001: the decoupled look-back (the VARCHAR offsets are a
    scan over the rows, the record starts a scan over the text tiles)"""
    before = ctx.scan_forms()
    for n in (1, 255, 256, 257, 5000, 70001):
        text = b"".join(rec(i, b"v%d" % (i % 300 if n < 1000 else i)) for i in range(n))
        assert load_and_compare(ctx, text).nrows == n
    after = ctx.scan_forms()
    ran = {k for k in after if after[k] > before[k]}
    assert {"loop", "small", "lookback"} <= ran, (before, after)


# ---------------------------------------------------------------- NULLs, validity, statistics

def test_nulls_validity_and_zeroed_slots(ctx):
    rows = [b"1|10|1999-01-01|1.25|a|", b"|20|1999-01-02|2|b|", b"3||1999-01-03||c|", b"4|40||4.5||", b"5|50|1999-01-05|5|e|",
            b"6|60|1999-01-06|6|f|", b"7|70|1999-01-07|7|g|", b"|80|1999-01-08|8|h|", b"||||i|", b"10|100|1999-01-10|10|j|", b"11||1999-01-11|11|k|"]
    want = load_and_compare(ctx, b"\n".join(rows) + b"\n")
    assert want.nrows == 11
    assert want.columns[0][2].tolist() == [r.split(b"|")[0] == b"" for r in rows] and want.columns[0][2][7:9].all()   # rows 7 and 8: across a byte
    assert not want.columns[3][2].any() and want.columns[3][1].tolist()[2] == 0                     # the empty DECIMAL: 0 and valid
    assert want.columns[4][2][want.columns[4][1][3]] == b""                                          # the empty VARCHAR: "" and valid


def test_null_free_columns_carry_the_statistics_of_ph_table_create(ctx):
    """no bitmap, and min / max, order, run and narrowed-copy statistics equal those of a table built from the same values"""
    n = 1000
    key = np.arange(n, dtype=np.int64) * 3 + 7                 # strictly ascending
    run = (np.arange(n) // 4 + 100).astype(np.int32)           # runs of four over consecutive values
    date = (np.arange(n) * 37 % 2000 + 9000).astype(np.int32)  # fits two bytes above its minimum
    dec = (np.arange(n, dtype=np.int64) * 7919 % 100000) - 500
    wide = np.where(np.arange(n) % 2 == 0, 2**40, -2**40).astype(np.int64)

    def dtext(v):
        return ("-" if v < 0 else "") + "%d.%02d" % (abs(v) // 100, abs(v) % 100)
    text = "".join("%d|%d|%s|%s|%d|\n" % (key[i], run[i], np.datetime64(int(date[i]), "D"), dtext(int(dec[i])), wide[i]) for i in range(n)).encode()
    cols = [("key", 0, I64, 0), ("run", 1, I32, 0), ("date", 2, DATE, 0), ("dec", 3, DEC, 2), ("wide", 4, I64, 0)]
    t = loader.table_from_csv(ctx, text, cols)
    ref = hip.Table(ctx, [(I64, key), (I32, run), (DATE, date), (DEC, dec, 2), (I64, wide)], n)
    try:
        for k in range(5):
            assert not t.col(k).validity
            assert hip.table_col_range_of(t, k) == hip.table_col_range_of(ref, k), k
            assert hip.table_col_stats(t, k) == hip.table_col_stats(ref, k), k
            assert t.col_run_len(k) == ref.col_run_len(k), k
            assert t.col_narrow(k) == ref.col_narrow(k), k
        assert hip.table_col_stats(t, 0) == hip.PH_STAT_ASCENDING | hip.PH_STAT_STRICT and hip.table_col_stats(t, 1) == hip.PH_STAT_ASCENDING
        assert t.col_run_len(1) == 4 and t.col_narrow(2) is not None and t.col_narrow(4) is None
        assert t.narrow_bytes() == ref.narrow_bytes()
    finally:
        t.free()
        ref.free()


# ---------------------------------------------------------------- field selection

def test_fields_in_any_order_with_gaps(ctx):
    text = b"".join(rec(i) for i in range(100))
    cols = [("s", 4, STR, 0), ("m", 3, DEC, 2), ("i", 0, I32, 0), ("i_again", 0, I64, 0), ("d", 2, DATE, 0)]      # field 1 and the trailing field: never read
    assert load_and_compare(ctx, text, cols).nrows == 100
    assert load_and_compare(ctx, text, [("trail", 5, STR, 0)]).columns[0][2] == [b""]        # the trailing delimiter's field exists and is empty
    with pytest.raises(hip.PlanHipError) as e:
        loader.table_from_csv(ctx, text, [("i", 0, I32, 0), ("past", 6, I32, 0)])
    assert e.value.code == EINVAL and "no enough fields" in str(e.value) and "row 0" in str(e.value)
    assert load_and_compare(ctx, text.replace(b"|", b","), FIVE, ",").nrows == 100
    assert load_and_compare(ctx, text.replace(b"|", b"\t"), FIVE, "\t").nrows == 100


# ---------------------------------------------------------------- errors: the lowest failing row

def faulty(bad_137, bad_200=None):
    rows = [rec(i) for i in range(300)]
    rows[137] = bad_137
    if bad_200 is not None:
        rows[200] = bad_200
    return b"".join(rows)


ERROR_CASES = {
    "field_count": (b"1|2|1999-01-01|1.5|\n", EINVAL),
    "bad_date": (b"1|2|1999-02-29|1.5|x|\n", EINVAL),
    "bad_integer": (b"1x|2|1999-01-01|1.5|x|\n", EINVAL),
    "int32_overflow": (b"2147483648|2|1999-01-01|1.5|x|\n", EOVERFLOW),
    "int64_overflow": (b"1|9223372036854775808|1999-01-01|1.5|x|\n", EOVERFLOW),
    "decimal_digits": (b"1|2|1999-01-01|1.555|x|\n", EUNSUPPORTED),
    "decimal_form": (b"1|2|1999-01-01|1e2|x|\n", EUNSUPPORTED),
    "decimal_overflow": (b"1|2|1999-01-01|92233720368547758.08|x|\n", EOVERFLOW),
}


@pytest.mark.parametrize("name", sorted(ERROR_CASES))
def test_errors_name_the_lowest_failing_row(ctx, name):
    bad, code = ERROR_CASES[name]
    cols = [(f, t, s) for _n, f, t, s in FIVE]
    for later in (None, b"zz|2|1999-01-01|1.5|x|\n", b"1|2|\n"):       # alone, then with another fault (another cause) on row 200
        text = faulty(bad, later)
        want = R.load(text, cols)
        assert (want.code, want.row) == (code, 137)
        with pytest.raises(hip.PlanHipError) as e:
            loader.table_from_csv(ctx, text, FIVE)
        assert e.value.code == code and "row 137" in str(e.value), str(e.value)
        assert load_and_compare(ctx, faulty(rec(137))).nrows == 300                     # nothing of the error is left on the context
    # the earlier row wins whichever cause it has
    with pytest.raises(hip.PlanHipError) as e:
        loader.table_from_csv(ctx, faulty(b"1|2|1999-01-01|1.5|x|\n", bad)[: -1], FIVE)
    assert e.value.code == code and "row 200" in str(e.value)


def test_quote_byte_and_bad_delimiters(ctx):
    text = faulty(b'1|2|1999-01-01|1.5|say "x"|\n', b"zz|2|\n")
    assert R.load(text, [(f, t, s) for _n, f, t, s in FIVE]).code == EUNSUPPORTED
    with pytest.raises(hip.PlanHipError) as e:
        loader.table_from_csv(ctx, text, FIVE)
    assert e.value.code == EUNSUPPORTED
    good = faulty(rec(137))
    assert load_and_compare(ctx, good).nrows == 300
    for delim in ('"', "\n", "\r", "\0", "ab", "é"):
        with pytest.raises(hip.PlanHipError) as e:
            loader.table_from_csv(ctx, good, FIVE, delim)
        assert e.value.code == EINVAL, delim
    with pytest.raises(hip.PlanHipError) as e:
        loader.table_from_csv(ctx, good, [("i", 0, hip.PH_F64, 0)])
    assert e.value.code == EINVAL
    assert load_and_compare(ctx, good).nrows == 300


# ---------------------------------------------------------------- VARCHAR encodings

def distinct_strings(k):
    base = [b"", b"ab", b"abc", b"abcd", b"a", b"caf\xc3\xa9", b"\xc3\xbcber", b"\xff\xfe raw", b"\x80", b"Z", b"z", b" lead", b"trail "]
    return base + [b"str %05d" % (i * 7919 % 100000) for i in range(k - len(base))]


@pytest.mark.parametrize("k,kind", [(256, "code8"), (257, "str")])
def test_varchar_encoding_by_distinct_count(ctx, k, kind):
    d = distinct_strings(k)
    assert len(set(d)) == k
    rng = np.random.default_rng(k)
    pick = np.concatenate([np.arange(k), rng.integers(0, k, 1000 - k)])
    rng.shuffle(pick)
    text = b"".join(b"%d|%s|\n" % (i, d[j]) for i, j in enumerate(pick))
    cols = [("i", 0, I32, 0), ("s", 1, STR, 0)]
    want = load_and_compare(ctx, text, cols)
    assert want.columns[1][0] == kind
    t = loader.table_from_csv(ctx, text, cols)
    try:
        assert strings_of(ctx, t, 1, 1000) == [d[j] for j in pick]
        if kind == "code8":
            assert [s.encode("utf-8", "surrogateescape") for s in t.dicts[1]] == sorted(set(d))       # unsigned byte order
            assert hip.lib().ph_table_dict_size(t.h, hip.i32(1)) == 256
        else:
            c = t.col(1)
            assert ctx.download(hip.vp(c.data), np.int32, 1001)[1000] == c.aux_bytes == sum(len(d[j]) for j in pick)
    finally:
        t.free()


def test_varchar_distinct_count_beyond_the_first_rows(ctx):
    """the library interns the first 65 536 rows alone before it interns all: a column with few distinct strings throughout is a
    dictionary, one whose distinct strings only show behind those rows is not"""
    n = 66000
    text = b"".join(b"%d|k%d|late%d|\n" % (i, i % 200, 0 if i < 65536 else i) for i in range(n))
    want = load_and_compare(ctx, text, [("i", 0, I32, 0), ("few", 1, STR, 0), ("late", 2, STR, 0)])
    assert want.nrows == n and want.columns[1][0] == "code8" and want.columns[2][0] == "str"


def test_varchar_value_with_a_nul_byte_stays_offsets_and_bytes(ctx):
    want = load_and_compare(ctx, b"1|a\0b|x|\n2|c|y|\n3||x|\n", [("i", 0, I32, 0), ("s", 1, STR, 0), ("t", 2, STR, 0)])
    assert want.columns[1][0] == "str" and want.columns[1][2] == b"a\0bc" and want.columns[2][0] == "code8"


# ---------------------------------------------------------------- TPC-H at SF0.01 as dbgen .tbl text

def dec2(a):
    a = np.asarray(a, dtype=np.int64)
    return [("-" if v < 0 else "") + "%d.%02d" % (abs(v) // 100, abs(v) % 100) for v in a.tolist()]


def dates(a):
    return np.datetime_as_string(np.asarray(a, dtype="int64").astype("datetime64[D]")).tolist()


def strs(src, name):
    off, byts = src[name + "_off"], src[name + "_bytes"].tobytes()
    return [byts[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)]


def tbl_text(name, src):
    """dbgen field order, '|' after every field including the last; columns the fixture does not hold are a filler"""
    n = len(src[tpch.SCHEMA[name][0][0]])
    fields = [["x"] * n for _ in tpch.TBL_COLUMNS[name]]
    for cname, typ, _scale, dic in tpch.SCHEMA[name]:
        f = tpch.TBL_FIELDS[name][cname]
        if typ == hip.PH_STR:
            if cname + "_off" in src:
                fields[f] = strs(src, cname)
        elif typ == hip.PH_CODE8:
            fields[f] = np.array(dic)[src[cname]].tolist()
        elif typ == hip.PH_DEC64:
            fields[f] = dec2(src[cname])
        elif typ == hip.PH_DATE:
            fields[f] = dates(src[cname])
        else:
            fields[f] = [str(v) for v in src[cname].tolist()]
    return "".join("|".join(r) + "|\n" for r in zip(*fields)).encode()


@pytest.fixture(scope="module")
def tbl(sf001):
    return {name: tbl_text(name, sf001[name]) for name in ("lineitem", "orders", "customer")}


def test_tbl_text_has_dbgen_layout(tbl, sf001):
    first = tbl["lineitem"].split(b"\n")[0].split(b"|")
    L = sf001["lineitem"]
    assert len(first) == 17 and first[16] == b"" and int(first[0]) == L["l_orderkey"][0] and int(first[3]) == L["l_linenumber"][0]
    assert first[10] == str(np.datetime64(int(L["l_shipdate"][0]), "D")).encode() and first[8].decode() == tpchgen.RETURNFLAG_DICT[L["l_returnflag"][0]]
    assert tpch.TBL_FIELDS["lineitem"]["l_quantity"] == 4 and tpch.TBL_FIELDS["orders"]["o_orderdate"] == 4 and tpch.TBL_FIELDS["customer"]["c_mktsegment"] == 6


def test_from_tbl_columns_equal_the_fixture(ctx, tbl, sf001, tmp_path):
    path = tmp_path / "lineitem.tbl"
    path.write_bytes(tbl["lineitem"])
    db = tpch.Database.from_tbl(ctx, {"lineitem": str(path), "orders": tbl["orders"], "customer": tbl["customer"]})   # a path is memory-mapped
    try:
        for name in ("lineitem", "orders", "customer"):
            src, t = sf001[name], db.t(name)
            n = t.nrows
            assert n == len(src[tpch.SCHEMA[name][0][0]])
            assert db.index[name] == {c: i for i, (c, _t, _s, _d) in enumerate(tpch.SCHEMA[name])}
            for cname, typ, scale, dic in tpch.SCHEMA[name]:
                k = db.index[name][cname]
                col = t.col(k)
                if typ == hip.PH_CODE8:
                    assert [s.decode() for s in strings_of(ctx, t, k, n)] == np.array(dic)[src[cname]].tolist(), cname
                elif typ == hip.PH_STR:
                    want = strs(src, cname) if cname + "_off" in src else ["x"] * n
                    assert [s.decode() for s in strings_of(ctx, t, k, n)] == want, cname
                else:
                    assert (col.type, col.scale) == (typ, scale) and not col.validity, cname
                    got = ctx.download(hip.vp(col.data), hip.NP_TYPES[typ], n)
                    assert got.dtype == src[cname].dtype and got.tobytes() == src[cname].tobytes(), cname
        assert hip.table_col_stats(db.t("orders"), db.index["orders"]["o_orderkey"]) & hip.PH_STAT_DECLARED_UNIQUE
    finally:
        db.free()


def test_q1_over_text_loaded_lineitem_equals_the_oracle(ctx, tbl, sf001):
    L = sf001["lineitem"]
    names = ["l_quantity", "l_extendedprice", "l_discount", "l_tax", "l_returnflag", "l_linestatus", "l_shipdate"]      # test_loader.py's order
    types = {c: (hip.PH_STR if typ == hip.PH_CODE8 else typ, scale) for c, typ, scale, _d in tpch.SCHEMA["lineitem"]}
    t = loader.table_from_csv(ctx, tbl["lineitem"], [(c, tpch.TBL_FIELDS["lineitem"][c]) + types[c] for c in names])
    direct = queries.lineitem_table(ctx, L)
    try:
        assert t.dicts[4] == tpchgen.RETURNFLAG_DICT and t.dicts[5] == tpchgen.LINESTATUS_DICT
        p, pd = queries.q1_plan(ctx, t), queries.q1_plan(ctx, direct)
        p.run()
        r = p.fetch()
        want = O.q1(L, queries.q1_shipdate_cutoff())
        assert r["ngroups"] == len(want) == 4
        for g, w in enumerate(want):
            assert tuple(r["keys"][g]) == (w.returnflag, w.linestatus)
            assert r["sum"][g][0] == w.sum_qty.value() and r["sum"][g][1] == w.sum_base_price.unscaled(2)
            assert r["sum"][g][2] == w.sum_disc_price.unscaled(4) and r["sum"][g][3] == w.sum_charge.unscaled(6)
            assert r["count"][g][7] == w.count_order
        assert p.bytes_per_row == pd.bytes_per_row < 34         # the narrowed copies are there: the fused scan reads as few bytes as ever
        assert t.narrow_bytes() == direct.narrow_bytes() > 0
        p.free()
        pd.free()
    finally:
        t.free()
        direct.free()


def test_q3_over_from_tbl_equals_the_generated_database(ctx, tbl, sf001):
    db_text = tpch.Database.from_tbl(ctx, tbl)
    db_gen = tpch.Database(ctx, sf001)
    try:
        out = []
        for db in (db_text, db_gen):
            res = []
            for topk in (10, 0):
                p = tpch.q3_plan(db, topk=topk)
                p.run()
                r = p.fetch()
                p.free()
                groups = [(int(r["keys"][g][0]), r["sum"][g][0], int(r["keys"][g][1]), int(r["keys"][g][2])) for g in range(r["ngroups"])]
                res.append((r["ngroups"], sorted(groups), tpch.q3_top(r)))
            out.append(res)
        assert out[0] == out[1] and out[0][1][0] > 10
    finally:
        db_text.free()
        db_gen.free()
