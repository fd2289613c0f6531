"""PH_CSV_QUOTES on the device: text with encoding/csv's quoted fields -> resident table, every device array compared with the
sequential restatement (tests/csv_quoted_reference.py). The shapes sit on the seams of the record-start pass (the quote parity carried
across 16-byte pieces, a thread's 128 bytes, a wave's 8 KiB and the 32 KiB tiles) and of the bounded field walk."""
import numpy as np
import pytest

import csv_quoted_reference as Q
from plan_amd import hip, loader, tpch
from test_gpu_csv_load import assert_table_equals, strings_of, tbl_text

pytestmark = pytest.mark.gpu

T = 32768            # plan_amd/csrc/csv_load.hip: CSV_TILE
ROW_PAD = 8192       # plan_amd/csrc/common.h: PH_ROW_PAD
I32, I64, DATE, DEC, STR = hip.PH_I32, hip.PH_I64, hip.PH_DATE, hip.PH_DEC64, hip.PH_STR
OK, EINVAL, EUNSUPPORTED, EOVERFLOW = hip.PH_OK, hip.PH_EINVAL, hip.PH_EUNSUPPORTED, hip.PH_EOVERFLOW
THREE = [("i", 0, I32, 0), ("a", 1, STR, 0), ("b", 2, STR, 0)]
FIVE = [("i", 0, I32, 0), ("b", 1, I64, 0), ("d", 2, DATE, 0), ("m", 3, DEC, 2), ("s", 4, STR, 0)]


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


def load_and_compare(ctx, text, columns=THREE, delimiter="|"):
    want = Q.load(text, [(f, t, s) for _n, f, t, s in columns], delimiter.encode())
    assert want.code == OK, (want.code, want.row)
    t = loader.table_from_csv(ctx, text, columns, delimiter, quoting=True)
    try:
        assert_table_equals(ctx, t, want, columns)
    finally:
        t.free()
    return want


def strings(want, k):
    kind, a, b = want.columns[k]
    if kind == "code8":
        return [b[c] for c in a]
    return [b[a[i]:a[i + 1]] for i in range(len(a) - 1)]


def rec5(i, s=None, eol=b"\n"):
    """one record of FIVE; every fifth holds a quoted line break, every seventh a quoted number"""
    if s is None:
        s = b'"s\n%d"' % (i % 7) if i % 5 == 0 else b"s%d" % (i % 7)
    first = b'"%d"' % (i - 3) if i % 7 == 0 else b"%d" % (i - 3)
    return b"%s|%d|19%02d-%02d-%02d|%d.%02d|%s|" % (first, (i - 5) * 10**10, 60 + i % 40, 1 + i % 12, 1 + i % 28, i % 1000, i % 100, s) + eol


# ---------------------------------------------------------------- quote-free text under the flag

def download_column(ctx, t, k, n):
    col = t.col(k)
    padded = (n + ROW_PAD - 1) // ROW_PAD * ROW_PAD
    out = [col.type, col.scale, bool(col.validity), int(col.aux_bytes), t.dicts[k]]
    if col.type == hip.PH_STR:
        out.append(ctx.download(hip.vp(col.data), np.int32, n + 1).tobytes())
        out.append(ctx.download(hip.vp(col.aux), np.uint8, int(col.aux_bytes)).tobytes())
    else:
        out.append(ctx.download(hip.vp(col.data), hip.NP_TYPES[col.type], padded).tobytes())
    if col.validity:
        out.append(ctx.download(hip.vp(col.validity), np.uint8, padded // 8).tobytes())
    return out


def test_quote_free_text_gives_the_table_of_the_default_load(ctx):
    n = 3000
    text = b"".join(b"%d|%d|19%02d-%02d-%02d|%d.%02d|s%d|c%d|%s|\n" % (i * 3 + 7, i // 4 + 100, 60 + i % 40, 1 + i % 12, 1 + i % 28, i % 1000, i % 100, i % 9, i,
                                                                     b"" if i % 11 == 0 else b"%d" % i) for i in range(n))
    cols = [("key", 0, I64, 0), ("run", 1, I32, 0), ("date", 2, DATE, 0), ("dec", 3, DEC, 2), ("few", 4, STR, 0), ("many", 5, STR, 0), ("nullable", 6, I32, 0)]
    a = loader.table_from_csv(ctx, text, cols)
    b = loader.table_from_csv(ctx, text, cols, quoting=True)
    try:
        assert a.nrows == b.nrows == n
        for k in range(len(cols)):
            assert download_column(ctx, a, k, n) == download_column(ctx, b, k, n), k
            if k < 4:
                assert hip.table_col_range_of(a, k) == hip.table_col_range_of(b, k), k
                assert hip.table_col_stats(a, k) == hip.table_col_stats(b, k), k
                assert a.col_run_len(k) == b.col_run_len(k) and a.col_narrow(k) == b.col_narrow(k), k
        assert a.narrow_bytes() == b.narrow_bytes() > 0
        assert a.col(4).type == hip.PH_CODE8 and a.col(5).type == hip.PH_STR and a.col(6).validity
    finally:
        a.free()
        b.free()


# ---------------------------------------------------------------- tile, wave, thread and piece edges

# one record whose marked byte (index `mark` of the tail) is placed at a chosen position of the text; "%s" takes the filler
EDGE_CASES = {
    "newline_inside_quotes": (b'7|"%s', b'\nzz"|x\n', 0),
    "opening_quote": (b'7|%s', b'|"q\nr"\n', 1),
    "closing_quote_delimiter_behind": (b'7|"%s', b'"|x\n', 0),
    "escaped_pair": (b'7|"%s', b'""zz"|x\n', 0),
    "crlf_inside_quotes": (b'7|"%s', b'\r\nzz"|x\n', 0),
    "closing_quote_crlf_ends_the_record": (b'7|x|"%s', b'"\r\n', 1),
}
HEAD = b'1|"h\nh"|y\n'
AFTER = b'8|"k\nk""|"|"z"\r\n9|u|v'


def edge_text(case, at):
    """HEAD, the case's record with its marked byte at position `at`, AFTER: one record before and two behind"""
    front, tail, mark = EDGE_CASES[case]
    fill = at - mark - len(HEAD) - len(front % b"")
    assert fill > 0
    text = HEAD + front % (b"p" * fill) + tail
    assert text[at:at + 1] == tail[mark:mark + 1] and len(text) == at - mark + len(tail)
    return text + AFTER


@pytest.mark.parametrize("tiles", [1, 2])
@pytest.mark.parametrize("case", sorted(EDGE_CASES))
def test_quoting_around_a_tile_edge(ctx, case, tiles):
    """d = 0: the marked byte is the last of a tile and what follows it the first of the next"""
    for d in (-2, -1, 0, 1, 2):
        want = load_and_compare(ctx, edge_text(case, tiles * T - 1 + d))
        assert want.nrows == 4, d


@pytest.mark.parametrize("edge", [2160, 2176, 3072, 8192])
@pytest.mark.parametrize("case", ["newline_inside_quotes", "escaped_pair"])
def test_quoting_around_the_seams_inside_a_tile(ctx, case, edge):
    """the prefix XOR's seams: a 16-byte piece (2160), the 128 bytes of one thread (2176), the 1 KiB of one wave load (3072), the 8 KiB of
    one wave's threads (8192)"""
    for d in (-1, 0, 1):
        assert load_and_compare(ctx, edge_text(case, edge - 1 + d)).nrows == 4, d


def test_quoted_field_of_three_tiles_without_a_quote_inside(ctx):
    """the parity is carried through tiles that hold no quote and no record start"""
    head = b"".join(b'%d|"a\n%d"|b\n' % (i, i) for i in range(20))
    text = head + b'99|"' + b"line\n" * (3 * T // 5 + 7) + b'"|x\n' + b"".join(b'%d|c|"d\n"\n' % i for i in range(20))
    want = load_and_compare(ctx, text)
    assert want.nrows == 41 and max(len(s) for s in strings(want, 1)) > 3 * T


def test_escaped_pairs_make_odd_and_even_quote_counts_per_tile(ctx):
    """a tile's incoming parity is the parity of the COUNT of '"' bytes before it, not a state: tiles with odd and with even counts,
    tiles that begin inside and outside a quoted field"""
    rng = np.random.default_rng(8)
    rows = []
    for i in range(5000):
        a = b"".join((b'""', b"x", b"\n", b"|")[j] for j in rng.integers(0, 4, rng.integers(0, 30)))
        rows.append(b'%d|"%s"|"%s"\n' % (i, a, b'""' * int(rng.integers(0, 4))))
    text = b"".join(rows)
    ntiles = len(text) // T
    assert ntiles >= 3
    counts = [text[k * T:(k + 1) * T].count(b'"') % 2 for k in range(ntiles)]
    before = [text[:k * T].count(b'"') % 2 for k in range(1, ntiles + 1)]
    assert {0, 1} <= set(counts) and {0, 1} <= set(before)
    assert load_and_compare(ctx, text).nrows == 5000


def test_row_counts_through_every_scan_form(ctx):
    """1, 255, 256, 257 rows: the one-workgroup loop; 5 000: the one-step form; 70 001: the decoupled look-back — every fifth record
    holds a quoted line break"""
    before = ctx.scan_forms()
    for n in (1, 255, 256, 257, 5000, 70001):
        text = b"".join(rec5(i, (b'"v\n%d"' if i % 5 == 0 else b"v%d") % (i % 300 if n < 1000 else i)) for i in range(n))
        assert load_and_compare(ctx, text, FIVE).nrows == n
    after = ctx.scan_forms()
    assert {"loop", "small", "lookback"} <= {k for k in after if after[k] > before[k]}, (before, after)


# ---------------------------------------------------------------- values

def test_quoted_values_and_the_empty_quoted_field(ctx):
    rows = [b'"1"|"10"|"1999-01-01"|"1.25"|"a"|', b'""|20|1999-01-02|2|b|', b'3|""|"1999-01-03"|""|""|', b'4|40|""|4.5||', b'"-5"|"+50"|1999-01-05|"-0.05"|"e"|',
            b'|"60"||""|"f|\n"|', b'"007"|70|"2000-02-29"|7|g|']
    want = load_and_compare(ctx, b"\r\n".join(rows) + b"\r\n", FIVE)
    assert want.nrows == 7 and want.columns[0][1].tolist() == [1, 0, 3, 4, -5, 0, 7]
    assert want.columns[0][2].tolist() == [False, True, False, False, False, True, False]
    assert want.columns[1][2].tolist() == [False, False, True, False, False, False, False]
    assert want.columns[2][2].tolist() == [False, False, False, True, False, True, False]
    assert not want.columns[3][2].any() and want.columns[3][1].tolist() == [125, 200, 0, 450, -5, 0, 700]      # the empty DECIMAL: 0 and valid
    assert strings(want, 4) == [b"a", b"b", b"", b"", b"e", b"f|\n", b"g"]
    # no NULL anywhere: no bitmap (assert_table_equals checks that a bitmap exists only where a NULL does)
    want = load_and_compare(ctx, b'"1"|"2"|"1999-01-01"|""|""|\n', FIVE)
    assert not any(want.columns[k][2].any() for k in range(4))


def test_escape_inside_a_quoted_number_is_no_number(ctx):
    good = [rec5(i) for i in range(300)]
    for bad, code in ((b'"1""2"|2|1999-01-01|1.5|x|\n', EINVAL), (b'1|"2\r\n3"|1999-01-01|1.5|x|\n', EINVAL), (b'1|2|"1999-01""-01"|1.5|x|\n', EINVAL),
                      (b'1|2|1999-01-01|"1""5"|x|\n', EUNSUPPORTED)):
        text = b"".join(good[:137] + [bad] + good[138:])
        want = Q.load(text, [(f, t, s) for _n, f, t, s in FIVE])
        assert (want.code, want.row) == (code, 137)
        with pytest.raises(hip.PlanHipError) as e:
            loader.table_from_csv(ctx, text, FIVE, quoting=True)
        assert e.value.code == code and "row 137" in str(e.value), str(e.value)


# ---------------------------------------------------------------- VARCHAR

def distinct_strings(k):
    base = [b"", b'"', b'""', b"|", b"\n", b"a|b", b'say "x"', b"two\nlines", b"cr\rkept", b'",', b"\n\n", b' "lead', b"caf\xc3\xa9", b"\xff raw"]
    return base + [b"str %05d" % (i * 7919 % 100000) for i in range(k - len(base))]


def quoted(s, crlf=False):
    s = s.replace(b'"', b'""')
    return b'"' + (s.replace(b"\n", b"\r\n") if crlf else s) + b'"'


@pytest.mark.parametrize("k,kind", [(256, "code8"), (257, "str")])
def test_varchar_encoding_by_distinct_count(ctx, k, kind):
    d = distinct_strings(k)
    assert len(set(d)) == k
    rng = np.random.default_rng(k)
    pick = np.concatenate([np.arange(k), rng.integers(0, k, 1000 - k)])
    rng.shuffle(pick)
    plain = [not any(c in d[j] for c in b'|\n\r"') and i % 3 == 0 for i, j in enumerate(pick)]
    text = b"".join(b"%d|%s|\n" % (i, d[j] if plain[i] else quoted(d[j], crlf=i % 2 == 0)) for i, j in enumerate(pick))
    cols = [("i", 0, I32, 0), ("s", 1, STR, 0)]
    want = load_and_compare(ctx, text, cols)
    assert want.columns[1][0] == kind and strings(want, 1) == [d[j] for j in pick]
    t = loader.table_from_csv(ctx, text, cols, quoting=True)
    try:
        assert strings_of(ctx, t, 1, 1000) == [d[j] for j in pick]
        if kind == "code8":
            assert [s.encode("utf-8", "surrogateescape") for s in t.dicts[1]] == sorted(set(d))
            assert {b'"', b"|", b"\n", b'say "x"'} <= set(d)
        else:
            assert t.col(1).aux_bytes == sum(len(d[j]) for j in pick)
    finally:
        t.free()


def test_escapes_only_behind_the_first_65536_rows(ctx):
    """the marked-row copy must reach rows behind the head that the library interns first; a column without any escape beside it"""
    n = 66000
    text = b"".join(b'%d|"k%d"|%s|\n' % (i, i % 200, (b'"late ""%d"" \r\n"' % i) if i >= 65536 else b'"e|%d"' % (i % 50)) for i in range(n))
    want = load_and_compare(ctx, text, [("i", 0, I32, 0), ("few", 1, STR, 0), ("late", 2, STR, 0)])
    assert want.nrows == n and want.columns[1][0] == "code8" and want.columns[2][0] == "str"
    assert strings(want, 2)[65538] == b'late "65538" \n'


# ---------------------------------------------------------------- errors

def faulty(bad_137, bad_200=None, last=None):
    rows = [rec5(i) for i in range(300)]
    rows[137] = bad_137
    if bad_200 is not None:
        rows[200] = bad_200
    if last is not None:
        rows[299] = last
    return b"".join(rows)


QUOTE_ERRORS = {
    "bare_quote": (b'1|2|1999-01-01|1.5|say "x"|\n', "bare quote"),
    "extraneous_quote": (b'1|2|1999-01-01|1.5|"x"y|\n', "extraneous or missing quote"),
    "quote_then_lone_cr": (b'1|2|1999-01-01|1.5|"x"\ry|\n', "extraneous or missing quote"),
}


@pytest.mark.parametrize("name", sorted(QUOTE_ERRORS))
def test_quote_errors_name_the_lowest_failing_row(ctx, name):
    bad, kind = QUOTE_ERRORS[name]
    cols = [(f, t, s) for _n, f, t, s in FIVE]
    # alone; with a bad integer / a short record on row 200; with a bad integer and a wrong field count IN the failing row
    for text in (faulty(bad), faulty(bad, b"zz|2|1999-01-01|1.5|x|\n"), faulty(bad, b"1|2|\n"), faulty(b"zz|" + bad)):
        want = Q.load(text, cols)
        assert (want.code, want.row) == (EINVAL, 137)
        with pytest.raises(hip.PlanHipError) as e:
            loader.table_from_csv(ctx, text, FIVE, quoting=True)
        assert e.value.code == EINVAL and "row 137" in str(e.value) and kind in str(e.value), str(e.value)
        assert load_and_compare(ctx, faulty(rec5(137)), FIVE).nrows == 300                 # nothing of the error is left on the context
    # an earlier row wins whatever its cause
    text = faulty(b"1|2|1999-02-30|1.5|x|\n", bad)
    assert (Q.load(text, cols).code, Q.load(text, cols).row) == (EINVAL, 137)
    with pytest.raises(hip.PlanHipError) as e:
        loader.table_from_csv(ctx, text, FIVE, quoting=True)
    assert e.value.code == EINVAL and "row 137" in str(e.value) and "date" in str(e.value)


def test_unterminated_quote(ctx):
    cols = [(f, t, s) for _n, f, t, s in FIVE]
    cases = [(faulty(b'1|2|1999-01-01|1.5|"x|\n'), 137, "missing quote"),                              # swallows the rest of the text: row 137 fails
             (faulty(rec5(137), last=b'1|2|1999-01-01|1.5|"never closed|'), 299, "missing quote"),      # the end of input inside the quotes
             (faulty(rec5(137), last=b'1|2|1999-01-01|1.5|"never closed|\n')[:-1] + b"\r", 299, "missing quote")]
    for text, row, kind in cases:
        want = Q.load(text, cols)
        assert (want.code, want.row) == (EINVAL, row)
        with pytest.raises(hip.PlanHipError) as e:
            loader.table_from_csv(ctx, text, FIVE, quoting=True)
        assert e.value.code == EINVAL and "row %d" % row in str(e.value) and kind in str(e.value), str(e.value)
    # the unterminated quote on the last row and a bad date on row 10: row 10
    rows = [rec5(i) for i in range(300)]
    rows[10] = b"1|2|1999-13-01|1.5|x|\n"
    rows[299] = b'1|2|1999-01-01|1.5|"never closed|'
    text = b"".join(rows)
    assert (Q.load(text, cols).code, Q.load(text, cols).row) == (EINVAL, 10)
    with pytest.raises(hip.PlanHipError) as e:
        loader.table_from_csv(ctx, text, FIVE, quoting=True)
    assert e.value.code == EINVAL and "row 10," in str(e.value) and "date" in str(e.value)
    assert load_and_compare(ctx, faulty(rec5(137)), FIVE).nrows == 300


def test_default_is_unchanged_and_unknown_flags_are_refused(ctx):
    text = faulty(b'1|2|1999-01-01|1.5|"x"|\n')
    with pytest.raises(hip.PlanHipError) as e:
        loader.table_from_csv(ctx, text, FIVE)
    assert e.value.code == EUNSUPPORTED
    cols = [(f, t, s) for _n, f, t, s in FIVE]
    for flags in (2, 3, 1 << 31):
        with pytest.raises(hip.PlanHipError) as e:
            hip.table_create_csv(ctx, text, len(text), ord("|"), cols, flags)
        assert e.value.code == EINVAL and "flags" in str(e.value)
    assert load_and_compare(ctx, text, FIVE).nrows == 300


# ---------------------------------------------------------------- TPC-H at SF0.01, every VARCHAR field quoted

@pytest.mark.parametrize("name,comment", [("orders", "o_comment"), ("customer", "c_comment")])
def test_tpch_tables_with_quoted_varchar_fields(ctx, sf001, name, comment):
    """every tenth comment gets a "" and a "\\r\\n" inside its quotes; the other columns are those of the .tbl load, byte for byte"""
    plain = tbl_text(name, sf001[name])
    is_str = {tpch.TBL_FIELDS[name][c]: c for c, typ, _s, _d in tpch.SCHEMA[name] if typ in (hip.PH_CODE8, hip.PH_STR)}
    fcomment = tpch.TBL_FIELDS[name][comment]
    lines, comments = [], []
    for r, line in enumerate(plain.split(b"\n")[:-1]):
        fields = line.split(b"|")
        value = fields[fcomment]
        for f in is_str:
            fields[f] = b'"' + fields[f] + b'"'
        if r % 10 == 0:
            fields[fcomment] = b'"' + value[:3] + b'""' + value[3:6] + b"\r\n" + value[6:] + b'"'
            value = value[:3] + b'"' + value[3:6] + b"\n" + value[6:]
        comments.append(value)
        lines.append(b"|".join(fields) + b"\n")
    text = b"".join(lines)
    cols = [(c, tpch.TBL_FIELDS[name][c], STR if typ in (hip.PH_CODE8, hip.PH_STR) else typ, scale) for c, typ, scale, _d in tpch.SCHEMA[name]]
    a = loader.table_from_csv(ctx, plain, cols)
    b = loader.table_from_csv(ctx, text, cols, quoting=True)
    try:
        n = a.nrows
        assert b.nrows == n == len(comments)
        for k, (c, _f, _t, _s) in enumerate(cols):
            if c != comment:
                assert download_column(ctx, a, k, n) == download_column(ctx, b, k, n), c
        k = [c for c, _f, _t, _s in cols].index(comment)
        want = Q.load(text, [(fcomment, STR, 0)])
        assert want.code == OK and strings(want, 0) == comments
        assert strings_of(ctx, b, k, n) == comments
        one = loader.table_from_csv(ctx, text, [(comment, fcomment, STR, 0)], quoting=True)
        try:
            assert_table_equals(ctx, one, want, [(comment, fcomment, STR, 0)])
        finally:
            one.free()
    finally:
        a.free()
        b.free()
