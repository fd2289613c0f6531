"""PH_CSV_QUOTES without a device: the sequential restatement of encoding/csv's quoted fields (tests/csv_quoted_reference.py) against a
literal table, Python's csv module and pyarrow.csv; ph_csv_split_record — the walker the field kernel runs — against the restatement;
and the device form (record starts by quote parity, every record walked up to the next start) against the sequential one on random
texts, most of them malformed."""
import csv
import io
import random

import pytest

import csv_quoted_reference as Q
import csv_reference as R
from plan_amd import hip

I32, I64, DATE, DEC, STR = hip.PH_I32, hip.PH_I64, hip.PH_DATE, hip.PH_DEC64, hip.PH_STR
OK, EINVAL, EUNSUPPORTED = hip.PH_OK, hip.PH_EINVAL, hip.PH_EUNSUPPORTED
BARE, QUOTE = Q.BARE, Q.QUOTE

# text -> the records' values, written out by hand, and the first quoting error (row, kind) or None
LITERAL = [
    (b'"a|b"|c', [[b"a|b", b"c"]], None),
    (b'"a\nb"|c\n', [[b"a\nb", b"c"]], None),
    (b'"a""b"', [[b'a"b']], None),
    (b'""|x\n', [[b"", b"x"]], None),
    (b'"a"\r\n"b"', [[b"a"], [b"b"]], None),
    (b'"a\r\nb"', [[b"a\nb"]], None),                                  # "\r\n" inside quotes is the one byte '\n'
    (b'"a\rb"', [[b"a\rb"]], None),                                    # a lone '\r' is kept
    (b'x\n"abc"', [[b"x"], [b"abc"]], None),                           # no newline at the end of input
    (b'"abc"\r', [[b"abc"]], None),                                    # one '\r' at the end of input is dropped
    (b'"a\n\n\r\nb"|1\n2|3', [[b"a\n\n\nb", b"1"], [b"2", b"3"]], None),   # empty lines inside quotes are data
    (b'\n\r\n"a"\n\n"b"\r\n\r\n', [[b"a"], [b"b"]], None),            # empty lines between records are skipped
    (b'""""|""""""', [[b'"', b'""']], None),
    (b'"|"|"\n"|\n', [[b"|", b"\n", b""]], None),
    (b'"a"|', [[b"a", b""]], None),
    (b'a|"b"\r\nc|"d\r\r\n"\n', [[b"a", b"b"], [b"c", b"d\r\n"]], None),   # "\r\r\n": only the last '\r' belongs to the line end
    (b'x\na"b\n', [[b"x"]], (1, BARE)),
    (b' "x"\n', [], (0, BARE)),
    (b'x|"y"z\n', [], (0, QUOTE)),
    (b'"a"b', [], (0, QUOTE)),
    (b'"a"\rb', [], (0, QUOTE)),                                       # a lone '\r' behind the closing quote, not at the end of input
    (b'"a"\r\r\n', [], (0, QUOTE)),
    (b'x\n"abc', [[b"x"]], (1, QUOTE)),                                # the end of input inside a quoted field
    (b'x\n"abc\r', [[b"x"]], (1, QUOTE)),
    (b'x\n"abc"\n"', [[b"x"], [b"abc"]], (2, QUOTE)),
    (b'a|b\nc|d|e"f\n', [[b"a", b"b"]], (1, BARE)),
]


def values(records):
    return [[v for v, _quoted, _escaped in rec] for rec in records]


def test_restatement_holds_the_literal_table():
    for text, want, err in LITERAL:
        got, got_err = Q.read_all(text)
        assert (values(got), got_err) == (want, err), text
    assert Q.read_all(b'"a,b",c', b",") == ([[(b"a,b", True, False), (b"c", False, False)]], None)
    assert Q.read_all(b'"a""b\r\nc"|"d"|e')[0] == [[(b'a"b\nc', True, True), (b"d", True, False), (b"e", False, False)]]


def test_load_orders_the_errors_as_the_reader_does():
    """(text, columns) -> (code, failing row)"""
    two = [(0, I32, 0), (1, STR, 0)]
    cases = [
        (b'1|"a"\n"2"|b\n""|"c""d"\n', two, (OK, None)),
        (b'1|a\n2|b|c"d\n3|e\n', two, (EINVAL, 1)),               # a field-count mismatch and a bare quote in one row: the quote error
        (b'1|a\nx|b\n3|c\n4|d"e\n', two, (EINVAL, 1)),            # a bad integer on row 1, a bare quote on row 3: row 1
        (b'1|a\n2|b\n3|"c\n', two, (EINVAL, 2)),
        (b'1|a\n2|b"\nx|c\n', two, (EINVAL, 1)),                  # the quote error on row 1 hides the bad integer behind it
        (b'1|a\n2\n3|"c\n', two, (EINVAL, 1)),                    # a field-count mismatch before the quote error
        (b'1|a\n"2""3"|b\n', two, (EINVAL, 1)),                   # an escape inside a quoted integer: no integer
        (b'99999999999|a\n2|b"\n', two, (hip.PH_EOVERFLOW, 0)),
    ]
    for text, cols, want in cases:
        got = Q.load(text, cols)
        assert (got.code, got.row) == want, text
    got = Q.load(b'1|"a"\n"2"|b\n""|"c""d\r\ne"\n', two)
    assert got.nrows == 3 and got.columns[0][1].tolist() == [1, 2, 0] and got.columns[0][2].tolist() == [False, False, True]
    assert got.columns[1] [0] == "code8" and got.columns[1][2] == [b"a", b"b", b'c"d\ne']
    dec = Q.load(b'""|""\n"1.5"|"2001-02-03"\n', [(0, DEC, 2), (1, DATE, 0)])
    assert dec.columns[0][1].tolist() == [0, 150] and not dec.columns[0][2].any() and dec.columns[1][2].tolist() == [True, False]
    assert Q.load(b'1|"a"\n', two, quoting=False).code == EUNSUPPORTED and Q.load(b"1|a\n", two, b'"').code == EINVAL


# ---------------------------------------------------------------- seeded random texts

TOKENS = [b'"', b"|", b"\n", b"\r", b"\r\n", b'""', b'"|', b'|"', b'"\n', b'\n"', b"a", b"b", b"xy"]


def random_text(rng):
    """up to 14 tokens; about two thirds of such texts are malformed"""
    return b"".join(rng.choice(TOKENS) for _ in range(rng.randint(0, 14)))


def well_formed_text(rng, cr=False):
    """records of one fixed field count (2..4), fields quoted at random over contents that hold the delimiter, line breaks and quotes"""
    nf = rng.randint(2, 4)
    pieces = [b"a", b"bc", b"|", b"\n", b'"', b"\n\n", b" "] + ([b"\r\n", b"\r"] if cr else [])
    out = []
    for _ in range(rng.randint(1, 5)):
        fields = []
        for _ in range(nf):
            content = b"".join(rng.choice(pieces) for _ in range(rng.randint(0, 4)))
            if rng.random() < 0.5 or any(c in content for c in b'|\n\r"'):
                fields.append(b'"' + content.replace(b'"', b'""') + b'"')
            else:
                fields.append(content)
        out.append(b"|".join(fields))
        out.append(rng.choice([b"\n", b"\n", b"\n\n"]))
    if rng.random() < 0.3:
        out.pop()                                # the final record without a newline
    return b"".join(out)


def test_restatement_agrees_with_the_csv_module_on_well_formed_text():
    rng = random.Random(20240)
    for _ in range(4000):
        text = well_formed_text(rng)
        got, err = Q.read_all(text)
        want = [[f.encode() for f in row] for row in csv.reader(io.StringIO(text.decode(), newline=""), delimiter="|", strict=True) if row]
        assert err is None and values(got) == want, text


def test_restatement_agrees_with_pyarrow_csv_on_well_formed_text():
    pa = pytest.importorskip("pyarrow")
    import pyarrow.csv as pacsv
    rng = random.Random(20241)
    for _ in range(1500):
        text = well_formed_text(rng)
        got, err = Q.read_all(text)
        nf = len(got[0])
        names = ["c%d" % i for i in range(nf)]
        tbl = pacsv.read_csv(io.BytesIO(text), read_options=pacsv.ReadOptions(column_names=names),
                             parse_options=pacsv.ParseOptions(delimiter="|", quote_char='"', double_quote=True, newlines_in_values=True),
                             convert_options=pacsv.ConvertOptions(column_types={n: pa.binary() for n in names}, strings_can_be_null=False))
        want = [list(row) for row in zip(*[tbl.column(n).to_pylist() for n in names])]
        assert err is None and values(got) == want, text


def split_all(text, flags=hip.PH_CSV_QUOTES):
    """ph_csv_split_record chained through *next -> (records as the restatement writes them, None or (row, kind))"""
    out, pos = [], 0
    while True:
        rc, fields, nf, nxt = hip.csv_split_record(text, pos, "|", flags)
        if rc != OK:
            assert rc == EINVAL
            msg = hip.last_error()
            kind = BARE if BARE in msg else QUOTE
            assert kind in msg
            return out, (len(out), kind)
        if nf == 0:
            assert nxt == len(text)
            return out, None
        assert nf == len(fields)
        out.append([(Q.unescape(text[b:e]) if fl & 1 else text[b:e], bool(fl & 1), bool(fl & 2)) for b, e, fl in fields])
        if nxt >= len(text):
            return out, None
        assert nxt > pos
        pos = nxt


def test_split_record_equals_the_restatement():
    """fields, flags, error or none and its kind: the literal table, well-formed texts with '\\r', random texts"""
    for text, want, err in LITERAL:
        got, got_err = split_all(text)
        assert (values(got), got_err) == (want, err) and (got, got_err) == Q.read_all(text), text
    rng = random.Random(20242)
    for _ in range(3000):
        text = well_formed_text(rng, cr=True)
        assert split_all(text) == Q.read_all(text), text
    malformed = 0
    for _ in range(20000):
        text = random_text(rng)
        want = Q.read_all(text)
        assert split_all(text) == want, text
        malformed += want[1] is not None
    assert 10000 < malformed < 16000
    # flags 0: a '"' is a byte like any other (the load refuses such a text as a whole), and the records are csv_reference's
    for text in (b'a"b|c\n"d|e\r\n\nf|g', b"1|2|\n\n3|4|\r"):
        got, err = split_all(text, 0)
        assert err is None and values(got) == R.records(text)
    assert hip.csv_split_record(b"a|b\n", 0, "|", 2)[0] == EINVAL and hip.csv_split_record(b"a|b\n", 0, '"', 1)[0] == EINVAL
    assert hip.csv_split_record(b"a|b|c\n", 0, "|", 1, cap=2)[1:3] == ([(0, 1, 0), (2, 3, 0)], 3)      # more fields than cap: counted, not stored


def test_device_form_equals_the_sequential_restatement():
    """record starts by quote parity + every record walked up to the next start give the reader's records on every well-formed text, and
    its first failing row, the error's kind and all rows before it on every malformed one"""
    for text, _want, _err in LITERAL:
        assert Q.device_records(text) == Q.read_all(text), text
    rng = random.Random(20243)
    malformed = 0
    for _ in range(100000):
        text = random_text(rng)
        want = Q.read_all(text)
        assert Q.device_records(text) == want, text
        malformed += want[1] is not None
    assert 55000 < malformed < 75000
    for _ in range(2000):
        text = well_formed_text(rng, cr=True)
        assert Q.device_records(text) == Q.read_all(text), text
