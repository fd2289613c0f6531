"""Delimited-text load path without a device: the Python restatement of the reference's CSV scan (tests/csv_reference.py) against
pyarrow.csv on benign text and against a literal table where pyarrow differs; ph_csv_parse_field — the SAME function the device parser
runs — against the restatement over an edge table; and the two new ABI entry points."""
import datetime
import decimal
import os
import re

import numpy as np
import pytest

import csv_reference as R
from plan_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32, I64, DATE, DEC, STR = hip.PH_I32, hip.PH_I64, hip.PH_DATE, hip.PH_DEC64, hip.PH_STR
OK, EINVAL, EUNSUPPORTED, EOVERFLOW = hip.PH_OK, hip.PH_EINVAL, hip.PH_EUNSUPPORTED, hip.PH_EOVERFLOW

# CRLF and LF mixed, empty lines, a trailing delimiter, a last line without newline, empty INTEGER / DATE fields, dates before 1970 and
# on 2000-02-29 — and no '+' sign or empty DECIMAL (pyarrow rejects the first and makes the second NULL: pinned literally below)
BENIGN = (b"1|10000000000|1998-12-01|12.50|first|\r\n"
          b"\n"
          b"-2|-5|1969-12-31|-0.05|second|\n"
          b"|7|2000-02-29|3|third|\r\n"
          b"\r\n"
          b"\n"
          b"007||1900-01-01|0.5||\n"
          b"2147483647|-9223372036854775808||99999999999.99|caf\xc3\xa9|\r\n"
          b"5|6|1970-01-01|1|last|")
BENIGN_COLS = [(0, I32, 0), (1, I64, 0), (2, DATE, 0), (3, DEC, 2), (4, STR, 0)]


def test_restatement_agrees_with_pyarrow_csv_on_benign_text():
    pa = pytest.importorskip("pyarrow")
    import io

    import pyarrow.csv as pacsv
    names = ["a", "b", "c", "d", "e", "trail"]
    types = {"a": pa.int32(), "b": pa.int64(), "c": pa.date32(), "d": pa.decimal128(15, 2), "e": pa.string(), "trail": pa.string()}
    tbl = pacsv.read_csv(io.BytesIO(BENIGN), read_options=pacsv.ReadOptions(column_names=names),
                         parse_options=pacsv.ParseOptions(delimiter="|", quote_char=False),
                         convert_options=pacsv.ConvertOptions(column_types=types, strings_can_be_null=False))
    got = R.load(BENIGN, BENIGN_COLS)
    assert got.code == OK and got.nrows == tbl.num_rows == 6
    epoch = datetime.date(1970, 1, 1)
    for k, name in enumerate(names[:4]):
        kind, vals, nulls = got.columns[k]
        want = tbl.column(name).to_pylist()
        assert kind == "fixed" and nulls.tolist() == [w is None for w in want], name
        for v, null, w in zip(vals.tolist(), nulls.tolist(), want):
            if null:
                assert v == 0
            elif name == "c":
                assert v == (w - epoch).days
            elif name == "d":
                assert v == int(w.scaleb(2)) and isinstance(w, decimal.Decimal)
            else:
                assert v == w
    kind, codes, dic = got.columns[4]
    assert kind == "code8" and [dic[c].decode() for c in codes] == tbl.column("e").to_pylist()
    assert tbl.column("trail").to_pylist() == [""] * 6            # the trailing delimiter is one more empty field


def test_restatement_pinned_where_pyarrow_differs_and_on_every_error():
    """literal expectations: (text, columns) -> (code, failing row or None, rows, first column's values / NULLs when it loads)"""
    cases = [
        (b"+7|\n", [(0, I32, 0)], (OK, None, 1, [7], [False])),                                   # '+' is ParseInt's
        (b"|x\n", [(0, DEC, 2)], (OK, None, 1, [0], [False])),                                    # the empty DECIMAL is 0, not NULL
        (b"+0.05|\n-0.05|\n", [(0, DEC, 2)], (OK, None, 2, [5, -5], [False, False])),
        (b"", [(0, I32, 0)], (OK, None, 0, [], [])),
        (b"\n\n\r\n", [(0, I32, 0)], (OK, None, 0, [], [])),
        (b"1|2\n3|4\r", [(1, I32, 0)], (OK, None, 2, [2, 4], [False, False])),                    # one trailing '\r' at the end of input is dropped
        (b"1|2\n3\n5|6\n", [(0, I32, 0)], (EINVAL, 1, 0, None, None)),                            # field count differs from the first record's
        (b"1|2\n3|4\n", [(2, I32, 0)], (EINVAL, 0, 0, None, None)),                               # no enough fields in the line
        (b'1|a"b\n', [(0, I32, 0)], (EUNSUPPORTED, None, 0, None, None)),                         # quoting is the host's
        (b"1\n2x\n", [(0, I32, 0)], (EINVAL, 1, 0, None, None)),
        (b"1\n2147483648\n", [(0, I32, 0)], (EOVERFLOW, 1, 0, None, None)),                       # the reference truncates; the library refuses
        (b"1\n9223372036854775808\n", [(0, I64, 0)], (EOVERFLOW, 1, 0, None, None)),
        (b"1998-02-30\n", [(0, DATE, 0)], (EINVAL, 0, 0, None, None)),
        (b"1.5\n1.555\n", [(0, DEC, 2)], (EUNSUPPORTED, 1, 0, None, None)),
        (b"1e2\n", [(0, DEC, 2)], (EUNSUPPORTED, 0, 0, None, None)),
        (b"12345678901234567890\n", [(0, DEC, 2)], (EOVERFLOW, 0, 0, None, None)),
        (b"1\n2x\n1|2\n", [(0, I32, 0)], (EINVAL, 1, 0, None, None)),                             # the lowest failing row is the one reported
    ]
    for text, cols, (code, row, nrows, vals, nulls) in cases:
        got = R.load(text, cols)
        assert (got.code, got.row) == (code, row), text
        if code == OK:
            assert got.nrows == nrows and got.columns[0][1].tolist() == vals and got.columns[0][2].tolist() == nulls, text
    assert R.load(b"1,2\n", [(0, I32, 0)], b'"').code == EINVAL
    assert R.load(b"1,2\n", [(0, I32, 0)], b"\n").code == EINVAL


def days(y, m, d):
    return (datetime.date(y, m, d) - datetime.date(1970, 1, 1)).days


# (type, scale, field) -> (code, value, NULL): written out, so that the restatement and the library are BOTH held to it
EDGES = [
    (I64, 0, b"0", (OK, 0, False)), (I64, 0, b"-0", (OK, 0, False)), (I64, 0, b"+7", (OK, 7, False)), (I64, 0, b"007", (OK, 7, False)),
    (I32, 0, b"2147483647", (OK, 2**31 - 1, False)), (I32, 0, b"-2147483648", (OK, -2**31, False)),
    (I32, 0, b"2147483648", (EOVERFLOW, 0, False)), (I32, 0, b"-2147483649", (EOVERFLOW, 0, False)),
    (I64, 0, b"9223372036854775807", (OK, 2**63 - 1, False)), (I64, 0, b"-9223372036854775808", (OK, -2**63, False)),
    (I64, 0, b"9223372036854775808", (EOVERFLOW, 0, False)), (I64, 0, b"-9223372036854775809", (EOVERFLOW, 0, False)),
    (I64, 0, b"18446744073709551616", (EOVERFLOW, 0, False)), (I64, 0, b"99999999999999999999x", (EOVERFLOW, 0, False)),
    (I64, 0, b"9223372036854775808x", (EINVAL, 0, False)),
    (I32, 0, b"", (OK, 0, True)), (I64, 0, b"", (OK, 0, True)), (DATE, 0, b"", (OK, 0, True)),
    (I64, 0, b" 1", (EINVAL, 0, False)), (I64, 0, b"1 ", (EINVAL, 0, False)), (I64, 0, b"1_0", (EINVAL, 0, False)),
    (I64, 0, b"-", (EINVAL, 0, False)), (I64, 0, b"+", (EINVAL, 0, False)), (I64, 0, b"0x1", (EINVAL, 0, False)), (I32, 0, b"1.0", (EINVAL, 0, False)),
    (DATE, 0, b"0001-01-01", (OK, days(1, 1, 1), False)), (DATE, 0, b"1969-12-31", (OK, -1, False)), (DATE, 0, b"1970-01-01", (OK, 0, False)),
    (DATE, 0, b"1900-02-29", (EINVAL, 0, False)), (DATE, 0, b"2000-02-29", (OK, days(2000, 2, 29), False)),
    (DATE, 0, b"1998-02-30", (EINVAL, 0, False)), (DATE, 0, b"1998-2-03", (EINVAL, 0, False)), (DATE, 0, b"1998-12-011", (EINVAL, 0, False)),
    (DATE, 0, b"9999-12-31", (OK, days(9999, 12, 31), False)), (DATE, 0, b"1998-13-01", (EINVAL, 0, False)), (DATE, 0, b"1998-00-10", (EINVAL, 0, False)),
    (DATE, 0, b"1998-04-31", (EINVAL, 0, False)), (DATE, 0, b"1998/04/30", (EINVAL, 0, False)), (DATE, 0, b"1996-02-29", (OK, days(1996, 2, 29), False)),
    (DATE, 0, b"0000-01-01", (OK, days(1, 1, 1) - 366, False)),
    (DEC, 2, b"1", (OK, 100, False)), (DEC, 2, b"1.5", (OK, 150, False)), (DEC, 2, b"1.50", (OK, 150, False)),
    (DEC, 2, b"-0.05", (OK, -5, False)), (DEC, 2, b"+0.05", (OK, 5, False)), (DEC, 2, b"", (OK, 0, False)),
    (DEC, 2, b"1.555", (EUNSUPPORTED, 0, False)), (DEC, 2, b".5", (EUNSUPPORTED, 0, False)), (DEC, 2, b"5.", (EUNSUPPORTED, 0, False)),
    (DEC, 2, b"1e2", (EUNSUPPORTED, 0, False)), (DEC, 2, b"-", (EUNSUPPORTED, 0, False)), (DEC, 2, b"1.2.3", (EUNSUPPORTED, 0, False)),
    (DEC, 2, b"1234567890123456.78", (OK, 123456789012345678, False)), (DEC, 2, b"12345678901234567890", (EOVERFLOW, 0, False)),
    (DEC, 2, b"92233720368547758.07", (OK, 2**63 - 1, False)), (DEC, 2, b"92233720368547758.08", (EOVERFLOW, 0, False)),
    (DEC, 2, b"-92233720368547758.08", (OK, -2**63, False)), (DEC, 2, b"-92233720368547758.09", (EOVERFLOW, 0, False)),
    (DEC, 2, b"92233720368547758.1", (EOVERFLOW, 0, False)),          # fits before the padding, not after
    (DEC, 0, b"42", (OK, 42, False)), (DEC, 0, b"-42", (OK, -42, False)), (DEC, 0, b"42.0", (EUNSUPPORTED, 0, False)),
    (DEC, 18, b"1.000000000000000001", (OK, 10**18 + 1, False)), (DEC, 18, b"10", (EOVERFLOW, 0, False)),
]


def test_restatement_holds_the_edge_table():
    for typ, scale, field, want in EDGES:
        assert R.field_value(typ, scale, field) == want, (typ, scale, field)


def test_ph_csv_parse_field_agrees_with_the_restatement_on_the_edges():
    """the host entry point runs the function the kernel runs (plan_amd/csrc/csv_parse.h)"""
    for typ, scale, field, want in EDGES:
        assert hip.csv_parse_field(typ, scale, field) == R.field_value(typ, scale, field) == want, (typ, scale, field)
    # every date of a leap and a non-leap February, and a sweep of integers around the powers of ten
    for y in (1900, 1999, 2000, 2024):
        for d in range(0, 32):
            f = b"%04d-02-%02d" % (y, d)
            assert hip.csv_parse_field(DATE, 0, f) == R.field_value(DATE, 0, f), f
    for e in range(0, 20):
        for delta in (-1, 0, 1):
            for sign in (b"", b"-"):
                f = sign + str(10**e + delta).encode()
                assert hip.csv_parse_field(I64, 0, f) == R.field_value(I64, 0, f), f
                assert hip.csv_parse_field(DEC, 2, f) == R.field_value(DEC, 2, f), f
    assert hip.lib().ph_csv_parse_field(hip.i32(STR), hip.i32(0), b"x", hip.i64(1), None, None) == EINVAL
    rc, _v, _n = hip.csv_parse_field(I64, 0, b"12a")
    assert rc == EINVAL and "integer" in hip.last_error()


def test_abi_declares_and_exports_the_text_load_entry_points():
    header = open(os.path.join(ROOT, "include", "planhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = hip.lib()
    for name in ("ph_table_create_csv", "ph_csv_parse_field"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name), f"libplanhip.so does not export {name}"
    assert "ph_csv_col" in code and "executor_scan.go:107-120" in header and "vector.go:195-264" in header
    # bad arguments are codes, not aborts — and need no device
    out = hip.vp()
    cols = (hip.CsvCol * 1)(hip.CsvCol(0, I32, 0))
    import ctypes
    assert lib.ph_table_create_csv(None, b"1\n", hip.i64(2), hip.i32(ord("|")), cols, hip.i32(1), ctypes.byref(out)) == EINVAL
