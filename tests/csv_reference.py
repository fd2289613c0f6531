"""Plain-Python restatement of the reference's delimited-text scan, the yardstick of ph_table_create_csv / ph_csv_parse_field.

Test infrastructure only. What it restates:
  records   encoding/csv's Reader with only Comma set (pkg/compute/executor_scan.go:107-120): a record ends at "\\n", "\\r\\n" counts as
            "\\n", the last record needs no newline, one trailing "\\r" at the end of input is dropped, empty lines are skipped, every record
            has as many fields as the first; readCsvTable (:311-344) adds "no enough fields in the line" for a column past the record.
  values    fieldToValue (:364-408) + Vector.SetValue (pkg/chunk/vector.go:195-264): strconv.ParseInt(s, 10, 64), time.Parse("2006-01-02"),
            ParseExact(field, scale); the empty INTEGER / BIGINT / DATE field is NULL, the empty DECIMAL is 0, the empty VARCHAR is "".
The library's documented deviations are restated too (include/planhip.h): a '"' byte anywhere -> PH_EUNSUPPORTED, an INTEGER outside int32 ->
PH_EOVERFLOW (the reference truncates), a decimal outside the plain form or with too many fractional digits -> PH_EUNSUPPORTED.
"""
import re

import numpy as np

from plan_amd import hip

OK, EINVAL, EUNSUPPORTED, EOVERFLOW = hip.PH_OK, hip.PH_EINVAL, hip.PH_EUNSUPPORTED, hip.PH_EOVERFLOW
_DATE = re.compile(rb"\A([0-9]{4})-([0-9]{2})-([0-9]{2})\Z")
_DEC = re.compile(rb"\A([+-]?)([0-9]+)(?:\.([0-9]+))?\Z")
_DAYS_BEFORE = [0, 31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334]


def parse_int(s):
    """strconv.ParseInt(s, 10, 64) over a non-empty field -> (code, value): ParseUint walks the bytes (a bad byte is a syntax error where it
    stands, a value past uint64 a range error where it happens), ParseInt checks the int64 bounds afterwards"""
    neg = s[:1] == b"-"
    if s[:1] in (b"+", b"-"):
        s = s[1:]
    if not s:
        return EINVAL, 0
    n, out_of_range = 0, False
    for c in s:
        if not 48 <= c <= 57:
            return EINVAL, 0
        n = n * 10 + (c - 48)
        if n >= 1 << 64:
            out_of_range = True
            break
    if out_of_range or (n > 1 << 63 if neg else n >= 1 << 63):
        return EOVERFLOW, 0
    return OK, -n if neg else n


def parse_date(s):
    """time.Parse("2006-01-02", s) -> (code, days since 1970-01-01)"""
    m = _DATE.match(s)
    if not m:
        return EINVAL, 0
    y, mo, d = (int(g) for g in m.groups())
    leap = (y % 4 == 0 and y % 100 != 0) or y % 400 == 0
    if not 1 <= mo <= 12:
        return EINVAL, 0
    dim = [31, 29 if leap else 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31][mo - 1]
    if not 1 <= d <= dim:
        return EINVAL, 0
    # days before year y since year 0 (year 0 is a leap year of the proleptic calendar), counted from 0000-01-01
    before = y * 365 + (0 if y == 0 else (y - 1) // 4 - (y - 1) // 100 + (y - 1) // 400 + 1)
    doy = _DAYS_BEFORE[mo - 1] + (1 if leap and mo > 2 else 0) + d - 1
    return OK, before + doy - 719528          # 719528 = days from 0000-01-01 to 1970-01-01


def parse_dec(s, scale):
    """ParseExact(field, scale) for the plain form -> (code, unscaled int)"""
    if s == b"":
        return OK, 0
    m = _DEC.match(s)
    if not m:
        return EUNSUPPORTED, 0
    sign, ip, fp = m.group(1), m.group(2), m.group(3) or b""
    if len(fp) > scale:
        return EUNSUPPORTED, 0
    v = int(ip + fp + b"0" * (scale - len(fp)))
    v = -v if sign == b"-" else v
    if not -(1 << 63) <= v < 1 << 63:
        return EOVERFLOW, 0
    return OK, v


def field_value(typ, scale, field):
    """one field -> (code, value, is_null), the contract of ph_csv_parse_field"""
    if typ == hip.PH_DEC64:
        code, v = parse_dec(field, scale)
        return code, v, False
    if field == b"":
        return OK, 0, True
    if typ == hip.PH_DATE:
        code, v = parse_date(field)
        return code, v, False
    code, v = parse_int(field)
    if code == OK and typ == hip.PH_I32 and not -(1 << 31) <= v < 1 << 31:
        return EOVERFLOW, 0, False
    return code, v, False


def records(text, delimiter=b"|"):
    """the records encoding/csv reads (quoting aside): lists of fields"""
    out = []
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()                      # what follows the last newline is no line
    for line in lines:
        if line.endswith(b"\r"):
            line = line[:-1]             # "\r\n" -> "\n"; one "\r" at the end of input is dropped
        if line == b"":
            continue                     # empty lines are skipped
        out.append(line.split(delimiter))
    return out


class Loaded:
    """what a load gives: code (PH_OK or the error), row (the failing record, None for a whole-text error), nrows and per column
    ("fixed", int64 values with 0 in NULL slots, bool NULL mask) / ("code8", uint8 codes, [bytes]) / ("str", int32 offsets, bytes)"""

    def __init__(self, code, row=None, nrows=0, columns=None):
        self.code, self.row, self.nrows, self.columns = code, row, nrows, columns


def load(text, columns, delimiter=b"|"):
    """columns: [(field, type, scale)] -> Loaded"""
    if len(delimiter) != 1 or delimiter in (b'"', b"\r", b"\n", b"\0") or delimiter[0] >= 128:
        return Loaded(EINVAL)
    if b'"' in text:
        return Loaded(EUNSUPPORTED)
    recs = records(text, delimiter)
    vals = [[] for _ in columns]
    nulls = [[] for _ in columns]
    for r, rec in enumerate(recs):
        if len(rec) != len(recs[0]):
            return Loaded(EINVAL, r)
        for k, (field, typ, scale) in enumerate(columns):
            if field >= len(rec):
                return Loaded(EINVAL, r)
            if typ == hip.PH_STR:
                vals[k].append(rec[field])
                continue
            code, v, null = field_value(typ, scale, rec[field])
            if code != OK:
                return Loaded(code, r)
            vals[k].append(v)
            nulls[k].append(null)
    out = []
    for k, (_field, typ, _scale) in enumerate(columns):
        if typ != hip.PH_STR:
            out.append(("fixed", np.array(vals[k], dtype=np.int64), np.array(nulls[k], dtype=bool)))
            continue
        distinct = sorted(set(vals[k]))
        if len(distinct) <= 256 and not any(b"\0" in x for x in distinct):   # (a dictionary entry is a C string: a NUL byte keeps PH_STR)
            code_of = {s: i for i, s in enumerate(distinct)}
            out.append(("code8", np.array([code_of[s] for s in vals[k]], dtype=np.uint8), distinct))
        else:
            off = np.zeros(len(vals[k]) + 1, dtype=np.int64)
            np.cumsum([len(s) for s in vals[k]], out=off[1:])
            if off[-1] >= 1 << 31:
                return Loaded(EINVAL)
            out.append(("str", off.astype(np.int32), b"".join(vals[k])))
    return Loaded(OK, None, len(recs), out)
