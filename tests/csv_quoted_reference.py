"""Plain-Python restatement of encoding/csv's quoted-field grammar, the yardstick of PH_CSV_QUOTES (ph_table_create_csv_ex,
ph_csv_split_record). Test infrastructure only; tests/csv_reference.py stays the yardstick of the flags-0 load and of the values.

Two restatements, held against each other by tests/test_csv_quoted_reference.py:
  sequential   read_line / read_record / read_all: Go's Reader.readLine and Reader.readRecord with only Comma set (LazyQuotes,
               TrimLeadingSpace and Comment off), line at a time, in Go's order of tests. A record is a list of (value, quoted, escaped):
               escaped says that the value is shorter than the bytes between the quotes (a "" or a "\\r\\n" inside them).
  device form  device_records: what the kernels do. Record starts are the positions that pass the flags-0 test (behind a '\\n', not an empty
               line) AND have an even number of '"' bytes before them; every record is then walked by walk_field (a port of
               plan_amd/csrc/csv_parse.h) from its start and never at or past the next start; the lowest failing row wins.
"""
import csv_reference as R

BARE, QUOTE = "bare quote", "extraneous or missing quote"      # Go's ErrBareQuote, ErrQuote (both PH_EINVAL)
NL, CR, DQ = 10, 13, 34


# ---------------------------------------------------------------- sequential, Go-shaped

def read_line(text, pos):
    """Reader.readLine -> (line, next position, whether "\\r\\n" was normalised) or None at the end of input"""
    if pos >= len(text):
        return None
    i = text.find(b"\n", pos)
    if i < 0:                                   # data and EOF: for backwards compatibility, drop trailing \r before EOF
        line = text[pos:]
        return (line[:-1] if line.endswith(b"\r") else line), len(text), False
    line = text[pos:i + 1]
    if line.endswith(b"\r\n"):                  # normalize \r\n to \n on all input lines
        return line[:-2] + b"\n", i + 1, True
    return line, i + 1, False


def read_record(text, pos, delimiter=b"|"):
    """Reader.readRecord -> (fields, error, next position); fields is None at the end of input, error None, BARE or QUOTE (fields then
    holds the fields before the failing one)"""
    while True:                                 # skip empty lines
        r = read_line(text, pos)
        if r is None:
            return None, None, pos
        line, pos, crlf = r
        if line not in (b"", b"\n"):
            break
    fields = []
    while True:                                 # parseField
        if line[:1] != b'"':                    # non-quoted string field
            i = line.find(delimiter)
            field = line[:i] if i >= 0 else (line[:-1] if line.endswith(b"\n") else line)
            if b'"' in field:
                return fields, BARE, pos
            fields.append((field, False, False))
            if i < 0:
                return fields, None, pos
            line = line[i + 1:]
            continue
        line = line[1:]                         # quoted string field
        buf, escaped = b"", False
        while True:
            i = line.find(b'"')
            if i >= 0:                          # hit next quote
                buf += line[:i]
                line = line[i + 1:]
                if line[:1] == b'"':            # `""` sequence (append quote)
                    buf += b'"'
                    line = line[1:]
                    escaped = True
                elif line[:1] == delimiter:     # `",` sequence (end of field)
                    line = line[1:]
                    fields.append((buf, True, escaped))
                    break
                elif line in (b"", b"\n"):      # `"\n` sequence (end of line)
                    fields.append((buf, True, escaped))
                    return fields, None, pos
                else:                           # `"*` sequence (invalid non-escaped quote)
                    return fields, QUOTE, pos
            elif line:                          # hit end of line (copy all data so far)
                buf += line
                escaped = escaped or crlf
                r = read_line(text, pos)
                line, pos, crlf = r if r is not None else (b"", pos, False)
            else:                               # abrupt end of file
                return fields, QUOTE, pos


def read_all(text, delimiter=b"|"):
    """every record up to the first quoting error -> (records, None or (row, BARE / QUOTE))"""
    out, pos = [], 0
    while True:
        fields, err, pos = read_record(text, pos, delimiter)
        if err is not None:
            return out, (len(out), err)
        if fields is None:
            return out, None
        out.append(fields)


# ---------------------------------------------------------------- the device form

def walk_field(t, delim, p, lim):
    """csv_parse.h walk_field<true> over bytes t -> (cause or None, begin, end, dropped bytes, quoted, last, next)"""
    if p >= lim:
        return QUOTE, p, p, 0, False, False, p
    if t[p] != DQ:
        q = p
        while True:
            if q >= lim:
                return QUOTE, p, q, 0, False, False, q
            c = t[q]
            if c == DQ:
                return BARE, p, q, 0, False, False, q
            if c == delim or c == NL:
                e = q - 1 if c == NL and q > p and t[q - 1] == CR else q
                return None, p, e, 0, False, c == NL, q + 1
            q += 1
    q, drop = p + 1, 0
    while True:
        if q >= lim:
            return QUOTE, p + 1, q, drop, True, False, q
        c = t[q]
        if c == DQ:
            if q + 1 >= lim:
                return QUOTE, p + 1, q, drop, True, False, q
            c1 = t[q + 1]
            if c1 == DQ:
                drop += 1
                q += 2
                continue
            if c1 == delim:
                return None, p + 1, q, drop, True, False, q + 2
            if c1 == NL:
                return None, p + 1, q, drop, True, True, q + 2
            if c1 == CR and q + 2 < lim and t[q + 2] == NL:
                return None, p + 1, q, drop, True, True, q + 3
            return QUOTE, p + 1, q, drop, True, False, q
        if c == CR and q + 1 < lim and t[q + 1] == NL:
            drop += 1
            q += 2
            continue
        q += 1


def unescape(raw):
    """the value of the bytes between a quoted field's quotes (already checked by the walk)"""
    return raw.replace(b"\r\n", b"\n").replace(b'""', b'"')


def device_starts(text):
    """the padded text (one '\\n' behind the input, as the device buffer has at least one) and the record starts by quote parity"""
    t = text + b"\n"
    starts, prev, inside = [], NL, False
    for p, c in enumerate(t):
        if prev == NL and not inside and c != NL and not (c == CR and t[p + 1] == NL):      # (the last byte is '\n': t[p + 1] is never read past it)
            starts.append(p)
        if c == DQ:
            inside = not inside
        prev = c
    return t, starts


def device_records(text, delimiter=b"|"):
    """-> (records before the lowest failing row, None or (row, BARE / QUOTE)): every row is walked on its own between its start and the
    next, as its thread does, and the lowest failing row is kept, as atomicMin keeps it"""
    t, starts = device_starts(text)
    delim = delimiter[0]
    out, err = [], None
    for r, p in enumerate(starts):
        lim = starts[r + 1] if r + 1 < len(starts) else len(t)
        fields, q, cause = [], p, None
        while True:
            cause, b, e, drop, quoted, last, q = walk_field(t, delim, q, lim)
            if cause is not None:
                break
            fields.append((unescape(t[b:e]) if quoted else t[b:e], quoted, drop > 0))
            if last:
                break
        while cause is None and q < lim:       # only empty lines up to the next start
            if t[q] == NL or (t[q] == CR and q + 1 < lim and t[q + 1] == NL):
                q += 1
            else:
                cause = QUOTE
        if cause is not None:
            err = (r, cause)
            break                               # (rows behind the lowest failing one may be cut anywhere: their reports lose)
        out.append(fields)
    return out, err


# ---------------------------------------------------------------- the load

def load(text, columns, delimiter=b"|", quoting=True):
    """columns: [(field, type, scale)] -> csv_reference.Loaded. With quoting the records are read_all's; the field-count rule, the value
    rules and the column encodings are csv_reference.load's own code, run over those records. A quoting error at row e is PH_EINVAL at e
    unless an earlier row fails for any cause."""
    if not quoting:
        return R.load(text, columns, delimiter)
    if len(delimiter) != 1 or delimiter in (b'"', b"\r", b"\n", b"\0") or delimiter[0] >= 128:
        return R.Loaded(R.EINVAL)
    recs, err = read_all(text, delimiter)
    values = [[value for value, _quoted, _escaped in rec] for rec in recs]
    saved = R.records
    R.records = lambda _text, _delimiter: values
    try:
        got = R.load(b"", columns, delimiter)
    finally:
        R.records = saved
    if got.code == R.OK and err is not None:
        return R.Loaded(R.EINVAL, err[0])
    return got
