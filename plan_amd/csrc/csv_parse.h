// The value rules of the delimited-text load path (ph_table_create_csv, planhip.h): ONE parser, compiled for the host
// (ph_csv_parse_field) and for the device (csv_load.hip's field kernel), so what a CPU test pins is what the kernel does.
//
// They restate fieldToValue (reference pkg/compute/executor_scan.go:364-408) + Vector.SetValue (pkg/chunk/vector.go:195-264):
// strconv.ParseInt(s, 10, 64) for INTEGER / BIGINT, time.Parse("2006-01-02") for DATE, ParseExact(field, scale) for DECIMAL.
// A field is addressed through a byte getter g(position) so that the kernel can read it out of LDS or global memory.
#pragma once
#include <cstdint>

#include "planhip.h"

#if defined(__HIPCC__)
#define PH_HD __host__ __device__ __forceinline__
#else
#define PH_HD inline
#endif

namespace ph {
namespace csv {

// why a record was refused; the host turns a cause into the return code and the message (csv_cause_code / csv_cause_text)
enum Cause : int {
    C_OK = 0,
    C_FIELD_COUNT = 1,   // the record's field count differs from the first record's            PH_EINVAL
    C_NO_FIELD = 2,      // a requested field lies past the record's last ("no enough fields")   PH_EINVAL
    C_INT_SYNTAX = 3,    // not [+-]digits                                                       PH_EINVAL
    C_INT_RANGE = 4,     // outside int64                                                        PH_EOVERFLOW
    C_I32_RANGE = 5,     // PH_I32: outside int32 (the reference truncates)                      PH_EOVERFLOW
    C_DATE = 6,          // not dddd-dd-dd, or no such day                                       PH_EINVAL
    C_DEC_FORM = 7,      // not [+-]digits[.digits] (a digit missing, an exponent, ...)          PH_EUNSUPPORTED
    C_DEC_SCALE = 8,     // more fractional digits than the column's scale                       PH_EUNSUPPORTED
    C_DEC_RANGE = 9,     // the unscaled value leaves int64                                      PH_EOVERFLOW
    C_TYPE = 10,         // no such column type                                                  PH_EINVAL
    C_BARE_QUOTE = 11,   // PH_CSV_QUOTES: a '"' inside an unquoted field (Go's ErrBareQuote)    PH_EINVAL
    C_QUOTE = 12,        // PH_CSV_QUOTES: extraneous or missing '"' in a quoted field (ErrQuote) PH_EINVAL
};

inline int cause_code(int cause) {
    switch (cause) {
    case C_OK: return PH_OK;
    case C_INT_RANGE: case C_I32_RANGE: case C_DEC_RANGE: return PH_EOVERFLOW;
    case C_DEC_FORM: case C_DEC_SCALE: return PH_EUNSUPPORTED;
    default: return PH_EINVAL;
    }
}

inline const char *cause_text(int cause) {
    switch (cause) {
    case C_FIELD_COUNT: return "the record's field count differs from the first record's";
    case C_NO_FIELD: return "no enough fields in the line";
    case C_INT_SYNTAX: return "not an integer ([+-]digits)";
    case C_INT_RANGE: return "integer outside the int64 range";
    case C_I32_RANGE: return "integer outside the int32 range of an INTEGER column";
    case C_DATE: return "not a date (YYYY-MM-DD, a day of the Gregorian calendar)";
    case C_DEC_FORM: return "decimal not of the plain form [+-]digits[.digits]";
    case C_DEC_SCALE: return "decimal with more fractional digits than the column's scale";
    case C_DEC_RANGE: return "decimal whose unscaled value leaves int64";
    case C_TYPE: return "column type without a text form";
    case C_BARE_QUOTE: return "bare quote: a '\"' inside a field that does not begin with one";
    case C_QUOTE: return "extraneous or missing quote: a '\"' in a quoted field not followed by '\"', the delimiter or the line end, or no closing quote";
    default: return "ok";
    }
}

// strconv.ParseInt(s, 10, 64) over a non-empty field: ParseUint walks the digits (a bad byte is a syntax error where it
// stands, a value past uint64 a range error where it happens), the int64 bounds are checked afterwards
template <class G>
PH_HD int parse_int(const G &g, int64_t b, int64_t e, int64_t *out) {
    bool neg = false;
    const unsigned char c0 = g(b);
    if (c0 == '+' || c0 == '-') { neg = c0 == '-'; b++; }
    if (b >= e) return C_INT_SYNTAX;
    unsigned long long v = 0;
    for (int64_t p = b; p < e; p++) {
        const unsigned d = (unsigned)g(p) - '0';
        if (d > 9u) return C_INT_SYNTAX;
        if (v > 0xffffffffffffffffull / 10) return C_INT_RANGE;
        v *= 10;
        if (v + d < v) return C_INT_RANGE;
        v += d;
    }
    if (neg ? v > (1ull << 63) : v >= (1ull << 63)) return C_INT_RANGE;
    *out = neg ? (int64_t)(0ull - v) : (int64_t)v;
    return C_OK;
}

// days since 1970-01-01 of a proleptic Gregorian date (year >= 0)
PH_HD int64_t days_from_civil(int64_t y, int m, int d) {
    y -= m <= 2;
    const int64_t era = (y >= 0 ? y : y - 399) / 400;
    const int64_t yoe = y - era * 400;
    const int64_t doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
    const int64_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
    return era * 146097 + doe - 719468;
}

// time.Parse("2006-01-02", s): four, two and two digits between '-', month 1..12, a day that month has
template <class G>
PH_HD int parse_date(const G &g, int64_t b, int64_t e, int64_t *out) {
    if (e - b != 10) return C_DATE;
    int v[3] = {0, 0, 0};
    const int at[3] = {0, 5, 8}, nd[3] = {4, 2, 2};
    for (int k = 0; k < 3; k++)
        for (int j = 0; j < nd[k]; j++) {
            const unsigned d = (unsigned)g(b + at[k] + j) - '0';
            if (d > 9u) return C_DATE;
            v[k] = v[k] * 10 + (int)d;
        }
    if (g(b + 4) != '-' || g(b + 7) != '-') return C_DATE;
    const int y = v[0], m = v[1], d = v[2];
    if (m < 1 || m > 12 || d < 1) return C_DATE;
    const bool leap = (y % 4 == 0 && y % 100 != 0) || y % 400 == 0;
    const int dim = m == 2 ? (leap ? 29 : 28) : (m == 4 || m == 6 || m == 9 || m == 11) ? 30 : 31;
    if (d > dim) return C_DATE;
    *out = days_from_civil(y, m, d);
    return C_OK;
}

// ParseExact(field, scale) for the plain form: the unscaled value at `scale`; the empty field is 0 (not NULL)
template <class G>
PH_HD int parse_dec(const G &g, int64_t b, int64_t e, int scale, int64_t *out) {
    *out = 0;
    if (b >= e) return C_OK;
    bool neg = false;
    const unsigned char c0 = g(b);
    if (c0 == '+' || c0 == '-') { neg = c0 == '-'; b++; }
    // the form first: digits [ '.' digits ], at least one digit on either side of a point
    int64_t point = -1;
    for (int64_t p = b; p < e; p++) {
        const unsigned char c = g(p);
        if (c == '.') { if (point >= 0) return C_DEC_FORM; point = p; }
        else if ((unsigned)c - '0' > 9u) return C_DEC_FORM;
    }
    const int64_t int_end = point >= 0 ? point : e;
    const int64_t nfrac = point >= 0 ? e - point - 1 : 0;
    if (int_end == b || (point >= 0 && nfrac == 0)) return C_DEC_FORM;
    if (nfrac > scale) return C_DEC_SCALE;
    unsigned long long v = 0;
    const unsigned long long lim = neg ? (1ull << 63) : (1ull << 63) - 1;
    for (int64_t p = b; p < e; p++) {
        if (p == point) continue;
        const unsigned d = (unsigned)g(p) - '0';
        if (v > (lim - d) / 10) return C_DEC_RANGE;
        v = v * 10 + d;
    }
    for (int64_t k = nfrac; k < scale; k++) {
        if (v > lim / 10) return C_DEC_RANGE;
        v *= 10;
    }
    *out = neg ? (int64_t)(0ull - v) : (int64_t)v;
    return C_OK;
}

// one fixed-width field [b, e) -> value (widened to int64) and NULL flag; the cause of a refusal otherwise
template <class G>
PH_HD int parse_field(int32_t type, int32_t scale, const G &g, int64_t b, int64_t e, int64_t *value, int *is_null) {
    *value = 0;
    *is_null = 0;
    if (type == PH_DEC64) return parse_dec(g, b, e, scale, value);
    if (type != PH_I32 && type != PH_I64 && type != PH_DATE) return C_TYPE;
    if (b >= e) { *is_null = 1; return C_OK; }
    if (type == PH_DATE) return parse_date(g, b, e, value);
    const int c = parse_int(g, b, e, value);
    if (c == C_OK && type == PH_I32 && (*value < INT32_MIN || *value > INT32_MAX)) { *value = 0; return C_I32_RANGE; }
    return c;
}

// ---- records: ONE walker over the byte getter, behind the field kernel, ph_csv_split_record and the host's count of the first record's fields.
//
// It restates encoding/csv's readRecord (strict: LazyQuotes, TrimLeadingSpace and Comment off) one field at a time. The caller
// guarantees that every record ends in '\n' (the device text is padded with '\n', the host getter reads '\n' behind the input: a final
// record without a newline, and one '\r' at the end of input, become ordinary lines) and names a bound: no byte at or past `lim` is read.
// On the device lim is the next record's start (the byte before it is a '\n'), so a malformed text cannot send a thread past its own
// stretch of the text; meeting the bound inside a quoted field is the missing closing quote.
struct Field {
    int64_t b, e;    // the content: inside the quotes for a quoted field, without the "\r" of a closing "\r\n" for an unquoted one
    int64_t drop;    // bytes of [b, e) the value does not hold: the second '"' of every "" and the '\r' of every "\r\n" (quoted fields only)
    int32_t quoted;  // the field began with '"'
    int32_t last;    // the record ends behind this field
};

constexpr int F_QUOTED = 1, F_ESCAPED = 2;   // ph_csv_split_record's field flags

// The field that starts at p. C_OK: *f is filled and *next is the byte behind the field's delimiter or behind the record's '\n'.
// QUOTES = false is the walk of the flags-0 load: '"' is no special byte there (the load refuses the text elsewhere) and lim is not looked at.
template <bool QUOTES, class G>
PH_HD int walk_field(const G &g, unsigned delim, int64_t p, int64_t lim, Field *f, int64_t *next) {
    f->b = p;
    f->drop = 0;
    f->quoted = 0;
    if (QUOTES && p >= lim) return C_QUOTE;
    if (!QUOTES || g(p) != '"') {
        for (int64_t q = p;; q++) {
            if (QUOTES && q >= lim) return C_QUOTE;   // (cannot happen while byte lim - 1 is a '\n': the walk stays bounded whatever it is given)
            const unsigned c = g(q);
            if (QUOTES && c == '"') return C_BARE_QUOTE;
            if (c != delim && c != '\n') continue;
            f->e = c == '\n' && q > p && g(q - 1) == '\r' ? q - 1 : q;   // "\r\n" ends a record like "\n"
            f->last = c == '\n';
            *next = q + 1;
            return C_OK;
        }
    }
    f->quoted = 1;
    f->b = p + 1;
    for (int64_t q = p + 1;;) {
        if (q >= lim) return C_QUOTE;                 // the end of input (or of this record's stretch) inside the quotes
        const unsigned c = g(q);
        if (c == '"') {
            if (q + 1 >= lim) return C_QUOTE;
            const unsigned c1 = g(q + 1);
            if (c1 == '"') { f->drop++; q += 2; continue; }                    // "" is one '"'
            f->e = q;
            if (c1 == delim) { f->last = 0; *next = q + 2; return C_OK; }
            if (c1 == '\n') { f->last = 1; *next = q + 2; return C_OK; }
            if (c1 == '\r' && q + 2 < lim && g(q + 2) == '\n') { f->last = 1; *next = q + 3; return C_OK; }
            return C_QUOTE;                                                     // "x, or " and a '\r' that ends no line
        }
        if (c == '\r' && q + 1 < lim && g(q + 1) == '\n') { f->drop++; q += 2; continue; }   // "\r\n" is the one byte '\n'
        q++;
    }
}

// an empty line ("\n" or "\r\n") at q, q < lim: its length, else 0
template <class G>
PH_HD int empty_line(const G &g, int64_t q, int64_t lim) {
    const unsigned c = g(q);
    if (c == '\n') return 1;
    return c == '\r' && q + 1 < lim && g(q + 1) == '\n' ? 2 : 0;
}

}  // namespace csv
}  // namespace ph
