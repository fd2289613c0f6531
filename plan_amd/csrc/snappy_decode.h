// Snappy's block format (a varint length, then elements), decoded by ONE set of functions compiled for the host (ph_snappy_decompress_host
// and the Parquet host twin, sequentially) and for the device (snappy_decompress.hip, whose kernel shares the preamble check and the
// element parser and carries the literals and copies out inside LDS). In the manner of parquet_decode.h: a byte getter g with u8(p).
//
// An element is a tag byte whose low two bits give its kind:
//   00 literal   upper 6 bits = len - 1 for 1..60; 60..63: 1..4 little-endian bytes of len - 1 follow; then len bytes
//   01 copy      len 4..11 = 4 + bits 2..4, offset 11 bits = bits 5..7 << 8 | next byte
//   10 copy      len 1..64 = 1 + upper 6 bits, offset = next 2 bytes, little-endian
//   11 copy      len 1..64 = 1 + upper 6 bits, offset = next 4 bytes, little-endian
// A copy takes bytes that lie `offset` behind the write position and may overlap what it writes (offset < len repeats a pattern).
//
// Bounds. parse_element reads at most 5 bytes, every one checked against the stream's end, and decides before anything is copied that a
// literal's bytes lie inside the stream, that a copy's offset is 1..produced, and that the element ends at or before the expected length.
// Every element consumes at least one input byte, so the element loop is bounded by the stream's length; nothing is written outside
// [dst, dst + expected) and nothing is read outside [pos, end).
#pragma once
#include <cstdint>

#include "planhip.h"

#if defined(__HIPCC__)
#define PH_SN_HD __host__ __device__ __forceinline__
#else
#define PH_SN_HD inline
#endif

namespace ph {
namespace snappy {

// why a stream is refused (all of them PH_EINVAL)
enum Sub : int {
    S_OK = 0,
    S_PREAMBLE = 1,       // the length preamble is missing, longer than 5 bytes or exceeds 32 bits
    S_LENGTH = 2,         // the preamble disagrees with the expected length
    S_IMPOSSIBLE = 3,     // the preamble promises more than 22 bytes per stream byte
    S_OFFSET_ZERO = 4,    // a copy with offset 0
    S_OFFSET_FAR = 5,     // a copy that reaches in front of the first byte produced
    S_INPUT_CUT = 6,      // a literal or a copy operand runs past the input
    S_OUTPUT_PAST = 7,    // an element writes past the expected length
    S_INPUT_SHORT = 8,    // the input ends before the expected length is reached
    S_INPUT_LEFT = 9,     // input is left over once the expected length is reached
};

inline const char *sub_text(int s) {
    switch (s) {
    case S_PREAMBLE: return "the length preamble is missing, longer than 5 bytes or exceeds 32 bits";
    case S_LENGTH: return "the length preamble disagrees with the expected length";
    case S_IMPOSSIBLE: return "the length preamble promises more than 22 bytes per stream byte";
    case S_OFFSET_ZERO: return "a copy with offset 0";
    case S_OFFSET_FAR: return "a copy offset beyond the bytes produced so far";
    case S_INPUT_CUT: return "a literal or a copy operand runs past the input";
    case S_OUTPUT_PAST: return "an element writes past the expected length";
    case S_INPUT_SHORT: return "the input ends before the expected length is reached";
    case S_INPUT_LEFT: return "input is left over once the expected length is reached";
    default: return "unknown cause";
    }
}

// No element yields more than 64 bytes from fewer than 3 input bytes (a copy with a 2-byte offset): 22 bytes per stream byte bound any
// honest stream, so what a stream is allowed to make a caller allocate is bounded by the stream's own size.
constexpr int64_t MAX_EXPANSION = 22;

// The preamble of the stream [pos, end): *len = the uncompressed length, *body = the first element's position. expected < 0: any length.
template <class G>
PH_SN_HD int read_preamble(const G &g, int64_t pos, int64_t end, int64_t expected, int64_t *len, int64_t *body) {
    uint64_t v = 0;
    int k = 0;
    for (;; k++) {
        if (k == 5 || pos + k >= end) return S_PREAMBLE;
        const uint32_t b = g.u8(pos + k);
        v |= (uint64_t)(b & 0x7fu) << (7 * k);
        if (!(b & 0x80u)) break;
    }
    if (v > 0xffffffffull) return S_PREAMBLE;
    *len = (int64_t)v;
    *body = pos + k + 1;
    if (expected >= 0 && (int64_t)v != expected) return S_LENGTH;
    if ((int64_t)v > MAX_EXPANSION * (end - pos)) return S_IMPOSSIBLE;
    return S_OK;
}

struct Element {
    int32_t copy;      // 0: a literal of `len` bytes that begin at `data`; 1: a copy of `len` bytes from `offset` behind the write position
    int64_t len;       // 1 .. 2^32
    int64_t offset;    // copy: 1 .. produced
    int64_t data;      // the first byte behind the tag and its operands (a literal's bytes; a copy: the next element)
};

// The element at `pos` of a stream that ends at `end`, with `produced` of `expected` bytes written so far. S_OK: the element is safe to
// carry out as it stands.
template <class G>
PH_SN_HD int parse_element(const G &g, int64_t pos, int64_t end, int64_t produced, int64_t expected, Element *e) {
    const uint32_t tag = g.u8(pos);   // (the caller has pos < end)
    const uint32_t kind = tag & 3u, up = tag >> 2;
    int64_t p = pos + 1;
    if (kind == 0) {
        uint32_t lm1 = up;
        if (up >= 60) {
            const int nb = (int)up - 59;
            if (nb > end - p) return S_INPUT_CUT;
            lm1 = 0;
            for (int k = 0; k < nb; k++) lm1 |= (uint32_t)g.u8(p + k) << (8 * k);
            p += nb;
        }
        e->copy = 0;
        e->len = (int64_t)lm1 + 1;
        e->offset = 0;
        e->data = p;
        if (e->len > expected - produced) return S_OUTPUT_PAST;
        if (e->len > end - p) return S_INPUT_CUT;
        return S_OK;
    }
    const int nb = kind == 1 ? 1 : kind == 2 ? 2 : 4;
    if (nb > end - p) return S_INPUT_CUT;
    uint32_t off = 0;
    for (int k = 0; k < nb; k++) off |= (uint32_t)g.u8(p + k) << (8 * k);
    e->copy = 1;
    if (kind == 1) { e->len = 4 + (up & 7u); off |= (up >> 3) << 8; }
    else e->len = 1 + (int64_t)up;
    e->offset = (int64_t)off;
    e->data = p + nb;
    if (off == 0) return S_OFFSET_ZERO;
    if ((int64_t)off > produced) return S_OFFSET_FAR;
    if (e->len > expected - produced) return S_OUTPUT_PAST;
    return S_OK;
}

// The elements of [pos, end) into a sink of `expected` bytes, one behind the other. The sink has literal(g, from, at, n) (n bytes of the
// stream from `from` to output position `at`) and copy(at, offset, n) (byte by byte, front to back: an overlapping copy repeats).
template <class G, class S>
PH_SN_HD int decode_elements(const G &g, int64_t pos, int64_t end, int64_t expected, S &sink) {
    int64_t produced = 0;
    while (produced < expected) {
        if (pos >= end) return S_INPUT_SHORT;
        Element e;
        const int s = parse_element(g, pos, end, produced, expected, &e);
        if (s != S_OK) return s;
        if (e.copy) { sink.copy(produced, e.offset, e.len); pos = e.data; }
        else { sink.literal(g, e.data, produced, e.len); pos = e.data + e.len; }
        produced += e.len;
    }
    return pos == end ? S_OK : S_INPUT_LEFT;
}

struct HostStream {
    const uint8_t *s;
    uint8_t u8(int64_t p) const { return s[p]; }
};

struct HostSink {
    uint8_t *d;
    void literal(const HostStream &g, int64_t from, int64_t at, int64_t n) { for (int64_t i = 0; i < n; i++) d[at + i] = g.s[from + i]; }
    void copy(int64_t at, int64_t offset, int64_t n) { for (int64_t i = 0; i < n; i++) d[at + i] = d[at - offset + i]; }
};

// One whole stream src[0, src_bytes) on the host into dst[0, expected). expected < 0: what the preamble says, at most dst_cap (*len tells).
// dst may be null when nothing is to be written (expected 0, or only the length is wanted: decode = false).
inline int decompress_host(const uint8_t *src, int64_t src_bytes, uint8_t *dst, int64_t expected, int64_t *len, bool decode = true) {
    const HostStream g{src};
    int64_t n = 0, body = 0;
    const int s = read_preamble(g, 0, src_bytes, expected, &n, &body);
    if (len) *len = n;
    if (s != S_OK || !decode) return s;
    HostSink sink{dst};
    return decode_elements(g, body, src_bytes, n, sink);
}

}  // namespace snappy
}  // namespace ph
