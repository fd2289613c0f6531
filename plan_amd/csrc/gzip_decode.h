// GZIP (Parquet codec 2: RFC 1952 members around RFC 1951 DEFLATE), decoded by ONE set of functions compiled for the host
// (ph_gzip_decompress_host and the Parquet host twin, sequentially) and for the device (gzip_decompress.hip, whose kernel instantiates
// decode_stream over an LDS window, LDS tables and an LDS ring). In the manner of lz4_decode.h: a getter g, a sink and, new here, a set of
// tables t that the caller places (the stack on the host, LDS on the device).
//
// A stream is one or more members back to back:
//   header    1f 8b, CM = 8, FLG, MTIME (4), XFL, OS; then by FLG: FEXTRA (2-byte length + bytes), FNAME and FCOMMENT (zero-terminated),
//             FHCRC (the low 16 bits of the CRC-32 of the header's bytes so far). The reserved FLG bits 5..7 must be 0.
//   DEFLATE   blocks of 3 header bits (BFINAL, BTYPE) and: stored (byte-aligned LEN, ~LEN, bytes), fixed Huffman, dynamic Huffman (HLIT, HDIST,
//             HCLEN, the code-length code's lengths in their permuted order, then the HLIT + HDIST code lengths, run-length coded).
//   trailer   byte-aligned: CRC-32 of the member's output, ISIZE = its length modulo 2^32.
// Nothing in a page's stream says how many bytes ALL members make together: the caller states `expected`.
//
// Rules, each decided before a byte moves. Bits are taken from a 64-bit buffer that is topped up to more than 32 bits before every symbol, so
// a length (15 + 5 bits) or a distance (15 + 13 bits) never meets a refill in its middle, and `code length > bits held` means the input ended.
// A stored block's LEN must equal ~NLEN. A dynamic header needs HLIT <= 286 and HDIST <= 30; repeat codes may cross from the literal/length
// lengths into the distance lengths but not pass HLIT + HDIST, and 16 needs a length before it; an over-subscribed code set is refused and so
// is an incomplete one, except where zlib accepts it: a set whose only code has length 1, and a distance set without any code (a block of
// literals only). The end-of-block code must have a length. Literal/length symbols 286 and 287 and distance symbols 30 and 31 take part in
// the fixed code and are refused when they are used. A match needs 1 <= distance <= bytes produced BY THIS MEMBER and must end at or before
// `expected`. Both trailer words are verified per member. All members together must produce exactly `expected` bytes and consume exactly the
// input. Every symbol consumes at least one bit, so the loops are bounded by the stream's length; nothing is read outside [pos, end).
//
// Stricter than pyarrow's codec: zlib framing (RFC 1950) and raw DEFLATE are refused (a Parquet page is gzip), and output short of `expected`
// is refused. As lenient as zlib: symbol 284 with extra bits 31 spells length 258; a code set whose only code has length 1.
//
// Tables: a symbol is looked up with the next PB bits of the stream in a primary table of 2^PB entries; a code longer than PB bits goes
// through a link entry to a second-level table of its PB-bit prefix, sized by the longest code under that prefix. A second-level table of
// 2^k entries holds at least k + 1 codes, so for n symbols and codes of up to 15 bits the second level takes at most n * 2^K / (K + 1)
// entries, K = 15 - PB: 286 * 32 / 6 < 1526 for literal/length (PB 10), 30 * 128 / 8 = 480 for distance (PB 8). LIT_CAP and DIST_CAP state
// that, and build_table checks every allocation against them all the same.
#pragma once
#include <cstdint>

#include "planhip.h"

#if defined(__HIPCC__)
#define PH_GZ_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PH_GZ_HD inline
#endif

namespace ph {
namespace gzip {

// why a stream is refused (all of them PH_EINVAL)
enum Sub : int {
    S_OK = 0,
    S_EMPTY = 1,          // a stream of 0 bytes for more than 0 bytes
    S_IMPOSSIBLE = 2,     // more than 1032 bytes are expected per stream byte
    S_TOO_SHORT = 3,      // a stream of fewer than 20 bytes: header, an empty fixed block and trailer take that
    S_HEADER = 4,         // a member does not begin 1f 8b 08
    S_RESERVED_FLAG = 5,  // a reserved FLG bit is set
    S_HEADER_CRC = 6,     // FHCRC does not match the header's bytes
    S_INPUT_CUT = 7,      // the input ends inside a header, a block or a trailer
    S_BLOCK_TYPE = 8,     // block type 3
    S_STORED_LEN = 9,     // a stored block's LEN is not the complement of NLEN
    S_CODE_LENGTHS = 10,  // a dynamic block's code lengths: counts, repeats, over-subscribed, incomplete, no end-of-block code
    S_SYMBOL = 11,        // a code that no symbol has, or literal/length symbol 286 / 287, or distance symbol 30 / 31
    S_DISTANCE = 12,      // a match that reaches in front of the first byte its member produced
    S_OUTPUT_PAST = 13,   // a literal, a stored block or a match writes past the expected length
    S_OUTPUT_SHORT = 14,  // the last member ends before the expected length is reached
    S_INPUT_LEFT = 15,    // bytes behind the last member that cannot hold another one
    S_DATA_CRC = 16,      // a member's CRC-32 does not match the bytes it produced
    S_ISIZE = 17,         // a member's ISIZE does not match the number of bytes it produced
};

inline const char *sub_text(int s) {
    switch (s) {
    case S_EMPTY: return "an empty stream for more than 0 bytes";
    case S_IMPOSSIBLE: return "more than 1032 bytes are expected per stream byte";
    case S_TOO_SHORT: return "fewer than the 20 bytes of the smallest member";
    case S_HEADER: return "a member that does not begin 1f 8b 08";
    case S_RESERVED_FLAG: return "a reserved FLG bit is set";
    case S_HEADER_CRC: return "the header's CRC16 does not match";
    case S_INPUT_CUT: return "the input ends inside a member";
    case S_BLOCK_TYPE: return "block type 3";
    case S_STORED_LEN: return "a stored block whose LEN is not the complement of NLEN";
    case S_CODE_LENGTHS: return "a dynamic block with bad code lengths";
    case S_SYMBOL: return "a code without a symbol, or a symbol outside the alphabet";
    case S_DISTANCE: return "a match distance beyond the bytes its member has produced";
    case S_OUTPUT_PAST: return "the members write past the expected length";
    case S_OUTPUT_SHORT: return "the last member ends before the expected length is reached";
    case S_INPUT_LEFT: return "input is left over behind the last member";
    case S_DATA_CRC: return "a member's CRC-32 does not match its bytes";
    case S_ISIZE: return "a member's ISIZE does not match its bytes";
    default: return "unknown cause";
    }
}

// A match of 258 bytes costs at least one bit of length code and one of distance code: 258 * 8 / 2 bytes of output per byte of input.
constexpr int64_t MAX_EXPANSION = 1032;
constexpr int64_t MIN_MEMBER = 20;  // 10 bytes of header, the 2 of an empty fixed block, 8 of trailer

constexpr int LIT_PB = 10, LIT_CAP = 2560;    // 1024 + 1526 rounded up
constexpr int DIST_PB = 8, DIST_CAP = 768;    // 256 + 480 rounded up; the code-length code (7 bits, 128 entries) is built here first
constexpr int CL_PB = 7;
constexpr int MAX_LENS = 320;                 // 288 + 32 (the fixed code), above 286 + 30

constexpr uint32_t K_LIT = 0, K_BASE = 1, K_EOB = 2, K_BAD = 3;   // an entry's kind
constexpr uint32_t E_LINK = 1u << 10;
// entry: bits 0..3 the code's length (0: no code; a link: the second level's index bits), 4..7 the extra bits, 8..9 the kind, 10 link,
// 16..31 the value (the literal, the base length or distance, a code length symbol; a link: where the second level begins)

struct Tables {
    uint32_t *lit, *dist;           // LIT_CAP, DIST_CAP entries
    uint32_t *count, *first;        // 16 each
    uint16_t *codes;                // MAX_LENS
    uint8_t *lens;                  // MAX_LENS
    const uint32_t *crc;            // the 256 words of the byte-wise CRC-32
    int fixed;                      // 1: lit / dist hold the fixed code
};

struct Bits {
    uint64_t buf;
    int cnt;
    int64_t pos, end;               // the next byte that is not in buf; the stream's end
};

template <class G>
PH_GZ_HD void refill(G &g, Bits &b) {
    if (b.cnt <= 32) {
        const int64_t left = b.end - b.pos;
        const int k = left < 4 ? (int)left : 4;
        if (k > 0) {
            b.buf |= (uint64_t)g.le(b.pos, k) << b.cnt;
            b.pos += k;
            b.cnt += 8 * k;
        }
    }
}
PH_GZ_HD uint32_t take(Bits &b, int n) {                        // n <= 16 and n <= b.cnt
    const uint32_t v = (uint32_t)b.buf & ((1u << n) - 1u);
    b.buf >>= n;
    b.cnt -= n;
    return v;
}
PH_GZ_HD void to_bytes(Bits &b) {                               // drops the bits up to a byte boundary and hands whole bytes back to the stream
    b.pos -= b.cnt >> 3;
    b.buf = 0;
    b.cnt = 0;
}

PH_GZ_HD uint32_t rev_bits(uint32_t x, int n) {                 // the low n <= 16 bits of x in reverse order
    x = ((x & 0x5555u) << 1) | ((x >> 1) & 0x5555u);
    x = ((x & 0x3333u) << 2) | ((x >> 2) & 0x3333u);
    x = ((x & 0x0f0fu) << 4) | ((x >> 4) & 0x0f0fu);
    x = ((x & 0x00ffu) << 8) | ((x >> 8) & 0x00ffu);
    return x >> (16 - n);
}

// kind_of_table: 0 the code-length code, 1 literal/length, 2 distance
PH_GZ_HD uint32_t make_entry(int table, int sym, int len) {
    uint32_t kind = K_LIT, extra = 0, value = (uint32_t)sym;
    if (table == 1 && sym >= 256) {
        const int s = sym - 257;
        if (sym == 256) kind = K_EOB;
        else if (sym > 285) kind = K_BAD;
        else {
            kind = K_BASE;
            if (s < 8) value = 3 + s;
            else if (s == 28) value = 258;
            else {
                extra = (uint32_t)((s - 4) >> 2);
                value = 3u + ((4u + (uint32_t)(s & 3)) << extra);
            }
        }
    } else if (table == 2) {
        if (sym > 29) kind = K_BAD;
        else {
            kind = K_BASE;
            if (sym < 4) value = 1 + sym;
            else {
                extra = (uint32_t)((sym - 2) >> 1);
                value = 1u + ((2u + (uint32_t)(sym & 1)) << extra);
            }
        }
    }
    return (uint32_t)len | (extra << 4) | (kind << 8) | (value << 16);
}

// The lookup tables of the code whose lengths are lens[0, n) into tbl (PB primary bits, cap entries). The lanes of g share the work:
// g.lane() of g.lanes() (0 of 1 on the host), g.sync() between the steps, g.inc() a shared counter.
template <class G>
PH_GZ_HD int build_table(G &g, Tables &t, uint32_t *tbl, int cap, int PB, const uint8_t *lens, int n, int table) {
    const int lane = g.lane(), nl = g.lanes();
    // 1. how many codes of each length; an empty primary table
    for (int l = lane; l < 16; l += nl) t.count[l] = 0;
    for (int j = lane; j < (1 << PB); j += nl) tbl[j] = 0;
    g.sync();
    for (int i = lane; i < n; i += nl) g.inc(&t.count[lens[i]]);
    g.sync();
    // 2. over-subscribed or incomplete; the first code of each length
    int left = 1, longest = 0;
    uint32_t code = 0;
    for (int l = 1; l <= 15; l++) {
        const int c = (int)g.uni(t.count[l]);
        left = 2 * left - c;
        if (left < 0) return S_CODE_LENGTHS;
        if (c) longest = l;
        if (lane == 0) t.first[l] = code;
        code = (code + (uint32_t)c) << 1;
    }
    if (left > 0 && (table == 0 || longest > 1)) return S_CODE_LENGTHS;
    g.sync();
    // 3. canonical codes: lane l walks the symbols for the codes of length l
    for (int l = 1 + lane; l <= 15; l += nl) {
        if (t.count[l] == 0) continue;
        uint32_t c = t.first[l];
        for (int i = 0; i < n; i++)
            if (lens[i] == l) t.codes[i] = (uint16_t)c++;
    }
    // 4. second-level tables: the long codes lie side by side in code order, so their PB-bit prefixes count up from the first one's
    if (longest > PB) {
        int l = PB + 1;
        while (g.uni(t.count[l]) == 0) l++;
        int c = (int)g.uni(t.count[l]);
        uint32_t prefix = g.uni(t.first[l]) >> (l - PB);
        int next = 1 << PB;
        while (c > 0) {
            int space = 1 << (15 - PB), top = l;                // what is left under this prefix, in codes of 15 bits
            while (space > 0 && c > 0) {
                int m = space >> (15 - l);
                if (m > c) m = c;
                space -= m << (15 - l);
                c -= m;
                if (m > 0) top = l;
                while (c == 0 && l < 15) c = (int)g.uni(t.count[++l]);
                if (m == 0) break;
            }
            if (next + (1 << (top - PB)) > cap) return S_CODE_LENGTHS;   // (never: the bound above)
            if (lane == 0) tbl[rev_bits(prefix, PB)] = (uint32_t)(top - PB) | E_LINK | ((uint32_t)next << 16);
            next += 1 << (top - PB);
            prefix++;
        }
    }
    g.sync();
    // 5. every symbol fills the entries whose low bits are its code, first bit lowest
    for (int i = lane; i < n; i += nl) {
        const int l = lens[i];
        if (l == 0) continue;
        const uint32_t c = t.codes[i], e = make_entry(table, i, l);
        if (l <= PB) {
            for (int j = (int)rev_bits(c, l); j < (1 << PB); j += 1 << l) tbl[j] = e;
        } else {
            const uint32_t link = tbl[rev_bits(c >> (l - PB), PB)];
            const int k = (int)(link & 15u), off = (int)(link >> 16), r = l - PB;
            for (int j = (int)rev_bits(c & ((1u << r) - 1u), r); j < (1 << k); j += 1 << r) tbl[off + j] = e;
        }
    }
    g.sync();
    return S_OK;
}

// One symbol of the code in tbl off the bit buffer (refilled by the caller). *e = its entry; the code's bits are consumed.
template <class G>
PH_GZ_HD int symbol(G &g, Bits &b, const uint32_t *tbl, int PB, uint32_t *out) {
    const uint32_t bits = (uint32_t)b.buf;
    uint32_t e = g.uni(tbl[bits & ((1u << PB) - 1u)]);
    if (e & E_LINK) e = g.uni(tbl[(e >> 16) + ((bits >> PB) & ((1u << (e & 15u)) - 1u))]);
    const int len = (int)(e & 15u);
    if (len > b.cnt || (len == 0 && b.cnt < 15)) return S_INPUT_CUT;    // (fewer than 15 bits are held only at the input's end)
    if (len == 0) return S_SYMBOL;
    b.buf >>= len;
    b.cnt -= len;
    *out = e;
    return S_OK;
}

template <class G>
PH_GZ_HD int fixed_tables(G &g, Tables &t) {
    const int lane = g.lane(), nl = g.lanes();
    for (int i = lane; i < 288; i += nl) t.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
    for (int i = lane; i < 32; i += nl) t.lens[288 + i] = 5;
    g.sync();
    int s = build_table(g, t, t.lit, LIT_CAP, LIT_PB, t.lens, 288, 1);
    if (s == S_OK) s = build_table(g, t, t.dist, DIST_CAP, DIST_PB, t.lens + 288, 32, 2);
    t.fixed = 1;
    return s;
}

template <class G>
PH_GZ_HD int dynamic_tables(G &g, Bits &b, Tables &t) {
    refill(g, b);
    if (b.cnt < 14) return S_INPUT_CUT;
    const int hlit = 257 + (int)take(b, 5), hdist = 1 + (int)take(b, 5), hclen = 4 + (int)take(b, 4);
    if (hlit > 286 || hdist > 30) return S_CODE_LENGTHS;
    t.fixed = 0;
    const int lane = g.lane(), nl = g.lanes();
    for (int i = lane; i < 19; i += nl) t.lens[i] = 0;
    g.sync();
    for (int i = 0; i < hclen; i++) {
        refill(g, b);
        if (b.cnt < 3) return S_INPUT_CUT;
        // the permuted order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, without an array
        const int at = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 8 - ((i - 3) >> 1) : 8 + ((i - 4) >> 1);
        const uint32_t v = take(b, 3);
        if (lane == 0) t.lens[at] = (uint8_t)v;
    }
    g.sync();
    int s = build_table(g, t, t.dist, DIST_CAP, CL_PB, t.lens, 19, 0);
    if (s != S_OK) return s;
    const int total = hlit + hdist;
    int i = 0;
    uint32_t prev = 0;
    while (i < total) {
        refill(g, b);
        uint32_t e;
        s = symbol(g, b, t.dist, CL_PB, &e);
        if (s != S_OK) return s;
        const uint32_t v = e >> 16;
        int rep = 1;
        uint32_t fill = v;
        if (v >= 16) {
            const int nb = v == 16 ? 2 : v == 17 ? 3 : 7;
            if (b.cnt < nb) return S_INPUT_CUT;
            rep = (v == 18 ? 11 : 3) + (int)take(b, nb);
            if (v == 16 && i == 0) return S_CODE_LENGTHS;
            fill = v == 16 ? prev : 0;
            if (i + rep > total) return S_CODE_LENGTHS;
        }
        // (every lane writes the same bytes: no lane waits for another's)
        for (int j = 0; j < rep; j++) t.lens[i + j] = (uint8_t)fill;
        i += rep;
        prev = fill;
    }
    g.sync();
    if (t.lens[256] == 0) return S_CODE_LENGTHS;
    s = build_table(g, t, t.lit, LIT_CAP, LIT_PB, t.lens, hlit, 1);
    if (s != S_OK) return s;
    return build_table(g, t, t.dist, DIST_CAP, DIST_PB, t.lens + hlit, hdist, 2);
}

// The DEFLATE blocks of one member from the bit position b on. *produced counts the output of the whole stream, mstart = where this member's
// began. The sink has lit(at, byte), literal(g, from, at, n) (n bytes of the stream from `from` to output position `at`) and
// match(at, distance, n) (as if byte by byte, front to back: an overlapping match repeats a pattern).
template <class G, class S>
PH_GZ_HD int inflate(G &g, Bits &b, Tables &t, int64_t expected, int64_t mstart, int64_t *produced_io, S &sink) {
    int64_t produced = *produced_io;
    for (;;) {
        refill(g, b);
        if (b.cnt < 3) return S_INPUT_CUT;
        const uint32_t last = take(b, 1), type = take(b, 2);
        if (type == 3) return S_BLOCK_TYPE;
        if (type == 0) {
            take(b, b.cnt & 7);
            refill(g, b);
            if (b.cnt < 32) return S_INPUT_CUT;
            const uint32_t len = take(b, 16), nlen = take(b, 16);
            if (len != (~nlen & 0xffffu)) return S_STORED_LEN;
            to_bytes(b);
            if ((int64_t)len > b.end - b.pos) return S_INPUT_CUT;
            if ((int64_t)len > expected - produced) return S_OUTPUT_PAST;
            if (len > 0) sink.literal(g, b.pos, produced, (int64_t)len);
            b.pos += len;
            produced += len;
        } else {
            int s = S_OK;
            if (type == 2) s = dynamic_tables(g, b, t);
            else if (!t.fixed) s = fixed_tables(g, t);
            if (s != S_OK) return s;
            for (;;) {
                refill(g, b);
                uint32_t e;
                s = symbol(g, b, t.lit, LIT_PB, &e);
                if (s != S_OK) return s;
                const uint32_t kind = (e >> 8) & 3u;
                if (kind == K_LIT) {
                    if (produced >= expected) return S_OUTPUT_PAST;
                    sink.lit(produced, e >> 16);
                    produced++;
                    continue;
                }
                if (kind == K_EOB) break;
                if (kind == K_BAD) return S_SYMBOL;
                int nb = (int)((e >> 4) & 15u);
                if (b.cnt < nb) return S_INPUT_CUT;
                const int64_t len = (int64_t)((e >> 16) + take(b, nb));   // (symbol 284 with all five extra bits set: 258, as in zlib)
                refill(g, b);
                s = symbol(g, b, t.dist, DIST_PB, &e);
                if (s != S_OK) return s;
                if (((e >> 8) & 3u) != K_BASE) return S_SYMBOL;
                nb = (int)((e >> 4) & 15u);
                if (b.cnt < nb) return S_INPUT_CUT;
                const int64_t dist = (int64_t)((e >> 16) + take(b, nb));
                if (dist > produced - mstart) return S_DISTANCE;
                if (len > expected - produced) return S_OUTPUT_PAST;
                sink.match(produced, dist, len);
                produced += len;
            }
        }
        if (last) break;
    }
    *produced_io = produced;
    return S_OK;
}

PH_GZ_HD uint32_t crc_byte(const uint32_t *table, uint32_t crc, uint32_t byte) { return table[(crc ^ byte) & 0xffu] ^ (crc >> 8); }

// The members of [pos, end) into a sink of `expected` bytes. The caller has end - pos >= MIN_MEMBER (check_sizes). The sink also has
// member_crc(mstart, produced): the CRC-32 of output [mstart, produced), asked for once a member, at its end.
template <class G, class S>
PH_GZ_HD int decode_stream(G &g, int64_t pos, int64_t end, int64_t expected, Tables &t, S &sink) {
    int64_t produced = 0;
    t.fixed = 0;
    for (;;) {
        if (end - pos < 10) return S_INPUT_CUT;
        if (g.u8(pos) != 0x1f || g.u8(pos + 1) != 0x8b || g.u8(pos + 2) != 8) return S_HEADER;
        const uint32_t flg = g.u8(pos + 3);
        if (flg & 0xe0u) return S_RESERVED_FLAG;
        const int64_t hstart = pos;
        pos += 10;
        if (flg & 4u) {                                         // FEXTRA
            if (end - pos < 2) return S_INPUT_CUT;
            const int64_t xlen = (int64_t)(g.u8(pos) | (g.u8(pos + 1) << 8));
            pos += 2;
            if (end - pos < xlen) return S_INPUT_CUT;
            pos += xlen;
        }
        for (uint32_t f = 8u; f <= 16u; f <<= 1) {              // FNAME, FCOMMENT
            if (!(flg & f)) continue;
            for (;;) {
                if (pos >= end) return S_INPUT_CUT;
                if (g.u8(pos++) == 0) break;
            }
        }
        if (flg & 2u) {                                         // FHCRC
            if (end - pos < 2) return S_INPUT_CUT;
            uint32_t c = 0xffffffffu;
            for (int64_t p = hstart; p < pos; p++) c = crc_byte(t.crc, c, g.u8(p));
            if (((~c) & 0xffffu) != (g.u8(pos) | (g.u8(pos + 1) << 8))) return S_HEADER_CRC;
            pos += 2;
        }
        Bits b{0, 0, pos, end};
        const int64_t mstart = produced;
        const int s = inflate(g, b, t, expected, mstart, &produced, sink);
        if (s != S_OK) return s;
        take(b, b.cnt & 7);
        to_bytes(b);
        pos = b.pos;
        if (end - pos < 8) return S_INPUT_CUT;
        const uint32_t crc = g.le(pos, 4), isize = g.le(pos + 4, 4);
        pos += 8;
        if (sink.member_crc(mstart, produced) != crc) return S_DATA_CRC;
        if ((uint32_t)(produced - mstart) != isize) return S_ISIZE;
        if (pos == end) break;
        if (end - pos < MIN_MEMBER) return S_INPUT_LEFT;
    }
    return produced == expected ? S_OK : S_OUTPUT_SHORT;
}

// what the host can decide from the two lengths alone (the Parquet page directory asks the same before anything is allocated)
PH_GZ_HD int check_sizes(int64_t src_bytes, int64_t expected) {
    if (src_bytes == 0) return expected == 0 ? S_OK : S_EMPTY;
    if (src_bytes < MIN_MEMBER) return S_TOO_SHORT;
    return expected > MAX_EXPANSION * src_bytes ? S_IMPOSSIBLE : S_OK;
}
// ... and from the first four bytes of a stream of at least MIN_MEMBER bytes
PH_GZ_HD int check_header(const uint8_t *s) {
    if (s[0] != 0x1f || s[1] != 0x8b || s[2] != 8) return S_HEADER;
    return (s[3] & 0xe0u) ? S_RESERVED_FLAG : S_OK;
}

inline const uint32_t *crc_table_host() {
    static const struct Table {
        uint32_t w[256];
        Table() {
            for (uint32_t i = 0; i < 256; i++) {
                uint32_t c = i;
                for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xedb88320u : c >> 1;
                w[i] = c;
            }
        }
    } table;
    return table.w;
}

struct HostStream {
    const uint8_t *s;
    uint32_t u8(int64_t p) const { return s[p]; }
    uint32_t le(int64_t p, int k) const {
        uint32_t v = 0;
        for (int i = 0; i < k; i++) v |= (uint32_t)s[p + i] << (8 * i);
        return v;
    }
    int lane() const { return 0; }
    int lanes() const { return 1; }
    void sync() const {}
    void inc(uint32_t *p) const { ++*p; }
    uint32_t uni(uint32_t v) const { return v; }
};

struct HostSink {
    uint8_t *d;
    const uint32_t *crc;
    void lit(int64_t at, uint32_t byte) { d[at] = (uint8_t)byte; }
    void literal(const HostStream &g, int64_t from, int64_t at, int64_t n) { for (int64_t i = 0; i < n; i++) d[at + i] = g.s[from + i]; }
    void match(int64_t at, int64_t dist, int64_t n) { for (int64_t i = 0; i < n; i++) d[at + i] = d[at - dist + i]; }
    uint32_t member_crc(int64_t mstart, int64_t produced) const {
        uint32_t c = 0xffffffffu;
        for (int64_t i = mstart; i < produced; i++) c = crc_byte(crc, c, d[i]);
        return ~c;
    }
};

struct HostTables : Tables {
    uint32_t lit_[LIT_CAP], dist_[DIST_CAP], count_[16], first_[16];
    uint16_t codes_[MAX_LENS];
    uint8_t lens_[MAX_LENS];
    HostTables() {
        lit = lit_, dist = dist_, count = count_, first = first_, codes = codes_, lens = lens_;
        crc = crc_table_host();
        fixed = 0;
    }
};

// One whole stream src[0, src_bytes) on the host into dst[0, expected). dst may be null when expected is 0.
inline int decompress_host(const uint8_t *src, int64_t src_bytes, uint8_t *dst, int64_t expected) {
    int s = check_sizes(src_bytes, expected);
    if (s != S_OK || src_bytes == 0) return s;
    s = check_header(src);
    if (s != S_OK) return s;
    HostStream g{src};
    HostTables t;
    HostSink sink{dst, t.crc};
    return decode_stream(g, 0, src_bytes, expected, t, sink);
}

}  // namespace gzip
}  // namespace ph
