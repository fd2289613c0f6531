// ZSTD (Parquet codec 6: RFC 8878 frames), decoded by ONE set of functions compiled for the host (ph_zstd_decompress_host and the Parquet host
// twin, sequentially) and for the device (zstd_decompress.hip, whose kernel instantiates decode_stream over two LDS windows, LDS tables and
// an LDS ring). In the manner of gzip_decode.h: a getter g, a sink and a set of tables t that the caller places (the stack on the host, LDS
// on the device). Everything of RFC 8878 except dictionaries.
//
// A stream is one or more frames back to back:
//   frame      magic 28 b5 2f fd, Frame_Header_Descriptor, then by it: Window_Descriptor (absent with Single_Segment), Dictionary_ID (0, 1, 2
//              or 4 bytes), Frame_Content_Size (0, 1, 2, 4 or 8 bytes); blocks; Content_Checksum (4 bytes) when the descriptor says so.
//   skippable  magic 5? 2a 4d 18, a 4-byte length, that many bytes: stepped over.
//   block      3 bytes (last, type, size), then Raw: size bytes; RLE: one byte, repeated size times; Compressed: a literals section and a
//              sequences section in size bytes.
//   literals   Raw, RLE, Compressed (a Huffman tree description, then one or four backward bitstreams) or Treeless (the last tree again).
//   sequences  a count, a byte of three modes (Predefined, RLE, FSE_Compressed, Repeat) for the literal-length, offset and match-length
//              tables, the tables' descriptions, one backward bitstream of three interleaved FSE states and the codes' extra bits.
// Nothing in a page's stream says how many bytes ALL frames make together: the caller states `expected`.
//
// Rules, each decided before a byte moves. A reserved descriptor bit, a non-zero Dictionary_ID, a window above 2^31 and block type 3 are
// refused. Block_Maximum_Size = min(Window_Size, 128 KiB) bounds a block's Block_Size and what a compressed block regenerates. A
// Frame_Content_Size must equal what its frame produced; a Content_Checksum (the low 32 bits of XXH64, seed 0, of the frame's output) is
// verified. Huffman weights come direct or FSE-compressed (accuracy log <= 6); their sum must be completed to a power of two of at most 11
// bits by a last weight that is itself a power of two, and there must be an even number, two at least, of weight 1 (libzstd's
// HUF_readStats). FSE table descriptions: accuracy log <= 9 / 8 / 9 (literal lengths / offsets / match lengths), the probabilities must sum
// exactly, no symbol above 35 / 31 / 52. Treeless and Repeat need a table from an earlier block of the same frame. Every backward
// bitstream needs its final-bit marker and must be consumed exactly. A sequence may not ask for more literals than its block has; a match
// needs 1 <= offset <= bytes produced BY THIS FRAME and must end at or before `expected`. The window size is NOT enforced beyond that, as
// in libzstd's one-shot decoder: an offset may reach back to the frame's first byte. All frames together must produce exactly `expected`
// bytes and consume exactly the input.
// Termination: every loop consumes input or produces output and is bounded by the stream's end, a table's size or `expected`.
//
// Stricter than libzstd's one-shot decoder: Huffman codes of 12 bits (the RFC's limit is 11); Block_Maximum_Size, which it holds no block
// to (the ratio bound below rests on it); a stream shorter than 9 bytes (a lone skippable frame of 8).
//
// Ratio bound: an RLE block makes Block_Maximum_Size = 128 KiB from 4 bytes (3 of header, the byte). A compressed block regenerates 128 KiB
// at most as well and needs more than 4 bytes for it (3 of header, a literals header, a sequence count, a mode byte, a bitstream), and a
// frame adds its header: no stream yields more than 32768 to one.
#pragma once
#include <cstdint>

#include "planhip.h"

#if defined(__HIPCC__)
#define PH_ZS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PH_ZS_HD inline
#endif

namespace ph {
namespace zstd {

// why a stream is refused (all of them PH_EINVAL)
enum Sub : int {
    S_OK = 0,
    S_EMPTY = 1,          // a stream of 0 bytes for more than 0 bytes
    S_IMPOSSIBLE = 2,     // more than 32768 bytes are expected per stream byte
    S_TOO_SHORT = 3,      // a stream of fewer than 9 bytes: magic, descriptor, one more header byte and a last block's header take that
    S_MAGIC = 4,          // a frame begins with neither 28 b5 2f fd nor 5? 2a 4d 18
    S_RESERVED = 5,       // the reserved bit of the Frame_Header_Descriptor is set
    S_DICTIONARY = 6,     // a non-zero Dictionary_ID
    S_WINDOW = 7,         // a Window_Descriptor above 2^31
    S_INPUT_CUT = 8,      // the input ends inside a frame header, a block or a checksum
    S_BLOCK_TYPE = 9,     // block type 3
    S_BLOCK_SIZE = 10,    // a Block_Size above Block_Maximum_Size
    S_BLOCK_CUT = 11,     // a compressed block ends inside one of its sections
    S_LITERALS = 12,      // a literals section header whose sizes do not fit: above 128 KiB, four streams for fewer than 6 bytes, a jump table beyond the section
    S_TREELESS = 13,      // Treeless literals without an earlier tree in this frame
    S_WEIGHTS = 14,       // a Huffman tree description: too many weights, a weight above 11, a sum that no last weight completes, an odd number of weight 1
    S_FSE_TABLE = 15,     // an FSE table description: accuracy log, probabilities that do not sum, a symbol above the alphabet
    S_SEQ_HEADER = 16,    // the sequences header: reserved mode bits, or bytes behind a count of 0
    S_REPEAT = 17,        // Repeat mode without an earlier table in this frame
    S_MARKER = 18,        // a backward bitstream without its final-bit marker
    S_STREAM_END = 19,    // a backward bitstream that is not consumed exactly
    S_LIT_COUNT = 20,     // a sequence asks for more literals than its block has
    S_OFFSET = 21,        // a match offset of 0 or beyond the bytes its frame has produced
    S_BLOCK_OUTPUT = 22,  // a compressed block regenerates more than Block_Maximum_Size
    S_OUTPUT_PAST = 23,   // a block writes past the expected length
    S_OUTPUT_SHORT = 24,  // the last frame ends before the expected length is reached
    S_INPUT_LEFT = 25,    // bytes behind the last frame that cannot hold another one
    S_CONTENT_SIZE = 26,  // a Frame_Content_Size that is not what its frame produces
    S_CHECKSUM = 27,      // a Content_Checksum that does not match the frame's bytes
};

inline const char *sub_text(int s) {
    switch (s) {
    case S_EMPTY: return "an empty stream for more than 0 bytes";
    case S_IMPOSSIBLE: return "more than 32768 bytes are expected per stream byte";
    case S_TOO_SHORT: return "fewer than the 9 bytes of the smallest frame";
    case S_MAGIC: return "a frame that begins with neither 28 b5 2f fd nor a skippable frame's magic";
    case S_RESERVED: return "the reserved bit of the frame header descriptor is set";
    case S_DICTIONARY: return "a dictionary ID (dictionaries are not supported)";
    case S_WINDOW: return "a window above 2^31 bytes";
    case S_INPUT_CUT: return "the input ends inside a frame";
    case S_BLOCK_TYPE: return "block type 3";
    case S_BLOCK_SIZE: return "a block size above the block maximum size";
    case S_BLOCK_CUT: return "a compressed block ends inside one of its sections";
    case S_LITERALS: return "a literals section whose sizes do not fit";
    case S_TREELESS: return "treeless literals without an earlier Huffman tree in this frame";
    case S_WEIGHTS: return "a Huffman tree description with bad weights";
    case S_FSE_TABLE: return "a bad FSE table description";
    case S_SEQ_HEADER: return "a bad sequences section header";
    case S_REPEAT: return "repeat mode without an earlier table in this frame";
    case S_MARKER: return "a bitstream without its final-bit marker";
    case S_STREAM_END: return "a bitstream that is not consumed exactly";
    case S_LIT_COUNT: return "a sequence asks for more literals than its block has";
    case S_OFFSET: return "a match offset of 0 or beyond the bytes its frame has produced";
    case S_BLOCK_OUTPUT: return "a compressed block regenerates more than the block maximum size";
    case S_OUTPUT_PAST: return "the frames write past the expected length";
    case S_OUTPUT_SHORT: return "the last frame ends before the expected length is reached";
    case S_INPUT_LEFT: return "input is left over behind the last frame";
    case S_CONTENT_SIZE: return "a frame content size that is not what its frame produces";
    case S_CHECKSUM: return "a content checksum that does not match the frame's bytes";
    default: return "unknown cause";
    }
}

constexpr int64_t MAX_EXPANSION = 32768;
constexpr int64_t MIN_FRAME = 9;               // magic, descriptor, one more header byte (window or content size), a 3-byte last-block header
constexpr int64_t BLOCK_MAX = 128 * 1024;
constexpr uint32_t MAGIC = 0xfd2fb528u, SKIP_MAGIC = 0x184d2a50u;

constexpr int HUF_MAX_BITS = 11, HUF_CAP = 1 << HUF_MAX_BITS;
constexpr int LL_LOG = 9, OF_LOG = 8, ML_LOG = 9, WT_LOG = 6;
constexpr int LL_MAX = 35, OF_MAX = 31, ML_MAX = 52;
constexpr int MAX_SYMS = 256;                  // the weights' FSE alphabet, as libzstd reads it

// FSE entry: bits 0..7 the symbol, 8..15 the bits the next state takes, 16..31 the next state's base. Huffman entry: bits 0..7 the code's
// length, 8..15 the byte.
struct Tables {
    uint16_t *huf;                  // HUF_CAP
    uint32_t *ll, *of, *ml, *wt;    // 1 << LL_LOG, OF_LOG, ML_LOG, WT_LOG entries
    uint8_t *weights;               // MAX_SYMS
    int16_t *norm;                  // MAX_SYMS: the normalized counts of the table being built
    uint16_t *cum;                  // MAX_SYMS: the cells in front of a symbol's (without the "less than 1" ones)
    uint32_t *rank;                 // 16: per weight, its symbols, then where its entries begin
};

// what a frame keeps from block to block (wave-uniform on the device)
struct Frame {
    int huf_bits;                   // the tree's longest code, 0: no tree yet
    int ll_log, of_log, ml_log;     // the tables' accuracy logs (0 for an RLE table), -1: no table yet
    int64_t rep1, rep2, rep3;
};

PH_ZS_HD int high_bit(uint32_t x) { return 31 - __builtin_clz(x); }   // x > 0

// ---- forward bits (FSE table descriptions), as gzip_decode.h's
struct Bits {
    uint64_t buf;
    int cnt;
    int64_t pos, end;
};
template <class G>
PH_ZS_HD void refill(G &g, Bits &b) {
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
PH_ZS_HD uint32_t take(Bits &b, int n) {                        // n <= 16 and n <= b.cnt
    const uint32_t v = (uint32_t)b.buf & ((1u << n) - 1u);
    b.buf >>= n;
    b.cnt -= n;
    return v;
}

// ---- backward bits: the stream's bytes [start, pos) are not in buf yet; the low cnt bits of buf are, the next one to take on top.
// W chooses the getter's window: 0 the literal streams' (and the weights'), 1 the sequence stream's.
struct Back {
    uint64_t buf;
    int cnt;
    int64_t pos, start;
};
template <int W, class G>
PH_ZS_HD void refill_back(G &g, Back &b) {
    if (b.cnt <= 32) {
        const int64_t left = b.pos - b.start;
        const int k = left < 4 ? (int)left : 4;
        if (k > 0) {
            const uint32_t v = W == 0 ? g.back_a(b.pos - k, k) : g.back_b(b.pos - k, k);
            b.buf = (b.buf << (8 * k)) | v;
            b.pos -= k;
            b.cnt += 8 * k;
        }
    }
}
template <int W, class G>
PH_ZS_HD int open_back(G &g, Back &b, int64_t start, int64_t end) {
    if (end <= start) return S_BLOCK_CUT;
    const uint32_t last = W == 0 ? g.back_a(end - 1, 1) : g.back_b(end - 1, 1);
    if (last == 0) return S_MARKER;
    b.buf = last;
    b.cnt = high_bit(last);
    b.pos = end - 1;
    b.start = start;
    return S_OK;
}
PH_ZS_HD uint32_t take_back(Back &b, int n) {                   // n <= 32 and n <= b.cnt
    if (n == 0) return 0;
    const uint32_t v = (uint32_t)(b.buf >> (b.cnt - n));
    b.cnt -= n;
    return n == 32 ? v : v & ((1u << n) - 1u);
}
PH_ZS_HD uint32_t peek_back(const Back &b, int n) {             // 1 <= n <= 16; bits that the stream does not have read as 0
    const uint32_t v = b.cnt >= n ? (uint32_t)(b.buf >> (b.cnt - n)) : (uint32_t)b.buf << (n - b.cnt);
    return v & ((1u << n) - 1u);
}
PH_ZS_HD bool back_done(const Back &b) { return b.cnt == 0 && b.pos == b.start; }

// ---- FSE
// the normalized counts of a table description from b on (RFC 8878 4.1.1) into t.norm / t.cum. *log_out, *nsym_out, *nlow_out: the
// accuracy log, the symbols described, how many of them have probability "less than 1".
template <class G>
PH_ZS_HD int read_ncount(G &g, Bits &b, Tables &t, int max_log, int max_sym, int *log_out, int *nsym_out, int *nlow_out) {
    refill(g, b);
    if (b.cnt < 4) return S_INPUT_CUT;
    const int log = 5 + (int)take(b, 4);
    if (log > max_log) return S_FSE_TABLE;
    int remaining = (1 << log) + 1, threshold = 1 << log, nbits = log + 1, sym = 0, nlow = 0, cells = 0;
    bool zero = false;
    while (remaining > 1 && sym <= max_sym) {
        if (zero) {
            for (;;) {
                refill(g, b);
                if (b.cnt < 2) return S_INPUT_CUT;
                const int r = (int)take(b, 2);
                if (sym + r > max_sym + 1) return S_FSE_TABLE;
                for (int j = 0; j < r; j++) t.norm[sym + j] = 0;   // (every lane writes the same values)
                sym += r;
                if (r < 3) break;
            }
            if (sym > max_sym) return S_FSE_TABLE;
        }
        refill(g, b);
        if (b.cnt < nbits) return S_INPUT_CUT;
        const int max = 2 * threshold - 1 - remaining;
        int count = (int)((uint32_t)b.buf & (uint32_t)(threshold - 1));
        if (count < max) take(b, nbits - 1);
        else {
            count = (int)take(b, nbits);
            if (count >= threshold) count -= max;
        }
        count--;                                                // -1: "less than 1", one cell at the table's end
        remaining -= count < 0 ? 1 : count;
        t.norm[sym] = (int16_t)count;
        t.cum[sym] = (uint16_t)cells;
        if (count > 0) cells += count;
        if (count < 0) nlow++;
        sym++;
        zero = count == 0;
        while (remaining < threshold) {
            nbits--;
            threshold >>= 1;
        }
    }
    if (remaining != 1) return S_FSE_TABLE;
    *log_out = log;
    *nsym_out = sym;
    *nlow_out = nlow;
    return S_OK;
}

// The decode table of t.norm[0, nsym) / t.cum into tbl (1 << log entries). The lanes of g share the work: g.lane() of g.lanes() (0 of 1 on
// the host), g.sync() between the steps. Without "less than 1" symbols cell k of the spread lies at k * step: one symbol a lane. With them
// the walk skips the table's end and is carried out plainly (every lane writes the same values).
template <class G>
PH_ZS_HD void build_fse(G &g, Tables &t, uint32_t *tbl, int log, int nsym, int nlow) {
    const int size = 1 << log, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
    const int lane = g.lane(), nl = g.lanes();
    g.sync();
    if (nlow == 0) {
        for (int s = lane; s < nsym; s += nl) {
            const int n = t.norm[s], c = t.cum[s];
            for (int k = c; k < c + n; k++) tbl[(k * step) & mask] = (uint32_t)s;
        }
    } else {
        int high = size - 1, pos = 0;
        for (int s = 0; s < nsym; s++)
            if (t.norm[s] < 0) tbl[high--] = (uint32_t)s;
        for (int s = 0; s < nsym; s++) {
            const int n = t.norm[s];
            for (int i = 0; i < n; i++) {
                tbl[pos] = (uint32_t)s;
                pos = (pos + step) & mask;
                while (pos > high) pos = (pos + step) & mask;
            }
        }
    }
    g.sync();
    // a symbol's cells in table order take the states n, n + 1, ... of its share
    for (int s = lane; s < nsym; s += nl) {
        const int n = t.norm[s];
        if (n == 0) continue;
        uint32_t x = n < 0 ? 1u : (uint32_t)n;
        for (int i = 0; i < size; i++) {
            if ((tbl[i] & 0xffu) != (uint32_t)s) continue;
            const int nb = log - high_bit(x);
            tbl[i] = (uint32_t)s | ((uint32_t)nb << 8) | (((x << nb) - (uint32_t)size) << 16);
            x++;
        }
    }
    g.sync();
}

// which: 0 literal lengths, 1 offsets, 2 match lengths
PH_ZS_HD int predefined_count(int which, int s) {
    if (which == 0) return s == 0 ? 4 : s == 1 ? 3 : s <= 12 ? 2 : s <= 15 ? 1 : s <= 24 ? 2 : s == 25 ? 3 : s == 26 ? 2 : s <= 31 ? 1 : -1;
    if (which == 1) return s <= 5 ? 1 : s <= 8 ? 2 : s <= 23 ? 1 : -1;
    return s == 0 ? 1 : s == 1 ? 4 : s == 2 ? 3 : s <= 8 ? 2 : s <= 45 ? 1 : -1;
}

// One of the three sequence tables by its mode, the description (if any) at *pos in [*pos, end). *log: the table's accuracy log, -1: none yet.
template <class G>
PH_ZS_HD int sequence_table(G &g, Tables &t, int which, int mode, int64_t *pos, int64_t end, int *log) {
    uint32_t *tbl = which == 0 ? t.ll : which == 1 ? t.of : t.ml;
    const int max_sym = which == 0 ? LL_MAX : which == 1 ? OF_MAX : ML_MAX;
    if (mode == 3) return *log < 0 ? S_REPEAT : S_OK;
    if (mode == 1) {
        if (*pos >= end) return S_BLOCK_CUT;
        const uint32_t sym = g.u8(*pos);
        ++*pos;
        if ((int)sym > max_sym) return S_FSE_TABLE;
        g.sync();
        tbl[0] = sym;                                           // (every lane writes the same value) no bits, next state 0
        g.sync();
        *log = 0;
        return S_OK;
    }
    int nsym = 0, nlow = 0, lg = 0;
    if (mode == 0) {
        lg = which == 1 ? 5 : 6;
        nsym = which == 0 ? 36 : which == 1 ? 29 : 53;
        int cells = 0;
        g.sync();
        for (int s = 0; s < nsym; s++) {                        // (every lane writes the same values)
            const int c = predefined_count(which, s);
            t.norm[s] = (int16_t)c;
            t.cum[s] = (uint16_t)cells;
            if (c > 0) cells += c;
            else nlow++;
        }
    } else {
        Bits b{0, 0, *pos, end};
        g.sync();
        int s = read_ncount(g, b, t, which == 0 ? LL_LOG : which == 1 ? OF_LOG : ML_LOG, max_sym, &lg, &nsym, &nlow);
        if (s == S_INPUT_CUT) s = S_BLOCK_CUT;
        if (s != S_OK) return s;
        *pos = b.pos - (b.cnt >> 3);
    }
    build_fse(g, t, tbl, lg, nsym, nlow);
    *log = lg;
    return S_OK;
}

// ---- Huffman
// The tree description at [pos, end) -> t.huf; *used = its bytes, *bits_out = the longest code.
template <class G>
PH_ZS_HD int huffman_tree(G &g, Tables &t, int64_t pos, int64_t end, int64_t *used, int *bits_out) {
    const int lane = g.lane(), nl = g.lanes();
    if (pos >= end) return S_BLOCK_CUT;
    const int hb = (int)g.u8(pos);
    int n = 0;                                                  // the weights that are stated
    g.sync();
    if (hb >= 128) {
        n = hb - 127;
        const int bytes = (n + 1) / 2;
        if (bytes > end - pos - 1) return S_BLOCK_CUT;
        for (int i = 0; i < bytes; i++) {                       // (every lane writes the same values)
            const uint32_t v = g.u8(pos + 1 + i);
            t.weights[2 * i] = (uint8_t)(v >> 4);
            if (2 * i + 1 < n) t.weights[2 * i + 1] = (uint8_t)(v & 15u);
        }
        *used = 1 + bytes;
    } else {
        if (hb == 0 || hb > end - pos - 1) return S_BLOCK_CUT;
        const int64_t wend = pos + 1 + hb;
        Bits fb{0, 0, pos + 1, wend};
        int lg = 0, nsym = 0, nlow = 0;
        int s = read_ncount(g, fb, t, WT_LOG, MAX_SYMS - 1, &lg, &nsym, &nlow);
        if (s == S_INPUT_CUT) s = S_WEIGHTS;
        if (s != S_OK) return s;
        build_fse(g, t, t.wt, lg, nsym, nlow);
        Back b;
        s = open_back<0>(g, b, fb.pos - (fb.cnt >> 3), wend);
        if (s != S_OK) return s;
        refill_back<0>(g, b);
        if (b.cnt < 2 * lg) return S_STREAM_END;
        uint32_t s1 = take_back(b, lg), s2 = take_back(b, lg);
        // two states take turns; the stream is over when a state asks for more bits than are left: the other state's symbol is the last
        // (libzstd's FSE_decompress)
        for (;;) {
            if (n > MAX_SYMS - 3) return S_WEIGHTS;
            const uint32_t e = g.uni(t.wt[s1]);
            t.weights[n++] = (uint8_t)(e & 0xffu);
            refill_back<0>(g, b);
            const int nb = (int)((e >> 8) & 0xffu);
            if (nb > b.cnt) {
                t.weights[n++] = (uint8_t)(g.uni(t.wt[s2]) & 0xffu);
                break;
            }
            s1 = (e >> 16) + take_back(b, nb);
            const uint32_t t2 = s1;                              // the states change roles
            s1 = s2;
            s2 = t2;
        }
        *used = 1 + hb;
    }
    g.sync();
    // the weights' sum, the last weight (HUF_readStats)
    for (int w = lane; w < 16; w += nl) t.rank[w] = 0;
    g.sync();
    uint32_t total = 0;
    for (int i = 0; i < n; i++) {
        const uint32_t w = g.uni(t.weights[i]);
        if (w > (uint32_t)HUF_MAX_BITS) return S_WEIGHTS;
        total += (1u << w) >> 1;
    }
    if (total == 0) return S_WEIGHTS;
    const int bits = high_bit(total) + 1;
    if (bits > HUF_MAX_BITS) return S_WEIGHTS;
    const uint32_t rest = (1u << bits) - total;
    if (rest & (rest - 1u)) return S_WEIGHTS;
    t.weights[n] = (uint8_t)(high_bit(rest) + 1);               // (every lane writes the same value)
    n++;
    g.sync();
    for (int i = lane; i < n; i += nl) g.inc(&t.rank[t.weights[i]]);
    g.sync();
    const uint32_t ones = g.uni(t.rank[1]);
    if (ones < 2 || (ones & 1u)) return S_WEIGHTS;
    // the entries of weight w begin behind those of the lower weights (the longer codes)
    uint32_t at = 0;
    for (int w = 1; w <= HUF_MAX_BITS; w++) {
        const uint32_t c = g.uni(t.rank[w]);
        g.sync();
        t.rank[w] = at;                                         // (every lane writes the same value)
        at += c << (w - 1);
    }
    g.sync();
    // one symbol a lane: its place among the symbols of its weight, 2^(w - 1) entries
    for (int i = lane; i < n; i += nl) {
        const uint32_t w = t.weights[i];
        if (w == 0) continue;
        uint32_t r = 0;
        for (int j = 0; j < i; j++) r += t.weights[j] == w ? 1u : 0u;
        const uint32_t len = 1u << (w - 1), from = t.rank[w] + r * len;
        const uint16_t e = (uint16_t)((uint32_t)(bits + 1 - (int)w) | ((uint32_t)i << 8));
        for (uint32_t j = 0; j < len; j++) t.huf[from + j] = e;
    }
    g.sync();
    *bits_out = bits;
    return S_OK;
}

// ---- a block's literals, handed out in order as the sequences ask for them
struct Lits {
    int type;                       // 0 Raw, 1 RLE, 2 Huffman
    int64_t left;                   // literals not handed out yet
    int64_t raw;                    // Raw: the next literal's position in the stream; RLE: the byte
    int streams, cur;               // Huffman: 1 or 4 streams; the one that is open (1..streams, 0: none yet)
    int64_t cur_left, seg, total;   // what the open stream still holds; the size of the first three; of all
    int64_t b0, b1, b2, b3, b4;     // the streams' bounds
    int bits;
    Back b;
};

// the next Huffman stream of the block's literals; the open one must be consumed exactly
template <class G>
PH_ZS_HD int next_literal_stream(G &g, Lits &L) {
    if (L.cur > 0 && (L.cur_left != 0 || !back_done(L.b))) return S_STREAM_END;
    L.cur++;
    const int64_t from = L.cur == 1 ? L.b0 : L.cur == 2 ? L.b1 : L.cur == 3 ? L.b2 : L.b3;
    const int64_t to = L.cur == 1 ? L.b1 : L.cur == 2 ? L.b2 : L.cur == 3 ? L.b3 : L.b4;
    L.cur_left = L.cur < L.streams ? L.seg : L.total - (L.streams - 1) * L.seg;
    return open_back<0>(g, L.b, from, to);
}

// n <= L.left literals to output position at
template <class G, class S>
PH_ZS_HD int put_literals(G &g, Tables &t, Lits &L, int64_t at, int64_t n, S &sink) {
    L.left -= n;
    if (L.type == 0) {
        if (n > 0) sink.literal(g, L.raw, at, n);
        L.raw += n;
        return S_OK;
    }
    if (L.type == 1) {
        if (n > 0) sink.fill(at, (uint32_t)L.raw, n);
        return S_OK;
    }
    while (n > 0) {
        if (L.cur_left == 0) {                                  // (n <= L.left: a later stream holds them)
            const int s = next_literal_stream(g, L);
            if (s != S_OK) return s;
        }
        int64_t m = n < L.cur_left ? n : L.cur_left;
        n -= m;
        L.cur_left -= m;
        for (; m > 0; m--) {
            refill_back<0>(g, L.b);
            const uint32_t e = g.uni(t.huf[peek_back(L.b, L.bits)]);
            const int nb = (int)(e & 0xffu);
            if (nb > L.b.cnt) return S_STREAM_END;
            L.b.cnt -= nb;
            sink.lit(at++, e >> 8);
        }
    }
    return S_OK;
}

// the literals section at [pos, end) of a compressed block: its header, the tree; *next = where the sequences section begins
template <class G>
PH_ZS_HD int open_literals(G &g, Tables &t, Frame &F, Lits &L, int64_t pos, int64_t end, int64_t *next) {
    if (pos >= end) return S_BLOCK_CUT;
    const uint32_t b0 = g.u8(pos);
    const int type = (int)(b0 & 3u), fmt = (int)((b0 >> 2) & 3u);
    L.cur = 0;
    L.cur_left = 0;
    if (type < 2) {
        const int hl = (fmt & 1) == 0 ? 1 : fmt == 1 ? 2 : 3;
        if (hl > end - pos) return S_BLOCK_CUT;
        const uint32_t v = g.le(pos, hl);
        const int64_t size = (int64_t)(v >> ((fmt & 1) == 0 ? 3 : 4));
        if (size > BLOCK_MAX) return S_LITERALS;
        L.type = type;
        L.left = size;
        if (type == 0) {
            if (size > end - pos - hl) return S_BLOCK_CUT;
            L.raw = pos + hl;
            *next = pos + hl + size;
        } else {
            if (end - pos - hl < 1) return S_BLOCK_CUT;
            L.raw = (int64_t)g.u8(pos + hl);
            *next = pos + hl + 1;
        }
        return S_OK;
    }
    const int hl = fmt < 2 ? 3 : fmt == 2 ? 4 : 5;
    if (hl > end - pos) return S_BLOCK_CUT;
    const uint32_t lo = g.le(pos, hl < 4 ? hl : 4), hi = hl == 5 ? g.u8(pos + 4) : 0u;
    const uint64_t v = ((uint64_t)hi << 32 | lo) >> 4;
    const int sb = fmt < 2 ? 10 : fmt == 2 ? 14 : 18;
    const int64_t size = (int64_t)(v & ((1u << sb) - 1u)), csize = (int64_t)((v >> sb) & ((1u << sb) - 1u));
    if (size > BLOCK_MAX || size == 0) return S_LITERALS;
    if (csize > end - pos - hl) return S_BLOCK_CUT;
    int64_t p = pos + hl;
    const int64_t lend = p + csize;
    if (type == 2) {
        int64_t used = 0;
        const int s = huffman_tree(g, t, p, lend, &used, &F.huf_bits);
        if (s != S_OK) return s;
        p += used;
    } else if (F.huf_bits == 0) return S_TREELESS;
    L.type = 2;
    L.left = L.total = size;
    L.bits = F.huf_bits;
    L.streams = fmt == 0 ? 1 : 4;
    if (L.streams == 1) {
        L.seg = size;
        L.b0 = p;
        L.b1 = L.b2 = L.b3 = L.b4 = lend;
        if (lend <= p) return S_BLOCK_CUT;
    } else {
        L.seg = (size + 3) / 4;
        if (size < 6) return S_LITERALS;                        // (the fourth stream would hold nothing)
        if (lend - p < 10) return S_LITERALS;                   // the jump table and a byte for each stream
        const int64_t s1 = (int64_t)g.le(p, 2), s2 = (int64_t)g.le(p + 2, 2), s3 = (int64_t)g.le(p + 4, 2);
        p += 6;
        if (s1 == 0 || s2 == 0 || s3 == 0 || s1 + s2 + s3 >= lend - p) return S_LITERALS;
        L.b0 = p;
        L.b1 = p + s1;
        L.b2 = L.b1 + s2;
        L.b3 = L.b2 + s3;
        L.b4 = lend;
    }
    *next = lend;
    return S_OK;
}

// a literal-length (which 0) or match-length (which 2) code's base and extra bits: base | bits << 24
PH_ZS_HD uint32_t length_code(int which, uint32_t c) {
    if (which == 0) {
        if (c < 16) return c;
        if (c < 20) return (16u + 2u * (c - 16u)) | (1u << 24);
        if (c < 22) return (24u + 4u * (c - 20u)) | (2u << 24);
        if (c < 24) return (32u + 8u * (c - 22u)) | (3u << 24);
        if (c == 24) return 48u | (4u << 24);
        if (c == 25) return 64u | (6u << 24);
        return (1u << (c - 19u)) | ((c - 19u) << 24);           // 26: 128, 7 bits ... 35: 65536, 16 bits
    }
    if (c < 32) return c + 3u;
    if (c < 36) return (35u + 2u * (c - 32u)) | (1u << 24);
    if (c < 38) return (43u + 4u * (c - 36u)) | (2u << 24);
    if (c < 40) return (51u + 8u * (c - 38u)) | (3u << 24);
    if (c < 42) return (67u + 16u * (c - 40u)) | (4u << 24);
    if (c == 42) return 99u | (5u << 24);
    return ((1u << (c - 36u)) + 3u) | ((c - 36u) << 24);        // 43: 131, 7 bits ... 52: 65539, 16 bits
}

// One compressed block [pos, end). fstart = where the frame's output began, limit = where this block's output must end at the latest
// (the expected length or the block maximum size, whichever comes first: past_sub says which).
template <class G, class S>
PH_ZS_HD int compressed_block(G &g, Tables &t, Frame &F, int64_t pos, int64_t end, int64_t fstart, int64_t limit, int past_sub, int64_t *produced_io,
                              S &sink) {
    int64_t produced = *produced_io;
    Lits L{};
    int s = open_literals(g, t, F, L, pos, end, &pos);
    if (s != S_OK) return s;
    // the sequences section
    if (pos >= end) return S_BLOCK_CUT;
    int64_t nseq = (int64_t)g.u8(pos++);
    if (nseq >= 128) {
        if (nseq == 255) {
            if (end - pos < 2) return S_BLOCK_CUT;
            nseq = (int64_t)g.le(pos, 2) + 0x7f00;
            pos += 2;
        } else {
            if (end - pos < 1) return S_BLOCK_CUT;
            nseq = ((nseq - 128) << 8) + (int64_t)g.u8(pos++);
        }
    }
    if (nseq == 0) {
        if (pos != end) return S_SEQ_HEADER;
    } else {
        if (pos >= end) return S_BLOCK_CUT;
        const uint32_t modes = g.u8(pos++);
        if (modes & 3u) return S_SEQ_HEADER;
        s = sequence_table(g, t, 0, (int)(modes >> 6), &pos, end, &F.ll_log);
        if (s == S_OK) s = sequence_table(g, t, 1, (int)((modes >> 4) & 3u), &pos, end, &F.of_log);
        if (s == S_OK) s = sequence_table(g, t, 2, (int)((modes >> 2) & 3u), &pos, end, &F.ml_log);
        if (s != S_OK) return s;
        Back b;
        s = open_back<1>(g, b, pos, end);
        if (s != S_OK) return s;
        refill_back<1>(g, b);
        if (b.cnt < F.ll_log + F.of_log) return S_STREAM_END;
        uint32_t ll_state = take_back(b, F.ll_log), of_state = take_back(b, F.of_log);
        refill_back<1>(g, b);
        if (b.cnt < F.ml_log) return S_STREAM_END;
        uint32_t ml_state = take_back(b, F.ml_log);
        for (int64_t i = 0; i < nseq; i++) {
            const uint32_t el = g.uni(t.ll[ll_state]), eo = g.uni(t.of[of_state]), em = g.uni(t.ml[ml_state]);
            const int ofc = (int)(eo & 0xffu);
            const uint32_t lc = length_code(0, el & 0xffu), mc = length_code(2, em & 0xffu);
            const int lb = (int)(lc >> 24), mb = (int)(mc >> 24);
            refill_back<1>(g, b);
            if (b.cnt < ofc) return S_STREAM_END;
            const int64_t ofv = ((int64_t)1 << ofc) + (int64_t)take_back(b, ofc);
            refill_back<1>(g, b);
            if (b.cnt < mb + lb) return S_STREAM_END;
            const int64_t ml = (int64_t)(mc & 0xffffffu) + (int64_t)take_back(b, mb);
            const int64_t ll = (int64_t)(lc & 0xffffffu) + (int64_t)take_back(b, lb);
            if (i + 1 < nseq) {
                refill_back<1>(g, b);
                const int nl = (int)((el >> 8) & 0xffu), nm = (int)((em >> 8) & 0xffu), no = (int)((eo >> 8) & 0xffu);
                if (b.cnt < nl + nm + no) return S_STREAM_END;
                ll_state = (el >> 16) + take_back(b, nl);
                ml_state = (em >> 16) + take_back(b, nm);
                of_state = (eo >> 16) + take_back(b, no);
            }
            int64_t off;
            if (ofv > 3) {
                off = ofv - 3;
                F.rep3 = F.rep2, F.rep2 = F.rep1, F.rep1 = off;
            } else {
                const int64_t idx = ofv + (ll == 0 ? 1 : 0);
                if (idx == 1) off = F.rep1;
                else if (idx == 2) {
                    off = F.rep2;
                    F.rep2 = F.rep1, F.rep1 = off;
                } else {
                    off = idx == 3 ? F.rep3 : F.rep1 - 1;
                    if (off == 0) return S_OFFSET;
                    F.rep3 = F.rep2, F.rep2 = F.rep1, F.rep1 = off;
                }
            }
            if (ll > L.left) return S_LIT_COUNT;
            if (ll + ml > limit - produced) return past_sub;
            if (off > produced + ll - fstart) return S_OFFSET;
            s = put_literals(g, t, L, produced, ll, sink);
            if (s != S_OK) return s;
            produced += ll;
            sink.match(produced, off, ml);
            produced += ml;
        }
        if (!back_done(b)) return S_STREAM_END;
    }
    // the literals behind the last sequence
    if (L.left > limit - produced) return past_sub;
    const int64_t rest = L.left;
    s = put_literals(g, t, L, produced, rest, sink);
    if (s != S_OK) return s;
    produced += rest;
    if (L.type == 2) {                                          // (the fourth of four streams may hold no literal: 9 of them)
        while (L.cur < L.streams) {
            s = next_literal_stream(g, L);
            if (s != S_OK) return s;
        }
        if (L.cur_left != 0 || !back_done(L.b)) return S_STREAM_END;
    }
    *produced_io = produced;
    return S_OK;
}

// The frames of [pos, end) into a sink of `expected` bytes. The caller has end - pos >= MIN_FRAME (check_sizes). The sink has
// frame_begin(fstart, hashed), lit(at, byte), literal(g, from, at, n) (n bytes of the stream), fill(at, byte, n), match(at, offset, n) (as if
// byte by byte, front to back) and frame_hash(fstart, produced): the low 32 bits of the XXH64 of output [fstart, produced).
template <class G, class S>
PH_ZS_HD int decode_stream(G &g, int64_t pos, int64_t end, int64_t expected, Tables &t, S &sink) {
    int64_t produced = 0;
    for (;;) {
        if (end - pos < 4) return S_INPUT_LEFT;
        const uint32_t magic = g.le(pos, 4);
        if ((magic & 0xfffffff0u) == SKIP_MAGIC) {
            if (end - pos < 8) return S_INPUT_CUT;
            const int64_t n = (int64_t)g.le(pos + 4, 4);
            if (n > end - pos - 8) return S_INPUT_CUT;
            pos += 8 + n;
            if (pos == end) break;
            continue;
        }
        if (magic != MAGIC) return S_MAGIC;
        pos += 4;
        if (end - pos < 1) return S_INPUT_CUT;
        const uint32_t fhd = g.u8(pos++);
        if (fhd & 8u) return S_RESERVED;
        const bool single = (fhd & 32u) != 0, checksum = (fhd & 4u) != 0;
        const int did = (int)(fhd & 3u), fcs_flag = (int)(fhd >> 6);
        const int did_bytes = did == 3 ? 4 : did, fcs_bytes = fcs_flag == 0 ? (single ? 1 : 0) : 1 << fcs_flag;
        if (end - pos < (single ? 0 : 1) + did_bytes + fcs_bytes) return S_INPUT_CUT;
        int64_t window = 0;
        if (!single) {
            const uint32_t wd = g.u8(pos++);
            const int wl = 10 + (int)(wd >> 3);
            if (wl > 31) return S_WINDOW;
            window = ((int64_t)1 << wl) + (((int64_t)1 << wl) >> 3) * (int64_t)(wd & 7u);
        }
        if (did_bytes) {
            if (g.le(pos, did_bytes) != 0) return S_DICTIONARY;
            pos += did_bytes;
        }
        int64_t fcs = -1;
        if (fcs_bytes) {
            const uint64_t lo = g.le(pos, fcs_bytes < 4 ? fcs_bytes : 4), hi = fcs_bytes == 8 ? g.le(pos + 4, 4) : 0u;
            pos += fcs_bytes;
            if (hi >> 31) return S_CONTENT_SIZE;
            fcs = (int64_t)(hi << 32 | lo) + (fcs_bytes == 2 ? 256 : 0);
            if (fcs > expected - produced) return S_CONTENT_SIZE;
            if (single) window = fcs;
        }
        const int64_t bmax = window < BLOCK_MAX ? window : BLOCK_MAX;
        const int64_t fstart = produced;
        Frame F{0, -1, -1, -1, 1, 4, 8};
        sink.frame_begin(fstart, checksum);
        for (;;) {
            if (end - pos < 3) return S_INPUT_CUT;
            const uint32_t bh = g.le(pos, 3);
            pos += 3;
            const int type = (int)((bh >> 1) & 3u);
            const int64_t size = (int64_t)(bh >> 3);
            if (type == 3) return S_BLOCK_TYPE;
            if (size > bmax) return S_BLOCK_SIZE;
            if (type == 0) {
                if (size > end - pos) return S_INPUT_CUT;
                if (size > expected - produced) return S_OUTPUT_PAST;
                if (size > 0) sink.literal(g, pos, produced, size);
                pos += size;
                produced += size;
            } else if (type == 1) {
                if (end - pos < 1) return S_INPUT_CUT;
                if (size > expected - produced) return S_OUTPUT_PAST;
                if (size > 0) sink.fill(produced, g.u8(pos), size);
                pos += 1;
                produced += size;
            } else {
                if (size > end - pos) return S_INPUT_CUT;
                const bool by_block = produced + bmax < expected;
                const int s = compressed_block(g, t, F, pos, pos + size, fstart, by_block ? produced + bmax : expected, by_block ? S_BLOCK_OUTPUT : S_OUTPUT_PAST,
                                               &produced, sink);
                if (s != S_OK) return s;
                pos += size;
            }
            if (bh & 1u) break;
        }
        if (fcs >= 0 && produced - fstart != fcs) return S_CONTENT_SIZE;
        if (checksum) {
            if (end - pos < 4) return S_INPUT_CUT;
            const uint32_t want = g.le(pos, 4);
            pos += 4;
            if (sink.frame_hash(fstart, produced) != want) return S_CHECKSUM;
        }
        if (pos == end) break;
    }
    return produced == expected ? S_OK : S_OUTPUT_SHORT;
}

// what the host can decide from the two lengths alone (the Parquet page directory asks the same before anything is allocated)
PH_ZS_HD int check_sizes(int64_t src_bytes, int64_t expected) {
    if (src_bytes == 0) return expected == 0 ? S_OK : S_EMPTY;
    if (src_bytes < MIN_FRAME) return S_TOO_SHORT;
    return expected > MAX_EXPANSION * src_bytes ? S_IMPOSSIBLE : S_OK;
}
// ... and from the first four bytes of a stream of at least MIN_FRAME bytes
PH_ZS_HD int check_header(const uint8_t *s) {
    const uint32_t magic = (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24;
    return magic == MAGIC || (magic & 0xfffffff0u) == SKIP_MAGIC ? S_OK : S_MAGIC;
}

// ---- XXH64 (seed 0), in the pieces that the host sink and the device sink share
constexpr uint64_t XP1 = 11400714785074694791ull, XP2 = 14029467366897019727ull, XP3 = 1609587929392839161ull, XP4 = 9650029242287828579ull,
                   XP5 = 2870177450012600261ull;
PH_ZS_HD uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
PH_ZS_HD uint64_t xxh_round(uint64_t acc, uint64_t in) { return rotl64(acc + in * XP2, 31) * XP1; }
PH_ZS_HD uint64_t xxh_init(int k) { return k == 0 ? XP1 + XP2 : k == 1 ? XP2 : k == 2 ? 0 : 0 - XP1; }   // accumulator k of 4
PH_ZS_HD uint64_t xxh_merge(uint64_t v1, uint64_t v2, uint64_t v3, uint64_t v4) {
    uint64_t h = rotl64(v1, 1) + rotl64(v2, 7) + rotl64(v3, 12) + rotl64(v4, 18);
    h = (h ^ xxh_round(0, v1)) * XP1 + XP4;
    h = (h ^ xxh_round(0, v2)) * XP1 + XP4;
    h = (h ^ xxh_round(0, v3)) * XP1 + XP4;
    h = (h ^ xxh_round(0, v4)) * XP1 + XP4;
    return h;
}
// h = the merged accumulators (or XP5 for fewer than 32 bytes) + the length; rd(i) = byte i of the n < 32 that are left
template <class R>
PH_ZS_HD uint32_t xxh_finish(uint64_t h, int n, R rd) {
    int i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t k = 0;
        for (int j = 0; j < 8; j++) k |= (uint64_t)rd(i + j) << (8 * j);
        h = rotl64(h ^ xxh_round(0, k), 27) * XP1 + XP4;
    }
    if (i + 4 <= n) {
        uint64_t k = 0;
        for (int j = 0; j < 4; j++) k |= (uint64_t)rd(i + j) << (8 * j);
        h = rotl64(h ^ (k * XP1), 23) * XP2 + XP3;
        i += 4;
    }
    for (; i < n; i++) h = rotl64(h ^ ((uint64_t)rd(i) * XP5), 11) * XP1;
    h ^= h >> 33;
    h *= XP2;
    h ^= h >> 29;
    h *= XP3;
    h ^= h >> 32;
    return (uint32_t)h;
}

struct HostStream {
    const uint8_t *s;
    uint32_t u8(int64_t p) const { return s[p]; }
    uint32_t le(int64_t p, int k) const {
        uint32_t v = 0;
        for (int i = 0; i < k; i++) v |= (uint32_t)s[p + i] << (8 * i);
        return v;
    }
    uint32_t back_a(int64_t p, int k) const { return le(p, k); }
    uint32_t back_b(int64_t p, int k) const { return le(p, k); }
    int lane() const { return 0; }
    int lanes() const { return 1; }
    void sync() const {}
    void inc(uint32_t *p) const { ++*p; }
    uint32_t uni(uint32_t v) const { return v; }
};

// what a stream was made of (ph_zstd_stream_stats_host): counted by the host sink
struct Stats {
    int64_t literals, sequences, match_bytes, far_match_bytes, far_limit;   // far: an offset above far_limit
};

struct HostSink {
    uint8_t *d;
    Stats *stats;
    void frame_begin(int64_t, bool) {}
    void lit(int64_t at, uint32_t byte) {
        d[at] = (uint8_t)byte;
        if (stats) stats->literals++;
    }
    void literal(const HostStream &g, int64_t from, int64_t at, int64_t n) {
        for (int64_t i = 0; i < n; i++) d[at + i] = g.s[from + i];
        if (stats) stats->literals += n;
    }
    void fill(int64_t at, uint32_t byte, int64_t n) {
        for (int64_t i = 0; i < n; i++) d[at + i] = (uint8_t)byte;
        if (stats) stats->literals += n;
    }
    void match(int64_t at, int64_t off, int64_t n) {
        for (int64_t i = 0; i < n; i++) d[at + i] = d[at - off + i];
        if (stats) {
            stats->sequences++;
            stats->match_bytes += n;
            if (off > stats->far_limit) stats->far_match_bytes += n;
        }
    }
    uint32_t frame_hash(int64_t fstart, int64_t produced) const {
        const uint8_t *p = d + fstart;
        const int64_t n = produced - fstart;
        int64_t i = 0;
        uint64_t h = XP5;
        if (n >= 32) {
            uint64_t v0 = xxh_init(0), v1 = xxh_init(1), v2 = xxh_init(2), v3 = xxh_init(3);
            auto rd64 = [&](int64_t a) {
                uint64_t k = 0;
                for (int j = 0; j < 8; j++) k |= (uint64_t)p[a + j] << (8 * j);
                return k;
            };
            for (; i + 32 <= n; i += 32) {
                v0 = xxh_round(v0, rd64(i));
                v1 = xxh_round(v1, rd64(i + 8));
                v2 = xxh_round(v2, rd64(i + 16));
                v3 = xxh_round(v3, rd64(i + 24));
            }
            h = xxh_merge(v0, v1, v2, v3);
        }
        return xxh_finish(h + (uint64_t)n, (int)(n - i), [&](int j) { return (uint32_t)p[i + j]; });
    }
};

struct HostTables : Tables {
    uint16_t huf_[HUF_CAP];
    uint32_t ll_[1 << LL_LOG], of_[1 << OF_LOG], ml_[1 << ML_LOG], wt_[1 << WT_LOG], rank_[16];
    uint8_t weights_[MAX_SYMS];
    int16_t norm_[MAX_SYMS];
    uint16_t cum_[MAX_SYMS];
    HostTables() { huf = huf_, ll = ll_, of = of_, ml = ml_, wt = wt_, weights = weights_, norm = norm_, cum = cum_, rank = rank_; }
};

// One whole stream src[0, src_bytes) on the host into dst[0, expected). dst may be null when expected is 0.
inline int decompress_host_stats(const uint8_t *src, int64_t src_bytes, uint8_t *dst, int64_t expected, Stats *stats) {
    int s = check_sizes(src_bytes, expected);
    if (s != S_OK || src_bytes == 0) return s;
    s = check_header(src);
    if (s != S_OK) return s;
    HostStream g{src};
    HostTables t;
    HostSink sink{dst, stats};
    return decode_stream(g, 0, src_bytes, expected, t, sink);
}
inline int decompress_host(const uint8_t *src, int64_t src_bytes, uint8_t *dst, int64_t expected) {
    return decompress_host_stats(src, src_bytes, dst, expected, nullptr);
}

}  // namespace zstd
}  // namespace ph
