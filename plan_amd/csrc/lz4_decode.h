// The LZ4 block format (Parquet's LZ4_RAW, codec 7: bare blocks, no frame, no length preamble), decoded by ONE set of functions compiled for
// the host (ph_lz4_decompress_host and the Parquet host twin, sequentially) and for the device (lz4_decompress.hip, whose kernel instantiates
// decode_block over an LDS window and an LDS ring). In the manner of snappy_decode.h: a byte getter g and a sink.
//
// A block is a chain of sequences:
//   token        high nibble = literal length, low nibble = match length - 4
//   [extension]  literal length 15: bytes that are added until one is below 255
//   literals
//   offset       2 bytes, little-endian: the match begins `offset` behind the write position and may overlap what it writes
//   [extension]  match length nibble 15: as above
// and the last sequence ends behind its literals. Nothing in the stream says how many bytes it holds: the caller states `expected`.
//
// Rules, each decided before a byte moves. Lengths are summed in 64 bits, at most 64 extension bytes between two checks, and a length is
// refused as soon as it passes what is left of the expected output (or, for literals, of the input): a run of 0xFF bytes neither overflows
// nor runs on. A match needs 1 <= offset <= bytes produced. The stream must produce exactly `expected` bytes and consume exactly its input.
// Every sequence consumes at least one input byte, so the loop is bounded by the stream's length; nothing is read outside [pos, end) and
// nothing is written outside [dst, dst + expected).
//
// NOT enforced: the format's end-of-block restrictions (the last 5 bytes are literals, the last match starts at least 12 bytes before the
// end). They bind compressors, which need them for their own fast paths; a stream that breaks them still decodes to exactly one byte string.
// liblz4 refuses such streams, so this decoder reads a few streams that liblz4 does not. The other way round, liblz4 accepts offset 0 (and
// writes zeros) and a stream that stops short of the buffer it was given; both are refused here.
//
// Codec 5, Parquet's deprecated LZ4, is a different thing: three incompatible framings exist under that number (Hadoop's 8-byte block
// headers, the LZ4 frame format that parquet-go writes, and bare blocks). pyarrow writes none of them, so none could be tested, and the
// Parquet load refuses codec 5 whatever its flags.
#pragma once
#include <cstdint>

#include "planhip.h"

#if defined(__HIPCC__)
#define PH_LZ_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PH_LZ_HD inline
#endif

namespace ph {
namespace lz4 {

// why a stream is refused (all of them PH_EINVAL)
enum Sub : int {
    S_OK = 0,
    S_EMPTY = 1,          // a stream of 0 bytes for more than 0 bytes
    S_IMPOSSIBLE = 2,     // more than 255 bytes are expected per stream byte
    S_OFFSET_ZERO = 3,    // a match with offset 0
    S_OFFSET_FAR = 4,     // a match that reaches in front of the first byte produced
    S_INPUT_CUT = 5,      // the input ends inside a sequence: in a length, in the literals or in the offset
    S_OUTPUT_PAST = 6,    // a literal run or a match writes past the expected length
    S_OUTPUT_SHORT = 7,   // the last sequence ends before the expected length is reached
    S_INPUT_LEFT = 8,     // input is left over once the expected length is reached
    S_NO_FINAL = 9,       // the stream ends behind a match, without the final token
};

inline const char *sub_text(int s) {
    switch (s) {
    case S_EMPTY: return "an empty stream for more than 0 bytes";
    case S_IMPOSSIBLE: return "more than 255 bytes are expected per stream byte";
    case S_OFFSET_ZERO: return "a match with offset 0";
    case S_OFFSET_FAR: return "a match offset beyond the bytes produced so far";
    case S_INPUT_CUT: return "the input ends inside a sequence";
    case S_OUTPUT_PAST: return "a literal run or a match writes past the expected length";
    case S_OUTPUT_SHORT: return "the last sequence ends before the expected length is reached";
    case S_INPUT_LEFT: return "input is left over once the expected length is reached";
    case S_NO_FINAL: return "the stream ends behind a match, without a final token";
    default: return "unknown cause";
    }
}

// No byte of a stream yields more than 255 bytes of output (an extension byte of a match length), so what a header is allowed to make a
// caller allocate is bounded by the stream's own size.
constexpr int64_t MAX_EXPANSION = 255;
constexpr int FF_STEP = 64;         // extension bytes a getter's ff_run looks at in one go

// The extension bytes of a length whose nibble was 15: *len (15 on entry) grows by each byte up to and with the first one below 255.
// out_left = the bytes the output still takes; literal: the length must also fit the input behind the extension bytes.
// g.ff_run(pos, end) = how many bytes from pos on are 0xFF, looking at no more than FF_STEP of them and never past `end`; 0: g.u8(pos) ends
// the run (the device counts a window's worth with one ballot).
template <class G>
PH_LZ_HD int read_extension(G &g, int64_t &pos, int64_t end, int64_t out_left, bool literal, int64_t *len) {
    int64_t n = *len;
    for (;;) {
        if (pos >= end) return S_INPUT_CUT;
        const int64_t k = g.ff_run(pos, end);
        if (k == 0) {
            n += (int64_t)g.u8(pos++);
            break;
        }
        n += 255 * k;
        pos += k;
        if (n > out_left) return S_OUTPUT_PAST;
        if (literal && n > end - pos) return S_INPUT_CUT;
    }
    *len = n;
    return S_OK;
}

// The sequences of [pos, end) into a sink of `expected` bytes. The sink has literal(g, from, at, n) (n bytes of the stream from `from` to
// output position `at`) and match(at, offset, n) (as if byte by byte, front to back: an overlapping match repeats a pattern).
// The caller has pos < end (an empty stream is the caller's case).
template <class G, class S>
PH_LZ_HD int decode_block(G &g, int64_t pos, int64_t end, int64_t expected, S &sink) {
    int64_t produced = 0;
    for (;;) {
        if (pos >= end) return S_NO_FINAL;                      // (only behind a match: the first round has pos < end)
        const uint32_t token = g.u8(pos++);
        int64_t lit = (int64_t)(token >> 4);
        if (lit == 15) {
            const int s = read_extension(g, pos, end, expected - produced, true, &lit);
            if (s != S_OK) return s;
        }
        if (lit > expected - produced) return S_OUTPUT_PAST;
        if (lit > end - pos) return S_INPUT_CUT;
        if (lit > 0) sink.literal(g, pos, produced, lit);
        pos += lit;
        produced += lit;
        if (pos == end) return produced == expected ? S_OK : S_OUTPUT_SHORT;   // the last sequence ends behind its literals
        if (produced == expected) return S_INPUT_LEFT;          // (a match yields at least 4 bytes)
        if (end - pos < 2) return S_INPUT_CUT;
        const int64_t offset = (int64_t)((uint32_t)g.u8(pos) | ((uint32_t)g.u8(pos + 1) << 8));
        pos += 2;
        if (offset == 0) return S_OFFSET_ZERO;
        if (offset > produced) return S_OFFSET_FAR;
        int64_t ml = (int64_t)(token & 15u);
        if (ml == 15) {
            const int s = read_extension(g, pos, end, expected - produced, false, &ml);
            if (s != S_OK) return s;
        }
        ml += 4;
        if (ml > expected - produced) return S_OUTPUT_PAST;
        sink.match(produced, offset, ml);
        produced += ml;
    }
}

struct HostStream {
    const uint8_t *s;
    uint8_t u8(int64_t p) const { return s[p]; }
    int64_t ff_run(int64_t pos, int64_t end) const {
        int64_t k = 0;
        while (k < FF_STEP && pos + k < end && s[pos + k] == 0xff) k++;
        return k;
    }
};

struct HostSink {
    uint8_t *d;
    void literal(const HostStream &g, int64_t from, int64_t at, int64_t n) { for (int64_t i = 0; i < n; i++) d[at + i] = g.s[from + i]; }
    void match(int64_t at, int64_t offset, int64_t n) { for (int64_t i = 0; i < n; i++) d[at + i] = d[at - offset + i]; }
};

// what the host can decide from the two lengths alone (the Parquet page directory asks the same before anything is allocated)
PH_LZ_HD int check_sizes(int64_t src_bytes, int64_t expected) {
    if (src_bytes == 0) return expected == 0 ? S_OK : S_EMPTY;
    return expected > MAX_EXPANSION * src_bytes ? S_IMPOSSIBLE : S_OK;
}

// One whole block src[0, src_bytes) on the host into dst[0, expected). dst may be null when expected is 0.
inline int decompress_host(const uint8_t *src, int64_t src_bytes, uint8_t *dst, int64_t expected) {
    const int s = check_sizes(src_bytes, expected);
    if (s != S_OK || src_bytes == 0) return s;
    HostStream g{src};
    HostSink sink{dst};
    return decode_block(g, 0, src_bytes, expected, sink);
}

}  // namespace lz4
}  // namespace ph
