// GZIP streams (Parquet codec 2) inflated on the device: one launch over n independent sections, ONE WAVE a section, on section_wave.h's
// frame (window, ring, flush, the section's end), and the two raw entry points ph_gzip_decompress / ph_gzip_decompress_host.
//
// A DEFLATE stream is a chain of Huffman symbols of 1 to 15 bits, each of which begins where the one before it ended, and a match reads what
// the same stream has just written: the parallelism is across sections and, inside one, across the entries of a table that is being built
// and the bytes of a match or a stored block. The wave IS the getter and the sink that gzip_decode.h's decode_stream is instantiated over:
//   - the decoder's bit buffer (64 bits, a uniform value) is topped up with le(p, k): up to four window bytes, re-loading the window when
//     p + k lies outside it, so a code, a stored block's LEN / NLEN, a dynamic header or a trailer may straddle a window edge anywhere, and a
//     step back of the bytes the bit buffer held (in front of a stored block and of a trailer) may cross the edge backwards;
//   - the tables live in LDS (gzip::Tables): build_table runs its steps lane-strided — counts by LDS adds, one lane per code length for
//     the canonical codes, one symbol a lane for the entries — and the chain reads one entry a symbol, two for a code above the primary
//     bits. The fixed code's tables are built the same way when a fixed block is met (and kept while fixed blocks follow each other);
//   - a literal is one LDS store into the ring. A match (3 to 258 bytes) is ONE step that reads all its source bytes, then writes
//     (section_wave.h, ring size): d <= 32768, so a ring of exactly 2^15 bytes serves every distance the format can state;
//   - completed ring bytes are, as they are flushed, folded into the member's CRC-32 in steps of GZ_FLUSH bytes straight from the ring: lane i
//     runs the byte-wise table over bytes [64 i, 64 i + 64) from a zero register, multiplies the result by x^(8 * bytes behind its slice)
//     modulo the CRC polynomial, the lanes' words are xor-ed, and the running register, multiplied by x^(8 * GZ_FLUSH), takes the sum. A
//     member's tail does the same with slices of its own size.
// Bounds beyond the frame's: table writes go to entries below the capacities build_table checks.
#include "gzip_decode.h"
#include "gzip_decompress.h"

namespace ph {

namespace {

constexpr uint32_t CRC_POLY = 0xedb88320u;
constexpr uint32_t X8 = 0x00800000u;                            // x^8 (bit 31 is x^0)

// a * b modulo the CRC-32 polynomial, bits reflected
__device__ __forceinline__ uint32_t mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
#pragma unroll 4
    for (int i = 0; i < 32; i++) {
        p ^= b & (0u - ((a >> (31 - i)) & 1u));
        b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}
__device__ __forceinline__ uint32_t xpow8(uint32_t n) {         // x^(8 n)
    uint32_t acc = 0x80000000u, p = X8;
    while (n) {
        if (n & 1u) acc = mulmod(acc, p);
        p = mulmod(p, p);
        n >>= 1;
    }
    return acc;
}
__device__ __forceinline__ uint32_t xor_lanes(uint32_t v) {
#pragma unroll
    for (int m = 1; m < GZ_THREADS; m <<= 1) v ^= (uint32_t)__shfl_xor((int)v, m, GZ_THREADS);
    return v;
}

struct GzWave : SectionWave<GZ_THREADS, GZ_TILE, GZ_RING> {
    using Base = SectionWave<GZ_THREADS, GZ_TILE, GZ_RING>;   // (Base::lane: build_table asks the getter for lane())
    const uint32_t *crc_tab;
    int64_t crc_done;                // the member's output up to here is in crc_reg
    uint32_t crc_reg, lane_pow, chunk_pow;

    // ---- the getter
    __device__ __forceinline__ int lane() const { return Base::lane; }
    __device__ __forceinline__ int lanes() const { return GZ_THREADS; }
    __device__ __forceinline__ void sync() const { wave_sync(); }
    __device__ __forceinline__ void inc(uint32_t *p) const { atomicAdd(p, 1u); }
    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

    // (decode_stream asks for positions inside [src0, src_end) only)
    __device__ __forceinline__ uint32_t u8(int64_t p) {
        if (p < win_base || p >= win_end) load_window(p);
        return uni(s_in[p - win_base]);
    }
    __device__ __forceinline__ uint32_t le(int64_t p, int k) {   // bytes [p, p + k), k <= 4, little-endian
        if (p < win_base || p + k > win_end) load_window(p);
        const int at = (int)(p - win_base);
        uint32_t v = s_in[at];
        if (k > 1) v |= (uint32_t)s_in[at + 1] << 8;
        if (k > 2) v |= (uint32_t)s_in[at + 2] << 16;
        if (k > 3) v |= (uint32_t)s_in[at + 3] << 24;
        return uni(v);
    }

    // ---- the sink
    // the CRC of ring bytes [crc_done, crc_done + n), n <= GZ_FLUSH, lane i over the `slice` bytes from i * slice on; pw = x^(8 * bytes
    // behind this lane's slice), all = x^(8 n)
    __device__ __forceinline__ void crc_fold(int n, int slice, uint32_t pw, uint32_t all) {
        const int from = Base::lane * slice;
        int to = from + slice;
        if (to > n) to = n;
        uint32_t c = 0;
        for (int j = from; j < to; j++) c = gzip::crc_byte(crc_tab, c, s_ring[(dst0 + crc_done + j) & MASK]);
        c = xor_lanes(mulmod(c, pw));
        crc_reg = mulmod(crc_reg, all) ^ c;
        crc_done += n;
    }
    __device__ __forceinline__ void flush_if_due(int64_t produced) {
        Base::flush_if_due(produced, GZ_FLUSH);
        while (produced - crc_done >= GZ_FLUSH) crc_fold(GZ_FLUSH, GZ_FLUSH / GZ_THREADS, lane_pow, chunk_pow);
    }
    __device__ __forceinline__ uint32_t member_crc(int64_t, int64_t produced) {
        flush_if_due(produced);
        const int n = (int)(produced - crc_done);                // < GZ_FLUSH
        if (n > 0) {
            const int slice = (n + GZ_THREADS - 1) / GZ_THREADS;
            int behind = n - (Base::lane + 1) * slice;
            if (behind < 0) behind = 0;
            crc_fold(n, slice, xpow8((uint32_t)behind), xpow8((uint32_t)n));
        }
        const uint32_t crc = ~crc_reg;
        crc_reg = 0xffffffffu;                                   // the next member's begins here
        return uni(crc);
    }
    __device__ __forceinline__ void lit(int64_t at, uint32_t byte) {
        s_ring[(dst0 + at) & MASK] = (unsigned char)byte;        // (every lane stores the same byte)
        flush_if_due(at + 1);
    }
    __device__ __forceinline__ void literal(GzWave &, int64_t from, int64_t at, int64_t n) {   // a stored block's bytes (inside the stream: inflate)
        wave_sync();
        while (n > 0) {
            if (from < win_base || from >= win_end) load_window(from);
            int64_t c = win_end - from;
            if (c > n) c = n;
            if (c > GZ_CHUNK) c = GZ_CHUNK;
            for (int i = Base::lane; i < (int)c; i += GZ_THREADS) s_ring[(dst0 + at + i) & MASK] = s_in[from - win_base + i];
            wave_sync();
            from += c;
            at += c;
            n -= c;
            flush_if_due(at);
        }
    }
    __device__ __forceinline__ void match(int64_t at, int64_t dist, int64_t n) {               // 1 <= dist <= at, dist <= 32768, 3 <= n <= 258
        constexpr int PER = GZ_MATCH / GZ_THREADS;
        const uint32_t off = (uint32_t)dist;
        const int64_t sbase = dst0 - dist;
        const int c = (int)n;
        wave_sync();
        if (c <= GZ_THREADS) {                                   // the common case: one byte a lane
            uint32_t j = (uint32_t)Base::lane;
            if (off < (uint32_t)c) j %= off;                     // byte j reads j mod off behind the step's first source byte
            unsigned char b = 0;
            if (Base::lane < c) b = s_ring[(sbase + at + j) & MASK];
            wave_sync();
            if (Base::lane < c) s_ring[(dst0 + at + Base::lane) & MASK] = b;
        } else {
            unsigned char b[PER];
            if (off >= (uint32_t)c) {
#pragma unroll
                for (int k = 0; k < PER; k++) {
                    const int j = Base::lane + k * GZ_THREADS;
                    b[k] = j < c ? s_ring[(sbase + at + j) & MASK] : 0;
                }
            } else {
                uint32_t r = (uint32_t)Base::lane, step = GZ_THREADS;
                if (off <= (uint32_t)GZ_THREADS) { r %= off; step %= off; }   // (r < off and step < off or 64 < off: one wrap a step at most)
#pragma unroll
                for (int k = 0; k < PER; k++) {
                    b[k] = Base::lane + k * GZ_THREADS < c ? s_ring[(sbase + at + r) & MASK] : 0;
                    r += step;
                    if (r >= off) r -= off;
                }
            }
            wave_sync();
#pragma unroll
            for (int k = 0; k < PER; k++) {
                const int j = Base::lane + k * GZ_THREADS;
                if (j < c) s_ring[(dst0 + at + j) & MASK] = b[k];
            }
        }
        wave_sync();
        flush_if_due(at + n);
    }
};

}  // namespace

__global__ __launch_bounds__(GZ_THREADS) void gzip_sections_kernel(SectionArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gz_lds[];
    const SnSection S = A.sec[blockIdx.x];
    const int lane = threadIdx.x;
    GzWave W;
    W.open(gz_lds, A, S);
    unsigned char *p = gz_lds + GZ_TILE + GZ_RING;               // behind the frame's window and ring: the tables
    gzip::Tables T;
    T.lit = reinterpret_cast<uint32_t *>(p), p += 4 * gzip::LIT_CAP;
    T.dist = reinterpret_cast<uint32_t *>(p), p += 4 * gzip::DIST_CAP;
    uint32_t *crc_tab = reinterpret_cast<uint32_t *>(p);
    p += 1024;
    T.count = reinterpret_cast<uint32_t *>(p), p += 64;
    T.first = reinterpret_cast<uint32_t *>(p), p += 64;
    T.codes = reinterpret_cast<uint16_t *>(p), p += 2 * gzip::MAX_LENS;
    T.lens = p;
    T.crc = crc_tab;
    T.fixed = 0;
    for (int i = lane; i < 256; i += GZ_THREADS) {
        uint32_t c = (uint32_t)i;
#pragma unroll
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (CRC_POLY & (0u - (c & 1u)));
        crc_tab[i] = c;
    }
    W.crc_tab = crc_tab;
    W.crc_done = 0;
    W.crc_reg = 0xffffffffu;
    W.lane_pow = xpow8((uint32_t)((GZ_THREADS - 1 - lane) * (GZ_FLUSH / GZ_THREADS)));
    W.chunk_pow = xpow8(GZ_FLUSH);
    wave_sync();

    int sub = gzip::check_sizes(S.src_bytes, S.dst_bytes);
    if (sub == gzip::S_OK && S.src_bytes > 0) sub = uni(gzip::decode_stream(W, W.src0, W.src_end, S.dst_bytes, T, W));
    W.close(A, S, sub, pq::C_GZIP);
}

int gzip_decompress_sections(ph_ctx *ctx, const uint8_t *src, uint8_t *dst, const SnSection *sections_dev, int32_t n, pq::PageDesc *pages_dev,
                             unsigned long long *err, int32_t *status_dev) {
    return launch_sections<gzip_sections_kernel, GZ_THREADS, GZ_LDS>(ctx, src, dst, sections_dev, n, pages_dev, err, status_dev);
}

}  // namespace ph

extern "C" int ph_gzip_decompress_host(const void *src, int64_t src_bytes, void *dst, int64_t expected, int64_t *produced) {
    PH_REQUIRE(src_bytes >= 0 && (src || src_bytes == 0) && expected >= 0 && (dst || expected == 0), "ph_gzip_decompress_host: bad arguments");
    if (produced) *produced = 0;
    const int sub = ph::gzip::decompress_host((const uint8_t *)src, src_bytes, (uint8_t *)dst, expected);
    PH_REQUIRE(sub == ph::gzip::S_OK, "ph_gzip_decompress_host: a corrupt GZIP stream of %lld bytes for %lld: %s", (long long)src_bytes, (long long)expected,
               ph::gzip::sub_text(sub));
    if (produced) *produced = expected;
    return PH_OK;
}

extern "C" int ph_gzip_decompress(ph_ctx *ctx, const void *src_dev, const int64_t *src_pos, const int64_t *src_bytes, void *dst_dev,
                                  const int64_t *dst_pos, const int64_t *dst_bytes, int32_t n, int32_t *status) {
    return ph::decompress_streams(ctx, "ph_gzip_decompress", ph::gzip_decompress_sections, src_dev, src_pos, src_bytes, dst_dev, dst_pos, dst_bytes, n, status);
}
