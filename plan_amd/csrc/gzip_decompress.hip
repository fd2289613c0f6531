// GZIP streams (Parquet codec 2) inflated on the device: one launch over n independent sections, ONE WAVE a section (gzip_decompress.h),
// and the two raw entry points ph_gzip_decompress / ph_gzip_decompress_host.
//
// A DEFLATE stream is a chain of Huffman symbols of 1 to 15 bits, each of which begins where the one before it ended, and a match reads what
// the same stream has just written: the parallelism is across sections and, inside one, across the entries of a table that is being built
// and the bytes of a match or a stored block. The wave IS the getter and the sink that gzip_decode.h's decode_stream is instantiated over:
//   - the compressed input is staged through LDS in GZ_TILE-byte windows, 16-byte loads. The decoder's bit buffer (64 bits, a uniform
//     value) is topped up with le(p, k): up to four window bytes, re-loading the window when p + k lies outside it, so a code, a stored
//     block's LEN / NLEN, a dynamic header or a trailer may straddle a window edge anywhere, and a step back of the bytes the bit buffer held
//     (in front of a stored block and of a trailer) may cross the edge backwards;
//   - the tables live in LDS (gzip::Tables): build_table runs its steps lane-strided — counts by LDS adds, one lane per code length for
//     the canonical codes, one symbol a lane for the entries — and the chain reads one entry a symbol, two for a code above the primary
//     bits. The fixed code's tables are built the same way when a fixed block is met (and kept while fixed blocks follow each other);
//   - output byte a of the stream lives at s_ring[a mod GZ_RING] (a counts from its destination's 16-byte boundary). A literal is one LDS
//     store. A match (3 to 258 bytes) is ONE step that reads all its source bytes into registers, then writes: source byte j of a step at
//     output position p is p - d + (j mod d), which lies in front of p whatever the overlap, and the slot that byte j takes is the slot of
//     position p + j - 32768, which no source of a LATER step is (d <= 32768) and which this step has read already if it is one of its own.
//     So every distance the format can state is served from LDS, with no fence and no global reload, by a ring of exactly 2^15 bytes;
//   - completed ring bytes are flushed to global memory with 16-byte stores whenever GZ_FLUSH of them are waiting, and folded into the
//     member's CRC-32 in steps of GZ_FLUSH bytes straight from the ring: lane i runs the byte-wise table over bytes [64 i, 64 i + 64) from a
//     zero register, multiplies the result by x^(8 * bytes behind its slice) modulo the CRC polynomial, the lanes' words are xor-ed, and the
//     running register, multiplied by x^(8 * GZ_FLUSH), takes the sum. A member's tail does the same with slices of its own size.
// One wave's LDS instructions execute in order; wave_sync() (a wavefront-scope fence around a wave barrier, no instruction) keeps the compiler
// from reordering them.
// Bounds: decode_stream checks every step against the stream's end and the expected length BEFORE a byte moves; the window is loaded in whole
// aligned 16-byte units that hold at least one byte of the stream (an aligned unit never leaves its page); stores go to [dst, dst + expected)
// only, the unaligned head and tail byte by byte; table writes go to entries below the capacities build_table checks.
#include <vector>

#include "gzip_decode.h"
#include "gzip_decompress.h"
#include "str_encode.h"

namespace ph {

namespace {

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

struct GzArgs {
    const uint8_t *src;
    uint8_t *dst;
    const SnSection *sec;
    pq::PageDesc *pages;
    unsigned long long *err;
    int32_t *status;
};

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

// one section's wave: the getter (stream positions count from the 16-byte boundary in front of the stream's first byte) and the sink
// (output positions count from 0; ring and flush positions from the 16-byte boundary in front of the destination's first byte)
struct GzWave {
    static constexpr int64_t MASK = GZ_RING - 1;
    unsigned char *s_in, *s_ring;
    const uint32_t *crc_tab;
    const uint8_t *srcb;
    uint8_t *dstb;
    int64_t src0, src_end, dst0;
    int64_t win_base, win_end, flushed;
    int64_t crc_done;                // the member's output up to here is in crc_reg
    uint32_t crc_reg, lane_pow, chunk_pow;
    int lane_;

    // ---- the getter
    __device__ __forceinline__ int lane() const { return lane_; }
    __device__ __forceinline__ int lanes() const { return GZ_THREADS; }
    __device__ __forceinline__ void sync() const { wave_sync(); }
    __device__ __forceinline__ void inc(uint32_t *p) const { atomicAdd(p, 1u); }
    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

    __device__ __forceinline__ void load_window(int64_t pos) {   // [pos & ~15, + GZ_TILE) of the stream into s_in
        win_base = pos & ~(int64_t)15;
        win_end = win_base + GZ_TILE < src_end ? win_base + GZ_TILE : src_end;
        wave_sync();                                             // (the lanes have read what they wanted of the old window)
        for (int i = lane_; i < GZ_TILE / 16; i += GZ_THREADS) {
            const int64_t a = win_base + (int64_t)i * 16;
            if (a < src_end) reinterpret_cast<uint4 *>(s_in)[i] = *reinterpret_cast<const uint4 *>(srcb + (a - src0));
        }
        wave_sync();
    }
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
    // ring bytes of output positions [from, to) -> global memory: the head up to a 16-byte boundary and the tail behind the last one byte
    // by byte, between them 16-byte stores. zero: zeros instead of the ring's bytes.
    __device__ __forceinline__ void store_span(int64_t from, int64_t to, bool zero) {
        const int64_t a0 = dst0 + from, a1 = dst0 + to;
        int64_t head_end = (a0 + 15) & ~(int64_t)15;
        if (head_end > a1) head_end = a1;
        if (a0 + lane_ < head_end) dstb[from + lane_] = zero ? 0 : s_ring[(a0 + lane_) & MASK];
        const int64_t body_end = head_end + ((a1 - head_end) & ~(int64_t)15);
        for (int64_t a = head_end + (int64_t)lane_ * 16; a < body_end; a += GZ_THREADS * 16)
            *reinterpret_cast<uint4 *>(dstb + (a - dst0)) = zero ? make_uint4(0, 0, 0, 0) : *reinterpret_cast<const uint4 *>(s_ring + (a & MASK));
        if (body_end + lane_ < a1) dstb[body_end - dst0 + lane_] = zero ? 0 : s_ring[(body_end + lane_) & MASK];
    }
    // the CRC of ring bytes [crc_done, crc_done + n), n <= GZ_FLUSH, lane i over the `slice` bytes from i * slice on; pw = x^(8 * bytes
    // behind this lane's slice), all = x^(8 n)
    __device__ __forceinline__ void crc_fold(int n, int slice, uint32_t pw, uint32_t all) {
        const int from = lane_ * slice;
        int to = from + slice;
        if (to > n) to = n;
        uint32_t c = 0;
        for (int j = from; j < to; j++) c = gzip::crc_byte(crc_tab, c, s_ring[(dst0 + crc_done + j) & MASK]);
        c = xor_lanes(mulmod(c, pw));
        crc_reg = mulmod(crc_reg, all) ^ c;
        crc_done += n;
    }
    __device__ __forceinline__ void flush_if_due(int64_t produced) {
        if (produced - flushed >= GZ_FLUSH) {
            const int64_t upto = ((dst0 + produced) & ~(int64_t)15) - dst0;
            store_span(flushed, upto, false);
            flushed = upto;
        }
        while (produced - crc_done >= GZ_FLUSH) crc_fold(GZ_FLUSH, GZ_FLUSH / GZ_THREADS, lane_pow, chunk_pow);
    }
    __device__ __forceinline__ uint32_t member_crc(int64_t, int64_t produced) {
        flush_if_due(produced);
        const int n = (int)(produced - crc_done);                // < GZ_FLUSH
        if (n > 0) {
            const int slice = (n + GZ_THREADS - 1) / GZ_THREADS;
            int behind = n - (lane_ + 1) * slice;
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
            for (int i = lane_; i < (int)c; i += GZ_THREADS) s_ring[(dst0 + at + i) & MASK] = s_in[from - win_base + i];
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
            uint32_t j = (uint32_t)lane_;
            if (off < (uint32_t)c) j %= off;                     // byte j reads j mod off behind the step's first source byte
            unsigned char b = 0;
            if (lane_ < c) b = s_ring[(sbase + at + j) & MASK];
            wave_sync();
            if (lane_ < c) s_ring[(dst0 + at + lane_) & MASK] = b;
        } else {
            unsigned char b[PER];
            if (off >= (uint32_t)c) {
#pragma unroll
                for (int k = 0; k < PER; k++) {
                    const int j = lane_ + k * GZ_THREADS;
                    b[k] = j < c ? s_ring[(sbase + at + j) & MASK] : 0;
                }
            } else {
                uint32_t r = (uint32_t)lane_, step = GZ_THREADS;
                if (off <= (uint32_t)GZ_THREADS) { r %= off; step %= off; }   // (r < off and step < off or 64 < off: one wrap a step at most)
#pragma unroll
                for (int k = 0; k < PER; k++) {
                    b[k] = lane_ + k * GZ_THREADS < c ? s_ring[(sbase + at + r) & MASK] : 0;
                    r += step;
                    if (r >= off) r -= off;
                }
            }
            wave_sync();
#pragma unroll
            for (int k = 0; k < PER; k++) {
                const int j = lane_ + k * GZ_THREADS;
                if (j < c) s_ring[(dst0 + at + j) & MASK] = b[k];
            }
        }
        wave_sync();
        flush_if_due(at + n);
    }
};

}  // namespace

__global__ __launch_bounds__(GZ_THREADS) void gzip_sections_kernel(GzArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gz_lds[];
    const SnSection S = A.sec[blockIdx.x];
    const int lane = threadIdx.x;
    // Positions: stream byte k is src0 + k, output byte k is dst0 + k in the ring, where src0 / dst0 = the low four bits of the byte's
    // address, so a position that is a multiple of 16 is a 16-byte boundary of global memory (and, for the output, of the ring).
    GzWave W;
    unsigned char *p = gz_lds;
    W.s_in = p, p += GZ_TILE;
    W.s_ring = p, p += GZ_RING;
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
    W.srcb = A.src + S.src_pos;
    W.dstb = A.dst + S.dst_pos;
    W.src0 = (int64_t)((uintptr_t)W.srcb & 15);
    W.src_end = W.src0 + S.src_bytes;
    W.dst0 = (int64_t)((uintptr_t)W.dstb & 15);
    W.win_base = W.win_end = W.src0;                             // (an empty window in front of the stream: the first read fills it)
    W.flushed = 0;
    W.crc_done = 0;
    W.crc_reg = 0xffffffffu;
    W.lane_pow = xpow8((uint32_t)((GZ_THREADS - 1 - lane) * (GZ_FLUSH / GZ_THREADS)));
    W.chunk_pow = xpow8(GZ_FLUSH);
    W.lane_ = lane;
    wave_sync();

    int sub = gzip::check_sizes(S.src_bytes, S.dst_bytes);
    if (sub == gzip::S_OK && S.src_bytes > 0) sub = uni(gzip::decode_stream(W, W.src0, W.src_end, S.dst_bytes, T, W));
    if (sub == gzip::S_OK) W.store_span(W.flushed, S.dst_bytes, false);
    else if (S.dst_bytes > 0) W.store_span(0, S.dst_bytes, true);   // a failed section reads as zeros: no decoder meets garbage in it

    // ---- the Parquet load's page on this section
    int cause = sub == gzip::S_OK ? pq::C_OK : pq::C_GZIP;
    uint32_t n_levels = 0;
    if (cause == pq::C_OK && S.v1_levels && S.desc >= 0) {       // (dst_bytes >= 4: resolve_column)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
        const uint8_t *q = W.dstb;
        n_levels = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
        if (lane == 0) {
            pq::PageDesc d = A.pages[S.desc];
            cause = pq::complete_v1_levels(d, d.lvl_pos, S.dst_bytes, n_levels);
            if (cause == pq::C_OK) A.pages[S.desc] = d;
        }
        cause = uni(cause);
    }
    if (lane == 0) {
        if (A.status) A.status[blockIdx.x] = sub;
        if (cause != pq::C_OK) {
            if (A.err && S.key >= 0) atomicMin(A.err, ((unsigned long long)(unsigned)S.key << 8) | (unsigned)cause);
            if (A.pages && S.desc >= 0) {                        // nothing is left of the page for the decoders: no values, no levels, no bytes
                pq::PageDesc &d = A.pages[S.desc];
                d.num_values = 0;
                d.val_bytes = 0;
                d.lvl_bytes = -1;
                d.dict_n = -1;
                d.dict_bytes = (int32_t)n_levels;                // (for the message of C_LVL_SECTION)
            }
        }
    }
}

int gzip_decompress_sections(ph_ctx *ctx, const uint8_t *src, uint8_t *dst, const SnSection *sections_dev, int32_t n, pq::PageDesc *pages_dev,
                             unsigned long long *err, int32_t *status_dev) {
    if (n <= 0) return PH_OK;
    PH_CHECK(raise_lds<gzip_sections_kernel>(ctx, GZ_LDS));
    gzip_sections_kernel<<<(unsigned)n, GZ_THREADS, GZ_LDS, ctx->stream>>>(GzArgs{src, dst, sections_dev, pages_dev, err, status_dev});
    PH_HIP(hipGetLastError());
    return PH_OK;
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
    PH_REQUIRE(ctx && n >= 0 && (n == 0 || (src_dev && dst_dev && src_pos && src_bytes && dst_pos && dst_bytes && status)), "ph_gzip_decompress: bad arguments");
    if (n == 0) return PH_OK;
    std::vector<ph::SnSection> secs((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        PH_REQUIRE(src_pos[i] >= 0 && src_bytes[i] >= 0 && dst_pos[i] >= 0 && dst_bytes[i] >= 0, "ph_gzip_decompress: stream %d: a negative position or length", i);
        secs[(size_t)i] = ph::SnSection{src_pos[i], src_bytes[i], dst_pos[i], dst_bytes[i], -1, -1, 0, 0};
    }
    PH_HIP(hipSetDevice(ctx->device));
    ph::Temps tmp;
    tmp.who = "ph_gzip_decompress";
    ph::SnSection *secs_dev = nullptr;
    int32_t *status_dev = nullptr;
    PH_CHECK(tmp.alloc((void **)&secs_dev, (int64_t)n * (int64_t)sizeof(ph::SnSection)));
    PH_CHECK(tmp.alloc((void **)&status_dev, (int64_t)n * 4));
    PH_CHECK(ph_dev_upload(ctx, secs_dev, secs.data(), (int64_t)n * (int64_t)sizeof(ph::SnSection)));
    PH_CHECK(ph::gzip_decompress_sections(ctx, (const uint8_t *)src_dev, (uint8_t *)dst_dev, secs_dev, n, nullptr, nullptr, status_dev));
    PH_CHECK(ctx->download(status, status_dev, (int64_t)n * 4));
    for (int32_t i = 0; i < n; i++) status[i] = status[i] == ph::gzip::S_OK ? PH_OK : PH_EINVAL;
    return PH_OK;
}
