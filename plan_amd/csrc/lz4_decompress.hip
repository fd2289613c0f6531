// LZ4 blocks (Parquet's LZ4_RAW) decompressed on the device: one launch over n independent sections, ONE WAVE a section (lz4_decompress.h),
// and the two raw-block entry points ph_lz4_decompress / ph_lz4_decompress_host.
//
// The sequence chain of a block is serial and a match reads what the same block has just written, so the parallelism is across sections and,
// inside a sequence, across its bytes. The wave IS the getter and the sink that lz4_decode.h's decode_block is instantiated over:
//   - the compressed input is staged through LDS in LZ_TILE-byte windows, 16-byte loads. u8(p) and ff_run(p) refill the window whenever p
//     lies behind it, so a sequence header may straddle a window edge anywhere: the token as a window's last byte, an extension run across an
//     edge or across whole windows, the two offset bytes on either side. u8(p) keeps the 64 stream bytes from the last miss on in one
//     register, a byte a lane, and answers from it with a lane read: a header and the short sequences behind it cost one LDS round trip
//     together, and a literal run that lies inside those bytes is written to the ring by the lanes that hold it. The chain's state lives
//     in scalar registers. An extension run is consumed up to 64 bytes at a time: one byte a lane and a ballot over "byte != 255";
//   - output byte a lives at s_ring[a mod LZ_RING] (a counts from its destination's 16-byte boundary, so 16-byte units of the ring are
//     16-byte units of global memory). A literal run is copied from the window, a match inside the ring, both LZ_CHUNK bytes a step (one
//     byte a lane for the short ones). A match step reads ALL its source bytes into registers, then writes: source byte j of a step at
//     output position p is p - offset + (j mod offset), which lies in front of p whatever the overlap, and the slot that the step's byte j
//     takes is the slot of position p + j - 65536, which no source of this or a later step is (offset <= 65535). So every offset the format
//     can state is served from LDS, with no fence and no global reload, by a ring of exactly 2^16 bytes: 72 KiB of LDS with the window, two
//     sections resident per CU of 160 KiB (a ring of 2^17 bytes that needs no read-before-write would leave one);
//   - completed ring bytes are flushed to global memory with 16-byte stores whenever LZ_FLUSH of them are waiting (never more than
//     LZ_FLUSH + LZ_CHUNK are, far below what the ring keeps).
// One wave's LDS instructions execute in order; wave_sync() (a wavefront-scope fence around a wave barrier, no instruction) keeps the compiler
// from reordering them.
// Bounds: decode_block checks a sequence against the stream's end and the expected length BEFORE a byte moves; the window is loaded in whole
// aligned 16-byte units that hold at least one byte of the stream (an aligned unit never leaves its page); stores go to [dst, dst + expected)
// only, the unaligned head and tail byte by byte.
#include <vector>

#include "lz4_decode.h"
#include "lz4_decompress.h"
#include "str_encode.h"

namespace ph {

namespace {

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

struct LzArgs {
    const uint8_t *src;
    uint8_t *dst;
    const SnSection *sec;
    pq::PageDesc *pages;
    unsigned long long *err;
    int32_t *status;
};

// one section's wave: the byte getter (stream positions count from the 16-byte boundary in front of the stream's first byte) and the sink
// (output positions count from 0; ring and flush positions from the 16-byte boundary in front of the destination's first byte)
struct LzWave {
    static constexpr int64_t MASK = LZ_RING - 1;
    unsigned char *s_in, *s_ring;
    const uint8_t *srcb;
    uint8_t *dstb;
    int64_t src0, src_end, dst0;
    int64_t win_base, win_end, flushed;
    int64_t look_pos, look_end;      // the stream positions whose bytes the lanes hold in `look`: lane i has byte look_pos + i
    uint32_t look;
    int lane;

    __device__ __forceinline__ void load_window(int64_t pos) {   // [pos & ~15, + LZ_TILE) of the stream into s_in
        win_base = pos & ~(int64_t)15;
        win_end = win_base + LZ_TILE < src_end ? win_base + LZ_TILE : src_end;
        wave_sync();                                             // (the lanes have read what they wanted of the old window)
        for (int i = lane; i < LZ_TILE / 16; i += LZ_THREADS) {
            const int64_t a = win_base + (int64_t)i * 16;
            if (a < src_end) reinterpret_cast<uint4 *>(s_in)[i] = *reinterpret_cast<const uint4 *>(srcb + (a - src0));
        }
        wave_sync();
    }
    // (decode_block asks for positions inside [src0, src_end) only, front to back)
    // One LDS read fetches the 64 bytes from p on, one a lane; the bytes of a header (token, extension bytes, offset) and of the short
    // sequences behind it are then lane reads, no further LDS round trip in the serial chain.
    __device__ __forceinline__ void look_at(int64_t p) {
        if (p >= win_end) load_window(p);
        look_pos = p;
        look_end = p + LZ_THREADS < win_end ? p + LZ_THREADS : win_end;
        look = p + lane < look_end ? s_in[p + lane - win_base] : 0;
    }
    __device__ __forceinline__ uint32_t u8(int64_t p) {
        if (p < look_pos || p >= look_end) look_at(p);
        return (uint32_t)__builtin_amdgcn_readlane((int)look, (int)(p - look_pos));
    }
    __device__ __forceinline__ int64_t ff_run(int64_t pos, int64_t end) {
        if (pos >= win_end) load_window(pos);
        const int64_t lim = win_end < end ? win_end : end;       // (a run that reaches the window's edge goes on in the next call)
        const bool stop = pos + lane >= lim || s_in[pos + lane - win_base] != 0xff;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(stop);
        return m ? (int64_t)__builtin_ctzll(m) : (int64_t)lz4::FF_STEP;
    }
    // ring bytes of output positions [from, to) -> global memory: the head up to a 16-byte boundary and the tail behind the last one byte
    // by byte, between them 16-byte stores. zero: zeros instead of the ring's bytes.
    __device__ __forceinline__ void store_span(int64_t from, int64_t to, bool zero) {
        const int64_t a0 = dst0 + from, a1 = dst0 + to;
        int64_t head_end = (a0 + 15) & ~(int64_t)15;
        if (head_end > a1) head_end = a1;
        if (a0 + lane < head_end) dstb[from + lane] = zero ? 0 : s_ring[(a0 + lane) & MASK];
        const int64_t body_end = head_end + ((a1 - head_end) & ~(int64_t)15);
        for (int64_t a = head_end + (int64_t)lane * 16; a < body_end; a += LZ_THREADS * 16)
            *reinterpret_cast<uint4 *>(dstb + (a - dst0)) = zero ? make_uint4(0, 0, 0, 0) : *reinterpret_cast<const uint4 *>(s_ring + (a & MASK));
        if (body_end + lane < a1) dstb[body_end - dst0 + lane] = zero ? 0 : s_ring[(body_end + lane) & MASK];
    }
    __device__ __forceinline__ void flush_if_due(int64_t produced) {
        if (produced - flushed >= LZ_FLUSH) {
            const int64_t upto = ((dst0 + produced) & ~(int64_t)15) - dst0;
            store_span(flushed, upto, false);
            flushed = upto;
        }
    }
    __device__ __forceinline__ void literal(LzWave &, int64_t from, int64_t at, int64_t n) {   // (the run lies inside the stream: decode_block)
        if (from >= look_pos && from + n <= look_end) {          // the common case: the lanes hold the run's bytes already
            const int64_t k = look_pos + lane - from;
            if (k >= 0 && k < n) s_ring[(dst0 + at + k) & MASK] = (unsigned char)look;
            wave_sync();
            flush_if_due(at + n);
            return;
        }
        while (n > 0) {
            if (from >= win_end) load_window(from);
            int64_t c = win_end - from;
            if (c > n) c = n;
            if (c > LZ_CHUNK) c = LZ_CHUNK;
            for (int i = lane; i < (int)c; i += LZ_THREADS) s_ring[(dst0 + at + i) & MASK] = s_in[from - win_base + i];
            wave_sync();
            from += c;
            at += c;
            n -= c;
            flush_if_due(at);
        }
    }
    __device__ __forceinline__ void match(int64_t at, int64_t offset, int64_t n) {           // (1 <= offset <= at, offset <= 65535)
        const uint32_t off = (uint32_t)offset;
        const int64_t sbase = dst0 - offset;
        if (n <= LZ_THREADS) {                                   // the common case: one byte a lane, nothing computed that it does not need
            const int c = (int)n;
            uint32_t j = (uint32_t)lane;
            if (off < (uint32_t)c) j %= off;                     // byte j of a step reads j mod off behind the step's first source byte
            unsigned char b = 0;
            if (lane < c) b = s_ring[(sbase + at + j) & MASK];
            wave_sync();
            if (lane < c) s_ring[(dst0 + at + lane) & MASK] = b;
            wave_sync();
            flush_if_due(at + c);
            return;
        }
        match_long(at, off, sbase, n);
    }
    __device__ __forceinline__ void match_long(int64_t at, uint32_t off, int64_t sbase, int64_t n) {
        constexpr int PER = LZ_CHUNK / LZ_THREADS;
        uint32_t r0 = (uint32_t)lane, rstep = LZ_THREADS;
        if (off <= (uint32_t)LZ_THREADS) { r0 %= off; rstep %= off; }
        while (n > 0) {
            const int c = n > LZ_CHUNK ? LZ_CHUNK : (int)n;
            unsigned char b[PER];
            if (off >= (uint32_t)c) {
#pragma unroll
                for (int k = 0; k < PER; k++) {
                    const int j = lane + k * LZ_THREADS;
                    b[k] = j < c ? s_ring[(sbase + at + j) & MASK] : 0;
                }
            } else {
                uint32_t r = r0;
                const uint32_t step = off > (uint32_t)LZ_THREADS ? (uint32_t)LZ_THREADS : rstep;   // (r < off and step < off or 64 < off: one wrap a step at most)
#pragma unroll
                for (int k = 0; k < PER; k++) {
                    b[k] = lane + k * LZ_THREADS < c ? s_ring[(sbase + at + r) & MASK] : 0;
                    r += step;
                    if (r >= off) r -= off;
                }
            }
            wave_sync();
#pragma unroll
            for (int k = 0; k < PER; k++) {
                const int j = lane + k * LZ_THREADS;
                if (j < c) s_ring[(dst0 + at + j) & MASK] = b[k];
            }
            wave_sync();
            at += c;
            n -= c;
            flush_if_due(at);
        }
    }
};

}  // namespace

__global__ __launch_bounds__(LZ_THREADS) void lz4_sections_kernel(LzArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lz_lds[];
    const SnSection S = A.sec[blockIdx.x];
    const int lane = threadIdx.x;
    // Positions: stream byte k is src0 + k, output byte k is dst0 + k in the ring, where src0 / dst0 = the low four bits of the byte's
    // address, so a position that is a multiple of 16 is a 16-byte boundary of global memory (and, for the output, of the ring).
    LzWave W;
    W.s_in = lz_lds;
    W.s_ring = lz_lds + LZ_TILE;
    W.srcb = A.src + S.src_pos;
    W.dstb = A.dst + S.dst_pos;
    W.src0 = (int64_t)((uintptr_t)W.srcb & 15);
    W.src_end = W.src0 + S.src_bytes;
    W.dst0 = (int64_t)((uintptr_t)W.dstb & 15);
    W.win_base = W.win_end = W.src0;                             // (an empty window in front of the stream: the first read fills it)
    W.look_pos = W.look_end = W.src0;
    W.look = 0;
    W.flushed = 0;
    W.lane = lane;

    int sub = lz4::check_sizes(S.src_bytes, S.dst_bytes);
    if (sub == lz4::S_OK && S.src_bytes > 0) sub = uni(lz4::decode_block(W, W.src0, W.src_end, S.dst_bytes, W));
    if (sub == lz4::S_OK) W.store_span(W.flushed, S.dst_bytes, false);
    else if (S.dst_bytes > 0) W.store_span(0, S.dst_bytes, true);   // a failed section reads as zeros: no decoder meets garbage in it

    // ---- the Parquet load's page on this section
    int cause = sub == lz4::S_OK ? pq::C_OK : pq::C_LZ4;
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

int lz4_decompress_sections(ph_ctx *ctx, const uint8_t *src, uint8_t *dst, const SnSection *sections_dev, int32_t n, pq::PageDesc *pages_dev,
                            unsigned long long *err, int32_t *status_dev) {
    if (n <= 0) return PH_OK;
    constexpr int lds = LZ_TILE + LZ_RING;
    PH_CHECK(raise_lds<lz4_sections_kernel>(ctx, lds));
    lz4_sections_kernel<<<(unsigned)n, LZ_THREADS, lds, ctx->stream>>>(LzArgs{src, dst, sections_dev, pages_dev, err, status_dev});
    PH_HIP(hipGetLastError());
    return PH_OK;
}

}  // namespace ph

extern "C" int ph_lz4_decompress_host(const void *src, int64_t src_bytes, void *dst, int64_t expected, int64_t *produced) {
    PH_REQUIRE(src_bytes >= 0 && (src || src_bytes == 0) && expected >= 0 && (dst || expected == 0), "ph_lz4_decompress_host: bad arguments");
    if (produced) *produced = 0;
    const int sub = ph::lz4::decompress_host((const uint8_t *)src, src_bytes, (uint8_t *)dst, expected);
    PH_REQUIRE(sub == ph::lz4::S_OK, "ph_lz4_decompress_host: a corrupt LZ4_RAW stream of %lld bytes for %lld: %s", (long long)src_bytes, (long long)expected,
               ph::lz4::sub_text(sub));
    if (produced) *produced = expected;
    return PH_OK;
}

extern "C" int ph_lz4_decompress(ph_ctx *ctx, const void *src_dev, const int64_t *src_pos, const int64_t *src_bytes, void *dst_dev,
                                 const int64_t *dst_pos, const int64_t *dst_bytes, int32_t n, int32_t *status) {
    PH_REQUIRE(ctx && n >= 0 && (n == 0 || (src_dev && dst_dev && src_pos && src_bytes && dst_pos && dst_bytes && status)), "ph_lz4_decompress: bad arguments");
    if (n == 0) return PH_OK;
    std::vector<ph::SnSection> secs((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        PH_REQUIRE(src_pos[i] >= 0 && src_bytes[i] >= 0 && dst_pos[i] >= 0 && dst_bytes[i] >= 0, "ph_lz4_decompress: stream %d: a negative position or length", i);
        secs[(size_t)i] = ph::SnSection{src_pos[i], src_bytes[i], dst_pos[i], dst_bytes[i], -1, -1, 0, 0};
    }
    PH_HIP(hipSetDevice(ctx->device));
    ph::Temps tmp;
    tmp.who = "ph_lz4_decompress";
    ph::SnSection *secs_dev = nullptr;
    int32_t *status_dev = nullptr;
    PH_CHECK(tmp.alloc((void **)&secs_dev, (int64_t)n * (int64_t)sizeof(ph::SnSection)));
    PH_CHECK(tmp.alloc((void **)&status_dev, (int64_t)n * 4));
    PH_CHECK(ph_dev_upload(ctx, secs_dev, secs.data(), (int64_t)n * (int64_t)sizeof(ph::SnSection)));
    PH_CHECK(ph::lz4_decompress_sections(ctx, (const uint8_t *)src_dev, (uint8_t *)dst_dev, secs_dev, n, nullptr, nullptr, status_dev));
    PH_CHECK(ctx->download(status, status_dev, (int64_t)n * 4));
    for (int32_t i = 0; i < n; i++) status[i] = status[i] == ph::lz4::S_OK ? PH_OK : PH_EINVAL;
    return PH_OK;
}
