// LZ4 blocks (Parquet's LZ4_RAW) decompressed on the device: one launch over n independent sections, ONE WAVE a section, on section_wave.h's
// frame (window, ring, flush, the section's end), and the two raw-block entry points ph_lz4_decompress / ph_lz4_decompress_host.
//
// The sequence chain of a block is serial and a match reads what the same block has just written, so the parallelism is across sections and,
// inside a sequence, across its bytes. The wave IS the getter and the sink that lz4_decode.h's decode_block is instantiated over:
//   - u8(p) and ff_run(p) refill the window whenever p lies behind it, so a sequence header may straddle a window edge anywhere: the token
//     as a window's last byte, an extension run across an edge or across whole windows, the two offset bytes on either side. u8(p) keeps
//     the 64 stream bytes from the last miss on in one register, a byte a lane, and answers from it with a lane read: a header and the
//     short sequences behind it cost one LDS round trip together, and a literal run that lies inside those bytes is written to the ring by
//     the lanes that hold it. An extension run is consumed up to 64 bytes at a time: one byte a lane and a ballot over "byte != 255";
//   - a literal run is copied from the window, a match inside the ring, both LZ_CHUNK bytes a step (one byte a lane for the short ones). A
//     match step reads all its source bytes, then writes (section_wave.h, ring size): offset <= 65535, so a ring of exactly 2^16 bytes
//     serves every offset the format can state: 72 KiB of LDS with the window, two sections resident per CU of 160 KiB (a ring of 2^17
//     bytes that needs no read-before-write would leave one);
//   - never more than LZ_FLUSH + LZ_CHUNK completed bytes wait in the ring, far below what it keeps.
#include "lz4_decode.h"
#include "lz4_decompress.h"

namespace ph {

namespace {

struct LzWave : SectionWave<LZ_THREADS, LZ_TILE, LZ_RING> {
    int64_t look_pos, look_end;      // the stream positions whose bytes the lanes hold in `look`: lane i has byte look_pos + i
    uint32_t look;

    // ---- the getter (decode_block asks for positions inside [src0, src_end) only, front to back)
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

    // ---- the sink
    __device__ __forceinline__ void literal(LzWave &, int64_t from, int64_t at, int64_t n) {   // (the run lies inside the stream: decode_block)
        if (from >= look_pos && from + n <= look_end) {          // the common case: the lanes hold the run's bytes already
            const int64_t k = look_pos + lane - from;
            if (k >= 0 && k < n) s_ring[(dst0 + at + k) & MASK] = (unsigned char)look;
            wave_sync();
            flush_if_due(at + n, LZ_FLUSH);
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
            flush_if_due(at, LZ_FLUSH);
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
            flush_if_due(at + c, LZ_FLUSH);
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
            flush_if_due(at, LZ_FLUSH);
        }
    }
};

}  // namespace

__global__ __launch_bounds__(LZ_THREADS) void lz4_sections_kernel(SectionArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lz_lds[];
    const SnSection S = A.sec[blockIdx.x];
    LzWave W;
    W.open(lz_lds, A, S);
    W.look_pos = W.look_end = W.src0;
    W.look = 0;

    int sub = lz4::check_sizes(S.src_bytes, S.dst_bytes);
    if (sub == lz4::S_OK && S.src_bytes > 0) sub = uni(lz4::decode_block(W, W.src0, W.src_end, S.dst_bytes, W));
    W.close(A, S, sub, pq::C_LZ4);
}

int lz4_decompress_sections(ph_ctx *ctx, const uint8_t *src, uint8_t *dst, const SnSection *sections_dev, int32_t n, pq::PageDesc *pages_dev,
                            unsigned long long *err, int32_t *status_dev) {
    return launch_sections<lz4_sections_kernel, LZ_THREADS, LZ_TILE + LZ_RING>(ctx, src, dst, sections_dev, n, pages_dev, err, status_dev);
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
    return ph::decompress_streams(ctx, "ph_lz4_decompress", ph::lz4_decompress_sections, src_dev, src_pos, src_bytes, dst_dev, dst_pos, dst_bytes, n, status);
}
