// What the section kernels (snappy_decompress.hip, lz4_decompress.hip, gzip_decompress.hip, zstd_decompress.hip) share: n independent compressed sections in one
// launch, ONE WAVE a section. A codec's wave derives from SectionWave and adds the chain that is its own; the frame is
//   open        — the positions of the section's stream and destination, an empty input window;
//   load_window — the compressed input staged through LDS in TILE-byte windows, 16-byte loads;
//   the ring    — output byte a lives at s_ring[a mod RING] (a counts from its destination's 16-byte boundary, so 16-byte units of the ring
//                 are 16-byte units of global memory);
//   flush_if_due / store_span — completed ring bytes go to global memory with 16-byte stores whenever FLUSH of them are waiting;
//   close       — the rest of the output (a failed section reads as zeros), and the Parquet load's page on this section.
// The serial chain's state is wave-uniform (uni) and lives in scalar registers. One wave's LDS instructions execute in order, so a ds_write is
// seen by a later ds_read of another lane; wave_sync() (a wavefront-scope fence around a wave barrier, no instruction) keeps the compiler
// from reordering them. Nothing of the frame needs global memory to be coherent between lanes.
// Ring size: a step that copies inside the ring reads ALL its source bytes into registers, then writes. Source byte j of a step at output
// position p is p - offset + (j mod offset), which lies in front of p whatever the overlap, and the slot that the step's byte j takes is the
// slot of position p + j - RING, which no source of a later step is while offset <= RING (and which this step has read already if it is one
// of its own). So a ring of exactly the format's longest reach serves every offset from LDS, with no fence and no global reload.
// Bounds: a decoder checks a step against the stream's end and the expected length BEFORE a byte moves; the window is loaded in whole
// aligned 16-byte units that hold at least one byte of the stream (an aligned unit never leaves its page); stores go to [dst, dst + expected)
// only, the unaligned head and tail byte by byte.
// Below the frame: the launch of a section kernel and the raw entry point over caller-given streams, once for the three codecs.
#pragma once
#include <vector>

#include "common.h"
#include "parquet_decode.h"
#include "str_encode.h"

namespace ph {

struct SnSection {
    int64_t src_pos, src_bytes;     // the stream (a Snappy stream's preamble included), relative to the launch's source base
    int64_t dst_pos, dst_bytes;     // where its output goes, relative to the destination base; what it must produce
    int32_t key;                    // Parquet: the page's index in the call's page list, the error key (-1: none)
    int32_t desc;                   // Parquet: the PageDesc that lives on this section (emptied when the section fails), -1: none
    int32_t v1_levels;              // Parquet: 1 = complete the PageDesc's level and value ranges from the decompressed bytes
    int32_t pad;
};

struct SectionArgs {
    const uint8_t *src;
    uint8_t *dst;
    const SnSection *sec;
    pq::PageDesc *pages;            // the Parquet load's page list and error word (lowest page << 8 | cause); both may be null
    unsigned long long *err;
    int32_t *status;                // status[i] = the codec's Sub of section i (may be null)
};

constexpr int SUB_OK = 0;           // every codec's S_OK
static_assert((int)snappy::S_OK == SUB_OK && (int)lz4::S_OK == SUB_OK && (int)gzip::S_OK == SUB_OK && (int)zstd::S_OK == SUB_OK, "one OK for every codec's sub-cases");

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t uni64(int64_t v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// One section's wave. Stream positions count from the 16-byte boundary in front of the stream's first byte: stream byte k is src0 + k.
// Output positions count from 0; ring and flush positions from the 16-byte boundary in front of the destination's first byte: output byte k
// is dst0 + k in the ring. src0 / dst0 = the low four bits of the byte's address, so a position that is a multiple of 16 is a 16-byte
// boundary of global memory (and, for the output, of the ring).
template <int THREADS, int TILE, int RING>
struct SectionWave {
    static constexpr int64_t MASK = RING - 1;
    unsigned char *s_in, *s_ring;    // LDS: the window (TILE bytes), the ring (RING bytes) behind it
    const uint8_t *srcb;
    uint8_t *dstb;
    int64_t src0, src_end, dst0;
    int64_t win_base, win_end, flushed;
    int lane;

    __device__ __forceinline__ void open(unsigned char *lds, const SectionArgs &A, const SnSection &S) {
        s_in = lds;
        s_ring = lds + TILE;
        srcb = A.src + S.src_pos;
        dstb = A.dst + S.dst_pos;
        src0 = (int64_t)((uintptr_t)srcb & 15);
        src_end = src0 + S.src_bytes;
        dst0 = (int64_t)((uintptr_t)dstb & 15);
        win_base = win_end = src0;                               // (an empty window in front of the stream: the first read fills it)
        flushed = 0;
        lane = threadIdx.x;
    }
    __device__ __forceinline__ void load_window(int64_t pos) {   // [pos & ~15, + TILE) of the stream into s_in
        win_base = pos & ~(int64_t)15;
        win_end = win_base + TILE < src_end ? win_base + TILE : src_end;
        wave_sync();                                             // (the lanes have read what they wanted of the old window)
        for (int i = lane; i < TILE / 16; i += THREADS) {
            const int64_t a = win_base + (int64_t)i * 16;
            if (a < src_end) reinterpret_cast<uint4 *>(s_in)[i] = *reinterpret_cast<const uint4 *>(srcb + (a - src0));
        }
        wave_sync();
    }
    // ring bytes of output positions [from, to) -> global memory: the head up to a 16-byte boundary and the tail behind the last one byte
    // by byte, between them 16-byte stores. zero: zeros instead of the ring's bytes.
    __device__ __forceinline__ void store_span(int64_t from, int64_t to, bool zero) {
        const int64_t a0 = dst0 + from, a1 = dst0 + to;
        int64_t head_end = (a0 + 15) & ~(int64_t)15;
        if (head_end > a1) head_end = a1;
        if (a0 + lane < head_end) dstb[from + lane] = zero ? 0 : s_ring[(a0 + lane) & MASK];
        const int64_t body_end = head_end + ((a1 - head_end) & ~(int64_t)15);
        for (int64_t a = head_end + (int64_t)lane * 16; a < body_end; a += THREADS * 16)
            *reinterpret_cast<uint4 *>(dstb + (a - dst0)) = zero ? make_uint4(0, 0, 0, 0) : *reinterpret_cast<const uint4 *>(s_ring + (a & MASK));
        if (body_end + lane < a1) dstb[body_end - dst0 + lane] = zero ? 0 : s_ring[(body_end + lane) & MASK];
    }
    // the whole 16-byte units of [flushed, produced) go out once flush_bytes (a codec's FLUSH constant) wait
    __device__ __forceinline__ void flush_if_due(int64_t produced, int flush_bytes) {
        if (produced - flushed >= flush_bytes) {
            const int64_t upto = ((dst0 + produced) & ~(int64_t)15) - dst0;
            store_span(flushed, upto, false);
            flushed = upto;
        }
    }
    // The section's end. sub = the decoder's verdict (wave-uniform); a good section has produced S.dst_bytes bytes, of which the ring still
    // holds [flushed, dst_bytes). Then the Parquet load's page on this section: fail_cause = the pq::Cause of this codec's corrupt stream.
    __device__ __forceinline__ void close(const SectionArgs &A, const SnSection &S, int sub, int fail_cause) {
        if (sub == SUB_OK) store_span(flushed, S.dst_bytes, false);
        else if (S.dst_bytes > 0) store_span(0, S.dst_bytes, true);   // a failed section reads as zeros: no decoder meets garbage in it

        int cause = sub == SUB_OK ? pq::C_OK : fail_cause;
        uint32_t n_levels = 0;
        if (cause == pq::C_OK && S.v1_levels && S.desc >= 0) {   // (dst_bytes >= 4: resolve_column)
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");   // (the level-section length is among the bytes the lanes have just stored)
            const uint8_t *q = dstb;
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
                if (A.pages && S.desc >= 0) {                    // nothing is left of the page for the decoders: no values, no levels, no bytes
                    pq::PageDesc &d = A.pages[S.desc];
                    d.num_values = 0;
                    d.val_bytes = 0;
                    d.lvl_bytes = -1;
                    d.dict_n = -1;
                    d.dict_bytes = (int32_t)n_levels;            // (for the message of C_LVL_SECTION)
                }
            }
        }
    }
};

// Decompresses sections_dev[0, n) on the context's stream (asynchronously) with Kernel, one wave of THREADS lanes and LDS bytes of dynamic
// LDS a section. status_dev[i] = the codec's Sub of section i. err / pages_dev (both may be null): the Parquet load's error word and page list.
template <auto Kernel, int THREADS, int LDS>
int launch_sections(ph_ctx *ctx, const uint8_t *src, uint8_t *dst, const SnSection *sections_dev, int32_t n, pq::PageDesc *pages_dev, unsigned long long *err,
                    int32_t *status_dev) {
    if (n <= 0) return PH_OK;
    PH_CHECK(raise_lds<Kernel>(ctx, LDS));
    Kernel<<<(unsigned)n, THREADS, LDS, ctx->stream>>>(SectionArgs{src, dst, sections_dev, pages_dev, err, status_dev});
    PH_HIP(hipGetLastError());
    return PH_OK;
}

using SectionLaunch = int (*)(ph_ctx *ctx, const uint8_t *src, uint8_t *dst, const SnSection *sections_dev, int32_t n, pq::PageDesc *pages_dev,
                              unsigned long long *err, int32_t *status_dev);

// ph_snappy_decompress / ph_lz4_decompress / ph_gzip_decompress / ph_zstd_decompress (planhip.h): n caller-given streams through `launch`, status[i] = PH_OK or PH_EINVAL
inline int decompress_streams(ph_ctx *ctx, const char *who, SectionLaunch launch, const void *src_dev, const int64_t *src_pos, const int64_t *src_bytes,
                              void *dst_dev, const int64_t *dst_pos, const int64_t *dst_bytes, int32_t n, int32_t *status) {
    PH_REQUIRE(ctx && n >= 0 && (n == 0 || (src_dev && dst_dev && src_pos && src_bytes && dst_pos && dst_bytes && status)), "%s: bad arguments", who);
    if (n == 0) return PH_OK;
    std::vector<SnSection> secs((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        PH_REQUIRE(src_pos[i] >= 0 && src_bytes[i] >= 0 && dst_pos[i] >= 0 && dst_bytes[i] >= 0, "%s: stream %d: a negative position or length", who, i);
        secs[(size_t)i] = SnSection{src_pos[i], src_bytes[i], dst_pos[i], dst_bytes[i], -1, -1, 0, 0};
    }
    PH_HIP(hipSetDevice(ctx->device));
    Temps tmp;
    tmp.who = who;
    SnSection *secs_dev = nullptr;
    int32_t *status_dev = nullptr;
    PH_CHECK(tmp.alloc((void **)&secs_dev, (int64_t)n * (int64_t)sizeof(SnSection)));
    PH_CHECK(tmp.alloc((void **)&status_dev, (int64_t)n * 4));
    PH_CHECK(ph_dev_upload(ctx, secs_dev, secs.data(), (int64_t)n * (int64_t)sizeof(SnSection)));
    PH_CHECK(launch(ctx, (const uint8_t *)src_dev, (uint8_t *)dst_dev, secs_dev, n, nullptr, nullptr, status_dev));
    PH_CHECK(ctx->download(status, status_dev, (int64_t)n * 4));
    for (int32_t i = 0; i < n; i++) status[i] = status[i] == SUB_OK ? PH_OK : PH_EINVAL;
    return PH_OK;
}

}  // namespace ph
