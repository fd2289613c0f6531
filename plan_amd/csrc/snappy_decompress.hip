// Snappy streams decompressed on the device: one launch over n independent sections, ONE WAVE a section (snappy_decompress.h), and the two
// raw-stream entry points ph_snappy_decompress / ph_snappy_decompress_host.
//
// The element chain of a stream is sequential and a copy reads what the same stream has just written, so the work inside a section is
// serial by nature; the parallelism is across sections (a file has thousands of pages) and, inside an element, across its bytes. The wave
//   - stages the compressed input through LDS in SN_TILE-byte windows, 16-byte loads (a window begins at the 16-byte unit that holds the
//     next unread byte and is refilled when fewer than 5 bytes — the longest tag with its operands — are left in it);
//   - parses each element with snappy_decode.h's parse_element, every lane the same bytes (an LDS broadcast), and makes the result
//     wave-uniform with readfirstlane, so the chain's state lives in scalar registers;
//   - carries the element out inside LDS: output byte a lives at s_ring[a mod SN_RING] (a counts from its destination's 16-byte
//     boundary, so 16-byte units of the ring are 16-byte units of global memory). A literal is copied from the window, 64 bytes a step; a copy of up to 64 bytes is ONE step even
//     when it overlaps itself: byte i reads produced - offset + (i mod offset), which was written by an earlier element;
//   - flushes completed ring bytes to global memory with 16-byte stores whenever SN_FLUSH of them are waiting.
// One wave's LDS instructions execute in order, so a ds_write is seen by a later ds_read of another lane; wave_sync() (a wavefront-scope
// fence around a wave barrier, no instruction) keeps the compiler from reordering them. Nothing of this needs global memory to be
// coherent between lanes, EXCEPT a copy whose offset reaches behind the ring (the format allows 32-bit offsets, compressors stay below
// 64 KiB): the wave then flushes everything it has produced, drains and invalidates with an agent-scope fence, and reads the bytes back
// from global memory. That path is correct and slow, and no standard compressor takes it.
// Bounds: parse_element checks an element against the stream's end and the expected length BEFORE a byte moves; the window is loaded in
// whole aligned 16-byte units that hold at least one byte of the stream (an aligned unit never leaves its page); stores go to
// [dst, dst + expected) only, the unaligned head and tail byte by byte.
#include <vector>

#include "snappy_decompress.h"
#include "str_encode.h"

namespace ph {

namespace {

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

// the input window: positions are addresses
struct LdsStream {
    const unsigned char *t;
    int64_t base;
    __device__ __forceinline__ uint8_t u8(int64_t p) const { return t[p - base]; }
};

struct SnArgs {
    const uint8_t *src;
    uint8_t *dst;
    const SnSection *sec;
    pq::PageDesc *pages;
    unsigned long long *err;
    int32_t *status;
};

}  // namespace

__global__ __launch_bounds__(SN_THREADS) void snappy_sections_kernel(SnArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sn_lds[];
    unsigned char *const s_in = sn_lds, *const s_ring = sn_lds + SN_TILE;
    constexpr int64_t MASK = SN_RING - 1;
    const SnSection S = A.sec[blockIdx.x];
    const int lane = threadIdx.x;
    // Positions: stream byte k is src0 + k, output byte k is dst0 + k, where src0 / dst0 = the low four bits of the byte's address, so
    // a position that is a multiple of 16 is a 16-byte boundary of global memory (and, for the output, of the ring).
    const uint8_t *const srcb = A.src + S.src_pos;
    uint8_t *const dstb = A.dst + S.dst_pos;
    const int64_t src0 = (int64_t)((uintptr_t)srcb & 15), src_end = src0 + S.src_bytes;
    const int64_t dst0 = (int64_t)((uintptr_t)dstb & 15);
    int64_t win_base = 0, win_end = 0;

    auto load_window = [&](int64_t pos) {      // [pos & ~15, + SN_TILE) of the stream into s_in
        win_base = pos & ~(int64_t)15;
        win_end = win_base + SN_TILE < src_end ? win_base + SN_TILE : src_end;
        wave_sync();                           // (the lanes have read what they wanted of the old window)
        for (int i = lane; i < SN_TILE / 16; i += SN_THREADS) {
            const int64_t a = win_base + (int64_t)i * 16;
            if (a < src_end) reinterpret_cast<uint4 *>(s_in)[i] = *reinterpret_cast<const uint4 *>(srcb + (a - src0));
        }
        wave_sync();
    };
    // ring bytes of output positions [from, to) -> global memory: the head up to a 16-byte boundary and the tail behind the last one byte
    // by byte, between them 16-byte stores. ZERO: zeros instead of the ring's bytes.
    auto store_span = [&](int64_t from, int64_t to, bool zero) {
        const int64_t a0 = dst0 + from, a1 = dst0 + to;
        int64_t head_end = (a0 + 15) & ~(int64_t)15;
        if (head_end > a1) head_end = a1;
        if (a0 + lane < head_end) dstb[from + lane] = zero ? 0 : s_ring[(a0 + lane) & MASK];
        const int64_t body_end = head_end + ((a1 - head_end) & ~(int64_t)15);
        for (int64_t a = head_end + (int64_t)lane * 16; a < body_end; a += SN_THREADS * 16)
            *reinterpret_cast<uint4 *>(dstb + (a - dst0)) = zero ? make_uint4(0, 0, 0, 0) : *reinterpret_cast<const uint4 *>(s_ring + (a & MASK));
        if (body_end + lane < a1) dstb[body_end - dst0 + lane] = zero ? 0 : s_ring[(body_end + lane) & MASK];
    };

    int sub = snappy::S_OK;
    int64_t expected = 0, pos = 0, produced = 0, flushed = 0;
    if (S.src_bytes <= 0) sub = snappy::S_PREAMBLE;
    else {
        load_window(src0);
        const LdsStream g{s_in, win_base};
        int64_t n = 0, body = 0;
        sub = uni(snappy::read_preamble(g, src0, src_end, S.dst_bytes, &n, &body));
        expected = S.dst_bytes;
        pos = uni64(body);
    }
    while (sub == snappy::S_OK && produced < expected) {     // (every element consumes at least one byte of [pos, src_end))
        if (pos >= src_end) { sub = snappy::S_INPUT_SHORT; break; }
        if (pos + 5 > win_end && win_end < src_end) load_window(pos);
        snappy::Element e;
        const int s = uni(snappy::parse_element(LdsStream{s_in, win_base}, pos, src_end, produced, expected, &e));
        if (s != snappy::S_OK) { sub = s; break; }
        const int64_t len = uni64(e.len), data = uni64(e.data);
        if (uni(e.copy)) {
            const int64_t off = uni64(e.offset);
            const int L = (int)len;                          // 1..64
            const int64_t from = produced - off + (off >= L ? lane : lane % (int)off);
            unsigned char b = 0;
            if (off <= SN_RING - 64) {
                if (lane < L) b = s_ring[(dst0 + from) & MASK];
            } else {                                         // behind the ring: through global memory, behind a drain and an invalidate
                store_span(flushed, produced, false);
                flushed = produced;
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
                if (lane < L) b = dstb[from];
            }
            if (lane < L) s_ring[(dst0 + produced + lane) & MASK] = b;
            wave_sync();
            pos = data;
            produced += L;
        } else {
            int64_t left = len, p = data;
            while (left > 0) {                               // (the literal lies inside the stream: parse_element)
                if (p >= win_end) load_window(p);
                int64_t c = win_end - p;
                if (c > left) c = left;
                if (c > SN_CHUNK) c = SN_CHUNK;
                for (int i = lane; i < (int)c; i += SN_THREADS) s_ring[(dst0 + produced + i) & MASK] = s_in[p - win_base + i];
                wave_sync();
                p += c;
                produced += c;
                left -= c;
                if (produced - flushed >= SN_FLUSH) {
                    const int64_t upto = ((dst0 + produced) & ~(int64_t)15) - dst0;
                    store_span(flushed, upto, false);
                    flushed = upto;
                }
            }
            pos = p;
        }
        if (produced - flushed >= SN_FLUSH) {
            const int64_t upto = ((dst0 + produced) & ~(int64_t)15) - dst0;
            store_span(flushed, upto, false);
            flushed = upto;
        }
    }
    if (sub == snappy::S_OK && pos != src_end) sub = snappy::S_INPUT_LEFT;
    if (sub == snappy::S_OK) store_span(flushed, produced, false);
    else if (S.dst_bytes > 0) store_span(0, S.dst_bytes, true);   // a failed section reads as zeros: no decoder meets garbage in it

    // ---- the Parquet load's page on this section
    int cause = sub == snappy::S_OK ? pq::C_OK : pq::C_SNAPPY;
    uint32_t n_levels = 0;
    if (cause == pq::C_OK && S.v1_levels && S.desc >= 0) {   // (dst_bytes >= 4: resolve_column)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
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

int snappy_decompress_sections(ph_ctx *ctx, const uint8_t *src, uint8_t *dst, const SnSection *sections_dev, int32_t n, pq::PageDesc *pages_dev,
                               unsigned long long *err, int32_t *status_dev) {
    if (n <= 0) return PH_OK;
    constexpr int lds = SN_TILE + SN_RING;
    PH_CHECK(raise_lds<snappy_sections_kernel>(ctx, lds));
    snappy_sections_kernel<<<(unsigned)n, SN_THREADS, lds, ctx->stream>>>(SnArgs{src, dst, sections_dev, pages_dev, err, status_dev});
    PH_HIP(hipGetLastError());
    return PH_OK;
}

}  // namespace ph

extern "C" int ph_snappy_decompress_host(const void *src, int64_t src_bytes, void *dst, int64_t dst_cap, int64_t *dst_bytes) {
    PH_REQUIRE(src_bytes >= 0 && (src || src_bytes == 0) && dst_cap >= 0 && (dst || dst_cap == 0), "ph_snappy_decompress_host: bad arguments");
    int64_t n = 0;
    int sub = ph::snappy::decompress_host((const uint8_t *)src, src_bytes, nullptr, -1, &n, false);
    if (dst_bytes) *dst_bytes = sub == ph::snappy::S_OK || sub == ph::snappy::S_IMPOSSIBLE ? n : 0;
    if (sub == ph::snappy::S_OK && dst) {
        if (n > dst_cap) {
            ph::set_error("ph_snappy_decompress_host: the stream holds %lld bytes, the buffer %lld", (long long)n, (long long)dst_cap);
            return PH_ECAPACITY;
        }
        sub = ph::snappy::decompress_host((const uint8_t *)src, src_bytes, (uint8_t *)dst, n, nullptr);
    }
    PH_REQUIRE(sub == ph::snappy::S_OK, "ph_snappy_decompress_host: a corrupt Snappy stream of %lld bytes: %s", (long long)src_bytes, ph::snappy::sub_text(sub));
    return PH_OK;
}

extern "C" int ph_snappy_decompress(ph_ctx *ctx, const void *src_dev, const int64_t *src_pos, const int64_t *src_bytes, void *dst_dev,
                                    const int64_t *dst_pos, const int64_t *dst_bytes, int32_t n, int32_t *status) {
    PH_REQUIRE(ctx && n >= 0 && (n == 0 || (src_dev && dst_dev && src_pos && src_bytes && dst_pos && dst_bytes && status)), "ph_snappy_decompress: bad arguments");
    if (n == 0) return PH_OK;
    std::vector<ph::SnSection> secs((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        PH_REQUIRE(src_pos[i] >= 0 && src_bytes[i] >= 0 && dst_pos[i] >= 0 && dst_bytes[i] >= 0, "ph_snappy_decompress: stream %d: a negative position or length", i);
        secs[(size_t)i] = ph::SnSection{src_pos[i], src_bytes[i], dst_pos[i], dst_bytes[i], -1, -1, 0, 0};
    }
    PH_HIP(hipSetDevice(ctx->device));
    ph::Temps tmp;
    tmp.who = "ph_snappy_decompress";
    ph::SnSection *secs_dev = nullptr;
    int32_t *status_dev = nullptr;
    PH_CHECK(tmp.alloc((void **)&secs_dev, (int64_t)n * (int64_t)sizeof(ph::SnSection)));
    PH_CHECK(tmp.alloc((void **)&status_dev, (int64_t)n * 4));
    PH_CHECK(ph_dev_upload(ctx, secs_dev, secs.data(), (int64_t)n * (int64_t)sizeof(ph::SnSection)));
    PH_CHECK(ph::snappy_decompress_sections(ctx, (const uint8_t *)src_dev, (uint8_t *)dst_dev, secs_dev, n, nullptr, nullptr, status_dev));
    PH_CHECK(ctx->download(status, status_dev, (int64_t)n * 4));
    for (int32_t i = 0; i < n; i++) status[i] = status[i] == ph::snappy::S_OK ? PH_OK : PH_EINVAL;
    return PH_OK;
}
