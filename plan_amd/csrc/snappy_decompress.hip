// Snappy streams decompressed on the device: one launch over n independent sections, ONE WAVE a section, on section_wave.h's frame (window,
// ring, flush, the section's end), and the two raw-stream entry points ph_snappy_decompress / ph_snappy_decompress_host.
//
// The element chain of a stream is sequential and a copy reads what the same stream has just written, so the work inside a section is
// serial by nature; the parallelism is across sections (a file has thousands of pages) and, inside an element, across its bytes. The wave
//   - refills the window when fewer than 5 bytes — the longest tag with its operands — are left in it;
//   - parses each element with snappy_decode.h's parse_element, every lane the same bytes (an LDS broadcast), and makes the result
//     wave-uniform with readfirstlane, so the chain's state lives in scalar registers;
//   - carries the element out inside the ring. A literal is copied from the window, SN_CHUNK bytes a step; a copy of up to 64 bytes is ONE
//     step even when it overlaps itself: byte i reads produced - offset + (i mod offset), which was written by an earlier element.
// A copy whose offset reaches behind the ring (the format allows 32-bit offsets, compressors stay below 64 KiB) is the one thing that needs
// global memory to be coherent between lanes: the wave then flushes everything it has produced, drains and invalidates with an agent-scope
// fence, and reads the bytes back from global memory. That path is correct and slow, and no standard compressor takes it.
#include "snappy_decompress.h"

namespace ph {

namespace {

// the input window: positions are addresses
struct LdsStream {
    const unsigned char *t;
    int64_t base;
    __device__ __forceinline__ uint8_t u8(int64_t p) const { return t[p - base]; }
};

struct SnWave : SectionWave<SN_THREADS, SN_TILE, SN_RING> {
    __device__ __forceinline__ void copy(int64_t produced, int64_t off, int L) {   // 1 <= L <= 64, 1 <= off <= produced
        const int64_t from = produced - off + (off >= L ? lane : lane % (int)off);
        unsigned char b = 0;
        if (off <= SN_RING - 64) {
            if (lane < L) b = s_ring[(dst0 + from) & MASK];
        } else {                                             // behind the ring: through global memory, behind a drain and an invalidate
            store_span(flushed, produced, false);
            flushed = produced;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
            if (lane < L) b = dstb[from];
        }
        if (lane < L) s_ring[(dst0 + produced + lane) & MASK] = b;
        wave_sync();
    }
    // (the literal lies inside the stream: parse_element) -> the stream position behind it
    __device__ __forceinline__ int64_t literal(int64_t p, int64_t &produced, int64_t left) {
        while (left > 0) {
            if (p >= win_end) load_window(p);
            int64_t c = win_end - p;
            if (c > left) c = left;
            if (c > SN_CHUNK) c = SN_CHUNK;
            for (int i = lane; i < (int)c; i += SN_THREADS) s_ring[(dst0 + produced + i) & MASK] = s_in[p - win_base + i];
            wave_sync();
            p += c;
            produced += c;
            left -= c;
            flush_if_due(produced, SN_FLUSH);
        }
        return p;
    }
};

}  // namespace

__global__ __launch_bounds__(SN_THREADS) void snappy_sections_kernel(SectionArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sn_lds[];
    const SnSection S = A.sec[blockIdx.x];
    SnWave W;
    W.open(sn_lds, A, S);

    int sub = snappy::S_OK;
    int64_t expected = 0, pos = 0, produced = 0;
    if (S.src_bytes <= 0) sub = snappy::S_PREAMBLE;
    else {
        W.load_window(W.src0);
        const LdsStream g{W.s_in, W.win_base};
        int64_t n = 0, body = 0;
        sub = uni(snappy::read_preamble(g, W.src0, W.src_end, S.dst_bytes, &n, &body));
        expected = S.dst_bytes;
        pos = uni64(body);
    }
    while (sub == snappy::S_OK && produced < expected) {     // (every element consumes at least one byte of [pos, src_end))
        if (pos >= W.src_end) { sub = snappy::S_INPUT_SHORT; break; }
        if (pos + 5 > W.win_end && W.win_end < W.src_end) W.load_window(pos);
        snappy::Element e;
        const int s = uni(snappy::parse_element(LdsStream{W.s_in, W.win_base}, pos, W.src_end, produced, expected, &e));
        if (s != snappy::S_OK) { sub = s; break; }
        const int64_t len = uni64(e.len), data = uni64(e.data);
        if (uni(e.copy)) {
            W.copy(produced, uni64(e.offset), (int)len);
            pos = data;
            produced += len;
        } else pos = W.literal(data, produced, len);
        W.flush_if_due(produced, SN_FLUSH);
    }
    if (sub == snappy::S_OK && pos != W.src_end) sub = snappy::S_INPUT_LEFT;
    W.close(A, S, sub, pq::C_SNAPPY);                        // (a good stream has produced S.dst_bytes: the preamble said so)
}

int snappy_decompress_sections(ph_ctx *ctx, const uint8_t *src, uint8_t *dst, const SnSection *sections_dev, int32_t n, pq::PageDesc *pages_dev,
                               unsigned long long *err, int32_t *status_dev) {
    return launch_sections<snappy_sections_kernel, SN_THREADS, SN_TILE + SN_RING>(ctx, src, dst, sections_dev, n, pages_dev, err, status_dev);
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
    return ph::decompress_streams(ctx, "ph_snappy_decompress", ph::snappy_decompress_sections, src_dev, src_pos, src_bytes, dst_dev, dst_pos, dst_bytes, n, status);
}
