// ZSTD streams (Parquet codec 6) decoded on the device: one launch over n independent sections, ONE WAVE a section, on section_wave.h's
// frame (ring, flush, the section's end), and the two raw entry points ph_zstd_decompress / ph_zstd_decompress_host.
//
// A compressed block is two serial chains: the Huffman symbols of its literal streams, and the FSE states of its sequence stream, each
// symbol beginning where the one before it ended; a match reads what the same stream has written. The parallelism is across sections and,
// inside one, across the entries of a table that is being built and the bytes of a copy. The wave IS the getter and the sink that
// zstd_decode.h's decode_stream is instantiated over:
//   - TWO input windows. A block is read at two places at once, both backwards: the literal streams near its start and the sequence stream
//     from its end; one window would be re-loaded for every sequence. Window A serves the headers, the table descriptions, raw runs and the
//     literal streams (back_a), window B the sequence stream (back_b). A backward read that leaves its window re-loads it so that the bytes
//     asked for are its LAST ones; a forward read so that they are its first;
//   - the tables live in LDS (zstd::Tables): 2^11 Huffman entries of 16 bits, 512 / 256 / 512 sequence entries and 64 for the weights, of
//     32 bits; the builds are lane-strided (zstd_decode.h);
//   - literals are decoded on demand, in literal order, straight into the ring as the sequences ask for them: one stream after the other
//     where a block has four (128 KiB of staged literals do not fit beside the ring);
//   - a copy goes in steps of ZS_CHUNK bytes that read all their sources, then write (section_wave.h). An offset of up to ZS_RING reads
//     the ring. A larger one is ORDINARY here (a ZSTD window spans the page) and reads global memory: the bytes it wants were flushed long
//     ago (they lie more than ZS_RING - ZS_CHUNK behind, the flush lags ZS_FLUSH + ZS_CHUNK at most), and `visible` — the flushed
//     position at the last agent-scope fence — says whether this wave may load them yet. Only a step whose sources end beyond it fences;
//   - completed ring bytes are, as they are flushed, folded into the frame's XXH64 straight from the ring: a 32-byte stripe feeds four
//     independent accumulators, lanes 0..3 hold one each and take their 8 bytes of every stripe. Frames without a checksum skip it.
// Bounds beyond the frame's: a far copy loads [at - offset, at - offset + n) of the destination, which the decoder has checked to lie in
// [the frame's first byte, at); table writes stay below the sizes zstd_decode.h checks the logs and the weights against.
#include "zstd_decompress.h"

namespace ph {

namespace {

struct ZsWave : SectionWave<ZS_THREADS, ZS_TILE, ZS_RING> {
    using Base = SectionWave<ZS_THREADS, ZS_TILE, ZS_RING>;
    unsigned char *s_in2;            // LDS: window B
    int64_t win2_base, win2_end;
    int64_t visible;                 // output below this position was flushed before the last agent-scope fence
    bool hashing;                    // the open frame has a checksum
    int64_t xx_done;                 // the frame's output up to here is in the accumulators
    uint64_t xx_acc;                 // lanes 0..3: accumulator `lane`

    // ---- the getter
    __device__ __forceinline__ int lane() const { return Base::lane; }
    __device__ __forceinline__ int lanes() const { return ZS_THREADS; }
    __device__ __forceinline__ void sync() const { wave_sync(); }
    __device__ __forceinline__ void inc(uint32_t *p) const { atomicAdd(p, 1u); }
    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

    // [base, base + ZS_TILE) of the stream into window w; base is a multiple of 16 and >= 0
    __device__ __forceinline__ void load(unsigned char *w, int64_t &wb, int64_t &we, int64_t base) {
        wb = base;
        we = base + ZS_TILE < src_end ? base + ZS_TILE : src_end;
        wave_sync();                                             // (the lanes have read what they wanted of the old window)
        for (int i = Base::lane; i < ZS_TILE / 16; i += ZS_THREADS) {
            const int64_t a = base + (int64_t)i * 16;
            if (a < src_end) reinterpret_cast<uint4 *>(w)[i] = *reinterpret_cast<const uint4 *>(srcb + (a - src0));
        }
        wave_sync();
    }
    __device__ __forceinline__ static int64_t back_base(int64_t e) {   // the window whose last 16-byte unit holds byte e - 1
        const int64_t b = ((e + 15) & ~(int64_t)15) - ZS_TILE;
        return b < 0 ? 0 : b;
    }
    __device__ __forceinline__ uint32_t bytes(const unsigned char *w, int at, int k) const {   // k <= 4, little-endian
        uint32_t v = w[at];
        if (k > 1) v |= (uint32_t)w[at + 1] << 8;
        if (k > 2) v |= (uint32_t)w[at + 2] << 16;
        if (k > 3) v |= (uint32_t)w[at + 3] << 24;
        return uni(v);
    }
    // (decode_stream asks for positions inside [src0, src_end) only)
    __device__ __forceinline__ uint32_t u8(int64_t p) { return le(p, 1); }
    __device__ __forceinline__ uint32_t le(int64_t p, int k) {
        if (p < win_base || p + k > win_end) load(s_in, win_base, win_end, p & ~(int64_t)15);
        return bytes(s_in, (int)(p - win_base), k);
    }
    __device__ __forceinline__ uint32_t back_a(int64_t p, int k) {
        if (p < win_base || p + k > win_end) load(s_in, win_base, win_end, back_base(p + k));
        return bytes(s_in, (int)(p - win_base), k);
    }
    __device__ __forceinline__ uint32_t back_b(int64_t p, int k) {
        if (p < win2_base || p + k > win2_end) load(s_in2, win2_base, win2_end, back_base(p + k));
        return bytes(s_in2, (int)(p - win2_base), k);
    }

    // ---- the sink
    __device__ __forceinline__ uint32_t ring_byte(int64_t at) const { return s_ring[(dst0 + at) & MASK]; }
    // n stripes of 32 bytes from xx_done on
    __device__ __forceinline__ void hash_stripes(int64_t n) {
        if (Base::lane < 4) {
            int64_t p = xx_done + 8 * Base::lane;
            for (int64_t i = 0; i < n; i++, p += 32) {
                uint64_t k = 0;
#pragma unroll
                for (int j = 0; j < 8; j++) k |= (uint64_t)ring_byte(p + j) << (8 * j);
                xx_acc = zstd::xxh_round(xx_acc, k);
            }
        }
        xx_done += 32 * n;
    }
    __device__ __forceinline__ void flush_if_due(int64_t produced) {
        Base::flush_if_due(produced, ZS_FLUSH);
        if (hashing && produced - xx_done >= ZS_FLUSH) hash_stripes((produced - xx_done) >> 5);
    }
    __device__ __forceinline__ void frame_begin(int64_t fstart, bool hashed) {
        hashing = hashed;
        xx_done = fstart;
        xx_acc = zstd::xxh_init(Base::lane & 3);
    }
    __device__ __forceinline__ uint64_t lane_acc(int k) const {
        const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)xx_acc, k, ZS_THREADS), hi = (uint32_t)__shfl((int)(uint32_t)(xx_acc >> 32), k, ZS_THREADS);
        return (uint64_t)hi << 32 | lo;
    }
    __device__ __forceinline__ uint32_t frame_hash(int64_t fstart, int64_t produced) {
        wave_sync();
        hash_stripes((produced - xx_done) >> 5);
        const int64_t n = produced - fstart;
        uint64_t h = zstd::XP5;
        if (n >= 32) h = zstd::xxh_merge(lane_acc(0), lane_acc(1), lane_acc(2), lane_acc(3));
        const int64_t from = xx_done;
        const uint32_t v = zstd::xxh_finish(h + (uint64_t)n, (int)(produced - xx_done), [&](int j) { return ring_byte(from + j); });
        hashing = false;
        return uni(v);
    }
    __device__ __forceinline__ void lit(int64_t at, uint32_t byte) {
        s_ring[(dst0 + at) & MASK] = (unsigned char)byte;        // (every lane stores the same byte)
        flush_if_due(at + 1);
    }
    __device__ __forceinline__ void literal(ZsWave &, int64_t from, int64_t at, int64_t n) {   // bytes of the stream (inside it: the decoder)
        wave_sync();
        while (n > 0) {
            if (from < win_base || from >= win_end) load(s_in, win_base, win_end, from & ~(int64_t)15);
            int64_t c = win_end - from;
            if (c > n) c = n;
            if (c > ZS_CHUNK) c = ZS_CHUNK;
            for (int i = Base::lane; i < (int)c; i += ZS_THREADS) s_ring[(dst0 + at + i) & MASK] = s_in[from - win_base + i];
            wave_sync();
            from += c;
            at += c;
            n -= c;
            flush_if_due(at);
        }
    }
    __device__ __forceinline__ void fill(int64_t at, uint32_t byte, int64_t n) {
        wave_sync();
        while (n > 0) {
            const int64_t c = n < ZS_CHUNK ? n : ZS_CHUNK;
            for (int i = Base::lane; i < (int)c; i += ZS_THREADS) s_ring[(dst0 + at + i) & MASK] = (unsigned char)byte;
            wave_sync();
            at += c;
            n -= c;
            flush_if_due(at);
        }
    }
    // 1 <= off <= at - the frame's first byte, at + n <= the expected length
    __device__ __forceinline__ void match(int64_t at, int64_t off, int64_t n) {
        constexpr int PER = ZS_CHUNK / ZS_THREADS;
        wave_sync();
        while (n > 0) {
            const int c = (int)(n < ZS_CHUNK ? n : ZS_CHUNK);
            unsigned char b[PER];
            if (off > ZS_RING) {                                 // behind the ring: global memory (off > c: the step's sources do not overlap its bytes)
                const int64_t lo = at - off, hi = lo + c;
                if (hi > flushed) {                              // (never: see the head comment)
                    const int64_t upto = ((dst0 + at) & ~(int64_t)15) - dst0;
                    if (upto > flushed) {
                        store_span(flushed, upto, false);
                        flushed = upto;
                    }
                }
                if (hi > visible) {
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
                    visible = flushed;
                }
#pragma unroll
                for (int k = 0; k < PER; k++) {
                    const int j = Base::lane + k * ZS_THREADS;
                    b[k] = j < c ? dstb[lo + j] : 0;
                }
            } else {
                const uint32_t o = (uint32_t)off;
                const int64_t sbase = dst0 + at - off;
                uint32_t r = (uint32_t)Base::lane, step = ZS_THREADS;
                if (o < (uint32_t)c && o <= (uint32_t)ZS_THREADS) {   // (r < o and step < o, or 64 < o: one wrap a step at most)
                    r %= o;
                    step %= o;
                }
                const bool wrap = o < (uint32_t)c;
#pragma unroll
                for (int k = 0; k < PER; k++) {
                    b[k] = Base::lane + k * ZS_THREADS < c ? s_ring[(sbase + r) & MASK] : 0;
                    r += step;
                    if (wrap && r >= o) r -= o;
                }
            }
            wave_sync();
#pragma unroll
            for (int k = 0; k < PER; k++) {
                const int j = Base::lane + k * ZS_THREADS;
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

__global__ __launch_bounds__(ZS_THREADS) void zstd_sections_kernel(SectionArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char zs_lds[];
    const SnSection S = A.sec[blockIdx.x];
    ZsWave W;
    W.open(zs_lds, A, S);
    unsigned char *p = zs_lds + ZS_TILE + ZS_RING;               // behind the frame's window and ring: window B, the tables
    W.s_in2 = p, p += ZS_TILE;
    W.win2_base = W.win2_end = W.src0;
    W.visible = 0;
    W.hashing = false;
    W.xx_done = 0;
    W.xx_acc = 0;
    zstd::Tables T;
    T.huf = reinterpret_cast<uint16_t *>(p), p += 2 * zstd::HUF_CAP;
    T.ll = reinterpret_cast<uint32_t *>(p), p += 4 << zstd::LL_LOG;
    T.of = reinterpret_cast<uint32_t *>(p), p += 4 << zstd::OF_LOG;
    T.ml = reinterpret_cast<uint32_t *>(p), p += 4 << zstd::ML_LOG;
    T.wt = reinterpret_cast<uint32_t *>(p), p += 4 << zstd::WT_LOG;
    T.rank = reinterpret_cast<uint32_t *>(p), p += 64;
    T.norm = reinterpret_cast<int16_t *>(p), p += 2 * zstd::MAX_SYMS;
    T.cum = reinterpret_cast<uint16_t *>(p), p += 2 * zstd::MAX_SYMS;
    T.weights = p;

    int sub = zstd::check_sizes(S.src_bytes, S.dst_bytes);
    if (sub == zstd::S_OK && S.src_bytes > 0) sub = ph::uni(zstd::decode_stream(W, W.src0, W.src_end, S.dst_bytes, T, W));
    W.close(A, S, sub, pq::C_ZSTD);
}

int zstd_decompress_sections(ph_ctx *ctx, const uint8_t *src, uint8_t *dst, const SnSection *sections_dev, int32_t n, pq::PageDesc *pages_dev,
                             unsigned long long *err, int32_t *status_dev) {
    return launch_sections<zstd_sections_kernel, ZS_THREADS, ZS_LDS>(ctx, src, dst, sections_dev, n, pages_dev, err, status_dev);
}

}  // namespace ph

extern "C" int ph_zstd_decompress_host(const void *src, int64_t src_bytes, void *dst, int64_t expected, int64_t *produced) {
    PH_REQUIRE(src_bytes >= 0 && (src || src_bytes == 0) && expected >= 0 && (dst || expected == 0), "ph_zstd_decompress_host: bad arguments");
    if (produced) *produced = 0;
    const int sub = ph::zstd::decompress_host((const uint8_t *)src, src_bytes, (uint8_t *)dst, expected);
    PH_REQUIRE(sub == ph::zstd::S_OK, "ph_zstd_decompress_host: a corrupt ZSTD stream of %lld bytes for %lld: %s", (long long)src_bytes, (long long)expected,
               ph::zstd::sub_text(sub));
    if (produced) *produced = expected;
    return PH_OK;
}

extern "C" int ph_zstd_stream_stats_host(const void *src, int64_t src_bytes, int64_t expected, int64_t far_limit, int64_t *stats) {
    PH_REQUIRE(src_bytes >= 0 && (src || src_bytes == 0) && expected >= 0 && stats, "ph_zstd_stream_stats_host: bad arguments");
    ph::zstd::Stats st{0, 0, 0, 0, far_limit};
    int sub = ph::zstd::check_sizes(src_bytes, expected);        // (before anything is allocated: expected <= 32768 * src_bytes)
    if (sub == ph::zstd::S_OK) {
        std::vector<uint8_t> out((size_t)expected + 1);
        sub = ph::zstd::decompress_host_stats((const uint8_t *)src, src_bytes, out.data(), expected, &st);
    }
    PH_REQUIRE(sub == ph::zstd::S_OK, "ph_zstd_stream_stats_host: a corrupt ZSTD stream of %lld bytes for %lld: %s", (long long)src_bytes, (long long)expected,
               ph::zstd::sub_text(sub));
    stats[0] = st.literals, stats[1] = st.sequences, stats[2] = st.match_bytes, stats[3] = st.far_match_bytes;
    return PH_OK;
}

extern "C" int ph_zstd_decompress(ph_ctx *ctx, const void *src_dev, const int64_t *src_pos, const int64_t *src_bytes, void *dst_dev,
                                  const int64_t *dst_pos, const int64_t *dst_bytes, int32_t n, int32_t *status) {
    return ph::decompress_streams(ctx, "ph_zstd_decompress", ph::zstd_decompress_sections, src_dev, src_pos, src_bytes, dst_dev, dst_pos, dst_bytes, n, status);
}
