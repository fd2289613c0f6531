// DELTA_BYTE_ARRAY (front coding) reconstructed on the device: one launch over the front-coded pages of a column, ONE WAVE a page, on
// section_wave.h's frame (window, ring, flush, the section's end). dba_decode.h says what comes before it.
//
// The chain is LZ-shaped, and as serial: value k is a COPY of prefix[k] bytes from distance len[k - 1] — the value in front, which ends
// where this one begins — and then a LITERAL of the suffix's bytes, which lie back to back in the page's suffix section. The lengths pass has
// judged prefix[k] <= len[k - 1], so a copy never overlaps its own output, and it is carried out like the codecs' matches: a step of up to
// DBA_CHUNK bytes reads ALL its sources into registers, then writes (section_wave.h, ring size).
//   - Lengths arrive 64 at a time, one value a lane (two loads per 64 values), and a lane read makes each step's pair wave-uniform: the
//     chain's state (positions, the length of the value in front) lives in scalar registers. One value a step.
//   - A value in front that is longer than DBA_RING may have left the ring; then the prefix is read from global memory, which this wave has
//     written itself. As in zstd_decompress.hip: the bytes wanted were flushed long ago (they lie more than DBA_RING - DBA_CHUNK behind,
//     the flush lags DBA_FLUSH + DBA_CHUNK at most), and `visible` — the flushed position at the last agent-scope fence — says whether
//     this wave may load them yet. Only a step whose sources end beyond it fences.
// Bounds: the chain has exactly nvalues steps (a number of the page's rows, not of the stream). Before a byte moves, every step is checked
// once more against the destination range [dst, dst + dst_bytes) and its literal against the suffix section, although the lengths pass
// has established both; a chain that leaves them stops, and its page reads as zeros.
#include "dba_decode.h"

namespace ph {

namespace {

struct DbaWave : SectionWave<DBA_THREADS, DBA_TILE, DBA_RING> {
    int64_t visible;                 // output below this position was flushed before the last agent-scope fence

    // n suffix bytes from stream position `from` (inside the section: the caller's check) to output position `at`
    __device__ __forceinline__ void literal(int64_t from, int64_t at, int64_t n) {
        while (n > 0) {
            if (from >= win_end) load_window(from);
            int64_t c = win_end - from;
            if (c > n) c = n;
            if (c > DBA_CHUNK) c = DBA_CHUNK;
            for (int i = lane; i < (int)c; i += DBA_THREADS) s_ring[(dst0 + at + i) & MASK] = s_in[from - win_base + i];
            wave_sync();
            from += c;
            at += c;
            n -= c;
            flush_if_due(at, DBA_FLUSH);
        }
    }
    // n bytes from `off` behind output position `at`: 1 <= n <= off <= at
    __device__ __forceinline__ void copy(int64_t at, int64_t off, int64_t n) {
        if (n <= DBA_THREADS && off <= DBA_RING) {               // the common case: one byte a lane
            unsigned char b = 0;
            if (lane < (int)n) b = s_ring[(dst0 + at - off + lane) & MASK];
            wave_sync();
            if (lane < (int)n) s_ring[(dst0 + at + lane) & MASK] = b;
            wave_sync();
            flush_if_due(at + n, DBA_FLUSH);
            return;
        }
        copy_long(at, off, n);
    }
    __device__ __forceinline__ void copy_long(int64_t at, int64_t off, int64_t n) {
        constexpr int PER = DBA_CHUNK / DBA_THREADS;
        while (n > 0) {
            const int c = (int)(n < DBA_CHUNK ? n : DBA_CHUNK);
            unsigned char b[PER];
            if (off > DBA_RING) {                                // behind the ring: global memory
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
                    const int j = lane + k * DBA_THREADS;
                    b[k] = j < c ? dstb[lo + j] : 0;
                }
            } else {
                const int64_t sbase = dst0 + at - off;
#pragma unroll
                for (int k = 0; k < PER; k++) {
                    const int j = lane + k * DBA_THREADS;
                    b[k] = j < c ? s_ring[(sbase + j) & MASK] : 0;
                }
            }
            wave_sync();
#pragma unroll
            for (int k = 0; k < PER; k++) {
                const int j = lane + k * DBA_THREADS;
                if (j < c) s_ring[(dst0 + at + j) & MASK] = b[k];
            }
            wave_sync();
            at += c;
            n -= c;
            flush_if_due(at, DBA_FLUSH);
        }
    }
};

}  // namespace

__global__ __launch_bounds__(DBA_THREADS) void dba_expand_kernel(DbaArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dba_lds[];
    const DbaPage P = A.pages[blockIdx.x];
    if (!P.ok) return;
    int64_t dst_pos = P.dst_pos, dst_bytes = P.dst_bytes;
    if (A.off) {
        dst_pos = A.off[P.row0];
        dst_bytes = (int64_t)A.off[P.row0 + P.nrows] - dst_pos;
    }
    const SnSection S{P.suf_pos, P.suf_bytes, dst_pos, dst_bytes, -1, -1, 0, 0};
    const SectionArgs F{A.src, A.dst, nullptr, nullptr, nullptr, nullptr};
    DbaWave W;
    W.open(dba_lds, F, S);
    W.visible = 0;

    int64_t at = 0, lit = W.src0, before = 0;                    // output position; the next suffix; the length of the value in front
    int bad = 0;
    for (int base = 0; base < P.nvalues && !bad; base += DBA_THREADS) {
        const int m = P.nvalues - base < DBA_THREADS ? P.nvalues - base : DBA_THREADS;
        int pre = 0, suf = 0;
        if (W.lane < m) {
            pre = A.pre[P.val0 + base + W.lane];
            suf = A.slen[P.val0 + base + W.lane];
        }
        for (int j = 0; j < m; j++) {
            const int64_t p = __builtin_amdgcn_readlane(pre, j), s = __builtin_amdgcn_readlane(suf, j);
            if (p < 0 || s < 0 || p > before || p + s > dst_bytes - at || s > W.src_end - lit) { bad = 1; break; }
            if (p) W.copy(at, before, p);
            if (s) W.literal(lit, at + p, s);
            before = p + s;
            at += before;
            lit += s;
        }
    }
    if (at != dst_bytes) bad = 1;
    W.close(F, S, bad ? 1 : SUB_OK, pq::C_LEN);
    if (A.status && W.lane == 0) A.status[blockIdx.x] = bad;
}

int dba_expand_pages(ph_ctx *ctx, const DbaArgs &A, int32_t n) {
    if (n <= 0) return PH_OK;
    PH_CHECK(raise_lds<dba_expand_kernel>(ctx, DBA_TILE + DBA_RING));
    dba_expand_kernel<<<(unsigned)n, DBA_THREADS, DBA_TILE + DBA_RING, ctx->stream>>>(A);
    PH_HIP(hipGetLastError());
    return PH_OK;
}

}  // namespace ph
