// ph_table_create_parquet: the column chunks of a Parquet file -> resident table, decoded on the device (see planhip.h), and the host-only
// entry points beside it (ph_parquet_schema, ph_parquet_pages, ph_parquet_read_column_host, ph_delta_decode_host, ph_delta_byte_array_decode_host).
//
// The host parses the footer and the page headers (parquet_meta.h), resolves every data page of the requested columns into byte ranges
// checked against the page (parquet_decode.h, resolve_column) and uploads those columns' chunks only. Then, per column, one workgroup per page:
//   pq_dict_walk_kernel — BYTE_ARRAY dictionary pages: the length chain, staged through LDS in 16 KiB tiles and walked by one lane
//                         out of LDS, gives every entry's position and length;
//   pq_page_kernel      — a data page: (1) the definition levels' hybrid runs -> validity bits (atomicOr: pages share bitmap words), the row of
//                         every value (a prefix over the wave ballots) and the non-NULL count; (2) the values: PLAIN value k read in place,
//                         dictionary pages' indices expanded run by run and gathered from the chunk's dictionary page, PLAIN BYTE_ARRAY through
//                         the same LDS walk. The run HEADERS are the sequential part: every lane walks them (the same address in all lanes: one
//                         broadcast load) and the workgroup expands each run, 256 values a step.
// VARCHAR lengths are then scanned into offsets and the bytes copied with the text path's kernels, and the column interned by the shared
// encode_strings (str_encode.h), which knows NULL rows. Every column is finished by ph::table_finish_column.
// Compressed pages (ph_table_create_parquet_ex + PH_PARQUET_SNAPPY / PH_PARQUET_LZ4_RAW / PH_PARQUET_GZIP / PH_PARQUET_ZSTD; parquet_codecs.h is the table of
// them): the chunks are uploaded as stored, and behind them the allocation holds a region of decompressed sections, each on a 16-byte
// boundary. The sections are listed per codec, and ONE launch per codec present — snappy_decompress.hip's, lz4_decompress.hip's,
// gzip_decompress.hip's and zstd_decompress.hip's kernel, in the table's order, one behind the other in front of the first column's kernels — fills the region; the
// PageDescs of compressed pages (and dict_pos behind a compressed dictionary page) point into it, so the kernels above run unchanged on
// one base pointer. A v1 page's level-section length lies inside its stream: the section kernel completes that PageDesc on the device
// (section_wave.h, close). A section that fails reads as zeros and its PageDesc is emptied there, so the page kernels decode nothing of it
// and the codec's cause (C_SNAPPY, C_LZ4, C_GZIP, C_ZSTD) stays the page's (no read-back between the launches; the good path pays nothing).
// Delta pages (PH_PARQUET_DELTA): a page whose PageDesc names DELTA_BINARY_PACKED or DELTA_LENGTH_BYTE_ARRAY takes pq_delta_stream in step 2 of
// pq_page_kernel — block headers walked by every lane into an LDS table of miniblocks, lane j unpacks delta j, a wrapping 64-bit scan over the
// workgroup turns deltas into values (for BYTE_ARRAY: into lengths, and a second scan into the values' positions) — and everything before
// and behind that step is what the other pages get. ph_delta_decode runs the same function over caller-given streams.
// Front-coded pages (PH_PARQUET_DELTA_BYTE_ARRAY): a page whose PageDesc names DELTA_BYTE_ARRAY takes pq_dba_lengths in step 2 — pq_delta_stream
// twice, prefixes and suffix lengths, into per-value temporaries of the column (8 bytes a value, sized by rows), the rules of
// parquet_decode.h judged in the host twin's order, len = prefix + suffix into the lengths column, a negative sbegin as the row's mark, and one
// DbaPage for the reconstruction — and, behind the offset scan, dba_expand.hip's kernel writes those rows' bytes straight into the column's
// byte buffer while copy_strings_kernel leaves them alone. ph_delta_byte_array_decode runs the same two functions over caller-given sections.
// Bounds: a kernel reads file bytes only inside ranges the host has checked against the upload, loops over runs and lengths are bounded by
// the page's num_values (a run holds at least one value), and what decoding finds wrong goes to one error word (lowest page wins).
#include <algorithm>

#include "common.h"
#include "dba_decode.h"
#include "ops.h"
#include "parquet_decode.h"
#include "gzip_decompress.h"
#include "lz4_decompress.h"
#include "snappy_decompress.h"
#include "zstd_decompress.h"
#include "str_encode.h"

namespace ph {

constexpr int PQ_THREADS = 256;   // workgroup of the page kernels (not A/B-measured)
constexpr int PQ_TILE = 16384;    // bytes of a BYTE_ARRAY page staged in LDS per step (not A/B-measured): 9 workgroups fit a CU's 160 KiB

struct GlobalBytes {
    const uint8_t *s;
    __device__ __forceinline__ uint8_t u8(int64_t p) const { return s[p]; }
    __device__ __forceinline__ uint32_t u32(int64_t p) const { uint32_t v; __builtin_memcpy(&v, s + p, 4); return v; }
    __device__ __forceinline__ uint64_t u64(int64_t p) const { uint64_t v; __builtin_memcpy(&v, s + p, 8); return v; }
};

// what the page kernels of one column work on
struct PqColArgs {
    const uint8_t *bytes;            // the uploaded chunks; PageDesc positions are relative to it
    const pq::PageDesc *pages;       // this launch's pages (blockIdx.x)
    int32_t page0;                   // their index in the call's page list: the error key
    int32_t flba_len, width;
    void *out;                       // fixed width: the values; BYTE_ARRAY: int32 lengths (scanned into offsets afterwards)
    unsigned *validity;              // nullable column: zeroed on entry
    int32_t *vrow;                   // nullable column: [first_row + k] = the page row of the page's k-th value
    int64_t *sbegin;                 // BYTE_ARRAY: where a row's bytes begin
    int64_t *vpos, *dpos;            // BYTE_ARRAY: PLAIN values by [first_row + k]; dictionary entries by [dict_base + index]
    int32_t *vlen, *dlen;
    unsigned long long *err, *nvalid;
    int32_t *dba_pre, *dba_suf;      // a column with front-coded pages: prefix and suffix length by [first_row + k]
    DbaPage *dba;                    // and what its reconstruction needs, by page of this launch (zeroed on entry)
};

__device__ __forceinline__ void pq_report(unsigned long long *err, int page, int cause) {
    atomicMin(err, ((unsigned long long)(unsigned)page << 8) | (unsigned)cause);
}

// The length chain of a PLAIN BYTE_ARRAY section [pos, end) of n values -> vpos[k], vlen[k]. The workgroup stages a tile that begins at the
// next length (rounded down to 16 bytes) in LDS, lane 0 walks the lengths that begin in it; a value longer than the tile is stepped over.
// Every step consumes at least one value, so there are at most n steps. Returns the cause (uniform).
__device__ int pq_walk_byte_arrays(const uint8_t *bytes, unsigned char *s_tile, int64_t *s_state, int64_t pos, int64_t end, int n, int64_t *vpos, int32_t *vlen) {
    int k = 0, cause = -1;
    if (n == 0) return pos == end ? pq::C_OK : pq::C_COUNT;
    for (int step = 0; step < n && cause < 0; step++) {
        const int64_t base = pos & ~(int64_t)15;
        {
            const uint4 *src = reinterpret_cast<const uint4 *>(bytes + base);   // (the allocation is padded by a tile behind the last chunk)
            uint4 *dst = reinterpret_cast<uint4 *>(s_tile);
            for (int i = threadIdx.x; i < PQ_TILE / 16; i += PQ_THREADS) dst[i] = src[i];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int64_t tile_end = end < base + PQ_TILE ? end : base + PQ_TILE;
            while (k < n && pos + 4 <= tile_end) {
                const unsigned char *q = s_tile + (pos - base);
                const uint32_t len = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
                if ((int64_t)len > end - pos - 4) { cause = pq::C_LEN; break; }
                vpos[k] = pos + 4;
                vlen[k] = (int32_t)len;
                pos += 4 + (int64_t)len;
                k++;
            }
            if (cause < 0) {
                if (k == n) cause = pos == end ? pq::C_OK : pq::C_COUNT;
                else if (end - pos < 4) cause = pq::C_COUNT;
            }
            s_state[0] = pos;
            s_state[1] = k;
            s_state[2] = cause;
        }
        __syncthreads();
        pos = s_state[0];
        k = (int)s_state[1];
        cause = (int)s_state[2];
        __syncthreads();   // (the state is read before lane 0 writes the next)
    }
    return cause < 0 ? pq::C_COUNT : cause;
}

// ---- DELTA_BINARY_PACKED (parquet_decode.h has the format and the shared header readers)
// The miniblock table of one step: where each needed miniblock begins, its width and its block's min_delta.
struct DeltaTab {
    int64_t start[pq::DELTA_MAX_MINIBLOCKS];
    uint64_t min_delta[pq::DELTA_MAX_MINIBLOCKS];
    int32_t width[pq::DELTA_MAX_MINIBLOCKS];
};
struct DeltaScan {
    unsigned long long wtot[2][PQ_THREADS / 64];   // the waves' totals of a 256-value step, double-buffered: one barrier a step
    int flag;                                      // the cause a consumer refused a value with (0: none)
};

// inclusive wrapping sum of x over the workgroup's 256 lanes (shuffles inside a wave, the four wave totals through LDS); it counts the calls
__device__ __forceinline__ unsigned long long pq_scan256(unsigned long long x, DeltaScan *sc, int it, unsigned long long *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int dl = 1; dl < 64; dl <<= 1) {
        const unsigned long long y = __shfl_up(x, dl, 64);
        if (lane >= dl) x += y;
    }
    if (lane == 63) sc->wtot[it & 1][wave] = x;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < PQ_THREADS / 64; w++) { const unsigned long long t = sc->wtot[it & 1][w]; before += w < wave ? t : 0ull; all += t; }
    *total = all;
    return before + x;
}

// One stream at [pos, end) by the whole workgroup -> a pq::DeltaSub (uniform); pos -> behind the last needed miniblock. Steps of as many
// whole blocks as the table holds (at least one: the limits of delta_header): (1) every lane walks the steps' block headers — the same
// addresses in all lanes, the sequential part, 2 + miniblocks bytes per block — and lane 0 fills the table; (2) lane j unpacks delta j
// of the step from its miniblock, 256 a time, and a wrapping scan over min_delta + delta plus the carry of everything before gives the
// values. emit(k, value k) -> a cause is called by ONE lane per value; a refusal ends the decode behind the step (DS_EMIT, sc->flag).
// A header that fails ends it behind the blocks in front of it, whose values are still judged: the order in which host_delta_stream meets
// the faults. Trip counts: blocks while values are wanted, and total <= cap is checked first.
template <class Emit>
__device__ int pq_delta_stream(const GlobalBytes &g, DeltaTab *tab, DeltaScan *sc, int64_t &pos, int64_t end, int bits, int64_t expected, int64_t cap, int64_t *count,
                               const Emit &emit) {
    const int tid = threadIdx.x;
    pq::DeltaHeader h;
    *count = 0;
    const int s = pq::delta_header(g, pos, end, &h);
    if (s != pq::DS_OK) return s;
    *count = h.total;
    if (expected >= 0 && h.total != expected) return pq::DS_COUNT;
    if (h.total > cap) return pq::DS_CAPACITY;
    if (h.total == 0) return pq::DS_OK;
    if (tid == 0) {
        sc->flag = emit((int64_t)0, pq::delta_value(h.first, bits));
    }
    uint64_t carry = h.first;
    const int per_step = pq::DELTA_MAX_MINIBLOCKS / h.mini;   // blocks a step (>= 1)
    int it = 0;
    for (int64_t done = 1; done < h.total;) {
        int nb = 0, walk = pq::DS_OK;
        while (nb < per_step && done + (int64_t)nb * h.block < h.total) {
            int64_t p2 = pos;
            const int base = nb * h.mini;
            walk = pq::delta_block(g, p2, end, h, h.total - done - (int64_t)nb * h.block, bits, [&](int m, int64_t at, int w, uint64_t md) {
                if (tid == 0) { tab->start[base + m] = at; tab->width[base + m] = w; tab->min_delta[base + m] = md; }
            });
            if (walk != pq::DS_OK) break;
            pos = p2;
            nb++;
        }
        __syncthreads();
        const int64_t left = h.total - done, n = (int64_t)nb * h.block < left ? (int64_t)nb * h.block : left;
        for (int64_t base = 0; base < n; base += PQ_THREADS, it++) {
            const int64_t j = base + tid;
            unsigned long long x = 0;
            if (j < n) {
                const int m = (int)(j / h.per_mini);
                x = tab->min_delta[m] + pq::packed_get64(g, tab->start[m], tab->width[m], j - (int64_t)m * h.per_mini);
            }
            unsigned long long total;
            const unsigned long long incl = pq_scan256(x, sc, it, &total);
            if (j < n) {
                const int c = emit(done + j, pq::delta_value(carry + incl, bits));
                if (c != pq::C_OK) sc->flag = c;
            }
            carry += total;
        }
        done += n;
        __syncthreads();          // the table is read, the flag written
        if (sc->flag != pq::C_OK) return pq::DS_EMIT;
        if (walk != pq::DS_OK) return walk;
    }
    __syncthreads();              // (a stream of one value: lane 0's flag)
    return sc->flag != pq::C_OK ? pq::DS_EMIT : pq::DS_OK;
}

// The lengths of one DELTA_BYTE_ARRAY section [pos, end) by the whole workgroup -> a pq::DbaSub (uniform), judged in host_dba_lengths' order:
// the prefix stream -> pre[k], the suffix-length stream -> suf[k] (room for cap values each), prefix[k] <= prefix[k - 1] + suffix[k - 1] (a
// neighbour comparison once both arrays exist), the suffixes' bytes against the section's end. *suf_pos = where the suffixes' bytes begin,
// *total = the bytes all values hold, summed in 64 bits.
__device__ int pq_dba_lengths(const GlobalBytes &g, DeltaTab *tab, DeltaScan *sc, int64_t pos, int64_t end, int64_t expected, int64_t cap, int32_t *pre, int32_t *suf,
                              int64_t *count, int64_t *suf_pos, unsigned long long *total) {
    const int tid = threadIdx.x;
    *total = 0;
    *suf_pos = pos;
    int s = pq_delta_stream(g, tab, sc, pos, end, 32, expected, cap, count, [&](int64_t k, int64_t v) {
        if (v < 0) return (int)pq::C_PREFIX;
        pre[k] = (int32_t)v;
        return (int)pq::C_OK;
    });
    if (s != pq::DS_OK) return s == pq::DS_EMIT ? (int)pq::DBA_PREFIX : s;
    __syncthreads();              // (every lane has read the first stream's flag before lane 0 writes the second's)
    const int64_t n = *count;
    int64_t n2 = 0;
    s = pq_delta_stream(g, tab, sc, pos, end, 32, n, n, &n2, [&](int64_t k, int64_t v) {
        if (v < 0) return (int)pq::C_LEN;
        suf[k] = (int32_t)v;
        return (int)pq::C_OK;
    });
    if (s != pq::DS_OK) return s == pq::DS_EMIT ? (int)pq::DBA_SUFFIX_NEG : (int)pq::DBA_SUFFIX_STREAM + s;
    __syncthreads();              // pre and suf are read below by other lanes than wrote them
    *suf_pos = pos;
    int bad = 0;
    unsigned long long bytes = 0, all = 0;
    for (int64_t base = 0, it = 0; base < n; base += PQ_THREADS, it += 2) {
        const int64_t k = base + tid;
        unsigned long long sl = 0, len = 0;
        if (k < n) {
            const int64_t before = k ? (int64_t)pre[k - 1] + suf[k - 1] : 0;
            bad |= pre[k] > before;
            sl = (unsigned long long)suf[k];
            len = sl + (unsigned long long)pre[k];
        }
        unsigned long long t;
        pq_scan256(sl, sc, (int)it, &t);
        bytes += t;
        pq_scan256(len, sc, (int)it + 1, &t);
        all += t;
    }
    if (__syncthreads_or(bad)) return pq::DBA_PREFIX;
    if ((int64_t)bytes != end - pos) return (int64_t)bytes > end - pos ? pq::DBA_SUFFIX_PAST : pq::DBA_SUFFIX_SHORT;
    *total = all;
    return pq::DBA_OK;
}

// n raw DELTA_BYTE_ARRAY sections, one workgroup each: the lengths pass of ph_delta_byte_array_decode. val0[i] = where section i's values
// lie in the per-value temporaries pre / suf (the sum of the rooms in front of it).
__global__ __launch_bounds__(PQ_THREADS) void pq_dba_raw_kernel(const uint8_t *src, int32_t *lens, ph_dba_stream *streams, const int64_t *val0, int32_t *pre, int32_t *suf,
                                                                DbaPage *pages) {
    __shared__ DeltaTab s_tab;
    __shared__ DeltaScan s_scan;
    const ph_dba_stream S = streams[blockIdx.x];
    const GlobalBytes g{src};
    const int64_t v0 = val0[blockIdx.x], end = S.src_pos + S.src_bytes;
    int64_t count = 0, suf_pos = 0;
    unsigned long long total = 0;
    int sub = pq_dba_lengths(g, &s_tab, &s_scan, S.src_pos, end, S.expected, S.len_cap, pre + v0, suf + v0, &count, &suf_pos, &total);
    if (sub == pq::DBA_OK) sub = total >= (1ull << 31) ? pq::DBA_2G : (int64_t)total > S.byte_cap ? pq::DBA_BYTE_CAP : pq::DBA_OK;
    if (sub == pq::DBA_OK)
        for (int64_t k = threadIdx.x; k < count; k += PQ_THREADS) lens[S.len_pos + k] = pre[v0 + k] + suf[v0 + k];
    if (threadIdx.x == 0) {
        ph_dba_stream &o = streams[blockIdx.x];
        o.count = count;
        o.total_bytes = (int64_t)total;
        o.consumed = sub == pq::DBA_OK ? S.src_bytes : 0;
        o.sub = sub;
        if (sub == pq::DBA_OK) pages[blockIdx.x] = DbaPage{suf_pos, end - suf_pos, v0, S.byte_pos, (int64_t)total, 0, 0, (int32_t)count, 1, 0};
    }
}

// n raw streams, one workgroup each: ph_delta_decode
__global__ __launch_bounds__(PQ_THREADS) void pq_delta_raw_kernel(const uint8_t *src, int64_t *dst, ph_delta_stream *streams) {
    __shared__ DeltaTab s_tab;
    __shared__ DeltaScan s_scan;
    ph_delta_stream S = streams[blockIdx.x];
    const GlobalBytes g{src};
    int64_t pos = S.src_pos, count = 0;
    const int64_t end = S.src_pos + S.src_bytes;
    int sub = pq_delta_stream(g, &s_tab, &s_scan, pos, end, S.bits, S.expected, S.dst_cap, &count, [&](int64_t k, int64_t v) { dst[S.dst_pos + k] = v; return (int)pq::C_OK; });
    if (sub == pq::DS_OK && S.exact && pos != end) sub = pq::DS_TRAILING;
    if (threadIdx.x == 0) {
        ph_delta_stream &o = streams[blockIdx.x];
        o.count = count;
        o.consumed = sub == pq::DS_OK ? pos - S.src_pos : 0;
        o.sub = sub;
    }
}

__global__ __launch_bounds__(PQ_THREADS) void pq_dict_walk_kernel(PqColArgs A) {
    __shared__ __attribute__((aligned(16))) unsigned char s_tile[PQ_TILE];
    __shared__ int64_t s_state[3];
    const pq::PageDesc d = A.pages[blockIdx.x];
    const int cause = pq_walk_byte_arrays(A.bytes, s_tile, s_state, d.val_pos, d.val_pos + d.val_bytes, d.num_values, A.dpos + d.dict_base, A.dlen + d.dict_base);
    if (cause != pq::C_OK && threadIdx.x == 0) pq_report(A.err, A.page0 + (int)blockIdx.x, cause);
}

// KIND: the physical type (pq::PhysKind); OUTW: bytes of an output value (BYTE_ARRAY: 4, the lengths)
template <int KIND, int OUTW>
__global__ __launch_bounds__(PQ_THREADS) void pq_page_kernel(PqColArgs A) {
    // (a delta page's miniblock table lives in the tile a PLAIN BYTE_ARRAY page stages its lengths in: a page is one or the other)
    constexpr bool DELTA = KIND == pq::K_INT32 || KIND == pq::K_INT64 || KIND == pq::K_BYTES;
    static_assert(sizeof(DeltaTab) <= PQ_TILE, "the miniblock table shares the BYTE_ARRAY tile");
    __shared__ __attribute__((aligned(16))) unsigned char s_tile[KIND == pq::K_BYTES ? PQ_TILE : DELTA ? (int)sizeof(DeltaTab) : 16];
    __shared__ int64_t s_state[3];
    __shared__ int s_wcnt[2][PQ_THREADS / 64];
    __shared__ DeltaScan s_scan;
    const pq::PageDesc d = A.pages[blockIdx.x];
    const int page = A.page0 + (int)blockIdx.x;
    const GlobalBytes g{A.bytes};
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nv = d.num_values;
    const bool nullable = d.lvl_bytes >= 0;
    int cause = pq::C_OK;

    // ---- 1. definition levels: validity bits, the row of every value, the count of values
    int nvalid = nv;
    if (nullable) {
        int64_t pos = d.lvl_pos;
        const int64_t end = d.lvl_pos + d.lvl_bytes;
        int done = 0, running = 0, it = 0;
        while (done < nv) {                                        // (at most nv runs: a run holds at least one level)
            pq::Run r;
            const int c = pq::next_run(g, pos, end, 1, &r);
            if (c != pq::C_OK) { cause = pos >= end ? pq::C_COUNT : c; break; }
            if (!r.packed && r.count > nv - done) { cause = pq::C_COUNT; break; }
            const int n = (int)(r.count < nv - done ? r.count : nv - done);
            for (int base = 0; base < n; base += PQ_THREADS, it++) {
                const int j = base + tid;
                const unsigned bit = j < n ? (r.packed ? pq::packed_get(g, r.data, 1, j) : (r.value & 1u)) : 0u;
                const unsigned long long ballot = __ballot(bit != 0);
                if (lane == 0) s_wcnt[it & 1][wave] = __popcll(ballot);
                __syncthreads();
                int before = 0, total = 0;
#pragma unroll
                for (int w = 0; w < PQ_THREADS / 64; w++) { const int c2 = s_wcnt[it & 1][w]; before += w < wave ? c2 : 0; total += c2; }
                if (bit) A.vrow[d.first_row + running + before + __popcll(ballot & ((1ull << lane) - 1))] = done + j;
                if (ballot && lane < 3) {                          // the wave's 64 rows begin at any bit of a bitmap word: up to three words
                    const int64_t R = d.first_row + done + base + wave * 64;
                    const int s = (int)(R & 31);
                    const unsigned piece = lane == 0 ? (unsigned)(ballot << s) : lane == 1 ? (unsigned)(ballot >> (32 - s)) : s ? (unsigned)(ballot >> (64 - s)) : 0u;
                    if (piece) atomicOr(&A.validity[(R >> 5) + lane], piece);
                }
                running += total;
            }
            done += n;
        }
        nvalid = running;
        if (cause != pq::C_OK) {
            if (tid == 0) pq_report(A.err, page, cause);
            return;
        }
        __syncthreads();   // vrow is read below by other lanes than wrote it
    }
    if (tid == 0) atomicAdd(A.nvalid, (unsigned long long)nvalid);
    auto row_of = [&](int k) -> int64_t { return d.first_row + (nullable ? A.vrow[d.first_row + k] : k); };
    auto store = [&](int64_t row, int64_t v) {
        if (KIND == pq::K_INT64 && OUTW == 4 && v != (int32_t)v) { pq_report(A.err, page, pq::C_I32_RANGE); v = 0; }
        if (OUTW == 4) ((int32_t *)A.out)[row] = (int32_t)v;
        else ((int64_t *)A.out)[row] = v;
    };

    // ---- 2. the values
    if constexpr (DELTA) {
        if (d.enc != 0) {                                          // a delta page: header walk, unpack, scan (pq_delta_stream)
            if (nvalid == 0 && d.val_bytes == 0) return;
            DeltaTab *const tab = reinterpret_cast<DeltaTab *>(s_tile);
            int64_t pos = d.val_pos, count = 0;
            const int64_t end = d.val_pos + d.val_bytes;
            if constexpr (KIND == pq::K_BYTES) {
                if (d.enc == pq::E_DELTA_BYTE_ARRAY) {             // a front-coded page: the lengths here, the bytes in dba_expand.hip behind the scan
                    int64_t suf_pos = 0;
                    unsigned long long total = 0;
                    int32_t *const pre = A.dba_pre + d.first_row, *const suf = A.dba_suf + d.first_row;
                    cause = pq::dba_cause(pq_dba_lengths(g, tab, &s_scan, pos, end, nvalid, nvalid, pre, suf, &count, &suf_pos, &total));
                    if (cause != pq::C_OK) {
                        if (tid == 0) pq_report(A.err, page, cause);
                        return;
                    }
                    for (int k = tid; k < nvalid; k += PQ_THREADS) {
                        const int64_t row = row_of(k);
                        // (below 2^32: sum_lengths_kernel reads the lengths as unsigned, so a value of 2^31 bytes or more trips the column's rule)
                        ((int32_t *)A.out)[row] = (int32_t)((uint32_t)pre[k] + (uint32_t)suf[k]);
                        A.sbegin[row] = -1;                        // copy_strings_kernel leaves the row alone
                    }
                    if (tid == 0) A.dba[blockIdx.x] = DbaPage{suf_pos, end - suf_pos, d.first_row, 0, 0, d.first_row, nv, nvalid, 1, 0};
                    return;
                }
                // the lengths, by value; then their exclusive prefix behind the stream's end is where each value's bytes begin
                const int s = pq_delta_stream(g, tab, &s_scan, pos, end, 32, nvalid, nvalid, &count, [&](int64_t k, int64_t v) {
                    if (v < 0) return (int)pq::C_LEN;
                    A.vlen[d.first_row + k] = (int32_t)v;
                    return (int)pq::C_OK;
                });
                cause = s == pq::DS_OK ? pq::C_OK : s == pq::DS_EMIT ? s_scan.flag : pq::delta_cause(s);
                if (cause != pq::C_OK) {
                    if (tid == 0) pq_report(A.err, page, cause);
                    return;
                }
                __syncthreads();   // vlen is read below by other lanes than wrote it
                unsigned long long sum = 0;
                for (int base = 0, it = 0; base < nvalid; base += PQ_THREADS, it++) {
                    const int k = base + tid;
                    const int32_t len = k < nvalid ? A.vlen[d.first_row + k] : 0;
                    unsigned long long total;
                    const unsigned long long incl = pq_scan256((unsigned long long)len, &s_scan, it, &total);
                    if (k < nvalid) {
                        const int64_t row = row_of(k);
                        ((int32_t *)A.out)[row] = len;
                        A.sbegin[row] = pos + (int64_t)(sum + incl) - len;
                    }
                    sum += total;
                }
                if ((int64_t)sum != end - pos && tid == 0) pq_report(A.err, page, (int64_t)sum > end - pos ? pq::C_LEN : pq::C_COUNT);
            } else {
                constexpr int BITS = KIND == pq::K_INT32 ? 32 : 64;
                const int s = pq_delta_stream(g, tab, &s_scan, pos, end, BITS, nvalid, nvalid, &count, [&](int64_t k, int64_t v) {
                    if (KIND == pq::K_INT64 && OUTW == 4 && v != (int32_t)v) return (int)pq::C_I32_RANGE;
                    store(row_of((int)k), v);
                    return (int)pq::C_OK;
                });
                cause = s == pq::DS_OK ? (pos == end ? pq::C_OK : pq::C_COUNT) : s == pq::DS_EMIT ? s_scan.flag : pq::delta_cause(s);
                if (cause != pq::C_OK && tid == 0) pq_report(A.err, page, cause);
            }
            return;
        }
    }
    if (d.dict_n < 0) {
        if constexpr (KIND == pq::K_BYTES) {
            cause = pq_walk_byte_arrays(A.bytes, s_tile, s_state, d.val_pos, d.val_pos + d.val_bytes, nvalid, A.vpos + d.first_row, A.vlen + d.first_row);
            if (cause != pq::C_OK) {
                if (tid == 0) pq_report(A.err, page, cause);
                return;
            }
            for (int k = tid; k < nvalid; k += PQ_THREADS) {
                const int64_t row = row_of(k);
                ((int32_t *)A.out)[row] = A.vlen[d.first_row + k];
                A.sbegin[row] = A.vpos[d.first_row + k];
            }
        } else {
            if ((int64_t)nvalid * A.width != d.val_bytes) {
                if (tid == 0) pq_report(A.err, page, pq::C_COUNT);
                return;
            }
            for (int k = tid; k < nvalid; k += PQ_THREADS) {
                int64_t v = 0;
                const int c = pq::plain_value<KIND>(g, d.val_pos + (int64_t)k * A.width, A.flba_len, &v);
                if (c != pq::C_OK) { pq_report(A.err, page, c); v = 0; }
                store(row_of(k), v);
            }
        }
        return;
    }
    // dictionary indices: bit width, then hybrid runs over the page's nvalid values
    if (nvalid == 0) return;
    if (d.val_bytes < 1) cause = pq::C_COUNT;
    const int bw = cause == pq::C_OK ? g.u8(d.val_pos) : 0;
    if (bw > 32) cause = pq::C_BIT_WIDTH;
    int64_t pos = d.val_pos + 1;
    const int64_t end = d.val_pos + d.val_bytes;
    int done = 0;
    while (cause == pq::C_OK && done < nvalid) {                   // (at most nvalid runs)
        pq::Run r;
        const int c = pq::next_run(g, pos, end, bw, &r);
        if (c != pq::C_OK) { cause = pos >= end ? pq::C_COUNT : c; break; }
        if (!r.packed && r.count > nvalid - done) { cause = pq::C_COUNT; break; }
        const int n = (int)(r.count < nvalid - done ? r.count : nvalid - done);
        for (int j = tid; j < n; j += PQ_THREADS) {
            const uint32_t idx = r.packed ? pq::packed_get(g, r.data, bw, j) : r.value;
            if (idx >= (uint32_t)d.dict_n) { pq_report(A.err, page, pq::C_INDEX); continue; }
            const int64_t row = row_of(done + j);
            if constexpr (KIND == pq::K_BYTES) {
                ((int32_t *)A.out)[row] = A.dlen[d.dict_base + idx];
                A.sbegin[row] = A.dpos[d.dict_base + idx];
            } else {
                int64_t v = 0;
                const int c2 = pq::plain_value<KIND>(g, d.dict_pos + (int64_t)idx * A.width, A.flba_len, &v);
                if (c2 != pq::C_OK) { pq_report(A.err, page, c2); v = 0; }
                store(row, v);
            }
        }
        done += n;
    }
    if (cause != pq::C_OK && tid == 0) pq_report(A.err, page, cause);
}

}  // namespace ph

namespace {

using ph::pq::ColPlan;
using ph::pq::FileMeta;
using ph::pq::PageDesc;
using ph::pq::Status;

int fail(const char *who, const Status &st) {
    ph::set_error("%s: %s", who, st.msg.c_str());
    return st.code;
}

// control block of a call on the device
struct PqControl {
    unsigned long long err;          // lowest (page << 8 | cause); all ones = none
    unsigned long long scan_total;
    unsigned long long count;        // encode_strings' counters
    unsigned long long per_col[1];   // str_bytes[ncols], then nvalid[ncols]
};

}  // namespace

extern "C" int ph_parquet_schema(const void *file, int64_t nbytes, int64_t *nrows, int32_t *nrow_groups, ph_parquet_colinfo *info, int32_t cap,
                                 int32_t *ncols) {
    PH_REQUIRE(file && nbytes >= 0 && ncols && cap >= 0 && (cap == 0 || info), "ph_parquet_schema: bad arguments");
    FileMeta fm;
    Status st;
    if (ph::pq::parse_footer((const uint8_t *)file, nbytes, &fm, &st) != PH_OK) return fail("ph_parquet_schema", st);
    if (nrows) *nrows = fm.num_rows;
    if (nrow_groups) *nrow_groups = (int32_t)fm.groups.size();
    *ncols = (int32_t)fm.leaves.size();
    for (int32_t i = 0; i < cap && i < *ncols; i++) {
        const ph::pq::Leaf &l = fm.leaves[(size_t)i];
        const bool flat = l.max_rep == 0 && l.max_def <= 1;
        info[i] = ph_parquet_colinfo{l.name_pos, (int32_t)l.name_len, l.phys, l.type_length, flat ? l.ph_type : 0, flat ? l.ph_scale : 0, l.max_def > 0 ? 1 : 0};
    }
    return PH_OK;
}

namespace {

int parquet_pages(const char *who, uint32_t dir_flags, const void *file, int64_t nbytes, int32_t column, ph_parquet_page *pages, ph_parquet_page_codec *codecs,
                  int32_t cap, int32_t *npages) {
    PH_REQUIRE(file && nbytes >= 0 && npages && cap >= 0 && (cap == 0 || pages), "%s: bad arguments", who);
    FileMeta fm;
    Status st;
    if (ph::pq::parse_footer((const uint8_t *)file, nbytes, &fm, &st) != PH_OK) return fail(who, st);
    PH_REQUIRE(column >= 0 && column < (int32_t)fm.leaves.size(), "%s: column %d: the file's schema has %zu leaf columns", who, column, fm.leaves.size());
    std::vector<ph::pq::Page> dir;
    const std::string what = "column " + std::to_string(column) + " (" + ph::pq::leaf_name((const uint8_t *)file, fm.leaves[(size_t)column]) + ")";
    if (ph::pq::page_directory((const uint8_t *)file, nbytes, fm, column, what.c_str(), &dir, &st, dir_flags) != PH_OK) return fail(who, st);
    *npages = (int32_t)dir.size();
    for (int32_t i = 0; i < cap && i < *npages; i++) {
        const ph::pq::Page &p = dir[(size_t)i];
        pages[i] = ph_parquet_page{p.row_group, p.kind, p.encoding, p.num_values, p.first_row, p.header_pos, p.data_pos, p.data_bytes, p.rep_bytes, p.def_bytes};
        if (codecs) codecs[i] = ph_parquet_page_codec{p.codec, p.compressed, p.uncompressed_bytes};
    }
    return PH_OK;
}

}  // namespace

extern "C" int ph_parquet_pages(const void *file, int64_t nbytes, int32_t column, ph_parquet_page *pages, int32_t cap, int32_t *npages) {
    return parquet_pages("ph_parquet_pages", 0, file, nbytes, column, pages, nullptr, cap, npages);
}

extern "C" int ph_parquet_pages_ex(const void *file, int64_t nbytes, int32_t column, ph_parquet_page *pages, ph_parquet_page_codec *codecs, int32_t cap,
                                   int32_t *npages) {
    return parquet_pages("ph_parquet_pages_ex", ph::pq::DIR_LIST_ONLY, file, nbytes, column, pages, codecs, cap, npages);
}

extern "C" int ph_parquet_read_column_host(const void *file, int64_t nbytes, const ph_parquet_col *col, int64_t *values, uint8_t *valid,
                                           int32_t *str_offsets, char *str_bytes, int64_t str_cap, int64_t *str_total) {
    return ph_parquet_read_column_host_ex(file, nbytes, col, 0, values, valid, str_offsets, str_bytes, str_cap, str_total);
}

extern "C" int ph_parquet_read_column_host_ex(const void *file, int64_t nbytes, const ph_parquet_col *col, uint32_t flags, int64_t *values, uint8_t *valid,
                                              int32_t *str_offsets, char *str_bytes, int64_t str_cap, int64_t *str_total) {
    PH_REQUIRE(file && nbytes >= 0 && col && str_cap >= 0, "ph_parquet_read_column_host: bad arguments");
    PH_REQUIRE((flags & ~(PH_PARQUET_SNAPPY | PH_PARQUET_DELTA | PH_PARQUET_DELTA_BYTE_ARRAY | PH_PARQUET_LZ4_RAW | PH_PARQUET_GZIP | PH_PARQUET_ZSTD)) == 0,
               "ph_parquet_read_column_host: flags %#x: only PH_PARQUET_SNAPPY, PH_PARQUET_DELTA, PH_PARQUET_DELTA_BYTE_ARRAY, PH_PARQUET_LZ4_RAW, PH_PARQUET_GZIP and PH_PARQUET_ZSTD are defined", flags);
    FileMeta fm;
    Status st;
    ColPlan cp;
    if (ph::pq::parse_footer((const uint8_t *)file, nbytes, &fm, &st) != PH_OK) return fail("ph_parquet_read_column_host", st);
    if (ph::pq::resolve_column((const uint8_t *)file, nbytes, fm, col->column, col->type, col->scale, &cp, &st, flags) != PH_OK) return fail("ph_parquet_read_column_host", st);
    PH_REQUIRE(fm.num_rows < (1ll << 31), "ph_parquet_read_column_host: %lld rows exceed the int32 row-id domain", (long long)fm.num_rows);
    PH_REQUIRE(cp.kind == ph::pq::K_BYTES ? str_offsets != nullptr : values != nullptr, "ph_parquet_read_column_host: %s: no output buffer for its values", cp.what.c_str());
    if (ph::pq::decode_column_host((const uint8_t *)file, cp, fm.num_rows, values, valid, str_offsets, str_bytes, str_cap, str_total, &st) != PH_OK)
        return fail("ph_parquet_read_column_host", st);
    return PH_OK;
}

extern "C" int ph_delta_decode_host(const void *src, int64_t *dst, ph_delta_stream *s) {
    PH_REQUIRE(s && s->src_pos >= 0 && s->src_bytes >= 0 && (src || s->src_bytes == 0) && s->dst_pos >= 0 && s->dst_cap >= 0 && (dst || s->dst_cap == 0) &&
               s->expected >= -1 && (s->bits == 32 || s->bits == 64), "ph_delta_decode_host: bad arguments");
    const ph::pq::HostBytes g((const uint8_t *)src);
    int64_t pos = s->src_pos, count = 0;
    const int64_t end = s->src_pos + s->src_bytes;
    int emit_cause = 0;
    int sub = ph::pq::host_delta_stream(g, pos, end, s->bits, s->expected, s->dst_cap, &count, &emit_cause, [&](int64_t k, int64_t v) { dst[s->dst_pos + k] = v; return 0; });
    if (sub == ph::pq::DS_OK && s->exact && pos != end) sub = ph::pq::DS_TRAILING;
    s->count = count;
    s->consumed = sub == ph::pq::DS_OK ? pos - s->src_pos : 0;
    s->sub = sub;
    s->status = sub == ph::pq::DS_OK ? PH_OK : sub == ph::pq::DS_CAPACITY ? PH_ECAPACITY : ph::pq::cause_code(ph::pq::delta_cause(sub));
    if (sub == ph::pq::DS_CAPACITY) ph::set_error("ph_delta_decode_host: the stream holds %lld values, the destination %lld", (long long)count, (long long)s->dst_cap);
    else if (sub != ph::pq::DS_OK) ph::set_error("ph_delta_decode_host: a DELTA_BINARY_PACKED stream of %lld bytes: %s", (long long)s->src_bytes, ph::pq::delta_sub_text(sub));
    return s->status;
}

extern "C" int ph_delta_decode(ph_ctx *ctx, const void *src_dev, void *dst_dev, ph_delta_stream *streams, int32_t n) {
    PH_REQUIRE(ctx && n >= 0 && (n == 0 || (src_dev && dst_dev && streams)), "ph_delta_decode: bad arguments");
    if (n == 0) return PH_OK;
    for (int32_t i = 0; i < n; i++) {
        const ph_delta_stream &s = streams[i];
        PH_REQUIRE(s.src_pos >= 0 && s.src_bytes >= 0 && s.dst_pos >= 0 && s.dst_cap >= 0 && s.expected >= -1 && (s.bits == 32 || s.bits == 64),
                   "ph_delta_decode: stream %d: a negative position or length, or bits other than 32 and 64", i);
    }
    PH_HIP(hipSetDevice(ctx->device));
    ph::Temps tmp;
    tmp.who = "ph_delta_decode";
    ph_delta_stream *streams_dev = nullptr;
    PH_CHECK(tmp.alloc((void **)&streams_dev, (int64_t)n * (int64_t)sizeof(ph_delta_stream)));
    PH_CHECK(ph_dev_upload(ctx, streams_dev, streams, (int64_t)n * (int64_t)sizeof(ph_delta_stream)));
    ph::pq_delta_raw_kernel<<<(unsigned)n, ph::PQ_THREADS, 0, ctx->stream>>>((const uint8_t *)src_dev, (int64_t *)dst_dev, streams_dev);
    PH_HIP(hipGetLastError());
    PH_CHECK(ctx->download(streams, streams_dev, (int64_t)n * (int64_t)sizeof(ph_delta_stream)));
    for (int32_t i = 0; i < n; i++) {
        const int sub = streams[i].sub;
        streams[i].status = sub == ph::pq::DS_OK ? PH_OK : sub == ph::pq::DS_CAPACITY ? PH_ECAPACITY : ph::pq::cause_code(ph::pq::delta_cause(sub));
    }
    return PH_OK;
}

namespace {

bool dba_stream_ok(const ph_dba_stream &s) {
    return s.src_pos >= 0 && s.src_bytes >= 0 && s.expected >= -1 && s.len_pos >= 0 && s.len_cap >= 0 && s.len_cap < (1ll << 31) && s.byte_pos >= 0 && s.byte_cap >= 0;
}

}  // namespace

extern "C" int ph_delta_byte_array_decode_host(const void *src, int32_t *lens, char *bytes, ph_dba_stream *s) {
    PH_REQUIRE(s && dba_stream_ok(*s) && (src || s->src_bytes == 0) && (lens || s->len_cap == 0) && (bytes || s->byte_cap == 0), "ph_delta_byte_array_decode_host: bad arguments");
    const int sub = ph::pq::host_dba_section((const uint8_t *)src, s, lens, bytes);
    if (sub != ph::pq::DBA_OK) ph::set_error("ph_delta_byte_array_decode_host: a DELTA_BYTE_ARRAY section of %lld bytes: %s", (long long)s->src_bytes, ph::pq::dba_sub_text(sub).c_str());
    return s->status;
}

extern "C" int ph_delta_byte_array_decode(ph_ctx *ctx, const void *src_dev, void *lens_dev, void *bytes_dev, ph_dba_stream *streams, int32_t n) {
    PH_REQUIRE(ctx && n >= 0 && (n == 0 || (src_dev && lens_dev && bytes_dev && streams)), "ph_delta_byte_array_decode: bad arguments");
    if (n == 0) return PH_OK;
    std::vector<int64_t> val0((size_t)n);
    int64_t values = 0;
    for (int32_t i = 0; i < n; i++) {
        PH_REQUIRE(dba_stream_ok(streams[i]), "ph_delta_byte_array_decode: stream %d: a negative position, length or room, or room for 2^31 or more lengths", i);
        val0[(size_t)i] = values;
        values += streams[i].len_cap;
    }
    PH_HIP(hipSetDevice(ctx->device));
    ph::Temps tmp;
    tmp.who = "ph_delta_byte_array_decode";
    ph_dba_stream *streams_dev = nullptr;
    int64_t *val0_dev = nullptr;
    int32_t *pre = nullptr, *suf = nullptr;
    ph::DbaPage *pages = nullptr;
    PH_CHECK(tmp.alloc((void **)&streams_dev, (int64_t)n * (int64_t)sizeof(ph_dba_stream)));
    PH_CHECK(tmp.alloc((void **)&val0_dev, (int64_t)n * 8));
    PH_CHECK(tmp.alloc((void **)&pre, (values + 1) * 4));   // (the per-value temporaries: sized by the callers' rooms)
    PH_CHECK(tmp.alloc((void **)&suf, (values + 1) * 4));
    PH_CHECK(tmp.alloc((void **)&pages, (int64_t)n * (int64_t)sizeof(ph::DbaPage)));
    PH_CHECK(ph_dev_upload(ctx, streams_dev, streams, (int64_t)n * (int64_t)sizeof(ph_dba_stream)));
    PH_CHECK(ph_dev_upload(ctx, val0_dev, val0.data(), (int64_t)n * 8));
    PH_HIP(hipMemsetAsync(pages, 0, (size_t)n * sizeof(ph::DbaPage), ctx->stream));
    ph::pq_dba_raw_kernel<<<(unsigned)n, ph::PQ_THREADS, 0, ctx->stream>>>((const uint8_t *)src_dev, (int32_t *)lens_dev, streams_dev, val0_dev, pre, suf, pages);
    PH_HIP(hipGetLastError());
    PH_CHECK(ph::dba_expand_pages(ctx, ph::DbaArgs{(const uint8_t *)src_dev, (uint8_t *)bytes_dev, nullptr, pages, pre, suf, nullptr}, n));
    PH_CHECK(ctx->download(streams, streams_dev, (int64_t)n * (int64_t)sizeof(ph_dba_stream)));
    for (int32_t i = 0; i < n; i++) {
        const int sub = streams[i].sub;
        streams[i].status = ph::pq::dba_status(sub);
        if (sub != ph::pq::DBA_OK && sub != ph::pq::DBA_2G && sub != ph::pq::DBA_BYTE_CAP) streams[i].total_bytes = 0;
    }
    return PH_OK;
}

extern "C" int ph_table_create_parquet(ph_ctx *ctx, const void *file, int64_t nbytes, const ph_parquet_col *cols, int32_t ncols, ph_table **out) {
    return ph_table_create_parquet_ex(ctx, file, nbytes, cols, ncols, 0, out);
}

extern "C" int ph_table_create_parquet_ex(ph_ctx *ctx, const void *file_, int64_t nbytes, const ph_parquet_col *cols, int32_t ncols, uint32_t flags,
                                          ph_table **out) {
    static const char *const who = "ph_table_create_parquet";
    PH_REQUIRE(ctx && out && file_ && nbytes >= 0 && ncols >= 0 && ncols < 65535 && (cols || ncols == 0), "ph_table_create_parquet: bad arguments");
    PH_REQUIRE((flags & ~(PH_PARQUET_SNAPPY | PH_PARQUET_DELTA | PH_PARQUET_DELTA_BYTE_ARRAY | PH_PARQUET_LZ4_RAW | PH_PARQUET_GZIP | PH_PARQUET_ZSTD)) == 0,
               "ph_table_create_parquet: flags %#x: only PH_PARQUET_SNAPPY, PH_PARQUET_DELTA, PH_PARQUET_DELTA_BYTE_ARRAY, PH_PARQUET_LZ4_RAW, PH_PARQUET_GZIP and PH_PARQUET_ZSTD are defined", flags);
    const uint8_t *file = (const uint8_t *)file_;
    FileMeta fm;
    Status st;
    if (ph::pq::parse_footer(file, nbytes, &fm, &st) != PH_OK) return fail(who, st);
    std::vector<ph_parquet_col> want;
    if (cols && ncols > 0) want.assign(cols, cols + ncols);
    else for (size_t i = 0; i < fm.leaves.size(); i++) want.push_back(ph_parquet_col{(int32_t)i, 0, 0});
    ncols = (int32_t)want.size();
    PH_REQUIRE(ncols > 0, "ph_table_create_parquet: the file's schema has no columns");
    std::vector<ColPlan> plans((size_t)ncols);
    for (int32_t k = 0; k < ncols; k++)
        if (ph::pq::resolve_column(file, nbytes, fm, want[(size_t)k].column, want[(size_t)k].type, want[(size_t)k].scale, &plans[(size_t)k], &st, flags) != PH_OK) return fail(who, st);
    const int64_t nrows = fm.num_rows;
    PH_REQUIRE(nrows < (1ll << 31), "ph_table_create_parquet: %lld rows exceed the int32 row-id domain", (long long)nrows);
    if (nrows == 0) {   // an empty table, as ph_table_create builds it
        const int64_t zero[2] = {0, 0};
        std::vector<ph_col> hc((size_t)ncols);
        for (int32_t k = 0; k < ncols; k++) {
            const ColPlan &cp = plans[(size_t)k];
            hc[(size_t)k] = ph_col{};
            hc[(size_t)k].type = cp.out_type == PH_STR ? PH_CODE8 : cp.out_type;
            hc[(size_t)k].scale = cp.out_type == PH_DEC64 ? cp.out_scale : 0;
            hc[(size_t)k].data = zero;
            if (cp.out_type == PH_STR) hc[(size_t)k].aux = "";
        }
        return ph_table_create(ctx, ncols, hc.data(), 0, out);
    }
    PH_HIP(hipSetDevice(ctx->device));
    ph::Temps tmp;
    tmp.who = who;

    // ---- the requested columns' chunks, one behind the other (16-byte aligned), and the pages rebased onto the upload
    struct Range { int64_t file_pos, bytes, dev_pos; };
    std::vector<Range> ranges;
    std::vector<PageDesc> all;                       // per column: its dictionary pages (BYTE_ARRAY), then its data pages
    std::vector<int32_t> col_first((size_t)ncols + 1), col_ndict((size_t)ncols), col_tail((size_t)ncols);
    std::vector<std::vector<int64_t>> deltas((size_t)ncols);
    int64_t dev_bytes = 0;
    bool any_nullable = false, any_bytes = false;
    for (int32_t k = 0; k < ncols; k++) {
        const ColPlan &cp = plans[(size_t)k];
        std::vector<int64_t> &delta = deltas[(size_t)k];
        delta.resize(fm.groups.size());
        for (size_t g = 0; g < fm.groups.size(); g++) {
            const ph::pq::Chunk &c = fm.groups[g].chunks[(size_t)cp.column];
            if (fm.groups[g].num_rows == 0) continue;
            ranges.push_back(Range{c.start(), c.total_compressed, dev_bytes});
            delta[g] = dev_bytes - c.start();
            dev_bytes = ph::round_up(dev_bytes + c.total_compressed, 16);
        }
    }
    // the region of decompressed sections lies behind the chunks, column by column; its size is bounded by 22 x (SNAPPY), 255 x (LZ4_RAW), 1032 x (GZIP) or 32768 x (ZSTD)
    // the file's (page_directory). One list per codec (a row of parquet_codecs.h's table): each is one launch.
    std::vector<ph::SnSection> sections[ph::pq::N_CODECS];         // (page kernels of a column never run over its tail: fixed-width dictionary pages, listed for the error key only)
    for (int32_t k = 0; k < ncols; k++) {
        const ColPlan &cp = plans[(size_t)k];
        const std::vector<int64_t> &delta = deltas[(size_t)k];
        const int64_t zbase = dev_bytes;
        dev_bytes += cp.z_bytes;
        auto rebase = [&](PageDesc d) {
            const int64_t dl = delta[(size_t)d.row_group];
            auto at = [&](int64_t p) { return p >= ph::pq::Z_BASE ? p - ph::pq::Z_BASE + zbase : p + dl; };
            d.val_pos = at(d.val_pos);
            if (d.lvl_bytes >= 0) d.lvl_pos = at(d.lvl_pos);
            if (d.dict_n >= 0) d.dict_pos = at(d.dict_pos);
            return d;
        };
        col_first[(size_t)k] = (int32_t)all.size();
        col_ndict[(size_t)k] = (int32_t)cp.dicts.size();
        for (const PageDesc &d : cp.dicts) all.push_back(rebase(d));
        for (const PageDesc &d : cp.pages) all.push_back(rebase(d));
        for (const ph::pq::Section &s : cp.sections) {
            ph::SnSection x{s.src_pos + delta[(size_t)s.row_group], s.src_bytes, zbase + s.out_pos, s.out_bytes, -1, -1, s.v1_levels, 0};
            if (s.owner == 2) {
                PageDesc d{};
                d.row_group = s.row_group;
                d.page = s.page;
                x.key = (int32_t)all.size();
                all.push_back(d);
                col_tail[(size_t)k]++;
            } else x.key = x.desc = col_first[(size_t)k] + (s.owner == 0 ? col_ndict[(size_t)k] : 0) + s.index;
            sections[ph::pq::codec_row(s.codec)].push_back(x);
        }
        any_nullable |= cp.nullable;
        any_bytes |= cp.kind == ph::pq::K_BYTES;
    }
    col_first[(size_t)ncols] = (int32_t)all.size();
    for (const std::vector<ph::SnSection> &list : sections) PH_REQUIRE(list.size() < (1u << 31), "ph_table_create_parquet: 2^31 or more compressed pages");
    uint8_t *dbytes = nullptr;
    PH_CHECK(tmp.alloc((void **)&dbytes, dev_bytes + ph::PQ_TILE + 32));
    for (const Range &r : ranges)
        if (r.bytes > 0) PH_CHECK(ph_dev_upload(ctx, dbytes + r.dev_pos, file + r.file_pos, r.bytes));
    PageDesc *pages_dev = nullptr;
    PH_CHECK(tmp.alloc((void **)&pages_dev, (int64_t)(all.size() + 1) * (int64_t)sizeof(PageDesc)));
    if (!all.empty()) PH_CHECK(ph_dev_upload(ctx, pages_dev, all.data(), (int64_t)all.size() * (int64_t)sizeof(PageDesc)));

    const int64_t ctl_bytes = (int64_t)offsetof(PqControl, per_col) + (int64_t)ncols * 16;
    std::vector<char> ctl_host((size_t)ctl_bytes, 0);
    PqControl *ctl = (PqControl *)ctl_host.data();
    ctl->err = ~0ull;
    char *ctl_dev = nullptr;
    PH_CHECK(tmp.alloc((void **)&ctl_dev, ctl_bytes));
    PH_CHECK(ph_dev_upload(ctx, ctl_dev, ctl_host.data(), ctl_bytes));
    unsigned long long *err_dev = (unsigned long long *)(ctl_dev + offsetof(PqControl, err));
    int64_t *total_dev = (int64_t *)(ctl_dev + offsetof(PqControl, scan_total));
    unsigned long long *str_bytes_dev = (unsigned long long *)(ctl_dev + offsetof(PqControl, per_col));
    unsigned long long *nvalid_dev = str_bytes_dev + ncols;

    // ---- every compressed section of the call, in one launch per codec present, in front of the first column's kernels
    static constexpr ph::SectionLaunch launches[] = {ph::snappy_decompress_sections, ph::lz4_decompress_sections, ph::gzip_decompress_sections, ph::zstd_decompress_sections};   // CODECS' rows
    static_assert(sizeof launches / sizeof launches[0] == ph::pq::N_CODECS && ph::pq::CODECS[0].id == 1 && ph::pq::CODECS[1].id == 7 && ph::pq::CODECS[2].id == 2 && ph::pq::CODECS[3].id == 6, "a launch per codec, in the table's order");
    for (int c = 0; c < ph::pq::N_CODECS; c++) {
        const std::vector<ph::SnSection> &list = sections[c];
        if (list.empty()) continue;
        ph::SnSection *sections_dev = nullptr;
        PH_CHECK(tmp.alloc((void **)&sections_dev, (int64_t)list.size() * (int64_t)sizeof(ph::SnSection)));
        PH_CHECK(ph_dev_upload(ctx, sections_dev, list.data(), (int64_t)list.size() * (int64_t)sizeof(ph::SnSection)));
        PH_CHECK(launches[c](ctx, dbytes, dbytes, sections_dev, (int32_t)list.size(), pages_dev, err_dev, nullptr));
    }

    // ---- the table's columns; temporaries shared by the columns (their kernels run one behind the other on the stream)
    ph::TableGuard guard;
    ph_table *t = guard.t = new ph_table();
    t->ctx = ctx;
    t->nrows = nrows;
    t->cols.resize((size_t)ncols);
    const int64_t padded = ph::round_up(nrows, PH_ROW_PAD);
    int32_t *vrow = nullptr, *vlen = nullptr;
    int64_t *vpos = nullptr;
    if (any_nullable) PH_CHECK(tmp.alloc((void **)&vrow, nrows * 4));
    if (any_bytes) { PH_CHECK(tmp.alloc((void **)&vlen, nrows * 4)); PH_CHECK(tmp.alloc((void **)&vpos, nrows * 8)); }
    std::vector<int64_t *> sbegin((size_t)ncols, nullptr);
    struct Front { int32_t *pre = nullptr, *suf = nullptr; ph::DbaPage *pages = nullptr; int32_t npages = 0; };   // a column with front-coded pages
    std::vector<Front> front((size_t)ncols);
    for (int32_t k = 0; k < ncols; k++) {
        const ColPlan &cp = plans[(size_t)k];
        ph_table::column &d = t->cols[(size_t)k];
        d.type = cp.out_type;
        d.scale = cp.out_type == PH_DEC64 ? cp.out_scale : 0;
        const bool str = cp.kind == ph::pq::K_BYTES;
        const int w = str ? 4 : ph::type_width(d.type);
        const int64_t bytes = str ? (padded + 1) * 4 : padded * w;
        PH_HIP(hipMalloc(&d.data, (size_t)bytes));
        if (cp.nullable || str) PH_HIP(hipMemsetAsync(d.data, 0, (size_t)bytes, ctx->stream));   // a NULL row keeps its zero
        else PH_HIP(hipMemsetAsync((char *)d.data + nrows * w, 0, (size_t)((padded - nrows) * w), ctx->stream));
        if (cp.nullable) {
            PH_HIP(hipMalloc((void **)&d.validity, (size_t)(padded / 8)));
            PH_HIP(hipMemsetAsync(d.validity, 0, (size_t)(padded / 8), ctx->stream));
        }
        ph::PqColArgs A{};
        A.bytes = dbytes;
        A.flba_len = cp.flba_len;
        A.width = cp.width;
        A.out = d.data;
        A.validity = (unsigned *)d.validity;
        A.vrow = vrow;
        A.vpos = vpos;
        A.vlen = vlen;
        A.err = err_dev;
        A.nvalid = nvalid_dev + k;
        if (str) {
            PH_CHECK(tmp.alloc((void **)&sbegin[(size_t)k], nrows * 8));
            PH_HIP(hipMemsetAsync(sbegin[(size_t)k], 0, (size_t)(nrows * 8), ctx->stream));
            A.sbegin = sbegin[(size_t)k];
            if (cp.dict_entries > 0) {
                PH_CHECK(tmp.alloc((void **)&A.dpos, cp.dict_entries * 8));
                PH_CHECK(tmp.alloc((void **)&A.dlen, cp.dict_entries * 4));
            }
            if (col_ndict[(size_t)k] > 0) {
                A.pages = pages_dev + col_first[(size_t)k];
                A.page0 = col_first[(size_t)k];
                ph::pq_dict_walk_kernel<<<(unsigned)col_ndict[(size_t)k], ph::PQ_THREADS, 0, ctx->stream>>>(A);
                PH_HIP(hipGetLastError());
            }
        }
        A.page0 = col_first[(size_t)k] + col_ndict[(size_t)k];
        A.pages = pages_dev + A.page0;
        const unsigned grid = (unsigned)(col_first[(size_t)k + 1] - col_tail[(size_t)k] - A.page0);
        if (grid == 0) continue;
        if (str && std::any_of(cp.pages.begin(), cp.pages.end(), [](const PageDesc &p) { return p.enc == ph::pq::E_DELTA_BYTE_ARRAY; })) {
            // (per column, not shared: the reconstruction reads them behind the other columns' page kernels. Sized by rows, not by the stream.)
            Front &f = front[(size_t)k];
            f.npages = (int32_t)grid;
            PH_CHECK(tmp.alloc((void **)&f.pre, nrows * 4));
            PH_CHECK(tmp.alloc((void **)&f.suf, nrows * 4));
            PH_CHECK(tmp.alloc((void **)&f.pages, (int64_t)grid * (int64_t)sizeof(ph::DbaPage)));
            PH_HIP(hipMemsetAsync(f.pages, 0, (size_t)grid * sizeof(ph::DbaPage), ctx->stream));
            A.dba_pre = f.pre;
            A.dba_suf = f.suf;
            A.dba = f.pages;
        }
        ph::dispatch_int<ph::pq::K_INT32, ph::pq::K_INT64, ph::pq::K_FLBA, ph::pq::K_BYTES>(cp.kind, [&](auto KIND) {
            ph::dispatch_int<4, 8>(w, [&](auto OUTW) {
                if constexpr (KIND() == ph::pq::K_BYTES && OUTW() == 8) return;                    // (lengths are int32)
                else if constexpr (KIND() == ph::pq::K_FLBA && OUTW() == 4) return;                // (a decimal is int64)
                else ph::pq_page_kernel<KIND(), OUTW()><<<grid, ph::PQ_THREADS, 0, ctx->stream>>>(A);
            });
        });
        PH_HIP(hipGetLastError());
        if (str) {
            ph::sum_lengths_kernel<<<ph::load_grid_for(ctx, nrows), 256, 0, ctx->stream>>>((const int32_t *)d.data, nrows, str_bytes_dev + k);
            PH_HIP(hipGetLastError());
        }
    }
    PH_CHECK(ctx->download(ctl_host.data(), ctl_dev, ctl_bytes));
    if (ctl->err != ~0ull) {
        const int page = (int)(ctl->err >> 8), cause = (int)(ctl->err & 0xff);
        int32_t k = 0;
        while (k + 1 < ncols && page >= col_first[(size_t)k + 1]) k++;
        const PageDesc &d = all[(size_t)page];
        if (cause == ph::pq::C_LVL_SECTION) {   // the message of a raw page's check: the length the kernel met is in the emptied PageDesc
            PageDesc seen{};
            PH_CHECK(ctx->download(&seen, pages_dev + page, (int64_t)sizeof(PageDesc)));
            long long bytes = 0;
            for (const ph::pq::Section &s : plans[(size_t)k].sections)
                if (s.page == d.page) bytes = (long long)s.out_bytes;
            ph::pq::level_section_error(&st, plans[(size_t)k].what.c_str(), d.row_group, d.page, (uint32_t)seen.dict_bytes, bytes);
            return fail(who, st);
        }
        ph::set_error("%s: %s: row group %d, page %d: %s", who, plans[(size_t)k].what.c_str(), d.row_group, d.page, ph::pq::cause_text(cause));
        return ph::pq::cause_code(cause);
    }
    const unsigned long long *str_bytes = ctl->per_col, *nvalid = ctl->per_col + ncols;
    for (int32_t k = 0; k < ncols; k++)
        PH_REQUIRE(plans[(size_t)k].kind != ph::pq::K_BYTES || str_bytes[k] < (1ull << 31), "ph_table_create_parquet: %s holds %llu string bytes (int32 offsets)",
                   plans[(size_t)k].what.c_str(), str_bytes[k]);

    // ---- a column without a NULL has no bitmap; VARCHAR: offsets, bytes, encoding
    for (int32_t k = 0; k < ncols; k++) {
        ph_table::column &d = t->cols[(size_t)k];
        if (d.validity && nvalid[k] == (unsigned long long)nrows) {
            PH_HIP(hipStreamSynchronize(ctx->stream));
            (void)hipFree(d.validity);
            d.validity = nullptr;
        }
        if (plans[(size_t)k].kind != ph::pq::K_BYTES) continue;
        PH_CHECK(ph::exclusive_scan_i32(ctx, (int32_t *)d.data, nrows + 1, total_dev));
        d.aux_bytes = (int64_t)str_bytes[k];
        PH_HIP(hipMalloc(&d.aux, (size_t)(d.aux_bytes + 64)));
        const Front &f = front[(size_t)k];
        if (f.npages) ph::copy_strings_kernel<false, true><<<(unsigned)((nrows + 255) / 256), 256, 0, ctx->stream>>>(dbytes, sbegin[(size_t)k], (const int32_t *)d.data, nrows, (unsigned char *)d.aux);
        else ph::copy_strings_kernel<false><<<(unsigned)((nrows + 255) / 256), 256, 0, ctx->stream>>>(dbytes, sbegin[(size_t)k], (const int32_t *)d.data, nrows, (unsigned char *)d.aux);
        PH_HIP(hipGetLastError());
        if (f.npages)   // the front-coded pages' bytes, at the offset of each page's first row: known only now
            PH_CHECK(ph::dba_expand_pages(ctx, ph::DbaArgs{dbytes, (uint8_t *)d.aux, (const int32_t *)d.data, f.pages, f.pre, f.suf, nullptr}, f.npages));
        PH_CHECK(ph::encode_strings(ctx, d, nrows, padded, (unsigned *)(ctl_dev + offsetof(PqControl, count)), tmp, d.validity));
    }

    // ---- the upload and the temporaries go; the shared finishing
    PH_HIP(hipStreamSynchronize(ctx->stream));
    tmp.release();
    for (int32_t k = 0; k < ncols; k++) PH_CHECK(ph::table_finish_column(ctx, t->cols[(size_t)k], nrows, padded, nullptr, 0));
    ph::register_table(t);
    guard.t = nullptr;
    *out = t;
    return PH_OK;
}
