// ORDER BY on the device: ph_sort_rows.
//
// Replaces LocalSort.SinkChunk / Sort for fixed-size keys (reference pkg/compute/sort_local.go:64-250,
// key layout sort_layout.go:29-88, encoders sort_encoder.go:33-114, RadixScatter
// sort_radix.go:242-380): every ORDER BY column becomes a byte-comparable key —
//   [1 byte: 0 = NULL, 1 = value (the reference always sorts NULLs first, sort_layout.go:46)]
//   [value bytes, big-endian, sign bit flipped; all value bytes inverted for DESC]
//   INTEGER: 4 bytes; DATE: (year, month, day) = the order of the day number; DECIMAL:
//   dec.Int64(2) -> (whole, frac): the value ROUNDED half-even to two decimals (a reference
//   quirk: finer decimals compare equal when they round to the same cents)
// and rows are ordered by memcmp of the concatenated keys. Ties keep no defined order in the
// reference (its radix/pdq sort is not stable); here they keep their input order.
//
// Device form: each column is normalised to an unsigned 64-bit word with the same order (value
// XOR sign bit, inverted for DESC; 0 for NULL) plus the NULL flag, and the permutation is sorted
// column by column from the LAST ORDER BY column to the first with stable LSD radix passes over
// the bytes that actually vary (an OR-reduction of key XOR first key finds them: a date column
// needs two passes, a constant column none). A pass is histogram -> scan -> stable scatter of
// (key word, row word) pairs; the row word carries the column's NULL flag in bit 31, which is the
// most significant digit of the column.
//
// VARCHAR keys (PH_STR; the reference's RadixScatterStringVector sort_radix.go:728-805 + the full
// compare of tied prefixes :180-230, CompareVal :898-933) order as bytes.Compare. Word j of a string
// is its bytes 8j..8j+7 read big-endian, zero-padded past the end. Round 0 sorts the column by
// (NULL flag, word 0) exactly as above. Refinement round j >= 1 takes only the rows of segments (runs
// of rows tied so far) of two or more rows whose strings go on past the words compared, compacts them
// in position order and sorts them stably by (segment id, word j, e_j) with the same passes over a
// two-word key, where e_j = min(len - 8(j-1), 17) is the length as the last component (a tied row with
// fewer bytes left is a prefix of the other; e_j = 17: bytes remain after word j, the tie goes on).
// Segments are contiguous, so the sorted rows go back to the positions they came from. DESC inverts
// the words and e_j; the NULL flag is not inverted. One read-back per round sizes the next one.
#include <algorithm>

#include "common.h"
#include "device_util.h"
#include "ops.h"

namespace ph {

constexpr int SORT_TILE = 256;          // rows ranked together (one per thread, in order)
constexpr int SORT_TILES_PER_WG = 16;   // consecutive tiles of a workgroup's chunk

struct SortCol {
    int type;       // PH_I32 / PH_DATE / PH_CODE8 / PH_DEC64 / PH_STR
    int scale;      // DEC64
    const void *data;        // PH_STR: int32 offsets[rows+1]
    const uint8_t *validity;
    int descending;
    const uint8_t *bytes;    // PH_STR
    int64_t nbytes;
};

// word j of row r's string: bytes 8j..8j+7 big-endian, zero past the end; *len = the string's length. Two aligned 8-byte loads
// (funnel-shifted, masked to the string, byte-swapped) when the byte buffer is 8-byte aligned and both words lie inside it; byte
// loads otherwise.
__device__ __forceinline__ unsigned long long str_word(const int32_t *__restrict__ off, const uint8_t *__restrict__ bytes, int64_t nbytes,
                                                       int64_t r, int j, int *len) {
    const int64_t s = off[r];
    const int l = off[r + 1] - (int)s;
    *len = l;
    const int64_t p = (int64_t)8 * j, rest = (int64_t)l - p;
    if (rest <= 0) return 0;
    const int64_t start = s + p, a0 = start & ~(int64_t)7;
    if ((((uintptr_t)bytes) & 7) == 0 && a0 + 16 <= nbytes) {
        const unsigned long long *w64 = (const unsigned long long *)(bytes + a0);
        const int sh = (int)(start - a0) * 8;
        unsigned long long raw = w64[0] >> sh;
        if (sh) raw |= w64[1] << (64 - sh);
        if (rest < 8) raw &= (1ull << (8 * rest)) - 1ull;
        return __builtin_bswap64(raw);
    }
    unsigned long long w = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) w = (w << 8) | (q < rest ? bytes[start + q] : 0u);
    return w;
}

__device__ __forceinline__ long long round_cents(long long x, int scale) {
    // dec.Int64(2): the unscaled value at scale 2, half-even (sort_encoder.go:65-70)
    // scale < 2: the reference's key is x * 10^(2 - scale) as (whole, fraction), which orders like x itself. The key is compared only
    // within its own column, so x stands for it: the multiplication wrapped for |x| > 9.2e16 (scale 0) / 9.2e17 (scale 1).
    // scale > 2: |q| <= |x| / 10, so the rounding step below cannot leave int64.
    if (scale <= 2) return x;
    long long p = 1;
    for (int s = 2; s < scale; s++) p *= 10;
    long long q = x / p, r = x % p;          // truncation toward zero
    long long ar = r < 0 ? -r : r, twice = 2 * ar;
    if (twice > p || (twice == p && (q & 1))) q += x < 0 ? -1 : 1;
    return q;
}

// perm[i] = row id at position i (in/out across columns); writes the (key, row|null<<31) pairs
__global__ __launch_bounds__(256) void sort_norm_kernel(SortCol C, const int32_t *__restrict__ perm, int64_t n,
                                                        unsigned long long *__restrict__ keys, unsigned *__restrict__ rows) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t r = perm[i];
        unsigned long long k = 0;
        unsigned nullbit = 1;   // digit of the NULL byte: 0 = NULL (first), 1 = value
        if (bit_valid(C.validity, r)) {
            if (C.type == PH_STR) {
                int len;
                k = str_word((const int32_t *)C.data, C.bytes, C.nbytes, r, 0, &len);
            } else {
                long long v;
                switch (C.type) {
                case PH_I32: case PH_DATE: v = ((const int32_t *)C.data)[r]; break;
                case PH_CODE8: v = ((const uint8_t *)C.data)[r]; break;
                default: v = round_cents(((const int64_t *)C.data)[r], C.scale); break;
                }
                k = (unsigned long long)v ^ (1ull << 63);
            }
            if (C.descending) k = ~k;
        } else {
            nullbit = 0;
        }
        keys[i] = k;
        rows[i] = (unsigned)r | (nullbit << 31);
    }
}

// OR of key ^ key[0] (bytes that vary) and of nullbit ^ nullbit[0]
__global__ __launch_bounds__(256) void sort_diff_kernel(const unsigned long long *__restrict__ keys,
                                                        const unsigned *__restrict__ rows, int64_t n,
                                                        unsigned long long *__restrict__ out) {
    const unsigned long long k0 = keys[0];
    const unsigned r0 = rows[0] >> 31;
    unsigned long long d = 0, dn = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        d |= keys[i] ^ k0;
        dn |= (rows[i] >> 31) ^ r0;
    }
    for (int o = 32; o > 0; o >>= 1) {
        d |= __shfl_xor(d, o);
        dn |= __shfl_xor(dn, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (d) atomicOr(&out[0], d);
        if (dn) atomicOr(&out[1], dn);
    }
}

// One-word key (TWO = false): shift 0..56 = a byte of the key word, 64 = the NULL flag in bit 31 of the row word.
// Two-word key (TWO = true, the refinement rounds of a VARCHAR column): shift 64..120 = a byte of the high word.
template <bool TWO>
__device__ __forceinline__ int sort_digit(unsigned long long k, unsigned long long h, unsigned rw, int shift) {
    if constexpr (TWO) return (int)((shift < 64 ? k >> shift : h >> (shift - 64)) & 0xFF);
    else return shift < 64 ? (int)((k >> shift) & 0xFF) : (int)(rw >> 31);
}

template <bool TWO>
__global__ __launch_bounds__(256) void sort_hist_kernel(const unsigned long long *__restrict__ keys,
                                                        const unsigned *__restrict__ rows, int64_t n, int shift,
                                                        int32_t *__restrict__ counts,
                                                        const unsigned long long *__restrict__ his = nullptr) {
    __shared__ int hist[256];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * SORT_TILE * SORT_TILES_PER_WG;
    const int64_t i1 = i0 + SORT_TILE * SORT_TILES_PER_WG < n ? i0 + SORT_TILE * SORT_TILES_PER_WG : n;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        if constexpr (TWO) atomicAdd(&hist[sort_digit<true>(keys[i], his[i], 0, shift)], 1);
        else atomicAdd(&hist[sort_digit<false>(keys[i], 0, rows[i], shift)], 1);
    }
    __syncthreads();
    counts[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = hist[threadIdx.x];
}

// Stable: a workgroup walks its chunk tile by tile in order; inside a tile a row's slot is the
// digit's cursor + rows of the same digit in earlier waves + rows of the same digit in lower
// lanes of its own wave (eight ballots find the lanes that share its digit).
template <bool TWO>
__global__ __launch_bounds__(256) void sort_scatter_kernel(const unsigned long long *__restrict__ keys_in,
                                                           const unsigned *__restrict__ rows_in, int64_t n, int shift,
                                                           const int32_t *__restrict__ offsets,
                                                           unsigned long long *__restrict__ keys_out,
                                                           unsigned *__restrict__ rows_out,
                                                           const unsigned long long *__restrict__ his_in = nullptr,
                                                           unsigned long long *__restrict__ his_out = nullptr) {
    __shared__ int cursor[256];
    __shared__ int wcount[4][256];
    cursor[threadIdx.x] = offsets[(int64_t)threadIdx.x * gridDim.x + blockIdx.x];
    for (int w = 0; w < 4; w++) wcount[w][threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * SORT_TILE * SORT_TILES_PER_WG;
    for (int t = 0; t < SORT_TILES_PER_WG; t++) {
        const int64_t base = i0 + (int64_t)t * SORT_TILE;
        if (base >= n) break;   // workgroup-uniform
        const int64_t i = base + threadIdx.x;
        const bool live = i < n;
        unsigned long long k = 0, h = 0;
        unsigned rw = 0;
        int d = 0;
        if (live) {
            k = keys_in[i];
            rw = rows_in[i];
            if constexpr (TWO) h = his_in[i];
            d = sort_digit<TWO>(k, h, rw, shift);
        }
        // lanes of this wave with the same digit
        unsigned long long same = __ballot(live);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const unsigned long long has = __ballot(live && ((d >> b) & 1));
            same &= ((d >> b) & 1) ? has : ~has;
        }
        const int rank = __popcll(same & ((1ull << lane) - 1ull));
        if (live && rank == 0) wcount[wv][d] = __popcll(same);   // the digit's lowest lane
        __syncthreads();
        if (live) {
            int pos = cursor[d] + rank;
            for (int w = 0; w < wv; w++) pos += wcount[w][d];
            keys_out[pos] = k;
            rows_out[pos] = rw;
            if constexpr (TWO) his_out[pos] = h;
        }
        __syncthreads();
        const int add = wcount[0][threadIdx.x] + wcount[1][threadIdx.x] + wcount[2][threadIdx.x] + wcount[3][threadIdx.x];
        cursor[threadIdx.x] += add;
        for (int w = 0; w < 4; w++) wcount[w][threadIdx.x] = 0;
        __syncthreads();
    }
}

// ---- refinement rounds of a VARCHAR key. A round's m candidates, in position order: cpos[t] (position in perm), crow[t] (row id); its
// sorted entries (keys = word j, his = segment id << 8 | e_j, rows = candidate index). R0: the round-0 output instead (keys = word 0, rows =
// row id | NULL flag << 31, position = index). Per sorted entry s: the row goes back to its position (not in R0: rows_out did it), and
// act[s] = the row takes part in the next round (non-NULL / e_j == cont, and its segment — run of equal (his, keys) — has >= 2 rows),
// hd[s] = act[s] and s starts its segment; fl[s] = act | hd << 1 (act / hd are scanned in place after this).
template <bool R0>
__global__ __launch_bounds__(256) void str_flags_kernel(const unsigned long long *__restrict__ keys, const unsigned long long *__restrict__ his,
                                                        const unsigned *__restrict__ rows, int64_t m, unsigned cont,
                                                        const int32_t *__restrict__ cpos, const int32_t *__restrict__ crow,
                                                        int32_t *__restrict__ perm, int32_t *__restrict__ act, int32_t *__restrict__ hd,
                                                        uint8_t *__restrict__ fl) {
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < m; s += (int64_t)gridDim.x * 256) {
        const unsigned long long k = keys[s];
        const unsigned long long h = R0 ? (rows[s] >> 31) : his[s];
        const bool head = s == 0 || keys[s - 1] != k || (R0 ? (rows[s - 1] >> 31) : his[s - 1]) != h;
        const bool last = s == m - 1 || keys[s + 1] != k || (R0 ? (rows[s + 1] >> 31) : his[s + 1]) != h;
        const bool goes_on = R0 ? h != 0 : (unsigned)(h & 0xFF) == cont;
        const bool a = goes_on && !(head && last);
        if (!R0) perm[cpos[s]] = crow[rows[s]];
        act[s] = a;
        hd[s] = a && head;
        fl[s] = (uint8_t)(a | ((a && head) << 1));
    }
}

// the next round's candidates and their keys: word j and e_j = min(len - 8(j-1), 17) (17 - e_j and ~word for DESC); OR / AND of the keys
// into red[0..3] (bytes that vary = OR ^ AND)
template <bool R0>
__global__ __launch_bounds__(256) void str_compact_kernel(const unsigned *__restrict__ rows, int64_t m, const uint8_t *__restrict__ fl,
                                                          const int32_t *__restrict__ act, const int32_t *__restrict__ hd,
                                                          const int32_t *__restrict__ cpos, const int32_t *__restrict__ crow,
                                                          SortCol C, int j, int32_t *__restrict__ npos, int32_t *__restrict__ nrow,
                                                          unsigned long long *__restrict__ keys_out, unsigned long long *__restrict__ his_out,
                                                          unsigned *__restrict__ rows_out, unsigned long long *__restrict__ red) {
    unsigned long long ok = 0, oh = 0, ak = ~0ull, ah = ~0ull;
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < m; s += (int64_t)gridDim.x * 256) {
        const int f = fl[s];
        if (!(f & 1)) continue;
        const int idx = act[s];
        const unsigned seg = (unsigned)(hd[s] + (f >> 1) - 1);
        const int32_t row = R0 ? (int32_t)(rows[s] & 0x7FFFFFFFu) : crow[rows[s]];
        int len;
        unsigned long long w = str_word((const int32_t *)C.data, C.bytes, C.nbytes, row, j, &len);
        const int64_t rest = (int64_t)len - (int64_t)8 * (j - 1);
        unsigned e = rest < 17 ? (unsigned)rest : 17u;
        if (C.descending) { w = ~w; e = 17u - e; }
        const unsigned long long h = ((unsigned long long)seg << 8) | e;
        npos[idx] = R0 ? (int32_t)s : cpos[s];
        nrow[idx] = row;
        keys_out[idx] = w;
        his_out[idx] = h;
        rows_out[idx] = (unsigned)idx;
        ok |= w; ak &= w; oh |= h; ah &= h;
    }
    for (int o = 32; o > 0; o >>= 1) {
        ok |= __shfl_xor(ok, o); ak &= __shfl_xor(ak, o);
        oh |= __shfl_xor(oh, o); ah &= __shfl_xor(ah, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (ok) atomicOr(&red[0], ok);
        if (oh) atomicOr(&red[1], oh);
        if (~ak) atomicAnd(&red[2], ak);
        if (~ah) atomicAnd(&red[3], ah);
    }
}

__global__ __launch_bounds__(256) void sort_rows_out_kernel(const unsigned *__restrict__ rows, int64_t n, int32_t *__restrict__ perm) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        perm[i] = (int32_t)(rows[i] & 0x7FFFFFFFu);
}

__global__ __launch_bounds__(256) void sort_iota_kernel(const int32_t *__restrict__ sel, int64_t n, int32_t *__restrict__ perm) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        perm[i] = sel ? sel[i] : (int32_t)i;
}

}  // namespace ph

extern "C" int ph_sort_rows(ph_ctx *ctx, const ph_col *keys, const int32_t *descending, int32_t nkeys, const int32_t *sel,
                            int64_t n, int32_t *out_rows_dev) {
    PH_REQUIRE(ctx && keys && descending && nkeys >= 1 && nkeys <= 8 && n >= 0 && n < (1ll << 31) && (n == 0 || out_rows_dev),
               "ph_sort_rows: bad arguments (1..8 keys)");
    bool any_str = false;
    for (int c = 0; c < nkeys; c++) {
        const int t = keys[c].type;
        if (t != PH_I32 && t != PH_DATE && t != PH_CODE8 && t != PH_DEC64 && t != PH_STR) {
            // the reference's RadixScatter has no case for BIGINT / DOUBLE keys either (sort_radix.go:257-321)
            ph::set_error("ph_sort_rows: key %d has type %d (INTEGER, DATE, DECIMAL, VARCHAR and ordered dictionary codes sort on the device)", c, t);
            return PH_EUNSUPPORTED;
        }
        if (t == PH_STR) {
            PH_REQUIRE(keys[c].aux_bytes >= 0 && keys[c].aux_bytes < (1ll << 31),
                       "ph_sort_rows: VARCHAR key %d has %lld bytes (int32 offsets: < 2^31)", c, (long long)keys[c].aux_bytes);
            PH_REQUIRE(n == 0 || (keys[c].data && (keys[c].aux || keys[c].aux_bytes == 0)), "ph_sort_rows: VARCHAR key %d without offsets / bytes", c);
            any_str = true;
        }
    }
    if (n == 0) return PH_OK;
    hipStream_t st = ctx->stream;
    auto grid = [&](int64_t m) { return (int)std::min<int64_t>((m + 255) / 256, (int64_t)ctx->cu_count * 8); };
    const int64_t chunk = (int64_t)ph::SORT_TILE * ph::SORT_TILES_PER_WG;
    const int nwg = (int)((n + chunk - 1) / chunk);
    char *tmp = nullptr;
    const int64_t o_k1 = ph::round_up(n * 8, 16), o_r0 = 2 * o_k1, o_r1 = o_r0 + ph::round_up(n * 4, 16);
    const int64_t o_cnt = o_r1 + ph::round_up(n * 4, 16), o_misc = o_cnt + ph::round_up((int64_t)256 * nwg * 4, 16);
    // VARCHAR refinement: high key words (2), candidate positions / rows (2 + 2), the two scanned flags, the flag bytes
    const int64_t o_h0 = o_misc + 64, o_c0 = o_h0 + 2 * o_k1, n4 = ph::round_up(n * 4, 16), o_fl = o_c0 + 6 * n4;
    PH_CHECK(ctx->pool_alloc(any_str ? o_fl + ph::round_up(n, 16) : o_misc + 64, (void **)&tmp));
    unsigned long long *kbuf[2] = {(unsigned long long *)tmp, (unsigned long long *)(tmp + o_k1)};
    unsigned *rbuf[2] = {(unsigned *)(tmp + o_r0), (unsigned *)(tmp + o_r1)};
    int32_t *counts = (int32_t *)(tmp + o_cnt);
    unsigned long long *diff = (unsigned long long *)(tmp + o_misc);   // [0] key diff, [1] null diff; refinement: OR key, OR high, AND key, AND high
    int64_t *total = (int64_t *)(tmp + o_misc + 32);
    int64_t *total2 = (int64_t *)(tmp + o_misc + 40);
    unsigned long long *hbuf[2] = {(unsigned long long *)(tmp + o_h0), (unsigned long long *)(tmp + o_h0 + o_k1)};
    int32_t *cpos[2] = {(int32_t *)(tmp + o_c0), (int32_t *)(tmp + o_c0 + n4)};
    int32_t *crow[2] = {(int32_t *)(tmp + o_c0 + 2 * n4), (int32_t *)(tmp + o_c0 + 3 * n4)};
    int32_t *act = (int32_t *)(tmp + o_c0 + 4 * n4), *hd = (int32_t *)(tmp + o_c0 + 5 * n4);
    uint8_t *fl = (uint8_t *)(tmp + o_fl);
    int rc = PH_OK;
    ph::sort_iota_kernel<<<grid(n), 256, 0, st>>>(sel, n, out_rows_dev);
    for (int c = nkeys - 1; c >= 0 && rc == PH_OK; c--) {   // LSD over the ORDER BY columns
        ph::SortCol C{keys[c].type, keys[c].scale, keys[c].data, keys[c].validity, descending[c] ? 1 : 0, (const uint8_t *)keys[c].aux,
                      keys[c].aux_bytes};
        int cur = 0;
        ph::sort_norm_kernel<<<grid(n), 256, 0, st>>>(C, out_rows_dev, n, kbuf[0], rbuf[0]);
        if (hipMemsetAsync(diff, 0, 16, st) != hipSuccess) { rc = PH_EHIP; break; }
        ph::sort_diff_kernel<<<grid(n), 256, 0, st>>>(kbuf[0], rbuf[0], n, diff);
        unsigned long long d[2] = {0, 0};
        if ((rc = ctx->download(d, diff, 16)) != PH_OK) break;
        for (int pass = 0; pass <= 8 && rc == PH_OK; pass++) {
            const int shift = pass * 8;   // pass 8 = the NULL byte
            const bool varies = pass < 8 ? ((d[0] >> shift) & 0xFF) != 0 : d[1] != 0;
            if (!varies) continue;
            ph::sort_hist_kernel<false><<<nwg, 256, 0, st>>>(kbuf[cur], rbuf[cur], n, shift, counts);
            rc = ph::exclusive_scan_i32(ctx, counts, (int64_t)256 * nwg, total);
            ph::sort_scatter_kernel<false><<<nwg, 256, 0, st>>>(kbuf[cur], rbuf[cur], n, shift, counts, kbuf[cur ^ 1], rbuf[cur ^ 1]);
            cur ^= 1;
        }
        ph::sort_rows_out_kernel<<<grid(n), 256, 0, st>>>(rbuf[cur], n, out_rows_dev);
        if (C.type != PH_STR || rc != PH_OK) continue;
        // refinement rounds j = 1, 2, ... over the rows still tied (see the top of this file)
        const unsigned cont = C.descending ? 0u : 17u;
        int64_t m = n;
        int cc = 0;   // current candidate buffers
        for (int j = 1; rc == PH_OK; j++) {
            const bool r0 = j == 1;
            if (r0) ph::str_flags_kernel<true><<<grid(m), 256, 0, st>>>(kbuf[cur], nullptr, rbuf[cur], m, cont, nullptr, nullptr, out_rows_dev, act, hd, fl);
            else ph::str_flags_kernel<false><<<grid(m), 256, 0, st>>>(kbuf[cur], hbuf[cur], rbuf[cur], m, cont, cpos[cc], crow[cc], out_rows_dev, act, hd, fl);
            if ((rc = ph::exclusive_scan_i32(ctx, act, m, total)) != PH_OK) break;
            if ((rc = ph::exclusive_scan_i32(ctx, hd, m, total2)) != PH_OK) break;
            if (hipMemsetAsync(diff, 0, 16, st) != hipSuccess || hipMemsetAsync(diff + 2, 0xFF, 16, st) != hipSuccess) { rc = PH_EHIP; break; }
            if (r0) ph::str_compact_kernel<true><<<grid(m), 256, 0, st>>>(rbuf[cur], m, fl, act, hd, nullptr, nullptr, C, j, cpos[cc ^ 1], crow[cc ^ 1],
                                                                         kbuf[cur ^ 1], hbuf[cur ^ 1], rbuf[cur ^ 1], diff);
            else ph::str_compact_kernel<false><<<grid(m), 256, 0, st>>>(rbuf[cur], m, fl, act, hd, cpos[cc], crow[cc], C, j, cpos[cc ^ 1], crow[cc ^ 1],
                                                                       kbuf[cur ^ 1], hbuf[cur ^ 1], rbuf[cur ^ 1], diff);
            cur ^= 1;
            cc ^= 1;
            unsigned long long r[5];   // OR key, OR high, AND key, AND high, the next round's row count
            if ((rc = ctx->download(r, diff, 40)) != PH_OK) break;
            m = (int64_t)r[4];
            if (m == 0) break;
            const unsigned long long dk = r[0] ^ r[2], dh = r[1] ^ r[3];
            if (dk == 0 && (dh & 0xFF) == 0) continue;   // word j and e_j equal everywhere: the rows are in order already
            const int mwg = (int)((m + chunk - 1) / chunk);
            // least significant first: e_j (high byte 0), word j, segment id (high bytes 1..4)
            const int shifts[13] = {64, 0, 8, 16, 24, 32, 40, 48, 56, 72, 80, 88, 96};
            for (int p = 0; p < 13 && rc == PH_OK; p++) {
                const int sh = shifts[p];
                if (!(((sh < 64 ? dk >> sh : dh >> (sh - 64)) & 0xFF))) continue;
                ph::sort_hist_kernel<true><<<mwg, 256, 0, st>>>(kbuf[cur], rbuf[cur], m, sh, counts, hbuf[cur]);
                rc = ph::exclusive_scan_i32(ctx, counts, (int64_t)256 * mwg, total2);
                ph::sort_scatter_kernel<true><<<mwg, 256, 0, st>>>(kbuf[cur], rbuf[cur], m, sh, counts, kbuf[cur ^ 1], rbuf[cur ^ 1],
                                                                   hbuf[cur], hbuf[cur ^ 1]);
                cur ^= 1;
            }
        }
    }
    if (rc == PH_OK && hipGetLastError() != hipSuccess) rc = PH_EHIP;
    ctx->pool_release(tmp);
    if (rc == PH_EHIP && ph_last_error()[0] == 0) ph::set_error("ph_sort_rows: HIP failure");
    return rc;
}
