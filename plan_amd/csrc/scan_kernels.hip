// Fused Scan(filter) -> HashAggregate kernels for the resident-table mode (the measured mode).
//
// They replace the reference's per-2048-row pull loop  aggExecutor.Execute -> scanExecutor.Execute
// -> runFilterExec -> executeExprs -> GroupedAggrHashTable.AddChunk -> UpdateStates
// (pkg/compute/executor_aggr.go:110-142, executor_scan.go:144-241, expr_exec.go:85-486,
// aggregate_hash.go:136-391, function_aggr.go:1034-1161) by ONE pass over the device-resident
// columns. Both are HBM-bandwidth-bound integer kernels (no MFMA): every column byte is loaded
// exactly once with 16-byte-per-lane coalesced loads, predicates and decimal arithmetic run in
// registers on unscaled int64, and aggregation state never leaves the CU until the last tile.
//
//   filter_sumprod  (TPC-H Q6 shape): range predicates on <=3 columns, SUM(a*b) -> 1 group.
//       24 B/row algorithmic (shipdate 4 + discount 8 + quantity 4 + extendedprice 8).
//   lowcard_chain   (TPC-H Q1 shape): one range predicate, group key = dense index of two
//       dictionary-code columns (<= 8 live slots), accumulators
//       {Σq, Σe, Σe(A1+B1 d), Σe(A1+B1 d)(A2+B2 t), Σd, count}.
//       34 B/row algorithmic (qty 4 + ext/disc/tax 3x8 + 2 code bytes + shipdate 4).
//       Group state is a per-thread-private column of LDS (ds_add_u64, conflict-free because
//       consecutive lanes hit consecutive banks), merged once per workgroup at the end.

#include "common.h"
#include "scan_kernels.h"
#include <type_traits>

namespace ph {

// ------------------------------------------------------------------ helpers

__device__ __forceinline__ long long wave_sum_i64(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

struct alignas(16) i64x2 { long long x, y; };
struct alignas(16) i32x4 { int x, y, z, w; };

typedef long long v2i64 __attribute__((ext_vector_type(2)));
typedef int v4i32 __attribute__((ext_vector_type(4)));

// Streaming loads: every byte of these columns is read exactly once per launch, so the loads are
// marked non-temporal (global_load_dwordx4 ... nt) to keep them from displacing anything useful in
// L2/MALL. NT = false keeps the default cache policy (A/B switch: PH_SCAN_NT=0).
template <bool NT> __device__ __forceinline__ i64x2 ld_i64x2(const int64_t *p) {
    if (NT) {
        v2i64 v = __builtin_nontemporal_load(reinterpret_cast<const v2i64 *>(p));
        return i64x2{v.x, v.y};
    }
    return *reinterpret_cast<const i64x2 *>(p);
}
template <bool NT> __device__ __forceinline__ i32x4 ld_i32x4(const int32_t *p) {
    if (NT) {
        v4i32 v = __builtin_nontemporal_load(reinterpret_cast<const v4i32 *>(p));
        return i32x4{v.x, v.y, v.z, v.w};
    }
    return *reinterpret_cast<const i32x4 *>(p);
}
typedef unsigned v4u32 __attribute__((ext_vector_type(4)));
template <bool NT> __device__ __forceinline__ v4u32 ld_u32x4(const uint8_t *p) {
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const v4u32 *>(p));
    return *reinterpret_cast<const v4u32 *>(p);
}
typedef unsigned v2u32 __attribute__((ext_vector_type(2)));
template <bool NT> __device__ __forceinline__ v2u32 ld_u32x2(const uint8_t *p) {
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const v2u32 *>(p));
    return *reinterpret_cast<const v2u32 *>(p);
}
template <bool NT> __device__ __forceinline__ unsigned ld_u32(const uint8_t *p) {
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const unsigned *>(p));
    return *reinterpret_cast<const unsigned *>(p);
}

// ------------------------------------------------------------------ fused merge + publish (ScanTail)
// one partial word of this workgroup, stored where the other XCDs can read it (a plain store would stay in this XCD's write-back L2 until a fence)
__device__ __forceinline__ void scan_tail_put(long long *partials, int nacc, int j, long long v) {
    __hip_atomic_store(partials + (int64_t)blockIdx.x * nacc + j, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Called by ALL threads of every workgroup (256 threads) after its scan_tail_put calls; lds: 2 * SCAN_TAIL_MAX_ACC + 1 words nothing else uses any more.
// A 64-bit partial is folded as two halves (a += low 32 bits, b += high 32 bits signed: no carries between LDS atomics), first-row minima as the
// maximum of the complement (zero is every word's identity).
__device__ __forceinline__ void scan_tail(const long long *partials, const ScanTail &T, unsigned long long *lds) {
    // Everything the workgroups tell each other travels in device-scope stores / atomics (performed at the device's coherent level, not in an XCD's
    // L2), so ordering is all that is needed: s_waitcnt returns when this wave's stores have been acknowledged, the barrier collects the waves, then
    // the ticket. A device-scope fence here (__threadfence: an L2 write-back + invalidate per workgroup) cost 36-50 us per launch.
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    int *s_flag = reinterpret_cast<int *>(lds + 2 * SCAN_TAIL_MAX_ACC);
    if (threadIdx.x == 0) *s_flag = __hip_atomic_fetch_add(T.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1 : 0;
    for (int j = threadIdx.x; j < 2 * SCAN_TAIL_MAX_ACC; j += 256) lds[j] = 0;
    __syncthreads();
    if (!*s_flag) return;
    unsigned long long *la = lds, *lb = lds + SCAN_TAIL_MAX_ACC;
    const int total = (int)gridDim.x * T.nacc;
    for (int i0 = 0; i0 < total; i0 += 256 * 16) {
        long long v[16];
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int i = i0 + k * 256 + (int)threadIdx.x;
            v[k] = i < total ? __hip_atomic_load(partials + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        }
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int i = i0 + k * 256 + (int)threadIdx.x;
            if (i >= total) break;
            const int j = i % T.nacc;
            if (T.min_stride > 0 && j % T.min_stride == T.min_stride - 1) atomicMax(la + j, ~(unsigned long long)v[k]);
            else {
                atomicAdd(la + j, (unsigned long long)v[k] & 0xffffffffull);
                atomicAdd(lb + j, (unsigned long long)(v[k] >> 32));   // arithmetic shift: the signed high half
            }
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < T.nacc; j += 256) {
        const unsigned long long a = la[j];
        const long long b = (long long)lb[j];
        unsigned long long lo;
        long long hi;
        if (T.min_stride > 0 && j % T.min_stride == T.min_stride - 1) {
            lo = ~a;
            hi = 0;
        } else {   // a + (b << 32) in 128 bits: a < 2^63 (2^31 workgroups x 2^32), b a signed sum of signed halves
            lo = a + ((unsigned long long)b << 32);
            hi = (b >> 32) + (lo < a ? 1 : 0);
        }
        T.out_lo[j] = lo;
        T.out_hi[j] = hi;
        if (T.mbox) {
            T.mbox[j] = lo;
            T.mbox[T.nacc + j] = (unsigned long long)hi;
        }
    }
    if (T.mbox) __threadfence_system();   // the mailbox words are visible to the host ...
    __syncthreads();                      // ... for every wave ...
    if (threadIdx.x == 0) {
        *T.done = 0;
        if (T.mbox) __hip_atomic_store(T.flag, T.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);   // ... before the number is
    }
}

// ------------------------------------------------------------------ narrowed columns (the *_for kernels)
// A lane owns 16 consecutive rows, so a column of w-byte codes is w 16-byte loads per lane and tile (w fixed by the kernel instance, or
// kernel-uniform: scalar branches).
// Row 16 i of the lane starts at byte 16 i w: every load is 16-byte aligned, and a tile that starts below row_end stays inside the
// column's padding (PH_ROW_PAD rows, a multiple of 16).
struct Codes16 {
    v4u32 r[4];   // w = 1: r[0]; w = 2: r[0..1]; w = 4: r[0..3] (the rest zero)
};

// W: the width when the kernel instance fixes it at compile time (the width tuples of TPC-H Q1 / Q6), 0 = f.w at run time
template <bool NT, int W> __device__ __forceinline__ void for_load(Codes16 &c, const ForCol &f, int64_t row) {
    const int w = W ? W : f.w;
    const uint8_t *p = f.data + row * w;
    c.r[0] = ld_u32x4<NT>(p);
    c.r[1] = c.r[2] = c.r[3] = v4u32{0, 0, 0, 0};
    if (w >= 2) c.r[1] = ld_u32x4<NT>(p + 16);
    if (w == 4) {
        c.r[2] = ld_u32x4<NT>(p + 32);
        c.r[3] = ld_u32x4<NT>(p + 48);
    }
}

// the 16 codes, one per row. A fixed width extracts only its own form. A run-time width extracts all three and selects on the
// kernel-uniform width, branch-free: written as `if (w == 1) .. else if (w == 2) .. else ..`, hipcc (ROCm 7.2, gfx950) compiled the
// w == 4 path of lowcard_chain_kernel_for without the copy of its last code, and Q1's sum of extendedprice came out wrong.
template <int W> __device__ __forceinline__ void for_unpack(const Codes16 &c, int w, unsigned (&v)[16]) {
    const bool w1 = W ? W == 1 : w == 1, w2 = W ? W == 2 : w == 2;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const unsigned b1 = (c.r[0][i >> 2] >> (8 * (i & 3))) & 0xffu;
        const unsigned b2 = (c.r[i >> 3][(i >> 1) & 3] >> (16 * (i & 1))) & 0xffffu;
        const unsigned b4 = c.r[i >> 2][i & 3];
        v[i] = w1 ? b1 : w2 ? b2 : b4;
    }
}

// for_unpack for a width fixed at compile time, over the words as values (the lean row bodies, whose tiles are structs of plain vectors).
// No word is chosen by the loop variable, here or through Codes16's array: the optimiser turns such a choice into one wide load at a
// variable index, and a part of both register buffers then stays in private memory.
__device__ __forceinline__ void codes_unpack1(const v4u32 r0, unsigned (&v)[16]) {
#pragma unroll
    for (int i = 0; i < 16; i++) v[i] = (r0[i >> 2] >> (8 * (i & 3))) & 0xffu;
}
__device__ __forceinline__ void codes_unpack2(const v4u32 r0, const v4u32 r1, unsigned (&v)[16]) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        v[i] = (r0[i >> 1] >> (16 * (i & 1))) & 0xffffu;
        v[8 + i] = (r1[i >> 1] >> (16 * (i & 1))) & 0xffffu;
    }
}
__device__ __forceinline__ void codes_unpack4(const v4u32 r0, const v4u32 r1, const v4u32 r2, const v4u32 r3, unsigned (&v)[16]) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        v[i] = r0[i];
        v[4 + i] = r1[i];
        v[8 + i] = r2[i];
        v[12 + i] = r3[i];
    }
}

__device__ __forceinline__ bool in_codes(unsigned c, unsigned lo, unsigned hi) { return c >= lo && c <= hi; }

// ------------------------------------------------------------------ filter_sumprod (Q6 shape)

struct FsTile {
    i32x4 p0;      // int32 predicate column (dates)
    i32x4 p2;      // int32 predicate column (quantity)
    i64x2 b0, b1;  // int64 predicate column that is also the second factor (discount)
    i64x2 a0, a1;  // int64 first factor (extendedprice)
};

template <bool NT> __device__ __forceinline__ FsTile fs_load(const FilterSumProdParams &P, int64_t row) {
    FsTile t;
    t.p0 = ld_i32x4<NT>(P.p0 + row);
    t.p2 = ld_i32x4<NT>(P.p2 + row);
    t.b0 = ld_i64x2<NT>(P.b + row);
    t.b1 = ld_i64x2<NT>(P.b + row + 2);
    t.a0 = ld_i64x2<NT>(P.a + row);
    t.a1 = ld_i64x2<NT>(P.a + row + 2);
    return t;
}

__device__ __forceinline__ void fs_row(const FilterSumProdParams &P, bool in_range, int p0, int p2,
                                       long long b, long long a, long long &sum, unsigned &cnt) {
    bool pass = in_range && p0 >= P.p0_lo && p0 <= P.p0_hi && p2 >= P.p2_lo && p2 <= P.p2_hi &&
                b >= P.b_lo && b <= P.b_hi;
    if (pass) {
        sum += a * b;
        cnt += 1;
    }
}

// the workgroup's {Σ a*b, count} -> partials (and the fused merge + publish when P.tail.done)
__device__ __forceinline__ void fs_finish(const FilterSumProdParams &P, long long sum, unsigned cnt) {
    sum = wave_sum_i64(sum);
    long long c64 = wave_sum_i64((long long)cnt);
    __shared__ long long ws[2][4];
    int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        ws[0][w] = sum;
        ws[1][w] = c64;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long s = ws[0][0] + ws[0][1] + ws[0][2] + ws[0][3], c = ws[1][0] + ws[1][1] + ws[1][2] + ws[1][3];
        if (P.tail.done) {
            scan_tail_put(P.partials, 2, 0, s);
            scan_tail_put(P.partials, 2, 1, c);
        } else {
            P.partials[(int64_t)blockIdx.x * 2 + 0] = s;
            P.partials[(int64_t)blockIdx.x * 2 + 1] = c;
        }
    }
    __shared__ unsigned long long tail_lds[2 * SCAN_TAIL_MAX_ACC + 1];
    if (P.tail.done) scan_tail(P.partials, P.tail, tail_lds);
}

template <bool NT> __global__ __launch_bounds__(256) void filter_sumprod_kernel(FilterSumProdParams P) {
    // tile = 1024 rows per workgroup iteration, 4 consecutive rows per lane
    const int64_t tile_rows = 1024;
    long long sum = 0;
    unsigned cnt = 0;
    int64_t first = P.row_begin + (int64_t)blockIdx.x * tile_rows + threadIdx.x * 4;
    const int64_t stride = (int64_t)gridDim.x * tile_rows;
    // row_begin is a multiple of 4 and columns are padded to PH_ROW_PAD rows, so a 4-row vector
    // load that starts below row_end stays inside the allocation.
    if (first < P.row_end) {
        FsTile cur = fs_load<NT>(P, first);
        for (int64_t row = first; row < P.row_end; row += stride) {
            int64_t nrow = row + stride;
            FsTile nxt = cur;
            if (nrow < P.row_end) nxt = fs_load<NT>(P, nrow);
            fs_row(P, row + 0 < P.row_end, cur.p0.x, cur.p2.x, cur.b0.x, cur.a0.x, sum, cnt);
            fs_row(P, row + 1 < P.row_end, cur.p0.y, cur.p2.y, cur.b0.y, cur.a0.y, sum, cnt);
            fs_row(P, row + 2 < P.row_end, cur.p0.z, cur.p2.z, cur.b1.x, cur.a1.x, sum, cnt);
            fs_row(P, row + 3 < P.row_end, cur.p0.w, cur.p2.w, cur.b1.y, cur.a1.y, sum, cnt);
            cur = nxt;
        }
    }
    fs_finish(P, sum, cnt);
}

// The same over the narrowed copies (P.form != FORM_WIDE): 16 rows per lane, 4096 per workgroup tile, from row_begin rounded down to a
// multiple of 16 (rows outside [row_begin, row_end) are masked). a = base + code in int64 as in fs_row; P32: |a|, |b| < 2^31 (proven at
// plan creation), so the product is one 32 x 32 -> 64-bit multiply.
struct FsnTile {
    Codes16 p0, p2, b, a;
};

template <bool NT, int W0, int W2, int WB, int WA>
__device__ __forceinline__ void fsn_load(FsnTile &x, const FilterSumProdParams &P, int64_t row) {
    for_load<NT, W0>(x.p0, P.np0, row);
    for_load<NT, W2>(x.p2, P.np2, row);
    for_load<NT, WB>(x.b, P.nb, row);
    for_load<NT, WA>(x.a, P.na, row);
}

// W0, W2, WB, WA: the code widths of p0, p2, b, a fixed at compile time (all 0: the widths of P, any tuple)
template <bool NT, bool P32, int W0, int W2, int WB, int WA>
__global__ __launch_bounds__(256) void filter_sumprod_kernel_for(FilterSumProdParams P) {
    const int64_t tile_rows = 4096;
    long long sum = 0;
    unsigned cnt = 0;
    const int64_t first = (P.row_begin & ~(int64_t)15) + (int64_t)blockIdx.x * tile_rows + threadIdx.x * 16;
    const int64_t stride = (int64_t)gridDim.x * tile_rows;
    if (first < P.row_end) {
        FsnTile cur, nxt;
        fsn_load<NT, W0, W2, WB, WA>(cur, P, first);
        for (int64_t row = first; row < P.row_end; row += stride) {
            const int64_t nrow = row + stride;
            nxt = cur;
            if (nrow < P.row_end) fsn_load<NT, W0, W2, WB, WA>(nxt, P, nrow);
            unsigned p0[16], p2[16], b[16], a[16];
            for_unpack<W0>(cur.p0, P.np0.w, p0);
            for_unpack<W2>(cur.p2, P.np2.w, p2);
            for_unpack<WB>(cur.b, P.nb.w, b);
            for_unpack<WA>(cur.a, P.na.w, a);
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const bool pass = row + i >= P.row_begin && row + i < P.row_end && in_codes(p0[i], P.np0_lo, P.np0_hi) &&
                                  in_codes(p2[i], P.np2_lo, P.np2_hi) && in_codes(b[i], P.nb_lo, P.nb_hi);
                if (pass) {
                    const long long av = P.na.base + (long long)a[i], bv = P.nb.base + (long long)b[i];
                    sum += P32 ? (long long)(int)av * (long long)(int)bv : av * bv;
                    cnt += 1;
                }
            }
            cur = nxt;
        }
    }
    fs_finish(P, sum, cnt);
}

// ------------------------------------------------------------------ the lean tile loop (P.lean, fixed code widths)
// A workgroup's tile starts at tile0 = (row_begin & ~15) + 4096 k. A tile with row_begin <= tile0 and tile0 + 4096 <= row_end is interior:
// every row of it is in range, so its row body (MASKED = false) has no row-range test; at most the first and the last tile of a launch take
// MASKED = true. The choice is workgroup-uniform: one scalar compare per tile. The two register buffers swap roles (the loop is unrolled by
// two) instead of being copied on the back edge. The loop hands LOAD the buffer, the lane's first row of the tile to load and that
// tile's first row, whether or not they lie below row_end; row_safe, the first row of the range rounded down to 16, is in scope for a
// LOAD that must read something valid in place of rows beyond the columns' padding (how a lane's rows lie in a tile is LOAD's business).
// A predicate lo <= code <= hi is (code - lo) <= (hi - lo) in unsigned arithmetic; lo > hi (nothing passes) is settled before the loop.
#define PH_LEAN_TILE_LOOP(DECL, LOAD, BODY)                                                               \
    if (tile0 < re) {                                                                                     \
        const int64_t row_safe = rb & ~(int64_t)15;                                                       \
        DECL(A);                                                                                          \
        DECL(B);                                                                                          \
        LOAD(A, row, tile0);                                                                              \
        for (;;) {                                                                                        \
            LOAD(B, row + stride, tile0 + stride);                                                        \
            if (tile0 >= rb && tile0 + tile_rows <= re) BODY(false, A); else BODY(true, A);               \
            row += stride;                                                                                \
            tile0 += stride;                                                                              \
            if (tile0 >= re) break;                                                                       \
            LOAD(A, row + stride, tile0 + stride);                                                        \
            if (tile0 >= rb && tile0 + tile_rows <= re) BODY(false, B); else BODY(true, B);               \
            row += stride;                                                                                \
            tile0 += stride;                                                                              \
            if (tile0 >= re) break;                                                                       \
        }                                                                                                 \
    }

// ------------------------------------------------------------------ lowcard_chain (Q1 shape)

struct LcTile {
    i32x4 p;          // predicate column (shipdate)
    i32x4 q;          // int32 summed column (quantity)
    i64x2 e0, e1;     // extendedprice
    i64x2 d0, d1;     // discount
    i64x2 t0, t1;     // tax
    unsigned k0, k1;  // 4 code bytes each
};

template <bool NT> __device__ __forceinline__ LcTile lc_load(const LowcardChainParams &P, int64_t row) {
    LcTile t;
    t.p = ld_i32x4<NT>(P.p + row);
    t.q = ld_i32x4<NT>(P.q + row);
    t.e0 = ld_i64x2<NT>(P.e + row);
    t.e1 = ld_i64x2<NT>(P.e + row + 2);
    t.d0 = ld_i64x2<NT>(P.d + row);
    t.d1 = ld_i64x2<NT>(P.d + row + 2);
    t.t0 = ld_i64x2<NT>(P.t + row);
    t.t1 = ld_i64x2<NT>(P.t + row + 2);
    t.k0 = ld_u32<NT>(P.k0 + row);
    t.k1 = ld_u32<NT>(P.k1 + row);
    return t;
}

// LDS layout per workgroup (nslots group slots, 256 threads):
//   u64 acc64[slot][5][256]   Σq, Σe, Σe·f1, Σe·f1·f2, Σd      (one 8-byte column per thread)
//   u32 acc32[slot][2][256]   count, first row id (min)
// Every thread owns one column, so the 64 lanes of a wave always touch 64 consecutive words
// whatever slot each lane is in (slot strides are multiples of 256 words): no bank conflicts,
// no inter-lane contention, plain ds_add/ds_min without return.
template <bool P32>
__device__ __forceinline__ void lc_add(const LowcardChainParams &P, unsigned long long *acc64, unsigned *acc32, unsigned row, long long q,
                                       long long e, long long d, long long t, unsigned k0, unsigned k1) {
    unsigned slot = k0 * (unsigned)P.nk1 + k1;
    unsigned long long *a = acc64 + (size_t)slot * 5 * 256;
    unsigned *c = acc32 + (size_t)slot * 2 * 256;
    long long dp, ch;
    if (P32) {   // |e|, |f1|, |e f1|, |f2| < 2^31 (proven at plan creation): f1, f2 exact in 32 bits, products 32 x 32 -> 64
        const int f1 = (int)((unsigned)P.A1 + (unsigned)P.B1 * (unsigned)d);
        const int f2 = (int)((unsigned)P.A2 + (unsigned)P.B2 * (unsigned)t);
        dp = (long long)(int)e * f1;
        ch = (long long)(int)dp * f2;
    } else {
        dp = e * (P.A1 + P.B1 * d);
        ch = dp * (P.A2 + P.B2 * t);
    }
    atomicAdd(a + 0 * 256, (unsigned long long)q);
    atomicAdd(a + 1 * 256, (unsigned long long)e);
    atomicAdd(a + 2 * 256, (unsigned long long)dp);
    atomicAdd(a + 3 * 256, (unsigned long long)ch);
    atomicAdd(a + 4 * 256, (unsigned long long)d);
    atomicAdd(c + 0 * 256, 1u);
    atomicMin(c + 1 * 256, row);
}

__device__ __forceinline__ void lc_row(const LowcardChainParams &P, unsigned long long *acc64,
                                       unsigned *acc32, bool in_range, unsigned row, int p, int q,
                                       long long e, long long d, long long t, unsigned k0,
                                       unsigned k1) {
    if (in_range && p >= P.p_lo && p <= P.p_hi) lc_add<false>(P, acc64, acc32, row, (long long)q, e, d, t, k0, k1);
}

__device__ __forceinline__ void lc_lds_init(unsigned long long *lds64, unsigned *lds32, int ns) {
    for (int i = threadIdx.x; i < ns * 5 * 256; i += 256) lds64[i] = 0;
    for (int s = 0; s < ns; s++) {
        lds32[(s * 2 + 0) * 256 + threadIdx.x] = 0;
        lds32[(s * 2 + 1) * 256 + threadIdx.x] = 0xffffffffu;
    }
    __syncthreads();
}

// workgroup merge: wave w reduces accumulator rows w, w+4, ...; partial layout
// [slot][LC_NACC+1] = {Σq, Σe, Σe·f1, Σe·f1·f2, Σd, count, first_row}
__device__ __forceinline__ void lc_merge(const LowcardChainParams &P, unsigned long long *lds_acc, const unsigned long long *lds64,
                                         const unsigned *lds32, int ns) {
    __syncthreads();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int per_slot = LC_NACC + 1;
    for (int j = w; j < ns * per_slot; j += 4) {
        int s = j / per_slot, a = j % per_slot;
        long long v;
        if (a < 5) {
            const unsigned long long *r = lds64 + (size_t)(s * 5 + a) * 256;
            v = (long long)(r[lane] + r[lane + 64] + r[lane + 128] + r[lane + 192]);
            v = wave_sum_i64(v);
        } else if (a == 5) {
            const unsigned *r = lds32 + (size_t)(s * 2 + 0) * 256;
            v = (long long)r[lane] + r[lane + 64] + r[lane + 128] + r[lane + 192];
            v = wave_sum_i64(v);
        } else {
            const unsigned *r = lds32 + (size_t)(s * 2 + 1) * 256;
            unsigned m = min(min(r[lane], r[lane + 64]), min(r[lane + 128], r[lane + 192]));
            for (int o = 32; o > 0; o >>= 1) m = min(m, (unsigned)__shfl_xor((int)m, o));
            v = (long long)m;
        }
        if (lane == 0) {
            if (P.tail.done) scan_tail_put(P.partials, ns * per_slot, j, v);
            else P.partials[(int64_t)blockIdx.x * ns * per_slot + j] = v;
        }
    }
    if (P.tail.done) {
        __syncthreads();   // the LDS accumulators have been read by every wave: their first 2 KiB serve the tail
        scan_tail(P.partials, P.tail, lds_acc);
    }
}

template <bool NT, int U> __global__ __launch_bounds__(256) void lowcard_chain_kernel(LowcardChainParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds_acc[];
    const int ns = P.nslots;
    unsigned long long *lds64 = lds_acc;
    unsigned *lds32 = reinterpret_cast<unsigned *>(lds_acc + (size_t)ns * 5 * 256);
    lc_lds_init(lds64, lds32, ns);
    unsigned long long *acc64 = lds64 + threadIdx.x;
    unsigned *acc32 = lds32 + threadIdx.x;

    // U tiles of 1024 rows per iteration (a lane owns 4 consecutive rows of each), register
    // double buffered: the loads of iteration i+1 are in flight while iteration i is aggregated.
    const int64_t tile_rows = 1024;
    int64_t first = P.row_begin + (int64_t)blockIdx.x * tile_rows * U + threadIdx.x * 4;
    const int64_t stride = (int64_t)gridDim.x * tile_rows * U;
    if (first < P.row_end) {
        LcTile cur[U], nxt[U];
#pragma unroll
        for (int u = 0; u < U; u++)
            if (first + u * tile_rows < P.row_end) cur[u] = lc_load<NT>(P, first + u * tile_rows);
        for (int64_t row0 = first; row0 < P.row_end; row0 += stride) {
            int64_t nrow = row0 + stride;
#pragma unroll
            for (int u = 0; u < U; u++) {
                nxt[u] = cur[u];
                if (nrow + u * tile_rows < P.row_end) nxt[u] = lc_load<NT>(P, nrow + u * tile_rows);
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                int64_t row = row0 + u * tile_rows;
                if (row >= P.row_end) break;
                const LcTile &c = cur[u];
                unsigned r = (unsigned)row;
                lc_row(P, acc64, acc32, row + 0 < P.row_end, r + 0, c.p.x, c.q.x, c.e0.x, c.d0.x, c.t0.x,
                       c.k0 & 0xff, c.k1 & 0xff);
                lc_row(P, acc64, acc32, row + 1 < P.row_end, r + 1, c.p.y, c.q.y, c.e0.y, c.d0.y, c.t0.y,
                       (c.k0 >> 8) & 0xff, (c.k1 >> 8) & 0xff);
                lc_row(P, acc64, acc32, row + 2 < P.row_end, r + 2, c.p.z, c.q.z, c.e1.x, c.d1.x, c.t1.x,
                       (c.k0 >> 16) & 0xff, (c.k1 >> 16) & 0xff);
                lc_row(P, acc64, acc32, row + 3 < P.row_end, r + 3, c.p.w, c.q.w, c.e1.y, c.d1.y, c.t1.y,
                       c.k0 >> 24, c.k1 >> 24);
            }
#pragma unroll
            for (int u = 0; u < U; u++) cur[u] = nxt[u];
        }
    }
    lc_merge(P, lds_acc, lds64, lds32, ns);
}

// The same over the narrowed copies (P.form != FORM_WIDE): 16 rows per lane, 4096 per workgroup tile, from row_begin rounded down to a
// multiple of 16 (rows outside [row_begin, row_end) are masked). The predicate compares codes; q, e, d, t = base + code in int64, then
// lc_row's arithmetic (P32: with 32-bit factors, lc_add).
struct LcnTile {
    Codes16 p, q, e, d, t;
    v4u32 k0, k1;   // 16 code bytes each
};

template <bool NT, int WP, int WQ, int WE, int WD, int WT>
__device__ __forceinline__ void lcn_load(LcnTile &x, const LowcardChainParams &P, int64_t row) {
    for_load<NT, WP>(x.p, P.np, row);
    for_load<NT, WQ>(x.q, P.nq, row);
    for_load<NT, WE>(x.e, P.ne, row);
    for_load<NT, WD>(x.d, P.nd, row);
    for_load<NT, WT>(x.t, P.nt, row);
    x.k0 = ld_u32x4<NT>(P.k0 + row);
    x.k1 = ld_u32x4<NT>(P.k1 + row);
}

// WP .. WT: the code widths of p, q, e, d, t fixed at compile time (all 0: the widths of P, any tuple)
template <bool NT, bool P32, int WP, int WQ, int WE, int WD, int WT>
__global__ __launch_bounds__(256) void lowcard_chain_kernel_for(LowcardChainParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds_acc[];
    const int ns = P.nslots;
    unsigned long long *lds64 = lds_acc;
    unsigned *lds32 = reinterpret_cast<unsigned *>(lds_acc + (size_t)ns * 5 * 256);
    lc_lds_init(lds64, lds32, ns);
    unsigned long long *acc64 = lds64 + threadIdx.x;
    unsigned *acc32 = lds32 + threadIdx.x;

    const int64_t tile_rows = 4096;
    const int64_t first = (P.row_begin & ~(int64_t)15) + (int64_t)blockIdx.x * tile_rows + threadIdx.x * 16;
    const int64_t stride = (int64_t)gridDim.x * tile_rows;
    if (first < P.row_end) {
        LcnTile cur, nxt;
        lcn_load<NT, WP, WQ, WE, WD, WT>(cur, P, first);
        for (int64_t row = first; row < P.row_end; row += stride) {
            const int64_t nrow = row + stride;
            nxt = cur;
            if (nrow < P.row_end) lcn_load<NT, WP, WQ, WE, WD, WT>(nxt, P, nrow);
            unsigned p[16], q[16], e[16], d[16], t[16];
            for_unpack<WP>(cur.p, P.np.w, p);
            for_unpack<WQ>(cur.q, P.nq.w, q);
            for_unpack<WE>(cur.e, P.ne.w, e);
            for_unpack<WD>(cur.d, P.nd.w, d);
            for_unpack<WT>(cur.t, P.nt.w, t);
#pragma unroll
            for (int i = 0; i < 16; i++) {
                if (row + i >= P.row_begin && row + i < P.row_end && in_codes(p[i], P.np_lo, P.np_hi))
                    lc_add<P32>(P, acc64, acc32, (unsigned)(row + i), P.nq.base + (long long)q[i], P.ne.base + (long long)e[i],
                                P.nd.base + (long long)d[i], P.nt.base + (long long)t[i], (cur.k0[i >> 2] >> (8 * (i & 3))) & 0xffu,
                                (cur.k1[i >> 2] >> (8 * (i & 3))) & 0xffu);
            }
            cur = nxt;
        }
    }
    lc_merge(P, lds_acc, lds64, lds32, ns);
}

// The lean row body (P.lean, fixed code widths). Per passing row: the slot's two LDS byte offsets in 32 bits (a 24-bit multiply-add and a
// shift on the one-byte codes: both offsets are below 160 KiB), f1 and f2 as one multiply-add on the code each (A1c, A2c fold the bases;
// v_mad_i32_i24, the only one-instruction 32-bit multiply-add: the codes are one byte here and |B1|, |B2| < 2^23 is part of P.lean),
// e as one 32-bit add, dp = e f1 as one 32-bit multiply (|e f1| < 2^31 by FORM_NARROW32's bound, so its low 32 bits are the product),
// ch = dp f2 as the one 32 x 32 -> 64 multiply, and the same seven LDS operations on the same layout and the same values as lc_add.
// (Summing q, e and d as codes with one base x count fix-up per workgroup was built and measured: it made Q1 slower)
typedef __attribute__((address_space(3))) char lds_char;
typedef __attribute__((address_space(3))) unsigned long long lds_u64;
typedef __attribute__((address_space(3))) unsigned lds_u32;

// the code widths of TPC-H Q1 (shipdate 2, quantity 1, extendedprice 4, discount 1, tax 1). A register buffer is eleven vector variables
// named by a prefix, not a struct: of a struct of vectors a part stayed in private memory (the optimiser merged the accesses to neighbouring
// members into wider ones, and the struct then was not split into registers).
#define LCL_DECL(T) v4u32 T##pa, T##pb, T##q, T##e0, T##e1, T##e2, T##e3, T##d, T##t, T##k0, T##k1
#define LCL_ARGS(T) T##pa, T##pb, T##q, T##e0, T##e1, T##e2, T##e3, T##d, T##t, T##k0, T##k1
// A lane owns four groups of four consecutive rows of a tile, LCL_GROUP rows apart: row = tile + 1024 wave + 256 j + 4 lane + k. Every load
// instruction of a wave then reads consecutive bytes (256, 512 or 1024 of them for 1-, 2- and 4-byte codes). With a lane's 16 rows
// consecutive, as in the *_for kernels, the lanes of a load of the 4-byte column lie 64 bytes apart, and reading these columns that way,
// with nothing else done, takes 10 % longer (scripts/read_pattern_gfx950.hip). The codes of group j are element j of a
// one-byte column's vector, half a vector of the two-byte column and one vector of the four-byte one, so index i = 4 j + k of
// codes_unpack's arrays is row lcl_row_off(i) of the lane.
constexpr int LCL_GROUP = 256;
__device__ __forceinline__ constexpr int lcl_row_off(int i) { return (i >> 2) * LCL_GROUP + (i & 3); }
#define LCL_LOAD_AT(T, R0, R1, R2, R3)                                     \
    do {                                                                   \
        const int64_t g_[4] = {(R0), (R1), (R2), (R3)};                    \
        _Pragma("unroll") for (int j_ = 0; j_ < 4; j_++) {                 \
            const v2u32 p_ = ld_u32x2<true>(P.np.data + g_[j_] * 2);       \
            (j_ < 2 ? T##pa : T##pb)[(j_ & 1) * 2] = p_.x;                 \
            (j_ < 2 ? T##pa : T##pb)[(j_ & 1) * 2 + 1] = p_.y;             \
            T##q[j_] = ld_u32<true>(P.nq.data + g_[j_]);                   \
            T##d[j_] = ld_u32<true>(P.nd.data + g_[j_]);                   \
            T##t[j_] = ld_u32<true>(P.nt.data + g_[j_]);                   \
            T##k0[j_] = ld_u32<true>(P.k0 + g_[j_]);                       \
            T##k1[j_] = ld_u32<true>(P.k1 + g_[j_]);                       \
        }                                                                  \
        T##e0 = ld_u32x4<true>(P.ne.data + g_[0] * 4);                     \
        T##e1 = ld_u32x4<true>(P.ne.data + g_[1] * 4);                     \
        T##e2 = ld_u32x4<true>(P.ne.data + g_[2] * 4);                     \
        T##e3 = ld_u32x4<true>(P.ne.data + g_[3] * 4);                     \
    } while (0)
// A tile that ends at or below row_end is loaded as it is. Of any other tile a lane loads the groups that start below row_end (they end
// at most three rows beyond it: the column padding covers that, and no more than that is relied on) and, without a branch, the first
// group of the range in place of each of the others; only a MASKED body ever sees those codes.
// LCL_SAFE: group J of the lane whose first row is R, or the first group of the range when it starts at or beyond row_end
#define LCL_SAFE(R, J) ((R) + (J) * LCL_GROUP < re ? (R) + (J) * LCL_GROUP : row_safe)
#define LCL_LOAD(T, R, T0)                                                                                      \
    do {                                                                                                        \
        const int64_t r_ = (R);                                                                                 \
        if ((T0) + tile_rows <= re) LCL_LOAD_AT(T, r_, r_ + LCL_GROUP, r_ + 2 * LCL_GROUP, r_ + 3 * LCL_GROUP); \
        else LCL_LOAD_AT(T, LCL_SAFE(r_, 0), LCL_SAFE(r_, 1), LCL_SAFE(r_, 2), LCL_SAFE(r_, 3));                \
    } while (0)

// one passing row of the lean bodies: the codes of q, e, d, t into the slot's records, at slot * (5 * 256 * 8) and slot * (2 * 256 * 4) bytes
__device__ __forceinline__ void lcl_add(const LowcardChainParams &P, lds_char *l64, lds_char *l32, unsigned slot, unsigned q, unsigned e, unsigned d,
                                        unsigned t, int a1c, int a2c, unsigned row) {
    lds_u64 *a = (lds_u64 *)(l64 + __umul24(slot, 5 * 256 * 8));
    lds_u32 *c = (lds_u32 *)(l32 + (slot << 11));
    const int f1 = __mul24((int)d, P.B1c) + a1c, f2 = __mul24((int)t, P.B2c) + a2c;
    const int ev = (int)((unsigned)P.e_base32 + e);   // modulo 2^32: a code may be >= 2^31
    const int dp32 = (int)((unsigned)ev * (unsigned)f1);
    const unsigned long long dp = (unsigned long long)(long long)dp32;
    const unsigned long long ch = (unsigned long long)((long long)dp32 * (long long)f2);
    __hip_atomic_fetch_add(a + 0 * 256, (unsigned long long)(P.nq.base + (long long)q), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(a + 1 * 256, (unsigned long long)(long long)ev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(a + 2 * 256, dp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(a + 3 * 256, ch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(a + 4 * 256, (unsigned long long)(P.nd.base + (long long)d), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(c + 0 * 256, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_min(c + 1 * 256, row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ------------------------------------------------------------------ the row bodies of the lean kernels
// Where a passing row goes is a body: its LDS (lds_bytes for the launch, init for the carve-up, the zeroing, the barrier and the lane's or
// wave's two base addresses), what it pins once per tile (tile), one row of a packed scan group's word (row; r is the row id), and the
// workgroup's partial words after the last tile (finish). How a tile is loaded is not its business: lcl_rows, lcp_rows and lcs_rows below.

// field F of a row's word (lo, hi) of a packed scan group: inside one dword, so a choice of dword (uniform) and two shifts, which also
// serve a 32-bit field
template <bool FIXED, int F> __device__ __forceinline__ unsigned lcp_field(const LowcardChainParams &P, unsigned lo, unsigned hi) {
    const unsigned sh = FIXED ? (unsigned)LCP_LINEITEM.shift[F] : P.pk_shift[F], w = FIXED ? (unsigned)LCP_LINEITEM.width[F] : P.pk_width[F];
    const unsigned src = (sh & 32u) ? hi : lo;
    return (src << (32u - (sh & 31u) - w)) >> (32u - w);
}

// The columns body: lc_add's layout, a passing row added by lcl_add. FIXED: lineitem's layout of the word at compile time; otherwise the
// shifts and widths of P.
template <bool FIXED> struct ColumnsBody {
    lds_char *l64, *l32;   // this thread's column of the two accumulator arrays, as 32-bit LDS addresses
    int a1c, a2c;

    static size_t lds_bytes(int ns) { return (size_t)ns * (5 * 256 * sizeof(unsigned long long) + 2 * 256 * sizeof(unsigned)); }

    // lc_add's layout: acc32 behind acc64's ns x 5 x 256 words
    static __device__ __forceinline__ unsigned *acc32(unsigned long long *lds_acc, int ns) {
        return reinterpret_cast<unsigned *>(lds_acc + (size_t)ns * 5 * 256);
    }
    __device__ __forceinline__ void init(unsigned long long *lds_acc, int ns) {
        lc_lds_init(lds_acc, acc32(lds_acc, ns), ns);
        l64 = (lds_char *)(lds_acc + threadIdx.x);
        l32 = (lds_char *)(acc32(lds_acc, ns) + threadIdx.x);
    }
    // the addends in VGPRs (a multiply-add takes one scalar operand): once per tile, not per row
    __device__ __forceinline__ void tile(const LowcardChainParams &P) {
        a1c = P.A1c;
        a2c = P.A2c;
        asm volatile("" : "+v"(a1c), "+v"(a2c));
    }
    template <bool MASKED>
    __device__ __forceinline__ void row(const LowcardChainParams &P, unsigned lo, unsigned hi, int64_t r, int64_t rb, int64_t re, unsigned sp) const {
        bool pass = lcp_field<FIXED, PF_P>(P, lo, hi) - P.np_lo <= sp;
        if (MASKED) pass = pass && r >= rb && r < re;
        if (pass)
            lcl_add(P, l64, l32, lcp_field<FIXED, PF_SLOT>(P, lo, hi), lcp_field<FIXED, PF_Q>(P, lo, hi), lcp_field<FIXED, PF_E>(P, lo, hi),
                    lcp_field<FIXED, PF_D>(P, lo, hi), lcp_field<FIXED, PF_T>(P, lo, hi), a1c, a2c, (unsigned)r);
    }
    __device__ __forceinline__ void finish(const LowcardChainParams &P, unsigned long long *lds_acc, int ns) const {
        lc_merge(P, lds_acc, lds_acc, acc32(lds_acc, ns), ns);
    }
};

// a tile of the seven narrowed arrays into the columns body (whose FIXED is then idle: no word is taken apart)
template <bool MASKED>
__device__ __forceinline__ void lcl_rows(const v4u32 xpa, const v4u32 xpb, const v4u32 xq, const v4u32 xe0, const v4u32 xe1, const v4u32 xe2, const v4u32 xe3,
                                         const v4u32 xd, const v4u32 xt, const v4u32 k0v, const v4u32 k1v, const LowcardChainParams &P, ColumnsBody<true> &body,
                                         int64_t row, int64_t rb, int64_t re, unsigned sp) {
    unsigned p[16], q[16], e[16], d[16], t[16];
    codes_unpack2(xpa, xpb, p);
    codes_unpack1(xq, q);
    codes_unpack4(xe0, xe1, xe2, xe3, e);
    codes_unpack1(xd, d);
    codes_unpack1(xt, t);
    const unsigned r0 = (unsigned)row;
    body.tile(P);
#pragma unroll
    for (int i = 0; i < 16; i++) {
        bool pass = p[i] - P.np_lo <= sp;
        if (MASKED) pass = pass && row + lcl_row_off(i) >= rb && row + lcl_row_off(i) < re;
        if (pass) {
            const unsigned k0 = (k0v[i >> 2] >> (8 * (i & 3))) & 0xffu, k1 = (k1v[i >> 2] >> (8 * (i & 3))) & 0xffu;
            // slot = k0 nk1 + k1
            unsigned k0n = __umul24(k0, (unsigned)P.nk1);
            asm volatile("" : "+v"(k0n));   // or the compiler fuses the sum below into a 64-bit multiply-add (v_mad_u64_u32)
            lcl_add(P, body.l64, body.l32, k0n + k1, q[i], e[i], d[i], t[i], body.a1c, body.a2c, r0 + lcl_row_off(i));
        }
    }
}

// The table's packed scan group as a 64-bit word a row (P.pk: the codes of p, q, e, d, t and the slot, 8 bytes a row instead of 11 from
// seven arrays), into either body. A lane owns eight groups of two consecutive rows of a tile, LCP_GROUP rows apart:
// row = tile + 1024 wave + 128 j + 2 lane + k, so each of a tile's eight 16-byte loads per lane reads 1024 consecutive bytes per wave
// (scripts/read_packed_gfx950.hip). Element i = 2 j + k of the lane is row lcp_row_off(i). The buffers are plain vector variables, as above.
#define LCP_DECL(T) v4u32 T##w0, T##w1, T##w2, T##w3, T##w4, T##w5, T##w6, T##w7
#define LCP_ARGS(T) T##w0, T##w1, T##w2, T##w3, T##w4, T##w5, T##w6, T##w7
constexpr int LCP_GROUP = 128;
__device__ __forceinline__ constexpr int lcp_row_off(int i) { return (i >> 1) * LCP_GROUP + (i & 1); }
#define LCP_LOAD_AT(T, R0, R1, R2, R3, R4, R5, R6, R7) \
    do {                                               \
        T##w0 = ld_u32x4<true>(P.pk + (R0) * 8);       \
        T##w1 = ld_u32x4<true>(P.pk + (R1) * 8);       \
        T##w2 = ld_u32x4<true>(P.pk + (R2) * 8);       \
        T##w3 = ld_u32x4<true>(P.pk + (R3) * 8);       \
        T##w4 = ld_u32x4<true>(P.pk + (R4) * 8);       \
        T##w5 = ld_u32x4<true>(P.pk + (R5) * 8);       \
        T##w6 = ld_u32x4<true>(P.pk + (R6) * 8);       \
        T##w7 = ld_u32x4<true>(P.pk + (R7) * 8);       \
    } while (0)
// As LCL_LOAD: of a tile that does not end at or below row_end a lane loads the groups that start below row_end (a group starts at an
// even row, so it ends at most one row beyond it, inside the padding) and the first group of the range in place of each of the others.
#define LCP_SAFE(R, J) ((R) + (J) * LCP_GROUP < re ? (R) + (J) * LCP_GROUP : row_safe)
#define LCP_LOAD(T, R, T0)                                                                                                          \
    do {                                                                                                                            \
        const int64_t r_ = (R);                                                                                                     \
        if ((T0) + tile_rows <= re)                                                                                                 \
            LCP_LOAD_AT(T, r_, r_ + LCP_GROUP, r_ + 2 * LCP_GROUP, r_ + 3 * LCP_GROUP, r_ + 4 * LCP_GROUP, r_ + 5 * LCP_GROUP,      \
                        r_ + 6 * LCP_GROUP, r_ + 7 * LCP_GROUP);                                                                    \
        else                                                                                                                        \
            LCP_LOAD_AT(T, LCP_SAFE(r_, 0), LCP_SAFE(r_, 1), LCP_SAFE(r_, 2), LCP_SAFE(r_, 3), LCP_SAFE(r_, 4), LCP_SAFE(r_, 5),    \
                        LCP_SAFE(r_, 6), LCP_SAFE(r_, 7));                                                                          \
    } while (0)

template <bool MASKED, class Body>
__device__ __forceinline__ void lcp_rows(const v4u32 w0, const v4u32 w1, const v4u32 w2, const v4u32 w3, const v4u32 w4, const v4u32 w5, const v4u32 w6,
                                         const v4u32 w7, const LowcardChainParams &P, Body &body, int64_t row, int64_t rb, int64_t re, unsigned sp) {
    body.tile(P);
#define LCP_PAIR(W, J)                                                              \
    body.template row<MASKED>(P, W.x, W.y, row + lcp_row_off(2 * (J)), rb, re, sp); \
    body.template row<MASKED>(P, W.z, W.w, row + lcp_row_off(2 * (J) + 1), rb, re, sp)
    LCP_PAIR(w0, 0);
    LCP_PAIR(w1, 1);
    LCP_PAIR(w2, 2);
    LCP_PAIR(w3, 3);
    LCP_PAIR(w4, 4);
    LCP_PAIR(w5, 5);
    LCP_PAIR(w6, 6);
    LCP_PAIR(w7, 7);
#undef LCP_PAIR
}

// The bins body: the prices binned by (slot, tax, discount) instead of multiplied per row ("Bins by (slot, discount,
// tax)"). In lineitem's layout d, t and the slot are bits 12..22 of a row's high dword: idx = slot << 8 | t << 4 | d names one of nslots x 256
// bins, and f1 f2 is the same for every row of a bin. A passing row adds (1 << 44 | e code) to bin idx of its wave's own table (the count in
// bits 44..63, Σ e code below), its q code to the lane's own column of the slot, and takes the minimum of its row id into the lane's other
// column, as the columns body does. lch_fold forms the workgroup's partial words from the bins once, after the last tile.
//   LDS: u64 bins[4 waves][nslots][256], u32 cols[nslots][2][256] (Σ q code, first row id), u64 red[nslots][LC_NACC+1][4 waves] for the fold
// A wave's table receives at most 1024 rows a tile and a lane's column 16, so LC_BINS_MAX_TILES tiles per workgroup (ph_scan_plan_run keeps
// to it) bound every field:
constexpr int LCH_CNT_SHIFT = 44;
static_assert(LCP_LINEITEM.shift[PF_D] == 32 + 12 && LCP_LINEITEM.shift[PF_T] == 32 + 16 && LCP_LINEITEM.shift[PF_SLOT] == 32 + 20 &&
                  LCP_LINEITEM.width[PF_D] == 4 && LCP_LINEITEM.width[PF_T] == 4 && LCP_LINEITEM.width[PF_SLOT] == 3,
              "idx = slot << 8 | t << 4 | d is bits 12..22 of the high dword");
static_assert((1 << LCP_LINEITEM.width[PF_SLOT]) >= LC_BINS_MAX_SLOTS, "every slot of a bins launch has a code");
static_assert((uint64_t)LC_BINS_MAX_TILES * 1024 < (1ull << (64 - LCH_CNT_SHIFT)), "a bin's row count fits above bit 44");
static_assert((uint64_t)LC_BINS_MAX_TILES * 1024 * ((1ull << LCP_LINEITEM.width[PF_E]) - 1) < (1ull << LCH_CNT_SHIFT), "a bin's sum of e codes fits below bit 44");
static_assert((uint64_t)LC_BINS_MAX_TILES * 16 * ((1ull << LCP_LINEITEM.width[PF_Q]) - 1) < (1ull << 32), "a lane's sum of q codes fits 32 bits");

// lane ^ O's copy of x: within a quad a DPP move, otherwise through the LDS crossbar
template <int O> __device__ __forceinline__ unsigned lane_xor(unsigned x) {
    if constexpr (O == 1) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, false);        // quad_perm [1, 0, 3, 2]
    else if constexpr (O == 2) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xF, 0xF, false);   // quad_perm [2, 3, 0, 1]
    else return (unsigned)__shfl_xor((int)x, O);
}
template <int O> __device__ __forceinline__ unsigned long long lane_xor(unsigned long long x) {
    return (unsigned long long)lane_xor<O>((unsigned)(x >> 32)) << 32 | lane_xor<O>((unsigned)x);
}
struct FoldSum {
    static constexpr unsigned long long id = 0;
    static __device__ __forceinline__ unsigned long long op(unsigned long long a, unsigned long long b) { return a + b; }
};
struct FoldMin {
    static constexpr unsigned id = 0xffffffffu;
    static __device__ __forceinline__ unsigned op(unsigned a, unsigned b) { return min(a, b); }
};
// One exchange of the halving fold. A lane holds words [base, base + N) of the fold in v[0..N), those at or beyond `end` being the
// identity. The lane whose bit O is clear keeps the first H = ceil(N / 2), its partner lane ^ O the others (padded to H with the identity),
// and each adds the other's copy of what it keeps: H exchanges, after which the pair's sums of N words lie in two lanes instead of twice in
// both. tests/test_hist_fold_halving.py restates the schedule.
template <int N, int O, class F, class T> __device__ __forceinline__ void lch_halve(T *v, int lane, int &base, int &end) {
    constexpr int H = (N + 1) / 2;
    const bool up = lane & O;
#pragma unroll
    for (int i = 0; i < H; i++) {
        const T lo = v[i], hi = i + H < N ? v[i + H] : (T)F::id;
        v[i] = F::op(up ? hi : lo, lane_xor<O>(up ? lo : hi));
    }
    if (up) base += H;
    else end = min(end, base + H);
}

// The workgroup's partial words from its bins. Thread j owns bin (d = j & 15, t = j >> 4) of every slot: n rows and Σ e code E over the four
// waves' tables give Σ e = e_base n + E, and f1(d), f2(t) are the bin's factors, so Σ e f1 = f1 Σ e and Σ e f1 f2 = f2 f1 Σ e over the bin's
// rows; Σ d = (d_base + d) n; Σ q = q_base n + the lane's q column. All in wrapping 64-bit arithmetic: each workgroup total is the integer
// the columns body sums row by row, which the plan's overflow proof keeps below 4e18, so no wrapped intermediate changes it.
// A lane so holds LC_NACC words per slot, word s LC_NACC + a of 36 (a slot beyond ns: zeros), and a first row id per slot. Six halving
// exchanges (18 + 9 + 5 + 3 + 2 + 1 = 38 of 64 bits, where a butterfly per word makes 36 x 6, and 3 + 2 + 1 + 1 + 1 + 1 = 9 of 32 bits for
// the minima) leave each word's wave total in one lane, which stores it to red; the four waves' totals are then summed and stored in
// lc_merge's order. The adds are the butterflies' in another order: wrapping and commutative, so every partial is the same integer.
constexpr int LCH_FOLD_WORDS = LC_BINS_MAX_SLOTS * LC_NACC;
__device__ __forceinline__ void lch_fold(const LowcardChainParams &P, unsigned long long *lds_acc, const unsigned long long *bins, const unsigned *cols,
                                         unsigned long long *red, int ns) {
    __syncthreads();
    const int j = threadIdx.x, w = j >> 6, lane = j & 63;
    const int per_slot = LC_NACC + 1;
    const long long d = j & 15, t = j >> 4;
    const long long f1 = (long long)P.A1c + (long long)P.B1c * d, f2 = (long long)P.A2c + (long long)P.B2c * t;
    unsigned long long v[LCH_FOLD_WORDS];
    unsigned m[LC_BINS_MAX_SLOTS];
#pragma unroll
    for (int s = 0; s < LC_BINS_MAX_SLOTS; s++) {
        const int sc = min(s, ns - 1);   // a slot beyond ns: the last slot's loads, the identities selected (no branch)
        unsigned long long n = 0, E = 0;
        for (int k = 0; k < 4; k++) {
            const unsigned long long b = bins[(size_t)(k * ns + sc) * 256 + j];
            n += b >> LCH_CNT_SHIFT;
            E += b & ((1ull << LCH_CNT_SHIFT) - 1);
        }
        const unsigned q = cols[(sc * 2 + 0) * 256 + j], r = cols[(sc * 2 + 1) * 256 + j];
        const bool live = s < ns;
        unsigned long long *x = v + s * LC_NACC;
        x[1] = (unsigned long long)(long long)P.e_base32 * n + E;
        x[0] = (unsigned long long)P.nq.base * n + q;
        x[2] = (unsigned long long)f1 * x[1];
        x[3] = (unsigned long long)f2 * x[2];
        x[4] = (unsigned long long)(P.nd.base + d) * n;
        x[5] = n;
#pragma unroll
        for (int a = 0; a < LC_NACC; a++) x[a] = live ? x[a] : 0;
        m[s] = live ? r : FoldMin::id;
    }
    static_assert(LCH_FOLD_WORDS == 36 && LC_BINS_MAX_SLOTS == 6, "the exchanges below are written for 36 words and 6 minima");
    int base = 0, end = LCH_FOLD_WORDS, mbase = 0, mend = LC_BINS_MAX_SLOTS;
    lch_halve<36, 1, FoldSum>(v, lane, base, end);
    lch_halve<18, 2, FoldSum>(v, lane, base, end);
    lch_halve<9, 4, FoldSum>(v, lane, base, end);
    lch_halve<5, 8, FoldSum>(v, lane, base, end);
    lch_halve<3, 16, FoldSum>(v, lane, base, end);
    lch_halve<2, 32, FoldSum>(v, lane, base, end);
    lch_halve<6, 1, FoldMin>(m, lane, mbase, mend);
    lch_halve<3, 2, FoldMin>(m, lane, mbase, mend);
    lch_halve<2, 4, FoldMin>(m, lane, mbase, mend);
    lch_halve<1, 8, FoldMin>(m, lane, mbase, mend);
    lch_halve<1, 16, FoldMin>(m, lane, mbase, mend);
    lch_halve<1, 32, FoldMin>(m, lane, mbase, mend);
    // the lane that ends with word `base` (every word of a slot below ns has exactly one) stores it for its wave
    if (base < end && base / LC_NACC < ns) red[(base / LC_NACC * per_slot + base % LC_NACC) * 4 + w] = v[0];
    if (mbase < mend && mbase < ns) red[(mbase * per_slot + LC_NACC) * 4 + w] = m[0];
    __syncthreads();
    if (j < ns * per_slot) {
        const unsigned long long *r = red + j * 4;
        long long v;
        if (j % per_slot < LC_NACC) v = (long long)(r[0] + r[1] + r[2] + r[3]);
        else v = (long long)min(min(r[0], r[1]), min(r[2], r[3]));
        if (P.tail.done) scan_tail_put(P.partials, ns * per_slot, j, v);
        else P.partials[(int64_t)blockIdx.x * ns * per_slot + j] = v;
    }
    if (P.tail.done) {
        __syncthreads();   // as lc_merge: the first 2 KiB of LDS serve the tail
        scan_tail(P.partials, P.tail, lds_acc);
    }
}

// lineitem's layout only (lcp_field<true, F>)
struct BinsBody {
    lds_char *b64, *c32;   // the wave's table and the lane's columns, as 32-bit LDS addresses

    struct Lds {
        unsigned long long *bins;
        unsigned *cols;
        unsigned long long *red;
        size_t nbins;   // 64-bit words of bins
    };
    static __device__ __forceinline__ Lds carve(unsigned long long *lds_acc, int ns) {
        const size_t nbins = (size_t)4 * ns * 256;
        return {lds_acc, reinterpret_cast<unsigned *>(lds_acc + nbins), lds_acc + nbins + (size_t)ns * 256, nbins};   // red: behind cols' ns x 512 words of 32 bits
    }
    static size_t lds_bytes(int ns) { return (size_t)ns * (4 * 256 * 8 + 2 * 256 * 4 + (LC_NACC + 1) * 4 * 8); }

    __device__ __forceinline__ void init(unsigned long long *lds_acc, int ns) {
        const Lds L = carve(lds_acc, ns);
        for (int i = threadIdx.x; i < (int)L.nbins; i += 256) L.bins[i] = 0;
        for (int s = 0; s < ns; s++) {
            L.cols[(s * 2 + 0) * 256 + threadIdx.x] = 0;
            L.cols[(s * 2 + 1) * 256 + threadIdx.x] = 0xffffffffu;
        }
        __syncthreads();
        b64 = (lds_char *)(L.bins + (size_t)(threadIdx.x >> 6) * ns * 256);
        c32 = (lds_char *)(L.cols + threadIdx.x);
    }
    __device__ __forceinline__ void tile(const LowcardChainParams &) {}
    template <bool MASKED>
    __device__ __forceinline__ void row(const LowcardChainParams &P, unsigned lo, unsigned hi, int64_t r, int64_t rb, int64_t re, unsigned sp) const {
        bool pass = lcp_field<true, PF_P>(P, lo, hi) - P.np_lo <= sp;
        if (MASKED) pass = pass && r >= rb && r < re;
        if (pass) {
            const unsigned idx = (hi >> 12) & 0x7ffu;
            lds_u64 *a = (lds_u64 *)(b64 + idx * 8);
            lds_u32 *c = (lds_u32 *)(c32 + (idx >> 8) * (2 * 256 * 4));
            __hip_atomic_fetch_add(a, 1ull << LCH_CNT_SHIFT | lcp_field<true, PF_E>(P, lo, hi), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(c, lcp_field<true, PF_Q>(P, lo, hi), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_min(c + 256, (unsigned)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    __device__ __forceinline__ void finish(const LowcardChainParams &P, unsigned long long *lds_acc, int ns) const {
        const Lds L = carve(lds_acc, ns);
        lch_fold(P, lds_acc, L.bins, L.cols, L.red, ns);
    }
};

// A group in the split form (pack_layout.h: 7 bytes a row, lineitem's layout), into either fixed-layout body. A wave reads one block
// of 1024 rows a tile, 7168 consecutive bytes: a lane's loads 0..3 are the low dwords of its four quads, rows 256 j + 4 lane + k of the
// block, and its loads 4..6 the twelve dwords of those quads' high parts, D[3 j + r] for quad j. Rows 0..2 of a quad take dwords A, B, C as
// their high dword as they are (no field reaches the top byte, and no row body looks at it); row 3's is put together from the three top
// bytes, two v_perm_b32 a quad. Blocks lie at absolute multiples of 1024 rows, so tiles start at row_begin rounded down to 4096 and the
// masked body masks the rows below row_begin. A tile at or beyond row_end (loaded ahead, never consumed) reads the range's first tile
// instead, one uniform select; a tile that starts below row_end lies inside the padded table.
#define LCS_DECL(T) v4u32 T##l0, T##l1, T##l2, T##l3, T##h0, T##h1, T##h2
#define LCS_ARGS(T) T##l0, T##l1, T##l2, T##l3, T##h0, T##h1, T##h2
#define LCS_LOAD(T, R, T0)                                                                       \
    do {                                                                                         \
        (void)row_safe;   /* the substitute is a whole tile, not a 16-row group */             \
        const int64_t t_ = (T0) < re ? (T0) : tile_first;                                        \
        const uint8_t *b_ = lane_base + t_ * (SPLIT_BLOCK_BYTES / SPLIT_BLOCK_ROWS);             \
        T##l0 = ld_u32x4<true>(b_);                                                              \
        T##l1 = ld_u32x4<true>(b_ + 1024);                                                       \
        T##l2 = ld_u32x4<true>(b_ + 2048);                                                       \
        T##l3 = ld_u32x4<true>(b_ + 3072);                                                       \
        T##h0 = ld_u32x4<true>(b_ + 4096);                                                       \
        T##h1 = ld_u32x4<true>(b_ + 5120);                                                       \
        T##h2 = ld_u32x4<true>(b_ + 6144);                                                       \
    } while (0)
static_assert(SPLIT_BLOCK_BYTES % SPLIT_BLOCK_ROWS == 0 && SPLIT_BLOCK_BYTES == 7 * 1024 && SPLIT_LOW_DWORDS * 4 == 4096,
              "a block is seven loads of 1024 bytes per wave, the high parts from byte 4096 on");

// the 24-bit high part of a quad's row 3 from the top bytes of its dwords A, B, C (split_quad_decode)
__device__ __forceinline__ unsigned lcs_row3(unsigned A, unsigned B, unsigned C) {
    const unsigned ab = __builtin_amdgcn_perm(B, A, 0x0c0c0703u);   // byte 0 = A's byte 3, byte 1 = B's byte 3
    return __builtin_amdgcn_perm(C, ab, 0x0c070100u);               // byte 2 = C's byte 3, byte 3 = 0
}

template <bool MASKED, class Body>
__device__ __forceinline__ void lcs_rows(const v4u32 l0, const v4u32 l1, const v4u32 l2, const v4u32 l3, const v4u32 h0, const v4u32 h1, const v4u32 h2,
                                         const LowcardChainParams &P, Body &body, int64_t row, int64_t rb, int64_t re, unsigned sp) {
    body.tile(P);
#define LCS_QUAD(L, A, B, C, J)                                            \
    body.template row<MASKED>(P, L.x, A, row + 256 * (J), rb, re, sp);     \
    body.template row<MASKED>(P, L.y, B, row + 256 * (J) + 1, rb, re, sp); \
    body.template row<MASKED>(P, L.z, C, row + 256 * (J) + 2, rb, re, sp); \
    body.template row<MASKED>(P, L.w, lcs_row3(A, B, C), row + 256 * (J) + 3, rb, re, sp)
    LCS_QUAD(l0, h0.x, h0.y, h0.z, 0);
    LCS_QUAD(l1, h0.w, h1.x, h1.y, 1);
    LCS_QUAD(l2, h1.z, h1.w, h2.x, 2);
    LCS_QUAD(l3, h2.y, h2.z, h2.w, 3);
#undef LCS_QUAD
}

// ------------------------------------------------------------------ the lean kernels: one frame
// A kernel instance is a loader and a body: the body's init, the tile geometry, the lean tile loop over the loader's register buffers and
// the body's finish. A loader is its DECL / LOAD / ARGS macros and rows function above and, here, a name for the instance with the two
// numbers of its geometry. Every loader gives a wave 1024 consecutive rows of a tile and a lane the first `lane_rows` of them; the first
// tile starts at row_begin rounded down to `anchor` rows: 16, or for the split form's absolute blocks a whole tile.
struct ArraysLoad {   // the seven narrowed arrays (LCL_*, lcl_rows: the columns body only)
    static constexpr int lane_rows = 4, anchor = 16;
};
struct WordLoad {     // a packed scan group, one 64-bit word a row (LCP_*, lcp_rows)
    static constexpr int lane_rows = 2, anchor = 16;
};
struct SplitLoad {    // a packed scan group in the split form, lineitem's layout (LCS_*, lcs_rows)
    static constexpr int lane_rows = 4, anchor = 4096;
};
static_assert(4 * LCL_GROUP == 1024 && 8 * LCP_GROUP == 1024 && SPLIT_BLOCK_ROWS == 1024, "a wave's rows of a tile");

#define LCL_BODY(M, T) lcl_rows<M>(LCL_ARGS(T), P, body, row, rb, re, sp)
#define LCP_BODY(M, T) lcp_rows<M>(LCP_ARGS(T), P, body, row, rb, re, sp)
#define LCS_BODY(M, T) lcs_rows<M>(LCS_ARGS(T), P, body, row, rb, re, sp)
template <class Loader, class Body> __global__ __launch_bounds__(256, 2) void lowcard_chain_kernel_group(LowcardChainParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds_acc[];
    const int ns = P.nslots;
    Body body;
    body.init(lds_acc, ns);

    const int64_t tile_rows = 4096;
    const bool none = P.np_lo > P.np_hi;
    const unsigned sp = P.np_hi - P.np_lo;
    const int64_t rb = P.row_begin, re = none ? 0 : P.row_end;
    const int64_t tile_first = rb & ~(int64_t)(Loader::anchor - 1);
    int64_t tile0 = tile_first + (int64_t)blockIdx.x * tile_rows;
    int64_t row = tile0 + (threadIdx.x >> 6) * 1024 + (threadIdx.x & 63) * Loader::lane_rows;   // the lane's first row of the tile
    const int64_t stride = (int64_t)gridDim.x * tile_rows;
    if constexpr (std::is_same_v<Loader, SplitLoad>) {
        const uint8_t *lane_base = P.pk + (threadIdx.x >> 6) * SPLIT_BLOCK_BYTES + (threadIdx.x & 63) * 16;
        PH_LEAN_TILE_LOOP(LCS_DECL, LCS_LOAD, LCS_BODY)
    } else if constexpr (std::is_same_v<Loader, WordLoad>) {
        PH_LEAN_TILE_LOOP(LCP_DECL, LCP_LOAD, LCP_BODY)
    } else {
        PH_LEAN_TILE_LOOP(LCL_DECL, LCL_LOAD, LCL_BODY)
    }
    body.finish(P, lds_acc, ns);
}
#undef LCL_BODY
#undef LCP_BODY
#undef LCS_BODY

// The end of a merge wave (one wave per accumulator word j; lane 0 holds the merged word): store it, and — when the merge is to publish (T.done) — take
// a ticket; the wave that finishes last copies all words into the mapped mailbox and stores the sequence number (what publish_kernel does as one more
// launch). Every host-visible store comes from that one wave, in publish_kernel's order: words, system fence, number.
__device__ __forceinline__ void merge_finish(const ScanTail &T, int j, unsigned long long lo, long long hi, unsigned long long *out_lo, long long *out_hi) {
    const int lane = threadIdx.x;
    if (!T.done) {
        if (lane == 0) {
            out_lo[j] = lo;
            out_hi[j] = hi;
        }
        return;
    }
    unsigned ticket = 0;
    if (lane == 0) {
        __hip_atomic_store(out_lo + j, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // where the other XCDs can read them (not this XCD's write-back L2)
        __hip_atomic_store(out_hi + j, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_s_waitcnt(0);   // acknowledged before the ticket
        ticket = __hip_atomic_fetch_add(T.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    ticket = (unsigned)__shfl((int)ticket, 0);
    if (ticket != gridDim.x - 1) return;
    for (int k = lane; k < T.nacc; k += 64) {
        T.mbox[k] = __hip_atomic_load(out_lo + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        T.mbox[T.nacc + k] = (unsigned long long)__hip_atomic_load(out_hi + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __threadfence_system();
    if (lane == 0) {
        *T.done = 0;
        __hip_atomic_store(T.flag, T.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ------------------------------------------------------------------ partial merge
// A lane's words of accumulator j come in batches of MERGE_BATCH: blocks b0, b0 + 64, ..., all loaded before the first is used, so a
// batch costs the wave one round trip to memory instead of one per word (512 blocks: one batch). A block at or beyond nblocks loads
// block b0's word again (b0 < nblocks: an address that is there, so no load hangs on a branch) and contributes `identity`.
constexpr int MERGE_BATCH = 8;
__device__ __forceinline__ void merge_load_batch(const long long *__restrict__ partials, int nblocks, int nacc, int j, int b0, long long identity,
                                                 long long (&v)[MERGE_BATCH]) {
#pragma unroll
    for (int i = 0; i < MERGE_BATCH; i++) {
        const int b = b0 + 64 * i;
        v[i] = partials[(int64_t)(b < nblocks ? b : b0) * nacc + j];
    }
#pragma unroll
    for (int i = 0; i < MERGE_BATCH; i++)
        if (b0 + 64 * i >= nblocks) v[i] = identity;
}

// a lane's 128-bit sum of its words of accumulator j: positives and negatives accumulated as unsigned magnitudes to keep carries simple
__device__ __forceinline__ void merge_lane_sum(const long long *__restrict__ partials, int nblocks, int nacc, int j, unsigned long long &lo, long long &hi) {
    lo = 0;
    hi = 0;
    for (int b0 = threadIdx.x; b0 < nblocks; b0 += 64 * MERGE_BATCH) {
        long long w[MERGE_BATCH];
        merge_load_batch(partials, nblocks, nacc, j, b0, 0, w);
#pragma unroll
        for (int i = 0; i < MERGE_BATCH; i++) {
            const long long v = w[i];
            unsigned long long nlo = lo + (unsigned long long)v;
            hi += (nlo < lo ? 1 : 0) + (v < 0 ? -1 : 0);
            lo = nlo;
        }
    }
}

// a lane's minimum (MAX = false) or maximum of its words of accumulator j
template <bool MAX> __device__ __forceinline__ long long merge_lane_minmax(const long long *__restrict__ partials, int nblocks, int nacc, int j) {
    const long long identity = MAX ? INT64_MIN : INT64_MAX;
    long long m = identity;
    for (int b0 = threadIdx.x; b0 < nblocks; b0 += 64 * MERGE_BATCH) {
        long long w[MERGE_BATCH];
        merge_load_batch(partials, nblocks, nacc, j, b0, identity, w);
#pragma unroll
        for (int i = 0; i < MERGE_BATCH; i++) m = MAX ? (w[i] > m ? w[i] : m) : (w[i] < m ? w[i] : m);
    }
    return m;
}

// out[j] = 128-bit sum over blocks of int64 partials[b*nacc + j]. One wave per accumulator.
// When min_stride > 0, accumulators with j % min_stride == min_stride-1 are minima (first row ids).
__global__ __launch_bounds__(64) void merge_partials_kernel(const long long *__restrict__ partials,
                                                            int nblocks, int nacc, int min_stride,
                                                            unsigned long long *__restrict__ out_lo,
                                                            long long *__restrict__ out_hi, ScanTail T) {
    int j = blockIdx.x;
    if (min_stride > 0 && j % min_stride == min_stride - 1) {
        long long m = merge_lane_minmax<false>(partials, nblocks, nacc, j);
        for (int o = 32; o > 0; o >>= 1) {
            long long v = __shfl_xor(m, o);
            m = v < m ? v : m;
        }
        merge_finish(T, j, (unsigned long long)m, 0, out_lo, out_hi);
        return;
    }
    unsigned long long lo;
    long long hi;
    merge_lane_sum(partials, nblocks, nacc, j, lo, hi);
    // tree-combine 128-bit lane values
    for (int o = 32; o > 0; o >>= 1) {
        unsigned long long olo = __shfl_xor(lo, o);
        long long ohi = __shfl_xor(hi, o);
        unsigned long long nlo = lo + olo;
        hi = hi + ohi + (nlo < lo ? 1 : 0);
        lo = nlo;
    }
    merge_finish(T, j, lo, hi, out_lo, out_hi);
}

// out[j] over blocks with a per-word operation: op = (opmask >> 2*(j % stride)) & 3 — 0: 128-bit sum,
// 1: signed min, 2: signed max (MIN/MAX accumulators and first-row ids of the generated kernels)
__global__ __launch_bounds__(64) void merge_partials_ops_kernel(const long long *__restrict__ partials,
                                                                int nblocks, int nacc, int stride, unsigned long long opmask,
                                                                unsigned long long *__restrict__ out_lo,
                                                                long long *__restrict__ out_hi, ScanTail T) {
    const int j = blockIdx.x;
    const int op = (int)((opmask >> (2 * (j % stride))) & 3);
    if (op != 0) {
        long long m = op == 1 ? merge_lane_minmax<false>(partials, nblocks, nacc, j) : merge_lane_minmax<true>(partials, nblocks, nacc, j);
        for (int o = 32; o > 0; o >>= 1) {
            long long v = __shfl_xor(m, o);
            m = op == 1 ? (v < m ? v : m) : (v > m ? v : m);
        }
        merge_finish(T, j, (unsigned long long)m, m < 0 ? -1 : 0, out_lo, out_hi);
        return;
    }
    unsigned long long lo;
    long long hi;
    merge_lane_sum(partials, nblocks, nacc, j, lo, hi);
    for (int o = 32; o > 0; o >>= 1) {
        unsigned long long olo = __shfl_xor(lo, o);
        long long ohi = __shfl_xor(hi, o);
        unsigned long long nlo = lo + olo;
        hi = hi + ohi + (nlo < lo ? 1 : 0);
        lo = nlo;
    }
    merge_finish(T, j, lo, hi, out_lo, out_hi);
}

// ------------------------------------------------------------------ launches
// Which instance runs is decided by scan_inst.h (fs_choose / lc_choose) in scan_plan.hip; what is left here is the kernel of each instance and,
// for the instances with run-time code widths, the load form (sw.nt) and the wide kernel's unroll (sw.unroll).

int launch_filter_sumprod(ph_ctx *ctx, const FilterSumProdParams &P, FsInst inst, const ScanSwitches &sw, int grid) {
    switch (inst) {
    case FSI_NARROW_FIXED32:
        filter_sumprod_kernel_for<true, true, 2, 1, 1, 4><<<grid, 256, 0, ctx->stream>>>(P);
        break;
    case FSI_NARROW_RT64: case FSI_NARROW_RT32:
        dispatch_bool(sw.nt, [&](auto NT) { dispatch_bool(inst == FSI_NARROW_RT32, [&](auto P32) {
            filter_sumprod_kernel_for<NT(), P32(), 0, 0, 0, 0><<<grid, 256, 0, ctx->stream>>>(P);
        }); });
        break;
    case FSI_WIDE:
        dispatch_bool(sw.nt, [&](auto NT) { filter_sumprod_kernel<NT()><<<grid, 256, 0, ctx->stream>>>(P); });
        break;
    }
    PH_HIP(hipGetLastError());
    return PH_OK;
}

// one instance of the lowcard_chain kernels: up to 160 KiB of LDS, above the default dynamic limit
template <auto Kernel>
static int launch_lowcard_inst(ph_ctx *ctx, const LowcardChainParams &P, int grid, size_t lds) {
    PH_CHECK(raise_lds<Kernel>(ctx, 160 * 1024));
    Kernel<<<grid, 256, lds, ctx->stream>>>(P);
    PH_HIP(hipGetLastError());
    return PH_OK;
}

template <class Loader, class Body> static int launch_lowcard_group(ph_ctx *ctx, const LowcardChainParams &P, int grid) {
    return launch_lowcard_inst<lowcard_chain_kernel_group<Loader, Body>>(ctx, P, grid, Body::lds_bytes(P.nslots));
}

int launch_lowcard_chain(ph_ctx *ctx, const LowcardChainParams &P, LcInst inst, const ScanSwitches &sw, int grid) {
    const size_t lds = ColumnsBody<true>::lds_bytes(P.nslots);   // the wide and *_for kernels keep their sums in the same columns
    switch (inst) {
    case LCI_BINS: return launch_lowcard_group<WordLoad, BinsBody>(ctx, P, grid);
    case LCI_SPLIT_BINS: return launch_lowcard_group<SplitLoad, BinsBody>(ctx, P, grid);
    case LCI_SPLIT_COLUMNS: return launch_lowcard_group<SplitLoad, ColumnsBody<true>>(ctx, P, grid);
    case LCI_PACKED_FIXED: return launch_lowcard_group<WordLoad, ColumnsBody<true>>(ctx, P, grid);
    case LCI_PACKED_RT: return launch_lowcard_group<WordLoad, ColumnsBody<false>>(ctx, P, grid);
    case LCI_LEAN: return launch_lowcard_group<ArraysLoad, ColumnsBody<true>>(ctx, P, grid);
    case LCI_NARROW_FIXED32: return launch_lowcard_inst<lowcard_chain_kernel_for<true, true, 2, 1, 4, 1, 1>>(ctx, P, grid, lds);
    case LCI_NARROW_RT64: case LCI_NARROW_RT32:
        return dispatch_bool(sw.nt, [&](auto NT) { return dispatch_bool(inst == LCI_NARROW_RT32, [&](auto P32) {
            return launch_lowcard_inst<lowcard_chain_kernel_for<NT(), P32(), 0, 0, 0, 0, 0>>(ctx, P, grid, lds);
        }); });
    case LCI_WIDE:
        if (!sw.nt) return launch_lowcard_inst<lowcard_chain_kernel<false, 1>>(ctx, P, grid, lds);
        return dispatch_int<3, 2, 1>(sw.unroll, [&](auto U) { return launch_lowcard_inst<lowcard_chain_kernel<true, U()>>(ctx, P, grid, lds); });
    }
    return PH_EINVAL;
}

int launch_merge_partials(ph_ctx *ctx, const long long *partials, int nblocks, int nacc,
                          int min_stride, unsigned long long *out_lo, long long *out_hi, const ScanTail *publish) {
    ScanTail T = {};
    if (publish && publish->mbox) T = *publish;
    merge_partials_kernel<<<nacc, 64, 0, ctx->stream>>>(partials, nblocks, nacc, min_stride, out_lo,
                                                        out_hi, T);
    PH_HIP(hipGetLastError());
    return PH_OK;
}


int launch_merge_partials_ops(ph_ctx *ctx, const long long *partials, int nblocks, int nacc, int stride,
                              unsigned long long opmask, unsigned long long *out_lo, long long *out_hi, const ScanTail *publish) {
    ScanTail T = {};
    if (publish && publish->mbox) T = *publish;
    merge_partials_ops_kernel<<<nacc, 64, 0, ctx->stream>>>(partials, nblocks, nacc, stride, opmask, out_lo, out_hi, T);
    PH_HIP(hipGetLastError());
    return PH_OK;
}

}  // namespace ph
