// Issue cost of the LDS atomics of the packed lowcard_chain scan per passing row: today's seven on lane-private columns against three into
// (slot, discount, tax) bins ("Bins by (slot, discount, tax)").
//
//   hipcc --offload-arch=gfx950 -O3 -o lds_hist_gfx950 lds_hist_gfx950.hip && ./lds_hist_gfx950 > profiles/lds_hist_gfx950.txt
//   hipcc --offload-arch=gfx950 -O3 -S --cuda-device-only lds_hist_gfx950.hip      (to see which instructions the streams became)
//
// As scripts/lds_issue_gfx950.hip: no-return atomics, every wave issues ITERS x ROWS rows of one stream, waits for the LDS queue to drain
// and takes the s_memtime delta around it; one workgroup per CU of 256 threads (4 waves per CU, one per SIMD) or 512 (8). A lane's bin of
// each of the ROWS rows of an iteration, idx = slot << 8 | t << 4 | d, comes from a table the host draws once with a fixed seed:
// slots with weights 0.50 / 0.246 / 0.246 / 0.008, d uniform over 11 values, t uniform over 9 (lineitem's shape).
//   (a) columns       5 x ds_add_u64 + ds_add_u32 + ds_min_u32 to the lane's own columns of slot idx >> 8 (what the kernel issues today)
//   (b) bins          ds_add_u64 and ds_add_u32 to bin idx of the wave's own tables, ds_min_u32 to the lane's own column of the slot
//   (c) one bin       (b) with every lane of every row on one bin: the worst case
//   (d) bins64 + col  (b) with the 32-bit add to the lane's own column of the slot instead
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                                      \
    do {                                                                           \
        hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) {                                                    \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                \
            exit(1);                                                               \
        }                                                                          \
    } while (0)

constexpr int ROWS = 8, ITERS = 2048, NSLOTS = 6, NBINS = NSLOTS * 256, MAXT = 512;

enum Stream { COLUMNS, BINS, BINS64_COL, NKERNELS };

typedef __attribute__((address_space(3))) char lds_char;
typedef __attribute__((address_space(3))) unsigned long long lds_u64;
typedef __attribute__((address_space(3))) unsigned lds_u32;

#define ADD64(p, v) __hip_atomic_fetch_add((lds_u64 *)(p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define ADD32(p, v) __hip_atomic_fetch_add((lds_u32 *)(p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define MIN32(p, v) __hip_atomic_fetch_min((lds_u32 *)(p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)

// bytes of LDS of a workgroup of T threads: the 64-bit part, the 32-bit sums, the first-row columns [NSLOTS][T] (in this order)
static __host__ __device__ unsigned bytes64(int s, unsigned T) { return s == COLUMNS ? NSLOTS * 5 * T * 8 : (T / 64) * NBINS * 8; }
static __host__ __device__ unsigned bytes32(int s, unsigned T) { return s == BINS ? (T / 64) * NBINS * 4 : NSLOTS * T * 4; }
static __host__ __device__ unsigned bytes_min(unsigned T) { return NSLOTS * T * 4; }

template <int S> __global__ void stream_kernel(const unsigned *idx, const unsigned *in, unsigned long long *ticks, unsigned long long *sink) {
    extern __shared__ __attribute__((aligned(16))) unsigned lds[];
    const unsigned T = blockDim.x, tid = threadIdx.x, wave = tid >> 6;
    const unsigned b64 = bytes64(S, T), b32 = bytes32(S, T), bmin = bytes_min(T);
    const unsigned nsum = (b64 + b32) / 4, nall = nsum + bmin / 4;
    for (unsigned i = tid; i < nall; i += T) lds[i] = i < nsum ? 0u : 0xffffffffu;
    __syncthreads();
    lds_char *base = (lds_char *)lds;
    // byte addresses of this lane's three targets of each of the ROWS rows of an iteration
    unsigned o64[ROWS], o32[ROWS], omin[ROWS];
    for (int r = 0; r < ROWS; r++) {
        const unsigned ix = idx[r * MAXT + tid], slot = ix >> 8;
        if (S == COLUMNS) o64[r] = slot * (5 * T * 8) + tid * 8;
        else o64[r] = wave * (NBINS * 8) + ix * 8;
        if (S == BINS) o32[r] = b64 + wave * (NBINS * 4) + ix * 4;
        else o32[r] = b64 + slot * (T * 4) + tid * 4;
        omin[r] = b64 + b32 + slot * (T * 4) + tid * 4;
    }
    unsigned long long v = ((unsigned long long)in[0] << 44) | (in[1] + tid);   // count 1 and a price code
    unsigned w = in[2] + (tid & 31);                                           // a quantity code
    unsigned row = in[3] + tid;
    asm volatile("" : "+v"(v), "+v"(w), "+v"(row));
    const unsigned s64 = T * 8;   // column stride of (a)
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    for (int it = 0; it < ITERS; it++) {
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            lds_char *a = base + o64[r];
            ADD64(a, v);
            if (S == COLUMNS) {
                ADD64(a + s64, v);
                ADD64(a + 2 * s64, v);
                ADD64(a + 3 * s64, v);
                ADD64(a + 4 * s64, v);
            }
            ADD32(base + o32[r], w);
            MIN32(base + omin[r], row);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    __syncthreads();
    unsigned long long s = 0;
    for (unsigned i = tid; i < nall; i += T) s += lds[i];
    const unsigned gid = blockIdx.x * T + tid;
    sink[gid] = s;
    if ((tid & 63) == 0) ticks[gid >> 6] = t1 - t0;
}

template <int S> static double run(int grid, int threads, const unsigned *idx, const unsigned *in, unsigned long long *ticks, unsigned long long *sink) {
    const int waves = grid * threads / 64;
    const size_t lds = (size_t)bytes64(S, threads) + bytes32(S, threads) + bytes_min(threads);
    if (lds > 160 * 1024) {
        fprintf(stderr, "stream %d: %zu bytes of LDS\n", S, lds);
        exit(1);
    }
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(&stream_kernel<S>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    double best = 0;
    for (int rep = 0; rep < 3; rep++) {   // the first launch also loads the code object
        stream_kernel<S><<<grid, threads, lds>>>(idx, in, ticks, sink);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        std::vector<unsigned long long> h((size_t)waves);
        CK(hipMemcpy(h.data(), ticks, sizeof(unsigned long long) * (size_t)waves, hipMemcpyDeviceToHost));
        double sum = 0;
        for (unsigned long long v : h) sum += (double)v;
        const double mean = sum / waves / ((double)ITERS * ROWS);   // per wave-row
        if (rep == 0 || mean < best) best = mean;
    }
    return best;
}

// a fixed-seed generator (splitmix64), uniform in [0, 1)
static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static double rnd() {
    unsigned long long z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return (double)(z >> 11) / 9007199254740992.0;
}

int main() {
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int grid = prop.multiProcessorCount;
    std::vector<unsigned> drawn((size_t)ROWS * MAXT), one((size_t)ROWS * MAXT);
    for (size_t i = 0; i < drawn.size(); i++) {
        const double u = rnd();
        const unsigned slot = u < 0.50 ? 0 : u < 0.746 ? 1 : u < 0.992 ? 2 : 3;
        const unsigned d = (unsigned)(rnd() * 11), t = (unsigned)(rnd() * 9);
        drawn[i] = slot << 8 | t << 4 | d;
        one[i] = 0u << 8 | 4u << 4 | 5u;
    }
    unsigned hin[4] = {1, 1000000, 7, 12345};   // the operands: count, price code, quantity code, row id
    unsigned *idx_drawn, *idx_one, *in;
    unsigned long long *ticks, *sink;
    CK(hipMalloc(&idx_drawn, sizeof(unsigned) * drawn.size()));
    CK(hipMalloc(&idx_one, sizeof(unsigned) * one.size()));
    CK(hipMemcpy(idx_drawn, drawn.data(), sizeof(unsigned) * drawn.size(), hipMemcpyHostToDevice));
    CK(hipMemcpy(idx_one, one.data(), sizeof(unsigned) * one.size(), hipMemcpyHostToDevice));
    CK(hipMalloc(&in, sizeof hin));
    CK(hipMemcpy(in, hin, sizeof hin, hipMemcpyHostToDevice));
    CK(hipMalloc(&ticks, sizeof(unsigned long long) * (size_t)grid * (MAXT / 64)));
    CK(hipMalloc(&sink, sizeof(unsigned long long) * (size_t)grid * MAXT));
    const char *const name[4] = {"(a) columns: 5 add_u64 + add_u32 + min_u32", "(b) bins: add_u64 + add_u32 + min_u32", "(c) as (b), every lane on one bin",
                                 "(d) bins add_u64, column add_u32 + min_u32"};
    const int insts[4] = {7, 3, 3, 3};
    double t[4][2];
    for (int w = 0; w < 2; w++) {
        const int th = w == 0 ? 256 : 512;
        t[0][w] = run<COLUMNS>(grid, th, idx_drawn, in, ticks, sink);
        t[1][w] = run<BINS>(grid, th, idx_drawn, in, ticks, sink);
        t[2][w] = run<BINS>(grid, th, idx_one, in, ticks, sink);
        t[3][w] = run<BINS64_COL>(grid, th, idx_drawn, in, ticks, sink);
    }
    printf("# %s, %d CUs, one workgroup per CU, %d rows per wave, %d slots of 256 bins, one table per wave\n", prop.gcnArchName, grid, ITERS * ROWS, NSLOTS);
    printf("# s_memtime ticks per wave-row (mean over waves, best of 3 launches), and per instruction = per row / instructions per row\n");
    printf("%-46s %6s %12s %12s %12s %12s\n", "stream", "insts", "4 waves/CU", "per inst", "8 waves/CU", "per inst");
    for (int o = 0; o < 4; o++) printf("%-46s %6d %12.3f %12.3f %12.3f %12.3f\n", name[o], insts[o], t[o][0], t[o][0] / insts[o], t[o][1], t[o][1] / insts[o]);
    CK(hipFree(idx_drawn));
    CK(hipFree(idx_one));
    CK(hipFree(in));
    CK(hipFree(ticks));
    CK(hipFree(sink));
    return 0;
}
