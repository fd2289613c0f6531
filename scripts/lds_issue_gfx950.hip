// Issue cost of the no-return LDS atomics the narrow lowcard_chain scan issues per passing row.
//
//   hipcc --offload-arch=gfx950 -O3 -o lds_issue_gfx950 lds_issue_gfx950.hip && ./lds_issue_gfx950 > profiles/lds_issue_gfx950.txt
//   hipcc --offload-arch=gfx950 -O3 -S --cuda-device-only lds_issue_gfx950.hip      (to see which instructions the streams became)
//
// The addressing is the kernel's: every thread owns one column of each accumulator array, address = slot stride + column + 8 tid (64-bit
// arrays) or 4 tid (32-bit arrays), slot strides multiples of 256 words, the slot changing from row to row and from lane to lane (eight
// slot offsets per lane, taken from the input so that the compiler cannot fold them). Every wave issues ITERS x ROWS "rows" of one
// instruction or of one per-row mix, waits for the LDS queue to drain and takes the s_memtime delta around it. One workgroup per CU:
// 256 threads are 4 waves per CU (one per SIMD), 512 threads 8. The table gives the mean delta per wave-instruction, and for the mixes
// also per row. s_memtime ticks are whatever the counter counts (the same unit as profiles/int_issue_gfx950.txt).
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

constexpr int ROWS = 8, ITERS = 2048, NSLOTS = 6, N64 = 5, N32 = 2;

enum Op { ADD_U64, ADD_U32, MIN_U32, MIX_5_1_1, MIX_4_0_1, MIX_4_0_0, NOPS };
static const char *const OP_NAME[NOPS] = {"ds_add_u64", "ds_add_u32", "ds_min_u32", "5 x add_u64 + add_u32 + min_u32", "4 x add_u64 + min_u32", "4 x add_u64"};
static const int OP_INSTS[NOPS] = {1, 1, 1, 7, 5, 4};   // per row

typedef __attribute__((address_space(3))) char lds_char;
typedef __attribute__((address_space(3))) unsigned long long lds_u64;
typedef __attribute__((address_space(3))) unsigned lds_u32;

#define ADD64(p, v) __hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define ADD32(p, v) __hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define MIN32(p, v) __hip_atomic_fetch_min((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)

// LDS: u64 [NSLOTS][N64][T] then u32 [NSLOTS][N32][T], T = blockDim.x
template <int OP> __global__ void stream_kernel(const unsigned *in, unsigned long long *ticks, unsigned long long *sink) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds[];
    const unsigned T = blockDim.x, tid = threadIdx.x;
    const unsigned n64 = NSLOTS * N64 * T, n32 = NSLOTS * N32 * T;
    unsigned *lds32 = reinterpret_cast<unsigned *>(lds + n64);
    for (unsigned i = tid; i < n64; i += T) lds[i] = 0;
    for (unsigned i = tid; i < n32; i += T) lds32[i] = 0xffffffffu;
    __syncthreads();
    lds_char *l64 = (lds_char *)(lds + tid), *l32 = (lds_char *)(lds32 + tid);
    // this lane's slot of each of the ROWS rows of an iteration, as byte offsets into the two arrays
    unsigned o64[ROWS], o32[ROWS];
    for (int r = 0; r < ROWS; r++) {
        const unsigned slot = (in[r] + tid * in[ROWS]) % NSLOTS;
        o64[r] = slot * (N64 * T * 8);
        o32[r] = slot * (N32 * T * 4);
    }
    unsigned long long v = in[ROWS + 1] + tid;
    unsigned w = in[ROWS + 2] + tid;
    asm volatile("" : "+v"(v), "+v"(w));
    const unsigned s64 = T * 8, s32 = T * 4;   // column strides
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    for (int it = 0; it < ITERS; it++) {
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            lds_char *a = l64 + o64[r], *c = l32 + o32[r];
            if (OP == ADD_U64) ADD64((lds_u64 *)a, v);
            if (OP == ADD_U32) ADD32((lds_u32 *)c, w);
            if (OP == MIN_U32) MIN32((lds_u32 *)(c + s32), w);
            if (OP == MIX_5_1_1 || OP == MIX_4_0_1 || OP == MIX_4_0_0) {
                ADD64((lds_u64 *)a, v);
                ADD64((lds_u64 *)(a + s64), v);
                ADD64((lds_u64 *)(a + 2 * s64), v);
                ADD64((lds_u64 *)(a + 3 * s64), v);
            }
            if (OP == MIX_5_1_1) {
                ADD64((lds_u64 *)(a + 4 * s64), v);
                ADD32((lds_u32 *)c, w);
            }
            if (OP == MIX_5_1_1 || OP == MIX_4_0_1) MIN32((lds_u32 *)(c + s32), w);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    __syncthreads();
    unsigned long long s = 0;
    for (unsigned i = tid; i < n64; i += T) s += lds[i];
    for (unsigned i = tid; i < n32; i += T) s += lds32[i];
    const unsigned gid = blockIdx.x * T + tid;
    sink[gid] = s;
    if ((tid & 63) == 0) ticks[gid >> 6] = t1 - t0;
}

template <int OP> static double run(int grid, int threads, const unsigned *in, unsigned long long *ticks, unsigned long long *sink) {
    const int waves = grid * threads / 64;
    const size_t lds = (size_t)NSLOTS * threads * (N64 * 8 + N32 * 4);
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(&stream_kernel<OP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    double best = 0;
    for (int rep = 0; rep < 3; rep++) {   // the first launch also loads the code object
        stream_kernel<OP><<<grid, threads, lds>>>(in, ticks, sink);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        std::vector<unsigned long long> h((size_t)waves);
        CK(hipMemcpy(h.data(), ticks, sizeof(unsigned long long) * (size_t)waves, hipMemcpyDeviceToHost));
        double sum = 0;
        for (unsigned long long v : h) sum += (double)v;
        const double mean = sum / waves / ((double)ITERS * ROWS);   // per row
        if (rep == 0 || mean < best) best = mean;
    }
    return best;
}

int main() {
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int grid = prop.multiProcessorCount;
    unsigned hin[ROWS + 3] = {0, 3, 1, 5, 2, 4, 3, 0, 1, 11, 13};   // eight slots, the lane step of the slot, the two operands
    unsigned *in;
    unsigned long long *ticks, *sink;
    CK(hipMalloc(&in, sizeof hin));
    CK(hipMemcpy(in, hin, sizeof hin, hipMemcpyHostToDevice));
    CK(hipMalloc(&ticks, sizeof(unsigned long long) * (size_t)grid * 8));
    CK(hipMalloc(&sink, sizeof(unsigned long long) * (size_t)grid * 512));
    double t[NOPS][2];
    for (int w = 0; w < 2; w++) {
        const int th = w == 0 ? 256 : 512;
        t[ADD_U64][w] = run<ADD_U64>(grid, th, in, ticks, sink);
        t[ADD_U32][w] = run<ADD_U32>(grid, th, in, ticks, sink);
        t[MIN_U32][w] = run<MIN_U32>(grid, th, in, ticks, sink);
        t[MIX_5_1_1][w] = run<MIX_5_1_1>(grid, th, in, ticks, sink);
        t[MIX_4_0_1][w] = run<MIX_4_0_1>(grid, th, in, ticks, sink);
        t[MIX_4_0_0][w] = run<MIX_4_0_0>(grid, th, in, ticks, sink);
    }
    printf("# %s, %d CUs, one workgroup per CU, %d rows per wave, %d slots, thread-private columns\n", prop.gcnArchName, grid, ITERS * ROWS, NSLOTS);
    printf("# s_memtime ticks per wave (mean over waves, best of 3 launches): per row, and per instruction = per row / instructions per row\n");
    printf("%-34s %6s %12s %12s %12s %12s\n", "stream", "insts", "4 waves/CU", "per inst", "8 waves/CU", "per inst");
    for (int o = 0; o < NOPS; o++)
        printf("%-34s %6d %12.3f %12.3f %12.3f %12.3f\n", OP_NAME[o], OP_INSTS[o], t[o][0], t[o][0] / OP_INSTS[o], t[o][1], t[o][1] / OP_INSTS[o]);
    CK(hipFree(in));
    CK(hipFree(ticks));
    CK(hipFree(sink));
    return 0;
}
