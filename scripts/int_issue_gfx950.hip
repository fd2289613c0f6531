// Issue cost of the integer multiplies the narrow scan kernels use, relative to v_add_u32.
//
//   hipcc --offload-arch=gfx950 -O3 -o int_issue_gfx950 int_issue_gfx950.hip && ./int_issue_gfx950 > profiles/int_issue_gfx950.txt
//   hipcc --offload-arch=gfx950 -O3 -S --cuda-device-only int_issue_gfx950.hip      (to see which instructions the streams became)
//
// Every wave runs a stream of CHAINS independent dependency chains of one operation, ITERS x REPS x CHAINS operations in all, and takes the
// s_memtime delta around it. One workgroup per CU: 256 threads put one wave on each SIMD, 512 threads two. The table gives the mean delta
// per operation and wave, and the same divided by v_add_u32's. s_memtime ticks are whatever the counter counts; the ratios are the result.
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

constexpr int CHAINS = 8, REPS = 4, ITERS = 2048;

enum Op { ADD_U32, MUL_U32_U24, MAD_U32_U24, MUL_I32_I24, MUL_LO_U32, MAD_U64_U32, MAD_I64_I32, NOPS };
static const char *const OP_NAME[NOPS] = {"v_add_u32", "v_mul_u32_u24", "v_mad_u32_u24", "v_mul_i32_i24", "v_mul_lo_u32", "v_mad_u64_u32", "v_mad_i64_i32"};

// keeps v in a VGPR and hides it from the optimiser: the chain stays a chain of the operation as written
#define OPAQUE32(v) asm volatile("" : "+v"(v))
#define OPAQUE64(v) asm volatile("" : "+v"(v))

template <int OP> __global__ void stream_kernel(const unsigned *in, unsigned long long *ticks, unsigned long long *sink) {
    const unsigned c = in[0], d = in[1];
    unsigned x[CHAINS];
    unsigned long long a[CHAINS];
    for (int k = 0; k < CHAINS; k++) {
        x[k] = in[2 + k] + threadIdx.x;
        a[k] = x[k];
    }
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < ITERS; it++) {
#pragma unroll
        for (int r = 0; r < REPS; r++) {
#pragma unroll
            for (int k = 0; k < CHAINS; k++) {
                if (OP == ADD_U32) { x[k] = x[k] + c; OPAQUE32(x[k]); }
                if (OP == MUL_U32_U24) { x[k] = __umul24(x[k], c); OPAQUE32(x[k]); }
                if (OP == MAD_U32_U24) { x[k] = __umul24(x[k], c) + d; OPAQUE32(x[k]); }
                if (OP == MUL_I32_I24) { x[k] = (unsigned)__mul24((int)x[k], (int)c); OPAQUE32(x[k]); }
                if (OP == MUL_LO_U32) { x[k] = x[k] * c; OPAQUE32(x[k]); }
                if (OP == MAD_U64_U32) { a[k] = (unsigned long long)(unsigned)a[k] * c + a[k]; OPAQUE64(a[k]); }
                if (OP == MAD_I64_I32) { a[k] = (unsigned long long)((long long)(int)(unsigned)a[k] * (int)c + (long long)a[k]); OPAQUE64(a[k]); }
            }
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    unsigned long long s = 0;
    for (int k = 0; k < CHAINS; k++) s += x[k] + a[k];
    const unsigned gid = blockIdx.x * blockDim.x + threadIdx.x;
    sink[gid] = s;
    if ((threadIdx.x & 63) == 0) ticks[gid >> 6] = t1 - t0;
}

template <int OP> static double run(int grid, int threads, const unsigned *in, unsigned long long *ticks, unsigned long long *sink) {
    const int waves = grid * threads / 64;
    double best = 0;
    for (int rep = 0; rep < 3; rep++) {   // the first launch also loads the code object
        stream_kernel<OP><<<grid, threads>>>(in, ticks, sink);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        std::vector<unsigned long long> h((size_t)waves);
        CK(hipMemcpy(h.data(), ticks, sizeof(unsigned long long) * (size_t)waves, hipMemcpyDeviceToHost));
        double sum = 0;
        for (unsigned long long v : h) sum += (double)v;
        const double mean = sum / waves / ((double)ITERS * REPS * CHAINS);
        if (rep == 0 || mean < best) best = mean;
    }
    return best;
}

int main() {
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int grid = prop.multiProcessorCount;
    unsigned hin[2 + CHAINS] = {3, 5};
    for (int k = 0; k < CHAINS; k++) hin[2 + k] = 7 + 2 * k;
    unsigned *in;
    unsigned long long *ticks, *sink;
    CK(hipMalloc(&in, sizeof hin));
    CK(hipMemcpy(in, hin, sizeof hin, hipMemcpyHostToDevice));
    CK(hipMalloc(&ticks, sizeof(unsigned long long) * (size_t)grid * 8));
    CK(hipMalloc(&sink, sizeof(unsigned long long) * (size_t)grid * 512));
    double t[NOPS][2];
    for (int w = 0; w < 2; w++) {
        const int th = w == 0 ? 256 : 512;
        t[ADD_U32][w] = run<ADD_U32>(grid, th, in, ticks, sink);
        t[MUL_U32_U24][w] = run<MUL_U32_U24>(grid, th, in, ticks, sink);
        t[MAD_U32_U24][w] = run<MAD_U32_U24>(grid, th, in, ticks, sink);
        t[MUL_I32_I24][w] = run<MUL_I32_I24>(grid, th, in, ticks, sink);
        t[MUL_LO_U32][w] = run<MUL_LO_U32>(grid, th, in, ticks, sink);
        t[MAD_U64_U32][w] = run<MAD_U64_U32>(grid, th, in, ticks, sink);
        t[MAD_I64_I32][w] = run<MAD_I64_I32>(grid, th, in, ticks, sink);
    }
    printf("# %s, %d CUs, one workgroup per CU, %d operations per wave in %d independent chains\n", prop.gcnArchName, grid, ITERS * REPS * CHAINS, CHAINS);
    printf("# s_memtime ticks per operation and wave (mean over waves, best of 3 launches); x = relative to v_add_u32\n");
    printf("%-16s %14s %8s %14s %8s\n", "instruction", "1 wave/SIMD", "x", "2 waves/SIMD", "x");
    for (int o = 0; o < NOPS; o++)
        printf("%-16s %14.4f %8.2f %14.4f %8.2f\n", OP_NAME[o], t[o][0], t[o][0] / t[ADD_U32][0], t[o][1], t[o][1] / t[ADD_U32][1]);
    CK(hipFree(in));
    CK(hipFree(ticks));
    CK(hipFree(sink));
    return 0;
}
