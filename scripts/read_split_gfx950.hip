// What reading a 7-byte split scan group costs against today's 64-bit word a row: the go / no-go of the split56 form.
//
//   hipcc --offload-arch=gfx950 -O3 -o read_split_gfx950 read_split_gfx950.hip && ./read_split_gfx950 > profiles/read_split_gfx950.txt
//
// 60 M rows read by 256, 512 or 1024 workgroups of 256 threads in 4096-row tiles, register double buffered, non-temporal 16-byte loads,
// trivial consumption (xor), as scripts/read_packed_gfx950.hip; hipEvent time over 20 launches. A wave reads one block of 1024 rows a tile:
//   packed64 (8 B/row): block of 8192 bytes, 8 loads per lane at byte 1024 j + 16 lane (row = 128 j + 2 lane + k, today's pattern)
//   split56  (7 B/row): block of 7168 bytes, 7 loads per lane at byte 1024 j + 16 lane (four of low dwords, three of 24-bit high parts)
// so every wave-instruction reads 1024 consecutive bytes and a wave's loads of a tile cover its block end to end.
// The two patterns run in turn at every grid, five rounds in one sitting; the last lines compare them at the default grid (512).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#define CK(x)                                                                      \
    do {                                                                           \
        hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) {                                                    \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                \
            exit(1);                                                               \
        }                                                                          \
    } while (0)

typedef unsigned v4u32 __attribute__((ext_vector_type(4)));

struct Group {
    const unsigned char *w;   // NL * 1024 bytes a block of 1024 rows
    long long ntiles;         // every tile is whole: rows = ntiles * 4096
};

template <int NL> struct Tile {
    v4u32 w[NL];
};

template <int NL> __device__ __forceinline__ void load(Tile<NL> &t, const Group &C, long long tile) {
    const unsigned char *p = C.w + (tile * 4 + (threadIdx.x >> 6)) * (NL * 1024) + (threadIdx.x & 63) * 16;
    for (int j = 0; j < NL; j++) t.w[j] = __builtin_nontemporal_load((const v4u32 *)(p + j * 1024));
}

template <int NL> __device__ __forceinline__ unsigned eat(const Tile<NL> &t) {
    v4u32 x = t.w[0];
    for (int j = 1; j < NL; j++) x ^= t.w[j];
    return x.x ^ x.y ^ x.z ^ x.w;
}

template <int NL> __global__ __launch_bounds__(256, 2) void read_kernel(Group C, unsigned *out) {
    unsigned acc = 0;
    long long tile = blockIdx.x;
    if (tile < C.ntiles) {
        Tile<NL> a, b;
        load(a, C, tile);
        for (;;) {
            const long long n1 = tile + gridDim.x;
            if (n1 < C.ntiles) load(b, C, n1);
            acc ^= eat(a);
            if (n1 >= C.ntiles) break;
            const long long n2 = n1 + gridDim.x;
            if (n2 < C.ntiles) load(a, C, n2);
            acc ^= eat(b);
            if (n2 >= C.ntiles) break;
            tile = n2;
        }
    }
    out[blockIdx.x * 256 + threadIdx.x] = acc;
}

template <int NL> static double run(const Group &C, unsigned *out, int grid, const char *name, int round) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int i = 0; i < 3; i++) read_kernel<NL><<<grid, 256>>>(C, out);
    CK(hipEventRecord(e0));
    for (int i = 0; i < 20; i++) read_kernel<NL><<<grid, 256>>>(C, out);
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    CK(hipGetLastError());
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
    const double us = ms / 20 * 1e3, bytes = (double)C.ntiles * 4 * NL * 1024;
    printf("round %d %s grid %4d: %.1f us per launch, %.2f TB/s\n", round, name, grid, us, bytes / (us * 1e-6) / 1e12);
    return us;
}

int main() {
    const long long ntiles = 14648, rows = ntiles * 4096;   // about SF10 lineitem
    unsigned char *buf;
    CK(hipMalloc(&buf, (size_t)rows * 8));
    CK(hipMemset(buf, 5, (size_t)rows * 8));
    const Group C = {buf, ntiles};   // split56 reads the first 7/8 of the same allocation
    unsigned *out;
    CK(hipMalloc(&out, 1024 * 256 * sizeof(unsigned)));
    const int default_grid = 512;
    double a_min = 1e30, b_max = 0;
    for (int round = 0; round < 5; round++)
        for (int grid : {256, 512, 1024}) {
            const double a = run<8>(C, out, grid, "packed64", round);
            const double b = run<7>(C, out, grid, "split56 ", round);
            if (grid == default_grid) {
                a_min = std::min(a_min, a);
                b_max = std::max(b_max, b);
            }
        }
    unsigned h[2];
    CK(hipMemcpy(h, out, sizeof h, hipMemcpyDeviceToHost));
    printf("check %u %u\n", h[0], h[1]);
    printf("grid %d: fastest packed64 %.1f us, slowest split56 %.1f us: %s\n", default_grid, a_min, b_max, b_max < a_min ? "go" : "no-go");
    return 0;
}
