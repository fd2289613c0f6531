// What the row-to-lane layout of the narrow scan kernels costs in reading alone.
//
//   hipcc --offload-arch=gfx950 -O3 -o read_pattern_gfx950 read_pattern_gfx950.hip && ./read_pattern_gfx950 > profiles/read_pattern_gfx950.txt
//
// The Q1 narrow column set (2-, 4- and five 1-byte code columns, 11 B/row, 60 M rows) read by 512 or 1024 workgroups of 256 threads in
// 4096-row tiles, register double buffered, non-temporal loads, trivial consumption (xor); hipEvent time over 20 launches, three times.
//   mode 0: a lane owns 16 consecutive rows (the kernels' layout): w 16-byte loads per lane for a w-byte column, lane stride 16 w bytes
//   mode 1: a lane owns 4 x 4 consecutive rows (row = wave * 1024 + j * 256 + lane * 4 + k): 4 loads of 4 w bytes, each wave-instruction contiguous
#include <hip/hip_runtime.h>

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
typedef unsigned v2u32 __attribute__((ext_vector_type(2)));

struct Cols {
    const unsigned char *p, *e, *b[5];   // 2-byte, 4-byte, five 1-byte columns
    long long ntiles;                    // every tile is whole: rows = ntiles * 4096, all buffers hold that many rows
};

struct Tile {
    v4u32 p[2], e[4], b[5];
};

template <int MODE> __device__ __forceinline__ void load(Tile &t, const Cols &C, long long tile) {
    const long long row0 = tile * 4096;
    if (MODE == 0) {
        const long long r = row0 + threadIdx.x * 16;
        for (int j = 0; j < 2; j++) t.p[j] = __builtin_nontemporal_load((const v4u32 *)(C.p + r * 2 + 16 * j));
        for (int j = 0; j < 4; j++) t.e[j] = __builtin_nontemporal_load((const v4u32 *)(C.e + r * 4 + 16 * j));
        for (int c = 0; c < 5; c++) t.b[c] = __builtin_nontemporal_load((const v4u32 *)(C.b[c] + r));
    } else {
        const long long r = row0 + (threadIdx.x >> 6) * 1024 + (threadIdx.x & 63) * 4;
        for (int j = 0; j < 4; j++) {
            const long long rj = r + j * 256;
            const v2u32 pv = __builtin_nontemporal_load((const v2u32 *)(C.p + rj * 2));
            t.p[j >> 1][(j & 1) * 2] = pv.x;
            t.p[j >> 1][(j & 1) * 2 + 1] = pv.y;
            t.e[j] = __builtin_nontemporal_load((const v4u32 *)(C.e + rj * 4));
            for (int c = 0; c < 5; c++) t.b[c][j] = __builtin_nontemporal_load((const unsigned *)(C.b[c] + rj));
        }
    }
}

__device__ __forceinline__ unsigned eat(const Tile &t) {
    v4u32 x = t.p[0] ^ t.p[1] ^ t.e[0] ^ t.e[1] ^ t.e[2] ^ t.e[3];
    for (int c = 0; c < 5; c++) x ^= t.b[c];
    return x.x ^ x.y ^ x.z ^ x.w;
}

template <int MODE> __global__ __launch_bounds__(256, 2) void read_kernel(Cols C, unsigned *out) {
    unsigned acc = 0;
    long long tile = blockIdx.x;
    if (tile < C.ntiles) {
        Tile a, b;
        load<MODE>(a, C, tile);
        for (;;) {
            const long long n1 = tile + gridDim.x;
            if (n1 < C.ntiles) load<MODE>(b, C, n1);
            acc ^= eat(a);
            if (n1 >= C.ntiles) break;
            const long long n2 = n1 + gridDim.x;
            if (n2 < C.ntiles) load<MODE>(a, C, n2);
            acc ^= eat(b);
            if (n2 >= C.ntiles) break;
            tile = n2;
        }
    }
    out[blockIdx.x * 256 + threadIdx.x] = acc;
}

template <int MODE> static void run(const Cols &C, unsigned *out, int grid, double bytes) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int rep = 0; rep < 3; rep++) {
        for (int i = 0; i < 3; i++) read_kernel<MODE><<<grid, 256>>>(C, out);
        CK(hipEventRecord(e0));
        for (int i = 0; i < 20; i++) read_kernel<MODE><<<grid, 256>>>(C, out);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        CK(hipGetLastError());
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        printf("mode %d grid %d: %.1f us per launch, %.2f TB/s\n", MODE, grid, ms / 20 * 1e3, bytes / (ms / 20 * 1e-3) / 1e12);
    }
}

int main() {
    const long long ntiles = 14648, rows = ntiles * 4096;   // about SF10 lineitem
    Cols C;
    C.ntiles = ntiles;
    unsigned char *buf[7];
    const int w[7] = {2, 4, 1, 1, 1, 1, 1};
    for (int i = 0; i < 7; i++) {
        CK(hipMalloc(&buf[i], (size_t)rows * w[i]));
        CK(hipMemset(buf[i], i + 1, (size_t)rows * w[i]));
    }
    C.p = buf[0];
    C.e = buf[1];
    for (int c = 0; c < 5; c++) C.b[c] = buf[2 + c];
    unsigned *out;
    CK(hipMalloc(&out, 1024 * 256 * sizeof(unsigned)));
    const double bytes = (double)rows * 11;
    for (int grid : {512, 1024}) {
        run<0>(C, out, grid, bytes);
        run<1>(C, out, grid, bytes);
    }
    unsigned h[2];
    CK(hipMemcpy(h, out, sizeof h, hipMemcpyDeviceToHost));
    printf("check %u %u\n", h[0], h[1]);
    return 0;
}
