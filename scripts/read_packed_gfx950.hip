// What reading one bit-packed 64-bit word a row costs, against the 11 B/row of read_pattern_gfx950.hip.
//
//   hipcc --offload-arch=gfx950 -O3 -o read_packed_gfx950 read_packed_gfx950.hip && ./read_packed_gfx950 > profiles/read_packed_gfx950.txt
//
// One uint64 per row (8 B/row, 60 M rows) read by 512 or 1024 workgroups of 256 threads in 4096-row tiles, register double buffered,
// non-temporal 16-byte loads, trivial consumption (xor); hipEvent time over 20 launches, three times.
//   row = tile * 4096 + wave * 1024 + j * 128 + lane * 2 + k, j = 0..7, k = 0..1: 8 loads of 16 bytes per lane, and every
//   wave-instruction reads 1024 consecutive bytes
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

struct Words {
    const unsigned char *w;   // 8 bytes a row
    long long ntiles;         // every tile is whole: rows = ntiles * 4096
};

struct Tile {
    v4u32 w[8];
};

__device__ __forceinline__ void load(Tile &t, const Words &C, long long tile) {
    const long long r = tile * 4096 + (threadIdx.x >> 6) * 1024 + (threadIdx.x & 63) * 2;
    for (int j = 0; j < 8; j++) t.w[j] = __builtin_nontemporal_load((const v4u32 *)(C.w + (r + j * 128) * 8));
}

__device__ __forceinline__ unsigned eat(const Tile &t) {
    v4u32 x = t.w[0];
    for (int j = 1; j < 8; j++) x ^= t.w[j];
    return x.x ^ x.y ^ x.z ^ x.w;
}

__global__ __launch_bounds__(256, 2) void read_kernel(Words C, unsigned *out) {
    unsigned acc = 0;
    long long tile = blockIdx.x;
    if (tile < C.ntiles) {
        Tile a, b;
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

static void run(const Words &C, unsigned *out, int grid, double bytes) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int rep = 0; rep < 3; rep++) {
        for (int i = 0; i < 3; i++) read_kernel<<<grid, 256>>>(C, out);
        CK(hipEventRecord(e0));
        for (int i = 0; i < 20; i++) read_kernel<<<grid, 256>>>(C, out);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        CK(hipGetLastError());
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        printf("packed64 grid %d: %.1f us per launch, %.2f TB/s\n", grid, ms / 20 * 1e3, bytes / (ms / 20 * 1e-3) / 1e12);
    }
}

int main() {
    const long long ntiles = 14648, rows = ntiles * 4096;   // about SF10 lineitem
    Words C;
    C.ntiles = ntiles;
    unsigned char *buf;
    CK(hipMalloc(&buf, (size_t)rows * 8));
    CK(hipMemset(buf, 5, (size_t)rows * 8));
    C.w = buf;
    unsigned *out;
    CK(hipMalloc(&out, 1024 * 256 * sizeof(unsigned)));
    const double bytes = (double)rows * 8;
    for (int grid : {512, 1024}) run(C, out, grid, bytes);
    unsigned h[2];
    CK(hipMemcpy(h, out, sizeof h, hipMemcpyDeviceToHost));
    printf("check %u %u\n", h[0], h[1]);
    return 0;
}
