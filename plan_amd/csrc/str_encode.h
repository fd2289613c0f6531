// What the device load paths (csv_load.hip, parquet_load.hip) share for VARCHAR columns: the byte copy behind scanned offsets, and the
// interning step that turns a column of <= 256 distinct strings into PH_CODE8 + a dictionary in byte order (encode_strings, defined in
// csv_load.hip). The kernels are static: each translation unit that launches one holds its own copy.
#pragma once
#include <algorithm>
#include <vector>

#include "common.h"

namespace ph {

// device temporaries of one call: released (hipFree waits for the device) when the call leaves, however it leaves
struct Temps {
    std::vector<void *> p;
    const char *who = "ph_table_create_csv";
    ~Temps() { release(); }
    void release() { for (void *q : p) (void)hipFree(q); p.clear(); }
    int alloc(void **out, int64_t bytes) {
        *out = nullptr;
        if (hipMalloc(out, (size_t)(bytes > 0 ? bytes : 1)) != hipSuccess) { (void)hipGetLastError(); ph::set_error("%s: no device memory for %lld bytes", who, (long long)bytes); return PH_EHIP; }
        p.push_back(*out);
        return PH_OK;
    }
};

struct TableGuard {
    ph_table *t = nullptr;
    ~TableGuard() { if (t) ph_table_free(t); }
};

inline int load_grid_for(ph_ctx *ctx, int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)ctx->cu_count * 8)); }

// 64-bit sum of non-negative int32 (a VARCHAR column's lengths; the tiles' row counts)
static __global__ __launch_bounds__(256) void sum_lengths_kernel(const int32_t *__restrict__ len, int64_t n, unsigned long long *__restrict__ total) {
    unsigned long long s = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) s += (unsigned)len[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    __shared__ unsigned long long s_part[4];
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0 && (s = s_part[0] + s_part[1] + s_part[2] + s_part[3]) != 0) atomicAdd(total, s);   // one add per workgroup
}

// VARCHAR bytes: a workgroup takes 256 rows, whose output bytes are one contiguous range; every lane writes one output byte at a time
// (coalesced stores) and finds its row by a binary search over the rows' offsets in LDS (reads are contiguous within a field)
// (MASK_SIGN, the text path under PH_CSV_QUOTES: a begin's sign bit marks a row with escapes; such a row gets raw bytes here and is written
// again by csv_copy_escaped_kernel; SKIP_NEGATIVE, the Parquet path over a column with front-coded pages: a negative begin marks a row whose
// bytes dba_expand.hip's kernel writes, and this one leaves them alone)
template <bool MASK_SIGN, bool SKIP_NEGATIVE = false>
static __global__ __launch_bounds__(256) void copy_strings_kernel(const unsigned char *__restrict__ text, const int64_t *__restrict__ sbegin,
                                                                  const int32_t *__restrict__ off, int64_t n, unsigned char *__restrict__ out) {
    __shared__ int32_t s_off[257];
    __shared__ int64_t s_beg[256];
    const int64_t r0 = (int64_t)blockIdx.x * 256;
    const int nr = (int)(n - r0 < 256 ? n - r0 : 256);
    for (int i = threadIdx.x; i <= nr; i += 256) s_off[i] = off[r0 + i];
    if ((int)threadIdx.x < nr) s_beg[threadIdx.x] = MASK_SIGN ? sbegin[r0 + threadIdx.x] & INT64_MAX : sbegin[r0 + threadIdx.x];
    __syncthreads();
    const int64_t lo = s_off[0], hi = s_off[nr];
    for (int64_t j = lo + threadIdx.x; j < hi; j += 256) {   // (64-bit: hi may sit within 256 of 2^31)
        int a = 0, b = nr;                                  // s_off[a] <= j < s_off[b]
        while (b - a > 1) {
            const int m = (a + b) >> 1;
            if (s_off[m] <= j) a = m; else b = m;
        }
        if (SKIP_NEGATIVE && s_beg[a] < 0) continue;
        out[j] = text[s_beg[a] + (j - (int64_t)s_off[a])];
    }
}

// A VARCHAR column whose offsets (d.data) and bytes (d.aux) are in place: <= 256 distinct strings -> PH_CODE8 + dictionary in byte order.
// count_dev: 8 zeroable bytes on the device for the step's counters. validity (device bitmap, or nullptr = no NULLs): a NULL row arrives as
// an empty string; it is no distinct value (unless a valid row is the empty string too) and its code is 0.
int encode_strings(ph_ctx *ctx, ph_table::column &d, int64_t nrows, int64_t padded, unsigned *count_dev, Temps &tmp, const uint8_t *validity);

}  // namespace ph
