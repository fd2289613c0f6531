// The device side of DELTA_BYTE_ARRAY (front coding; parquet_decode.h has the stream, its rules and the host twin). Two steps:
//   (a) lengths — parquet_load.hip's pq_dba_lengths, inside the page kernel: both DELTA_BINARY_PACKED streams, every rule judged, and per
//       value its prefix length, its suffix's length and where the suffix's bytes lie, plus one DbaPage a page for step (b);
//   (b) reconstruction — dba_expand.hip's kernel, ONE WAVE a page on section_wave.h's frame, once the offsets are known.
#pragma once
#include "section_wave.h"

namespace ph {

constexpr int DBA_THREADS = 64;     // one wave a page: value k needs value k - 1, the lanes carry out each copy and each literal
constexpr int DBA_TILE = 8192;      // bytes of the suffix section staged in LDS at a time
constexpr int DBA_RING = 16384;     // bytes of the most recent output kept in LDS: a prefix is copied from there when the value in front is no longer than this
constexpr int DBA_FLUSH = 4096;     // completed ring bytes that are flushed to global memory in one go
constexpr int DBA_CHUNK = 1024;     // bytes of a copy or a literal carried per step (16 a lane)

// what step (a) leaves for step (b), one a page (zeroed before the page kernels run: a page that is not front-coded, or that failed, has ok = 0)
struct DbaPage {
    int64_t suf_pos, suf_bytes;     // the suffixes' bytes, relative to the source base
    int64_t val0;                   // index of the page's first value in the per-value arrays
    int64_t dst_pos, dst_bytes;     // where the values go, relative to the destination base, and how many bytes they are; with an offsets
                                    // array the kernel takes both from it instead: off[row0], off[row0 + nrows] - off[row0]
    int64_t row0;
    int32_t nrows;
    int32_t nvalues;                // the chain's steps
    int32_t ok;
    int32_t pad;
};

struct DbaArgs {
    const uint8_t *src;
    uint8_t *dst;
    const int32_t *off;             // the column's offsets (null: DbaPage's dst_pos / dst_bytes)
    const DbaPage *pages;
    const int32_t *pre, *slen;      // per value: prefix length, suffix length
    int32_t *status;                // status[i] = 0, or 1 when the chain left its ranges (never, behind step (a); may be null)
};

// Reconstructs pages_dev[0, n) on the context's stream (asynchronously).
int dba_expand_pages(ph_ctx *ctx, const DbaArgs &A, int32_t n);

}  // namespace ph
