// The device side of lz4_decode.h: n independent LZ4 blocks, one workgroup each (lz4_decompress.hip). The Parquet load launches it over the
// LZ4_RAW sections of a call; ph_lz4_decompress over caller-given blocks. On section_wave.h's frame.
#pragma once
#include "section_wave.h"

namespace ph {

constexpr int LZ_THREADS = 64;      // one wave a section: the sequence chain is serial, the lanes carry out each literal run and match
constexpr int LZ_TILE = 8192;       // bytes of the compressed input staged in LDS at a time
constexpr int LZ_RING = 65536;      // bytes of the most recent output kept in LDS: a step reads its sources before it writes, so 2^16 serve offset 65535
constexpr int LZ_FLUSH = 4096;      // completed ring bytes that are flushed to global memory in one go
constexpr int LZ_CHUNK = 1024;      // bytes of a long literal run or a long match carried per step (16 a lane)

// Decompresses sections_dev[0, n) on the context's stream (asynchronously). status_dev[i] = the lz4::Sub of section i. err / pages_dev
// (both may be null): the Parquet load's error word (lowest page << 8 | cause) and its page list.
int lz4_decompress_sections(ph_ctx *ctx, const uint8_t *src, uint8_t *dst, const SnSection *sections_dev, int32_t n, pq::PageDesc *pages_dev,
                            unsigned long long *err, int32_t *status_dev);

}  // namespace ph
