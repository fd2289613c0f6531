// The device side of snappy_decode.h: n independent Snappy streams, one workgroup each (snappy_decompress.hip, on section_wave.h's frame). The
// Parquet load launches it over the SNAPPY sections of a call; ph_snappy_decompress over caller-given streams.
#pragma once
#include "section_wave.h"

namespace ph {

constexpr int SN_THREADS = 64;      // one wave a section: the element chain is sequential, the lanes carry out each element
constexpr int SN_TILE = 8192;       // bytes of the compressed input staged in LDS at a time
constexpr int SN_RING = 65536;      // bytes of the most recent output kept in LDS: what a copy's 16-bit offset can reach
constexpr int SN_FLUSH = 4096;      // completed ring bytes that are flushed to global memory in one go
constexpr int SN_CHUNK = 1024;      // bytes of a long literal carried per step

// Decompresses sections_dev[0, n) on the context's stream (asynchronously). status_dev[i] = the snappy::Sub of section i. err / pages_dev
// (both may be null): the Parquet load's error word (lowest page << 8 | cause) and its page list.
int snappy_decompress_sections(ph_ctx *ctx, const uint8_t *src, uint8_t *dst, const SnSection *sections_dev, int32_t n, pq::PageDesc *pages_dev,
                               unsigned long long *err, int32_t *status_dev);

}  // namespace ph
