// The device side of zstd_decode.h: n independent ZSTD streams, one workgroup each (zstd_decompress.hip). The Parquet load launches it over
// the ZSTD sections of a call; ph_zstd_decompress over caller-given streams. On section_wave.h's frame.
#pragma once
#include "section_wave.h"
#include "zstd_decode.h"

namespace ph {

constexpr int ZS_THREADS = 64;      // one wave a section: the symbol chains are serial, the lanes build the tables and carry out copies
constexpr int ZS_TILE = 4096;       // bytes of each of the TWO input windows: the literal streams' and the sequence stream's
constexpr int ZS_RING = 32768;      // bytes of the most recent output kept in LDS; an offset above it reads global memory
constexpr int ZS_FLUSH = 4096;      // completed ring bytes that are flushed to global memory, and folded into the XXH64, in one go
constexpr int ZS_CHUNK = 512;       // bytes of a match, a raw run or an RLE run carried per step (8 a lane)
static_assert(ZS_FLUSH + 2 * ZS_CHUNK + 64 < ZS_RING, "a step never overwrites ring bytes that wait for their flush or their hash");
// LDS: window + ring + second window + Huffman table + the three sequence tables + the weights' table + weights, counts, cells, ranks
constexpr int ZS_LDS = ZS_TILE + ZS_RING + ZS_TILE + 2 * zstd::HUF_CAP + 4 * ((1 << zstd::LL_LOG) + (1 << zstd::OF_LOG) + (1 << zstd::ML_LOG) + (1 << zstd::WT_LOG)) +
                       zstd::MAX_SYMS + 2 * zstd::MAX_SYMS + 2 * zstd::MAX_SYMS + 64;
static_assert(ZS_LDS == 51776 && 3 * ZS_LDS <= 160 * 1024, "three sections fit the 160 KiB of a CU");

// Decompresses sections_dev[0, n) on the context's stream (asynchronously). status_dev[i] = the zstd::Sub of section i. err / pages_dev
// (both may be null): the Parquet load's error word (lowest page << 8 | cause) and its page list.
int zstd_decompress_sections(ph_ctx *ctx, const uint8_t *src, uint8_t *dst, const SnSection *sections_dev, int32_t n, pq::PageDesc *pages_dev,
                             unsigned long long *err, int32_t *status_dev);

}  // namespace ph
