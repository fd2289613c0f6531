// The device side of gzip_decode.h: n independent GZIP streams, one workgroup each (gzip_decompress.hip). The Parquet load launches it over
// the GZIP sections of a call; ph_gzip_decompress over caller-given streams. On section_wave.h's frame.
#pragma once
#include "gzip_decode.h"
#include "section_wave.h"

namespace ph {

constexpr int GZ_THREADS = 64;      // one wave a section: the symbol chain is serial, the lanes build the tables and carry out matches and stored blocks
constexpr int GZ_TILE = 4096;       // bytes of the compressed input staged in LDS at a time
constexpr int GZ_RING = 32768;      // bytes of the most recent output kept in LDS: a step reads its sources before it writes, so 2^15 serve distance 32768
constexpr int GZ_FLUSH = 4096;      // completed ring bytes that are flushed to global memory, and folded into the CRC-32, in one go
constexpr int GZ_CHUNK = 1024;      // bytes of a stored block carried per step (16 a lane)
constexpr int GZ_MATCH = 320;       // a match is one step: 258 bytes at most, 5 a lane
// LDS: window + ring + literal/length table + distance table + CRC table + counts, first codes, codes, lengths
constexpr int GZ_LDS = GZ_TILE + GZ_RING + 4 * gzip::LIT_CAP + 4 * gzip::DIST_CAP + 1024 + 64 + 64 + 2 * gzip::MAX_LENS + gzip::MAX_LENS;
static_assert(GZ_LDS == 52288 && 3 * GZ_LDS <= 160 * 1024, "three sections fit the 160 KiB of a CU");

// Decompresses sections_dev[0, n) on the context's stream (asynchronously). status_dev[i] = the gzip::Sub of section i. err / pages_dev
// (both may be null): the Parquet load's error word (lowest page << 8 | cause) and its page list.
int gzip_decompress_sections(ph_ctx *ctx, const uint8_t *src, uint8_t *dst, const SnSection *sections_dev, int32_t n, pq::PageDesc *pages_dev,
                             unsigned long long *err, int32_t *status_dev);

}  // namespace ph
