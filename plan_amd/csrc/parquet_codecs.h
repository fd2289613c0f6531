// The compression codecs whose pages the Parquet load decodes, one row each: what page_directory (parquet_meta.h) accepts and how it words a
// refusal, what the host twin (parquet_decode.h) decompresses a section with and which cause a corrupt stream gets, and the order of the
// device load's section lists and launches (parquet_load.hip, which keeps the launch functions: no HIP in here). The per-codec size and
// header pre-checks of page_directory are real differences and stay there.
#pragma once
#include <cstdint>
#include <string>

#include "gzip_decode.h"
#include "lz4_decode.h"
#include "planhip.h"
#include "snappy_decode.h"
#include "zstd_decode.h"

namespace ph {
namespace pq {

struct Codec {
    int32_t id;          // parquet.thrift's CompressionCodec
    uint32_t flag;       // the PH_PARQUET_* bit that enables it
    const char *name;
    int cause;           // the Cause (parquet_decode.h, which checks these against its enum) of a page whose stream is corrupt
    int (*decompress_host)(const uint8_t *src, int64_t src_bytes, uint8_t *dst, int64_t expected);   // -> the codec's Sub; 0 is every codec's S_OK
};

inline int snappy_section_host(const uint8_t *src, int64_t src_bytes, uint8_t *dst, int64_t expected) {
    return snappy::decompress_host(src, src_bytes, dst, expected, nullptr);
}

constexpr int N_CODECS = 4;
// in the order of the refusal text, the section lists and the launches
constexpr Codec CODECS[N_CODECS] = {
    {1, PH_PARQUET_SNAPPY, "SNAPPY", 8, snappy_section_host},
    {7, PH_PARQUET_LZ4_RAW, "LZ4_RAW", 12, lz4::decompress_host},
    {2, PH_PARQUET_GZIP, "GZIP", 13, gzip::decompress_host},
    {6, PH_PARQUET_ZSTD, "ZSTD", 14, zstd::decompress_host},
};

// the row of codec `id`, -1: none
inline int codec_row(int32_t id) {
    for (int i = 0; i < N_CODECS; i++)
        if (CODECS[i].id == id) return i;
    return -1;
}

// "only UNCOMPRESSED, SNAPPY and GZIP pages are decoded": the codecs that `flags` enables
inline std::string decoded_codecs_text(uint32_t flags) {
    std::string s = "only UNCOMPRESSED";
    int last = -1;
    for (int i = 0; i < N_CODECS; i++)
        if (flags & CODECS[i].flag) last = i;
    for (int i = 0; i <= last; i++)
        if (flags & CODECS[i].flag) s += std::string(i == last ? " and " : ", ") + CODECS[i].name;
    return s + " pages are decoded";
}

}  // namespace pq
}  // namespace ph
