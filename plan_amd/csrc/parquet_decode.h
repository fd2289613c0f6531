// The decoding rules of the Parquet load path (ph_table_create_parquet, planhip.h): ONE set of decoders over a byte getter, compiled
// for the host (ph_parquet_read_column_host, the slow twin) and for the device (parquet_load.hip's kernels), so what a CPU test or
// a sanitizer pins is what the kernels do. The getter g has u8(p), u32(p), u64(p) (little-endian, any alignment): the kernels read
// global memory or an LDS tile through it, the host the file's bytes.
//
// Below the decoders: the host-side plan of one column (type mapping and overrides, the page directory resolved into level / value /
// dictionary byte ranges, every one checked against its page) and the sequential host decode that follows the plan.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "parquet_meta.h"

#if defined(__HIPCC__)
#define PH_HD __host__ __device__ __forceinline__
#else
#define PH_HD inline
#endif

namespace ph {
namespace pq {

// what only decoding can see; the host turns a cause into the return code and the message
enum Cause : int {
    C_OK = 0,
    C_RUN = 1,         // a run of the RLE / bit-packed hybrid is empty or runs past its section       PH_EINVAL
    C_LEN = 2,         // a BYTE_ARRAY length runs past its page                                       PH_EINVAL
    C_INDEX = 3,       // a dictionary index at or above the dictionary's size                         PH_EINVAL
    C_COUNT = 4,       // the page holds fewer or more values than its header's num_values             PH_EINVAL
    C_BIT_WIDTH = 5,   // a dictionary index width above 32                                            PH_EINVAL
    C_I32_RANGE = 6,   // PH_I32 over INT64: a value outside int32                                     PH_EOVERFLOW
    C_DEC_RANGE = 7,   // a FIXED_LEN_BYTE_ARRAY decimal outside int64                                 PH_EOVERFLOW
    C_SNAPPY = 8,      // a page's SNAPPY stream is corrupt (snappy_decode.h's sub-cases)              PH_EINVAL
    C_LVL_SECTION = 9, // a v1 page's level-section length, read from decompressed bytes, leaves it    PH_EINVAL
    C_DELTA = 10,      // a malformed DELTA_BINARY_PACKED header or miniblock (DeltaSub below)         PH_EINVAL
    C_DELTA_LIMIT = 11,// a DELTA_BINARY_PACKED block above DELTA_MAX_BLOCK / DELTA_MAX_MINIBLOCKS     PH_EUNSUPPORTED
    C_LZ4 = 12,        // a page's LZ4_RAW stream is corrupt (lz4_decode.h's sub-cases)                PH_EINVAL
    C_GZIP = 13,       // a page's GZIP stream is corrupt (gzip_decode.h's sub-cases)                  PH_EINVAL
    C_ZSTD = 14,       // a page's ZSTD stream is corrupt (zstd_decode.h's sub-cases)                  PH_EINVAL
    C_PREFIX = 15,     // a DELTA_BYTE_ARRAY prefix negative or above the length of the value before   PH_EINVAL
};

static_assert(CODECS[0].cause == C_SNAPPY && CODECS[1].cause == C_LZ4 && CODECS[2].cause == C_GZIP && CODECS[3].cause == C_ZSTD, "parquet_codecs.h names the causes by number");

inline int cause_code(int cause) {
    return cause == C_OK ? PH_OK : (cause == C_I32_RANGE || cause == C_DEC_RANGE) ? PH_EOVERFLOW : cause == C_DELTA_LIMIT ? PH_EUNSUPPORTED : PH_EINVAL;
}

inline const char *cause_text(int cause) {
    switch (cause) {
    case C_RUN: return "a run of the RLE / bit-packed hybrid is empty or runs past its section";
    case C_LEN: return "a BYTE_ARRAY length runs past its page";
    case C_INDEX: return "a dictionary index at or above the dictionary's size";
    case C_COUNT: return "the page holds fewer or more values than its header says";
    case C_BIT_WIDTH: return "a dictionary index width above 32 bits";
    case C_I32_RANGE: return "a value outside the int32 range of an INTEGER column";
    case C_DEC_RANGE: return "a decimal outside the int64 range";
    case C_SNAPPY: return "a corrupt SNAPPY stream";
    case C_LVL_SECTION: return "a level section longer than its page";
    case C_DELTA: return "a malformed DELTA_BINARY_PACKED header or miniblock";
    case C_DELTA_LIMIT: return "a DELTA_BINARY_PACKED block of more than 65536 values or 512 miniblocks";
    case C_LZ4: return "a corrupt LZ4_RAW stream";
    case C_GZIP: return "a corrupt GZIP stream";
    case C_ZSTD: return "a corrupt ZSTD stream";
    case C_PREFIX: return "a DELTA_BYTE_ARRAY prefix longer than the value in front of it";
    default: return "unknown cause";
    }
}

// ---- ULEB128 of at most 32 bits inside [pos, end)
template <class G>
PH_HD bool read_uvarint(const G &g, int64_t &pos, int64_t end, uint32_t *v) {
    uint32_t r = 0;
    for (int shift = 0; shift < 35; shift += 7) {
        if (pos >= end) return false;
        const uint32_t b = g.u8(pos++);
        r |= (b & 0x7fu) << shift;
        if (!(b & 0x80u)) { *v = r; return true; }
    }
    return false;
}

// ---- the RLE / bit-packed hybrid: one run. count > 0; a bit-packed run's count is its groups x 8 (the last group of a section may be padding)
struct Run {
    int32_t packed;    // 1: `count` values of `bw` bits each from byte `data` on, LSB first; 0: `count` times `value`
    int64_t count;
    uint32_t value;
    int64_t data;
};

template <class G>
PH_HD int next_run(const G &g, int64_t &pos, int64_t end, int bw, Run *r) {
    uint32_t h;
    if (!read_uvarint(g, pos, end, &h) || (h >> 1) == 0) return C_RUN;
    if (h & 1u) {
        const int64_t groups = h >> 1, bytes = groups * bw;
        if (bytes > end - pos) return C_RUN;
        r->packed = 1; r->count = groups * 8; r->value = 0; r->data = pos;
        pos += bytes;
        return C_OK;
    }
    const int vb = (bw + 7) >> 3;
    if (vb > end - pos) return C_RUN;
    uint32_t v = 0;
    for (int k = 0; k < vb; k++) v |= (uint32_t)g.u8(pos + k) << (8 * k);
    r->packed = 0; r->count = h >> 1; r->value = v; r->data = pos;
    pos += vb;
    return C_OK;
}

// value j of a bit-packed run (random access: j < run.count keeps every byte read inside the run)
template <class G>
PH_HD uint32_t packed_get(const G &g, int64_t data, int bw, int64_t j) {
    if (bw == 0) return 0;
    const int64_t bit = j * bw;
    const int64_t p = data + (bit >> 3);
    const int sh = (int)(bit & 7), nb = (sh + bw + 7) >> 3;
    uint64_t w = 0;
    for (int k = 0; k < nb; k++) w |= (uint64_t)g.u8(p + k) << (8 * k);
    return (uint32_t)((w >> sh) & (bw == 32 ? 0xffffffffull : ((1ull << bw) - 1)));
}

// ---- DELTA_BINARY_PACKED (PH_PARQUET_DELTA). The stream:
//   header   block_size, miniblocks_per_block, total_count (ULEB128), first_value (zigzag ULEB128 of up to 64 bits: 10 bytes)
//   a block  min_delta (zigzag ULEB128, 64 bits), one width byte per miniblock, then the miniblocks: block_size / miniblocks values of
//            `width` bits each, LSB first
// value[0] = first_value, value[i] = value[i - 1] + min_delta + delta, modulo 2^64 (an INT32 column keeps the low 32 bits, sign-extended).
// In the last block a miniblock that holds none of the total_count - 1 deltas has NO bytes in the stream and its width byte means nothing;
// the last miniblock that holds one is stored whole. A block's header must fit the decoders' staging, hence the two limits; a stream
// above them is valid Parquet this build does not decode (C_DELTA_LIMIT). No trip count comes from the stream alone: total_count is
// checked against the page's count of values (or the caller's room) before anything loops over it, and a block is walked only while
// values are still wanted, so the blocks number ceil((total_count - 1) / block_size).
constexpr int DELTA_MAX_BLOCK = 65536;      // values of a block
constexpr int DELTA_MAX_MINIBLOCKS = 512;   // miniblocks of a block: the entries of the kernels' miniblock table

// what exactly is wrong with a stream: the message of the raw decoders (ph_delta_decode_host); a page's message has the cause only
enum DeltaSub : int {
    DS_OK = 0,
    DS_VARINT = 1,       // a varint of more than 10 bytes or 64 bits, or one that leaves the stream
    DS_BLOCK_SIZE = 2,   // block_size 0 or no multiple of 128
    DS_MINIBLOCKS = 3,   // 0 miniblocks
    DS_MINI_VALUES = 4,  // block_size / miniblocks no whole multiple of 32
    DS_LIMIT = 5,        // above DELTA_MAX_BLOCK / DELTA_MAX_MINIBLOCKS
    DS_COUNT = 6,        // total_count differs from the count expected
    DS_WIDTHS = 7,       // a block's width bytes leave the stream
    DS_WIDTH = 8,        // a needed miniblock's width above the type's bits
    DS_MINIBLOCK = 9,    // a needed miniblock leaves the stream
    DS_TRAILING = 10,    // bytes behind the last needed miniblock of a stream that must end there
    DS_CAPACITY = 11,    // (the raw decoders) total_count above the caller's room
    DS_EMIT = 12,        // the consumer of the values refused one (the cause is the consumer's)
};

PH_HD int delta_cause(int sub) {
    return sub == DS_OK ? C_OK : sub == DS_LIMIT ? C_DELTA_LIMIT : (sub == DS_COUNT || sub == DS_TRAILING) ? C_COUNT : C_DELTA;
}

inline const char *delta_sub_text(int sub) {
    switch (sub) {
    case DS_VARINT: return "a varint of more than 10 bytes or 64 bits, or one that runs off the end";
    case DS_BLOCK_SIZE: return "a block size of 0 or no multiple of 128";
    case DS_MINIBLOCKS: return "0 miniblocks in a block";
    case DS_MINI_VALUES: return "a miniblock whose value count is no multiple of 32";
    case DS_LIMIT: return "a block of more than 65536 values or 512 miniblocks";
    case DS_COUNT: return "a header count that differs from the count expected";
    case DS_WIDTHS: return "a block's width bytes run off the end";
    case DS_WIDTH: return "a miniblock width above the type's bits";
    case DS_MINIBLOCK: return "a miniblock runs off the end";
    case DS_TRAILING: return "bytes left over behind the last miniblock";
    case DS_CAPACITY: return "more values than the destination holds";
    default: return "unknown";
    }
}

// ULEB128 of at most 64 bits (10 bytes, the tenth at most 1) inside [pos, end)
template <class G>
PH_HD bool read_uvarint64(const G &g, int64_t &pos, int64_t end, uint64_t *v) {
    uint64_t r = 0;
    for (int shift = 0; shift < 70; shift += 7) {
        if (pos >= end) return false;
        const uint64_t b = g.u8(pos++);
        if (shift == 63 && (b & 0x7eu)) return false;
        r |= (b & 0x7fu) << shift;
        if (!(b & 0x80u)) { *v = r; return true; }
    }
    return false;
}

PH_HD uint64_t unzigzag64(uint64_t u) { return (u >> 1) ^ (~(u & 1u) + 1u); }

struct DeltaHeader {
    int32_t block, mini, per_mini;   // values of a block, miniblocks of a block, values of a miniblock (a multiple of 32)
    int64_t total;                   // values of the stream (the first one included), at most 2^31
    uint64_t first;
};

template <class G>
PH_HD int delta_header(const G &g, int64_t &pos, int64_t end, DeltaHeader *h) {
    uint64_t b, m, t, f;
    if (!read_uvarint64(g, pos, end, &b) || !read_uvarint64(g, pos, end, &m) || !read_uvarint64(g, pos, end, &t) || !read_uvarint64(g, pos, end, &f)) return DS_VARINT;
    if (b == 0 || (b & 127u)) return DS_BLOCK_SIZE;
    if (m == 0) return DS_MINIBLOCKS;
    if (b > (uint64_t)DELTA_MAX_BLOCK || m > (uint64_t)DELTA_MAX_MINIBLOCKS) return DS_LIMIT;
    if (b % m || ((b / m) & 31u)) return DS_MINI_VALUES;
    if (t > (1ull << 31)) return DS_COUNT;          // (no page and no caller holds that many)
    h->block = (int32_t)b;
    h->mini = (int32_t)m;
    h->per_mini = (int32_t)(b / m);
    h->total = (int64_t)t;
    h->first = unzigzag64(f);
    return DS_OK;
}

// One block's header at pos, of which `need` (> 0) deltas are still wanted: min_delta, the width bytes, and for every miniblock that holds
// a wanted delta put(m, its first byte, its width, min_delta) once it is known to lie inside [pos, end). pos -> behind the last of them.
template <class G, class Put>
PH_HD int delta_block(const G &g, int64_t &pos, int64_t end, const DeltaHeader &h, int64_t need, int max_width, const Put &put) {
    uint64_t z;
    if (!read_uvarint64(g, pos, end, &z)) return DS_VARINT;
    const uint64_t min_delta = unzigzag64(z);
    if (h.mini > end - pos) return DS_WIDTHS;
    const int64_t widths = pos;
    pos += h.mini;
    for (int m = 0; m < h.mini && (int64_t)m * h.per_mini < need; m++) {
        const int w = g.u8(widths + m);
        if (w > max_width) return DS_WIDTH;
        const int64_t bytes = (int64_t)(h.per_mini >> 3) * w;
        if (bytes > end - pos) return DS_MINIBLOCK;
        put(m, pos, w, min_delta);
        pos += bytes;
    }
    return DS_OK;
}

// value j of `bw` (0..64) bits in a miniblock that begins at byte `data`: up to 9 bytes at any bit offset (j inside the miniblock keeps
// every byte read inside it)
template <class G>
PH_HD uint64_t packed_get64(const G &g, int64_t data, int bw, int64_t j) {
    if (bw == 0) return 0;
    const int64_t bit = j * bw;
    const int64_t p = data + (bit >> 3);
    const int sh = (int)(bit & 7), nb = (sh + bw + 7) >> 3;
    uint64_t w = 0;
    for (int k = 0; k < nb && k < 8; k++) w |= (uint64_t)g.u8(p + k) << (8 * k);
    w >>= sh;
    if (nb > 8) w |= (uint64_t)g.u8(p + 8) << (64 - sh);   // (sh > 0 here)
    return bw == 64 ? w : w & ((1ull << bw) - 1);
}

// the running value as the column's type sees it: INT32 keeps the low 32 bits
PH_HD int64_t delta_value(uint64_t v, int bits) { return bits == 32 ? (int64_t)(int32_t)(uint32_t)v : (int64_t)v; }

// ---- PLAIN: INT32 / INT64 are little-endian; FIXED_LEN_BYTE_ARRAY(len 1..16) decimals are big-endian two's complement
template <class G>
PH_HD bool flba_to_i64(const G &g, int64_t pos, int len, int64_t *out) {
    uint64_t v = (g.u8(pos) & 0x80u) ? ~0ull : 0ull;   // sign extension
    const uint64_t ext = v & 0xffu;
    bool fits = true;
    int k = 0;
    for (; k < len - 8; k++) fits &= g.u8(pos + k) == ext;
    const bool neg = ext != 0;
    for (; k < len; k++) v = (v << 8) | g.u8(pos + k);
    if (len > 8) fits &= ((v >> 63) != 0) == neg;
    *out = (int64_t)v;
    return fits;
}

enum PhysKind : int { K_INT32 = 0, K_INT64 = 1, K_FLBA = 2, K_BYTES = 3 };

// one fixed-width value at `pos` as int64; C_DEC_RANGE when a FLBA decimal does not fit
template <int KIND, class G>
PH_HD int plain_value(const G &g, int64_t pos, int flba_len, int64_t *v) {
    if (KIND == K_INT32) { *v = (int32_t)g.u32(pos); return C_OK; }
    if (KIND == K_INT64) { *v = (int64_t)g.u64(pos); return C_OK; }
    return flba_to_i64(g, pos, flba_len, v) ? C_OK : C_DEC_RANGE;
}

// ---- one data page as the decoders see it: byte ranges relative to the getter's origin, every one inside the page (checked by
// resolve_column on the host before anything decodes)
struct PageDesc {
    int64_t first_row;
    int64_t lvl_pos, val_pos, dict_pos;   // definition levels' hybrid runs; the values section; the chunk's dictionary page data
    int32_t lvl_bytes;                    // -1: a required column, no levels
    int32_t val_bytes, dict_bytes;
    int32_t num_values;                   // rows of the page (flat columns)
    int32_t dict_n;                       // entries of the dictionary page; -1: PLAIN values
    int32_t dict_base;                    // BYTE_ARRAY: where this chunk's dictionary entries begin in the column's entry arrays
    int32_t row_group, page;              // for messages: the row group, the page's index in the column's page directory
    int32_t enc;                          // 0: PLAIN or dictionary indices (dict_n); E_DELTA_BINARY_PACKED / E_DELTA_LENGTH_BYTE_ARRAY: a delta page;
                                          // E_DELTA_BYTE_ARRAY: a front-coded page
};

// Positions at or above Z_BASE lie in the column's region of decompressed sections, at (position - Z_BASE); all others in the file.
// resolve_column hands them out; the device route rebases both kinds onto its one allocation, the host twin reads through HostBytes.
constexpr int64_t Z_BASE = 1ll << 48;

struct HostBytes {
    const uint8_t *s;   // the file
    const uint8_t *z;   // the decompressed sections (null: the column has none)
    explicit HostBytes(const uint8_t *file, const uint8_t *sections = nullptr) : s(file), z(sections) {}
    const uint8_t *at(int64_t p) const { return p >= Z_BASE ? z + (p - Z_BASE) : s + p; }
    uint8_t u8(int64_t p) const { return *at(p); }
    uint32_t u32(int64_t p) const { uint32_t v; memcpy(&v, at(p), 4); return v; }
    uint64_t u64(int64_t p) const { uint64_t v; memcpy(&v, at(p), 8); return v; }
};

// one compressed section of a column: a page's stream in the file and where its bytes go
struct Section {
    int64_t src_pos, src_bytes;   // the stream as stored (SNAPPY: its length preamble included), checked against the page by page_directory
    int64_t out_pos, out_bytes;   // in the column's region (16-byte aligned); what the stream must produce
    int32_t row_group, page;      // for messages
    int32_t owner;                // whose bytes: 0 pages[index], 1 dicts[index] (a BYTE_ARRAY dictionary), 2 a fixed-width dictionary page
    int32_t index;
    int32_t v1_levels;            // 1: a v1 page of a nullable column; complete_v1_levels finishes its PageDesc from the decompressed bytes
    int32_t codec;                // the stream's CompressionCodec: 1 SNAPPY, 2 GZIP, 6 ZSTD, 7 LZ4_RAW
};

// A v1 page of a nullable column begins with the 4-byte length n of its level section. For a compressed page that length lies inside the
// stream: `at` = where the page's `bytes` decompressed bytes begin (>= 4: the host checked the header), n = their first four.
PH_HD int complete_v1_levels(PageDesc &d, int64_t at, int64_t bytes, uint32_t n) {
    if ((int64_t)n > bytes - 4) return C_LVL_SECTION;
    d.lvl_pos = at + 4;
    d.lvl_bytes = (int32_t)n;
    d.val_pos = at + 4 + (int64_t)n;
    d.val_bytes = (int32_t)(bytes - 4 - (int64_t)n);
    return C_OK;
}

// ---------------------------------------------------------------- the host-side plan of one column

struct ColPlan {
    int32_t column = 0;
    std::string what;            // "column 3 (l_comment)"
    int32_t kind = 0;            // PhysKind
    int32_t flba_len = 0;
    int32_t width = 0;           // bytes of a PLAIN value (0: BYTE_ARRAY)
    int32_t out_type = 0, out_scale = 0;
    bool nullable = false;
    std::vector<Page> dir;       // the page directory
    std::vector<PageDesc> pages; // the data pages, resolved
    std::vector<PageDesc> dicts; // BYTE_ARRAY: the dictionary pages as value sections (val_pos / val_bytes / num_values = entries; dict_base)
    int64_t dict_entries = 0;    // BYTE_ARRAY: the sum of the dictionary pages' entries
    std::vector<Section> sections;   // the compressed pages' streams, in page order
    int64_t z_bytes = 0;         // the region their output takes
};

inline int level_section_error(Status *st, const char *what, int row_group, long long page, uint32_t n, long long bytes) {
    return st->fail(PH_EINVAL, "%s: row group %d, page %lld: a level section of %u bytes in a page of %lld", what, row_group, page, n, bytes);
}

// type mapping + overrides (planhip.h), flatness, page directory, encodings, and the sections of every page
// flags: PH_PARQUET_SNAPPY / PH_PARQUET_LZ4_RAW / PH_PARQUET_GZIP / PH_PARQUET_ZSTD (page_directory) and / or PH_PARQUET_DELTA (delta pages become PageDescs with `enc` set instead of a refusal)
// and / or PH_PARQUET_DELTA_BYTE_ARRAY (so do DELTA_BYTE_ARRAY pages of a BYTE_ARRAY column; the flag enables nothing else)
inline int resolve_column(const uint8_t *file, int64_t nbytes, const FileMeta &fm, int32_t column, int32_t type, int32_t scale, ColPlan *cp, Status *st,
                          uint32_t flags = 0) {
    if (column < 0 || column >= (int32_t)fm.leaves.size()) return st->fail(PH_EINVAL, "column %d: the file's schema has %zu leaf columns", column, fm.leaves.size());
    const Leaf &l = fm.leaves[(size_t)column];
    cp->column = column;
    cp->what = "column " + std::to_string(column) + " (" + leaf_name(file, l) + ")";
    const char *what = cp->what.c_str();
    if (l.max_rep != 0 || l.max_def > 1) return st->fail(PH_EUNSUPPORTED, "%s: a nested or repeated column (max definition level %d, max repetition level %d); flat columns only", what, l.max_def, l.max_rep);
    if (l.ph_type == 0) {
        const bool dec = l.converted == CT_DECIMAL || l.logical == 5;
        if (dec) return st->fail(PH_EUNSUPPORTED, "%s: %s Decimal(%d, %d) has no device type (scale 0..18, at most 16 bytes)", what, phys_name(l.phys), l.precision, l.scale);
        return st->fail(PH_EUNSUPPORTED, "%s: %s (converted type %d, logical type %d) has no device type", what, phys_name(l.phys), l.converted, l.logical);
    }
    cp->out_type = l.ph_type;
    cp->out_scale = l.ph_scale;
    if (type != 0) {
        const bool plain_int = l.ph_type == PH_I32 || l.ph_type == PH_I64;
        if (type == l.ph_type && (type != PH_DEC64 || scale == l.ph_scale)) {}   // naming what the schema says is no override
        else if (type == PH_I64 && l.ph_type == PH_I32) cp->out_type = PH_I64;
        else if (type == PH_I32 && l.ph_type == PH_I64) cp->out_type = PH_I32;
        else if (type == PH_DEC64 && plain_int && scale >= 0 && scale <= 18) { cp->out_type = PH_DEC64; cp->out_scale = scale; }
        else return st->fail(PH_EINVAL, "%s: type override %d (scale %d) over a column the schema maps to type %d (scale %d)", what, type, scale, l.ph_type, l.ph_scale);
    }
    cp->nullable = l.max_def == 1;
    cp->kind = l.phys == T_INT32 ? K_INT32 : l.phys == T_INT64 ? K_INT64 : l.phys == T_FLBA ? K_FLBA : K_BYTES;
    cp->flba_len = l.type_length;
    cp->width = cp->kind == K_INT32 ? 4 : cp->kind == K_INT64 ? 8 : cp->kind == K_FLBA ? l.type_length : 0;
    if (page_directory(file, nbytes, fm, column, what, &cp->dir, st, flags) != PH_OK) return st->code;
    // a compressed page's stream becomes a section of the region; the position its bytes will have (an empty stream: no section, no bytes)
    auto place = [&](const Page &pg, size_t i, int32_t owner, size_t index, bool v1_levels) -> int64_t {
        if (pg.stream_bytes() == 0) return pg.stream_pos();
        const int64_t at = cp->z_bytes;
        cp->sections.push_back(Section{pg.stream_pos(), pg.stream_bytes(), at, pg.stream_out(), pg.row_group, (int32_t)i, owner, (int32_t)index, v1_levels ? 1 : 0, pg.codec});
        cp->z_bytes += (pg.stream_out() + 15) & ~(int64_t)15;
        return Z_BASE + at;
    };
    const PageDesc *dict = nullptr;   // the current row group's dictionary
    PageDesc dict_desc{};
    int32_t dict_rg = -1;
    for (size_t i = 0; i < cp->dir.size(); i++) {
        const Page &pg = cp->dir[i];
        if (fm.groups[(size_t)pg.row_group].chunks[(size_t)column].phys != l.phys)
            return st->fail(PH_EINVAL, "%s: row group %d: the chunk's physical type differs from the schema's", what, pg.row_group);
        if (pg.row_group != dict_rg) { dict = nullptr; dict_rg = pg.row_group; }
        PageDesc d{};
        d.first_row = pg.first_row;
        d.num_values = pg.num_values;
        d.row_group = pg.row_group;
        d.page = (int32_t)i;
        d.lvl_bytes = -1;
        d.dict_n = -1;
        if (pg.kind == P_DICTIONARY) {
            if (pg.encoding != E_PLAIN && pg.encoding != E_PLAIN_DICTIONARY)
                return st->fail(PH_EUNSUPPORTED, "%s: row group %d, page %zu: a %s dictionary page", what, pg.row_group, i, enc_name(pg.encoding));
            const int64_t bytes = pg.compressed ? pg.uncompressed_bytes : pg.data_bytes;
            if (cp->width && (int64_t)pg.num_values * cp->width != bytes)
                return st->fail(PH_EINVAL, "%s: row group %d, page %zu: a dictionary page of %lld bytes for %d values of %d bytes", what, pg.row_group, i, (long long)bytes, pg.num_values, cp->width);
            d.val_pos = pg.compressed ? place(pg, i, cp->width ? 2 : 1, cp->dicts.size(), false) : pg.data_pos;
            d.val_bytes = (int32_t)bytes;
            d.dict_base = (int32_t)cp->dict_entries;
            if (!cp->width) {
                if (cp->dict_entries + pg.num_values >= (1ll << 31)) return st->fail(PH_EINVAL, "%s: 2^31 or more dictionary entries", what);
                cp->dict_entries += pg.num_values;
                cp->dicts.push_back(d);
            }
            dict_desc = d;
            dict = &dict_desc;
            continue;
        }
        int64_t pos = pg.data_pos, left = pg.data_bytes;
        if (pg.kind == P_DATA_V2) {
            if (pg.rep_bytes != 0) return st->fail(PH_EINVAL, "%s: row group %d, page %zu: repetition levels in a flat column", what, pg.row_group, i);
            if (cp->nullable) { d.lvl_pos = pos; d.lvl_bytes = (int32_t)pg.def_bytes; }
            pos += pg.def_bytes;
            left -= pg.def_bytes;
            if (pg.compressed) { pos = place(pg, i, 0, cp->pages.size(), false); left = pg.stream_out(); }   // (the level section stays where it is)
        } else if (pg.compressed) {  // v1, compressed: levels and values are one stream, the length in front of the levels lies inside it
            left = pg.uncompressed_bytes;
            if (cp->nullable && left < 4) return st->fail(PH_EINVAL, "%s: row group %d, page %zu: no room for the level section's length", what, pg.row_group, i);
            pos = place(pg, i, 0, cp->pages.size(), cp->nullable);
            if (cp->nullable) { d.lvl_pos = pos; d.lvl_bytes = 0; }   // (until complete_v1_levels has seen the bytes)
        } else if (cp->nullable) {   // v1: a 4-byte length in front of the definition levels
            uint32_t n;
            if (left < 4) return st->fail(PH_EINVAL, "%s: row group %d, page %zu: no room for the level section's length", what, pg.row_group, i);
            memcpy(&n, file + pos, 4);
            if ((int64_t)n > left - 4) return level_section_error(st, what, pg.row_group, (long long)i, n, (long long)pg.data_bytes);
            d.lvl_pos = pos + 4;
            d.lvl_bytes = (int32_t)n;
            pos += 4 + (int64_t)n;
            left -= 4 + (int64_t)n;
        }
        d.val_pos = pos;
        d.val_bytes = (int32_t)left;
        if (pg.encoding == E_RLE_DICTIONARY || pg.encoding == E_PLAIN_DICTIONARY) {
            if (!dict) return st->fail(PH_EINVAL, "%s: row group %d, page %zu: dictionary-coded values without a dictionary page", what, pg.row_group, i);
            d.dict_pos = dict->val_pos;
            d.dict_bytes = dict->val_bytes;
            d.dict_n = dict->num_values;
            d.dict_base = dict->dict_base;
        } else if (pg.encoding == E_DELTA_BYTE_ARRAY && (flags & PH_PARQUET_DELTA_BYTE_ARRAY)) {
            if (cp->kind != K_BYTES)
                return st->fail(PH_EUNSUPPORTED, "%s: row group %d, page %zu: %s values of a %s column; DELTA_BYTE_ARRAY is decoded over BYTE_ARRAY only", what, pg.row_group, i,
                                enc_name(pg.encoding), phys_name(l.phys));
            d.enc = pg.encoding;
        } else if (pg.encoding != E_PLAIN) {
            if (!(flags & PH_PARQUET_DELTA))
                return st->fail(PH_EUNSUPPORTED, "%s: row group %d, page %zu: %s values; PLAIN and RLE_DICTIONARY only", what, pg.row_group, i, enc_name(pg.encoding));
            const bool ints = pg.encoding == E_DELTA_BINARY_PACKED && (cp->kind == K_INT32 || cp->kind == K_INT64);
            if (!ints && !(pg.encoding == E_DELTA_LENGTH_BYTE_ARRAY && cp->kind == K_BYTES))
                return st->fail(PH_EUNSUPPORTED, "%s: row group %d, page %zu: %s values of a %s column; PLAIN, RLE_DICTIONARY, DELTA_BINARY_PACKED (INT32 / INT64) and DELTA_LENGTH_BYTE_ARRAY (BYTE_ARRAY) only",
                                what, pg.row_group, i, enc_name(pg.encoding), phys_name(l.phys));
            d.enc = pg.encoding;
        }
        if (d.dict_n < 0 && d.enc == 0 && cp->width && !cp->nullable && (int64_t)d.num_values * cp->width != d.val_bytes)   // (a nullable column's count is the decoders' to find)
            return st->fail(PH_EINVAL, "%s: row group %d, page %zu: %s", what, pg.row_group, i, cause_text(C_COUNT));
        cp->pages.push_back(d);
    }
    return PH_OK;
}

inline int page_error(Status *st, const ColPlan &cp, const PageDesc &d, int cause) {
    return st->fail(cause_code(cause), "%s: row group %d, page %d: %s", cp.what.c_str(), d.row_group, d.page, cause_text(cause));
}

// the definition levels of a page -> valid[0..num_values) (1 = a value), *nvalid. A required column: all ones.
template <class G>
inline int host_levels(const G &g, const PageDesc &d, uint8_t *valid, int64_t *nvalid) {
    const int64_t nv = d.num_values;
    if (d.lvl_bytes < 0) { for (int64_t i = 0; i < nv; i++) valid[i] = 1; *nvalid = nv; return C_OK; }
    int64_t pos = d.lvl_pos, done = 0, count = 0;
    const int64_t end = d.lvl_pos + d.lvl_bytes;
    while (done < nv) {
        Run r;
        const int c = next_run(g, pos, end, 1, &r);
        if (c != C_OK) return pos >= end ? C_COUNT : c;   // the section ended before num_values levels: too few
        if (!r.packed && r.count > nv - done) return C_COUNT;
        const int64_t n = r.count < nv - done ? r.count : nv - done;
        for (int64_t j = 0; j < n; j++) {
            const uint32_t v = r.packed ? packed_get(g, r.data, 1, j) : (r.value & 1u);
            valid[done + j] = (uint8_t)v;
            count += v;
        }
        done += n;
    }
    *nvalid = count;
    return C_OK;
}

// the dictionary indices of a page's values section -> idx[0..nvalid)
template <class G>
inline int host_indices(const G &g, const PageDesc &d, int64_t nvalid, uint32_t *idx) {
    if (nvalid == 0) return C_OK;
    if (d.val_bytes < 1) return C_COUNT;
    const int bw = g.u8(d.val_pos);
    if (bw > 32) return C_BIT_WIDTH;
    int64_t pos = d.val_pos + 1, done = 0;
    const int64_t end = d.val_pos + d.val_bytes;
    while (done < nvalid) {
        Run r;
        const int c = next_run(g, pos, end, bw, &r);
        if (c != C_OK) return pos >= end ? C_COUNT : c;
        if (!r.packed && r.count > nvalid - done) return C_COUNT;
        const int64_t n = r.count < nvalid - done ? r.count : nvalid - done;
        for (int64_t j = 0; j < n; j++) idx[done + j] = r.packed ? packed_get(g, r.data, bw, j) : r.value;
        done += n;
    }
    return C_OK;
}

// the length chain of a PLAIN BYTE_ARRAY section: n values, each a 4-byte length and its bytes; the chain ends exactly at the section's end
template <class G>
inline int host_byte_arrays(const G &g, int64_t pos, int64_t bytes, int64_t n, int64_t *vpos, int32_t *vlen) {
    const int64_t end = pos + bytes;
    for (int64_t k = 0; k < n; k++) {
        if (end - pos < 4) return C_COUNT;
        const uint32_t len = g.u32(pos);
        if ((int64_t)len > end - pos - 4) return C_LEN;
        vpos[k] = pos + 4;
        vlen[k] = (int32_t)len;
        pos += 4 + (int64_t)len;
    }
    return pos == end ? C_OK : C_COUNT;
}

// One DELTA_BINARY_PACKED stream at pos, block by block: the header, then per block its header (delta_block) and its values.
// expected: the count the header must state (-1: any, up to cap). emit(k, value k as the type sees it) -> a cause, which ends the decode
// (DS_EMIT, *emit_cause). Returns a DeltaSub; pos -> behind the last needed miniblock; *count = the header's count once it is readable.
template <class G, class Emit>
inline int host_delta_stream(const G &g, int64_t &pos, int64_t end, int bits, int64_t expected, int64_t cap, int64_t *count, int *emit_cause, const Emit &emit) {
    DeltaHeader h;
    *count = 0;
    int s = delta_header(g, pos, end, &h);
    if (s != DS_OK) return s;
    *count = h.total;
    if (expected >= 0 && h.total != expected) return DS_COUNT;
    if (h.total > cap) return DS_CAPACITY;
    if (h.total == 0) return DS_OK;
    uint64_t v = h.first;
    if ((*emit_cause = emit((int64_t)0, delta_value(v, bits))) != C_OK) return DS_EMIT;
    std::vector<int64_t> start((size_t)h.mini);
    std::vector<int> width((size_t)h.mini);
    for (int64_t done = 1; done < h.total;) {
        const int64_t need = h.total - done, n = need < h.block ? need : h.block;
        uint64_t min_delta = 0;
        s = delta_block(g, pos, end, h, need, bits, [&](int m, int64_t at, int w, uint64_t md) { start[(size_t)m] = at; width[(size_t)m] = w; min_delta = md; });
        if (s != DS_OK) return s;
        for (int64_t j = 0; j < n; j++) {
            const size_t m = (size_t)(j / h.per_mini);
            v += min_delta + packed_get64(g, start[m], width[m], j % h.per_mini);
            if ((*emit_cause = emit(done + j, delta_value(v, bits))) != C_OK) return DS_EMIT;
        }
        done += n;
    }
    return DS_OK;
}

// a DELTA_BINARY_PACKED values section of nvalid values -> dv[0..nvalid); the stream ends exactly at the section's end (PLAIN's strictness).
// A page without a value may have no bytes at all.
template <class G>
inline int host_delta_values(const G &g, const PageDesc &d, int bits, bool i32_range, int64_t nvalid, int64_t *dv) {
    if (nvalid == 0 && d.val_bytes == 0) return C_OK;
    int64_t pos = d.val_pos, count = 0;
    const int64_t end = d.val_pos + d.val_bytes;
    int emit_cause = C_OK;
    const int s = host_delta_stream(g, pos, end, bits, nvalid, nvalid, &count, &emit_cause, [&](int64_t k, int64_t v) {
        if (i32_range && v != (int32_t)v) return (int)C_I32_RANGE;
        dv[k] = v;
        return (int)C_OK;
    });
    if (s != DS_OK) return s == DS_EMIT ? emit_cause : delta_cause(s);
    return pos == end ? C_OK : C_COUNT;
}

// a DELTA_LENGTH_BYTE_ARRAY section of n values: one DELTA_BINARY_PACKED stream of INT32 lengths, then the values' bytes back to back, which
// end exactly at the section's end
template <class G>
inline int host_delta_lengths(const G &g, const PageDesc &d, int64_t n, int64_t *vpos, int32_t *vlen) {
    if (n == 0 && d.val_bytes == 0) return C_OK;
    int64_t pos = d.val_pos, count = 0;
    const int64_t end = d.val_pos + d.val_bytes;
    int emit_cause = C_OK;
    const int s = host_delta_stream(g, pos, end, 32, n, n, &count, &emit_cause, [&](int64_t k, int64_t v) {
        if (v < 0) return (int)C_LEN;
        vlen[k] = (int32_t)v;
        return (int)C_OK;
    });
    if (s != DS_OK) return s == DS_EMIT ? emit_cause : delta_cause(s);
    int64_t sum = 0;
    for (int64_t k = 0; k < n; k++) {
        vpos[k] = pos + sum;
        sum += vlen[k];
        if (sum > end - pos) return C_LEN;
    }
    return sum == end - pos ? C_OK : C_COUNT;
}

// ---- DELTA_BYTE_ARRAY (PH_PARQUET_DELTA_BYTE_ARRAY): front coding. The section [pos, end) is a DELTA_BINARY_PACKED stream of INT32 prefix
// lengths, then a DELTA_LENGTH_BYTE_ARRAY section of the suffixes: value[k] = value[k - 1][0, prefix[k]) + suffix[k], the value in front of
// value[0] being empty. What is wrong with a section (ph_dba_stream.sub): a pq::DeltaSub of the prefix stream as it is, of the suffix-length
// stream plus DBA_SUFFIX_STREAM, or one of the cases below. The ORDER of the checks is part of the contract, since the kernels (parquet_load.hip,
// pq_dba_lengths) make them in the same order and so name the same cause when a section has two faults: the prefix stream, value by value;
// the suffix-length stream; prefix[k] <= len[k - 1] over all k; the suffix bytes against the section's end.
enum DbaSub : int {
    DBA_OK = 0,
    DBA_SUFFIX_STREAM = 32,  // + the DeltaSub of the suffix-length stream
    DBA_PREFIX = 64,         // a prefix negative, or above the length of the value in front of it (prefix[0] != 0 included)
    DBA_SUFFIX_NEG = 65,     // a negative suffix length
    DBA_SUFFIX_PAST = 66,    // the suffixes' bytes run past the section's end
    DBA_SUFFIX_SHORT = 67,   // they end in front of it
    DBA_BYTE_CAP = 68,       // (the raw decoders) the values hold more bytes than the caller's room
    DBA_2G = 69,             // (the raw decoders) the values hold 2^31 bytes or more
};

PH_HD int dba_cause(int sub) {
    return sub < DBA_SUFFIX_STREAM ? delta_cause(sub) : sub < DBA_PREFIX ? delta_cause(sub - DBA_SUFFIX_STREAM) : sub == DBA_PREFIX ? C_PREFIX
         : sub == DBA_SUFFIX_SHORT ? C_COUNT : C_LEN;
}

inline int dba_status(int sub) {
    const int in = sub < DBA_SUFFIX_STREAM ? sub : sub < DBA_PREFIX ? sub - DBA_SUFFIX_STREAM : -1;
    return sub == DBA_OK ? PH_OK : (in == DS_CAPACITY || sub == DBA_BYTE_CAP) ? PH_ECAPACITY : sub == DBA_2G ? PH_EINVAL : cause_code(dba_cause(sub));
}

inline std::string dba_sub_text(int sub) {
    if (sub < DBA_SUFFIX_STREAM) return std::string("the prefix-length stream: ") + delta_sub_text(sub);
    if (sub < DBA_PREFIX) return std::string("the suffix-length stream: ") + delta_sub_text(sub - DBA_SUFFIX_STREAM);
    switch (sub) {
    case DBA_PREFIX: return cause_text(C_PREFIX);
    case DBA_SUFFIX_NEG: return "a negative suffix length";
    case DBA_SUFFIX_PAST: return "suffix bytes that run past the end";
    case DBA_SUFFIX_SHORT: return "bytes left over behind the last suffix";
    case DBA_BYTE_CAP: return "more bytes than the destination holds";
    case DBA_2G: return "2^31 or more bytes of values";
    default: return "unknown";
    }
}

// The lengths of one section -> pre[k], slen[k], spos[k] (where suffix k's bytes lie) for k < *count, each array with room for cap values;
// *total = the bytes the values hold (64 bits). expected: the count both streams must state (-1: any, up to cap). Returns a DbaSub; every
// rule is judged here, before a byte moves.
template <class G>
inline int host_dba_lengths(const G &g, int64_t pos, int64_t end, int64_t expected, int64_t cap, int32_t *pre, int32_t *slen, int64_t *spos, int64_t *count, int64_t *total) {
    *count = 0;
    *total = 0;
    int emit_cause = C_OK;
    int s = host_delta_stream(g, pos, end, 32, expected, cap, count, &emit_cause, [&](int64_t k, int64_t v) {
        if (v < 0) return (int)C_PREFIX;
        pre[k] = (int32_t)v;
        return (int)C_OK;
    });
    if (s != DS_OK) return s == DS_EMIT ? (int)DBA_PREFIX : s;
    const int64_t n = *count;
    int64_t n2 = 0;
    s = host_delta_stream(g, pos, end, 32, n, n, &n2, &emit_cause, [&](int64_t k, int64_t v) {
        if (v < 0) return (int)C_LEN;
        slen[k] = (int32_t)v;
        return (int)C_OK;
    });
    if (s != DS_OK) return s == DS_EMIT ? (int)DBA_SUFFIX_NEG : (int)DBA_SUFFIX_STREAM + s;
    int64_t before = 0, sum = 0, all = 0;
    for (int64_t k = 0; k < n; k++) {
        if (pre[k] > before) return DBA_PREFIX;
        before = (int64_t)pre[k] + slen[k];
        all += before;
    }
    for (int64_t k = 0; k < n; k++) {
        spos[k] = pos + sum;
        sum += slen[k];
        if (sum > end - pos) return DBA_SUFFIX_PAST;
    }
    if (sum != end - pos) return DBA_SUFFIX_SHORT;
    *total = all;
    return DBA_OK;
}

// the values of a section whose lengths host_dba_lengths has passed, back to back into out (room for its *total): the sequential chain
template <class G>
inline void host_dba_expand(const G &g, int64_t n, const int32_t *pre, const int32_t *slen, const int64_t *spos, char *out) {
    int64_t at = 0, before = 0;   // where value k begins; the length of value k - 1, which ends there
    for (int64_t k = 0; k < n; k++) {
        if (pre[k]) memcpy(out + at, out + at - before, (size_t)pre[k]);          // (pre[k] <= before: the two ranges do not overlap)
        if (slen[k]) memcpy(out + at + pre[k], g.at(spos[k]), (size_t)slen[k]);
        before = (int64_t)pre[k] + slen[k];
        at += before;
    }
}

// ph_delta_byte_array_decode_host: one raw section. Temporaries are sized by the caller's room for lengths.
inline int host_dba_section(const uint8_t *src, ph_dba_stream *S, int32_t *lens, char *bytes) {
    const HostBytes g(src);
    std::vector<int32_t> pre((size_t)S->len_cap + 1), slen((size_t)S->len_cap + 1);
    std::vector<int64_t> spos((size_t)S->len_cap + 1);
    int sub = host_dba_lengths(g, S->src_pos, S->src_pos + S->src_bytes, S->expected, S->len_cap, pre.data(), slen.data(), spos.data(), &S->count, &S->total_bytes);
    if (sub == DBA_OK) sub = S->total_bytes >= (1ll << 31) ? DBA_2G : S->total_bytes > S->byte_cap ? DBA_BYTE_CAP : DBA_OK;
    if (sub == DBA_OK) {
        for (int64_t k = 0; k < S->count; k++) lens[S->len_pos + k] = pre[(size_t)k] + slen[(size_t)k];
        if (S->total_bytes > 0) host_dba_expand(g, S->count, pre.data(), slen.data(), spos.data(), bytes + S->byte_pos);
    }
    S->consumed = sub == DBA_OK ? S->src_bytes : 0;
    S->sub = sub;
    S->status = dba_status(sub);
    return sub;
}

template <int KIND>
inline int host_delta_fixed_page(const HostBytes &g, const ColPlan &cp, const PageDesc &d, const uint8_t *valid, int64_t nvalid, int64_t *values) {
    std::vector<int64_t> dv((size_t)nvalid + 1);
    const int c = host_delta_values(g, d, KIND == K_INT32 ? 32 : 64, cp.out_type == PH_I32, nvalid, dv.data());
    if (c != C_OK) return c;
    int64_t k = 0;
    for (int64_t i = 0; i < d.num_values; i++) values[d.first_row + i] = valid[i] ? dv[(size_t)k++] : 0;
    return C_OK;
}

template <int KIND>
inline int host_fixed_page(const HostBytes &g, const ColPlan &cp, const PageDesc &d, const uint8_t *valid, int64_t nvalid, const uint32_t *idx, int64_t *values) {
    if (d.dict_n < 0 && nvalid * cp.width != d.val_bytes) return C_COUNT;
    int64_t k = 0;
    for (int64_t i = 0; i < d.num_values; i++) {
        int64_t v = 0;
        if (valid[i]) {
            int64_t at;
            if (d.dict_n >= 0) {
                if (idx[k] >= (uint32_t)d.dict_n) return C_INDEX;
                at = d.dict_pos + (int64_t)idx[k] * cp.width;
            } else at = d.val_pos + k * cp.width;
            k++;
            const int c = plain_value<KIND>(g, at, cp.flba_len, &v);
            if (c != C_OK) return c;
            if (cp.out_type == PH_I32 && v != (int32_t)v) return C_I32_RANGE;
        }
        values[d.first_row + i] = v;
    }
    return C_OK;
}

// One column, sequentially, with the decoders above. Fixed types: values (widened to int64, NULL slots 0). BYTE_ARRAY: str_offsets[nrows + 1]
// and up to str_cap bytes; *str_total = the bytes the column holds (PH_ECAPACITY when str_cap is smaller). valid: one byte per row.
inline int decode_column_host(const uint8_t *file, const ColPlan &cp, int64_t nrows, int64_t *values, uint8_t *valid, int32_t *str_offsets,
                              char *str_bytes, int64_t str_cap, int64_t *str_total, Status *st) {
    // the compressed sections first, all of them, with the function the kernel instantiates; a failed one is zero-filled and reported when
    // the decode order reaches its page (dictionaries of BYTE_ARRAY columns, then the data pages, then fixed-width dictionaries: the
    // device's order of pages, so both name the same page when several are bad)
    std::vector<uint8_t> z((size_t)cp.z_bytes + 1);
    std::vector<int32_t> page_sec(cp.pages.size(), -1), dict_sec(cp.dicts.size(), -1);
    static_assert((int)snappy::S_OK == (int)lz4::S_OK && (int)snappy::S_OK == (int)gzip::S_OK && (int)snappy::S_OK == (int)zstd::S_OK, "one OK for every codec's sub-cases");
    std::vector<int> sec_sub(cp.sections.size(), snappy::S_OK);
    for (size_t i = 0; i < cp.sections.size(); i++) {
        const Section &s = cp.sections[i];
        sec_sub[i] = CODECS[codec_row(s.codec)].decompress_host(file + s.src_pos, s.src_bytes, z.data() + s.out_pos, s.out_bytes);   // (a row: page_directory)
        if (sec_sub[i] != snappy::S_OK) memset(z.data() + s.out_pos, 0, (size_t)s.out_bytes);
        if (s.owner == 0) page_sec[(size_t)s.index] = (int32_t)i;
        else if (s.owner == 1) dict_sec[(size_t)s.index] = (int32_t)i;
    }
    auto section_error = [&](int32_t sec) { const Section &s = cp.sections[(size_t)sec]; PageDesc d{}; d.row_group = s.row_group; d.page = s.page; return page_error(st, cp, d, CODECS[codec_row(s.codec)].cause); };
    const HostBytes g(file, z.data());
    std::vector<uint32_t> idx;
    std::vector<int64_t> vpos, dpos((size_t)cp.dict_entries);
    std::vector<int32_t> vlen, vpre, dlen((size_t)cp.dict_entries);
    std::vector<uint8_t> own_valid;
    if (!valid) { own_valid.resize((size_t)nrows + 1); valid = own_valid.data(); }
    for (size_t di = 0; di < cp.dicts.size(); di++) {
        const PageDesc &d = cp.dicts[di];
        if (dict_sec[di] >= 0 && sec_sub[(size_t)dict_sec[di]] != snappy::S_OK) return section_error(dict_sec[di]);
        const int c = host_byte_arrays(g, d.val_pos, d.val_bytes, d.num_values, dpos.data() + d.dict_base, dlen.data() + d.dict_base);
        if (c != C_OK) return page_error(st, cp, d, c);
    }
    int64_t total = 0;
    if (cp.kind == K_BYTES && str_offsets) str_offsets[0] = 0;
    for (size_t pi = 0; pi < cp.pages.size(); pi++) {
        PageDesc d = cp.pages[pi];
        if (page_sec[pi] >= 0) {
            const Section &s = cp.sections[(size_t)page_sec[pi]];
            if (sec_sub[(size_t)page_sec[pi]] != snappy::S_OK) return section_error(page_sec[pi]);
            if (s.v1_levels) {
                const uint32_t n = g.u32(Z_BASE + s.out_pos);
                if (complete_v1_levels(d, Z_BASE + s.out_pos, s.out_bytes, n) != C_OK) return level_section_error(st, cp.what.c_str(), d.row_group, d.page, n, (long long)s.out_bytes);
            }
        }
        int64_t nvalid = 0;
        uint8_t *pv = valid + d.first_row;
        int c = host_levels(g, d, pv, &nvalid);
        if (c != C_OK) return page_error(st, cp, d, c);
        if (d.dict_n >= 0) {
            idx.resize((size_t)nvalid + 1);
            c = host_indices(g, d, nvalid, idx.data());
            if (c != C_OK) return page_error(st, cp, d, c);
        }
        if (cp.kind != K_BYTES) {
            c = d.enc == E_DELTA_BINARY_PACKED ? (cp.kind == K_INT32 ? host_delta_fixed_page<K_INT32>(g, cp, d, pv, nvalid, values) : host_delta_fixed_page<K_INT64>(g, cp, d, pv, nvalid, values))
              : cp.kind == K_INT32 ? host_fixed_page<K_INT32>(g, cp, d, pv, nvalid, idx.data(), values)
              : cp.kind == K_INT64 ? host_fixed_page<K_INT64>(g, cp, d, pv, nvalid, idx.data(), values)
                                   : host_fixed_page<K_FLBA>(g, cp, d, pv, nvalid, idx.data(), values);
            if (c != C_OK) return page_error(st, cp, d, c);
            continue;
        }
        const bool front = d.enc == E_DELTA_BYTE_ARRAY;   // vlen = the suffixes' lengths, vpos = their bytes, vpre = the prefixes
        if (d.dict_n < 0) {
            vpos.resize((size_t)nvalid + 1);
            vlen.resize((size_t)nvalid + 1);
            if (front) {
                vpre.resize((size_t)nvalid + 1);
                int64_t count = 0, bytes = 0;
                c = nvalid == 0 && d.val_bytes == 0 ? (int)C_OK
                  : dba_cause(host_dba_lengths(g, d.val_pos, d.val_pos + d.val_bytes, nvalid, nvalid, vpre.data(), vlen.data(), vpos.data(), &count, &bytes));
            } else
            c = d.enc == E_DELTA_LENGTH_BYTE_ARRAY ? host_delta_lengths(g, d, nvalid, vpos.data(), vlen.data())
                                                   : host_byte_arrays(g, d.val_pos, d.val_bytes, nvalid, vpos.data(), vlen.data());
            if (c != C_OK) return page_error(st, cp, d, c);
        }
        int64_t k = 0, before = 0;                        // (a front-coded page: the length of the page's value in front of this one)
        for (int64_t i = 0; i < d.num_values; i++) {
            if (pv[i]) {
                int64_t at, len;
                if (d.dict_n >= 0) {
                    if (idx[(size_t)k] >= (uint32_t)d.dict_n) return page_error(st, cp, d, C_INDEX);
                    at = dpos[(size_t)d.dict_base + idx[(size_t)k]];
                    len = dlen[(size_t)d.dict_base + idx[(size_t)k]];
                } else { at = vpos[(size_t)k]; len = vlen[(size_t)k]; }
                k++;
                if (total + len >= (1ll << 31)) return st->fail(PH_EINVAL, "%s holds 2^31 or more string bytes (int32 offsets)", cp.what.c_str());
                if (front) {                              // the prefix lies `before` bytes back in the output: a page's values are contiguous there
                    const int64_t pre = vpre[(size_t)k - 1];
                    len += pre;
                    if (total + len >= (1ll << 31)) return st->fail(PH_EINVAL, "%s holds 2^31 or more string bytes (int32 offsets)", cp.what.c_str());
                    if (str_bytes && total + len <= str_cap) {
                        if (pre) memcpy(str_bytes + total, str_bytes + total - before, (size_t)pre);
                        if (len - pre) memcpy(str_bytes + total + pre, g.at(at), (size_t)(len - pre));
                    }
                    before = len;
                } else if (str_bytes && total + len <= str_cap && len) memcpy(str_bytes + total, g.at(at), (size_t)len);
                total += len;
            }
            if (str_offsets) str_offsets[d.first_row + i + 1] = (int32_t)total;
        }
    }
    for (size_t i = 0; i < cp.sections.size(); i++)
        if (cp.sections[i].owner == 2 && sec_sub[i] != snappy::S_OK) return section_error((int32_t)i);
    if (str_total) *str_total = total;
    if (cp.kind == K_BYTES && str_bytes && total > str_cap) return st->fail(PH_ECAPACITY, "%s holds %lld string bytes, the buffer %lld", cp.what.c_str(), (long long)total, (long long)str_cap);
    return PH_OK;
}

}  // namespace pq
}  // namespace ph
