// Parquet metadata on the host: the Thrift compact-protocol footer (FileMetaData) and the page headers of a column chunk, parsed
// into plain structs. O(pages) work; no HIP in here, a plain host compiler can include it (tests/test_parquet_reference.py).
//
// Every position and length read from the file is checked against the file's size, and against the enclosing chunk or page, before
// it is stored: what leaves this header describes byte ranges that exist. A failed check is PH_EINVAL; something the format allows
// but the device path does not decode is PH_EUNSUPPORTED. Both carry a message.
#pragma once

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "parquet_codecs.h"
#include "planhip.h"

namespace ph {
namespace pq {

// parquet.thrift's enums, as far as this reader names them
enum Phys : int32_t { T_BOOLEAN = 0, T_INT32 = 1, T_INT64 = 2, T_INT96 = 3, T_FLOAT = 4, T_DOUBLE = 5, T_BYTE_ARRAY = 6, T_FLBA = 7 };
enum Enc : int32_t { E_PLAIN = 0, E_PLAIN_DICTIONARY = 2, E_RLE = 3, E_BIT_PACKED = 4, E_DELTA_BINARY_PACKED = 5, E_DELTA_LENGTH_BYTE_ARRAY = 6,
                     E_DELTA_BYTE_ARRAY = 7, E_RLE_DICTIONARY = 8, E_BYTE_STREAM_SPLIT = 9 };
enum PageType : int32_t { P_DATA = 0, P_INDEX = 1, P_DICTIONARY = 2, P_DATA_V2 = 3 };
enum Converted : int32_t { CT_NONE = -1, CT_UTF8 = 0, CT_DECIMAL = 5, CT_DATE = 6, CT_INT_32 = 17, CT_INT_64 = 18 };

struct Status {
    int code = PH_OK;
    std::string msg;
    bool ok() const { return code == PH_OK; }
    int fail(int c, const char *fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        code = c;
        msg = buf;
        return c;
    }
};

inline const char *phys_name(int32_t t) {
    static const char *const n[] = {"BOOLEAN", "INT32", "INT64", "INT96", "FLOAT", "DOUBLE", "BYTE_ARRAY", "FIXED_LEN_BYTE_ARRAY"};
    return t >= 0 && t < 8 ? n[t] : "an unknown physical type";
}
inline const char *enc_name(int32_t e) {
    static const char *const n[] = {"PLAIN", "GROUP_VAR_INT", "PLAIN_DICTIONARY", "RLE", "BIT_PACKED", "DELTA_BINARY_PACKED", "DELTA_LENGTH_BYTE_ARRAY",
                                    "DELTA_BYTE_ARRAY", "RLE_DICTIONARY", "BYTE_STREAM_SPLIT"};
    return e >= 0 && e < 10 ? n[e] : "an unknown encoding";
}
inline const char *codec_name(int32_t c) {
    static const char *const n[] = {"UNCOMPRESSED", "SNAPPY", "GZIP", "LZO", "BROTLI", "LZ4", "ZSTD", "LZ4_RAW"};
    return c >= 0 && c < 8 ? n[c] : "an unknown codec";
}

// ---- Thrift compact protocol over [p, end): every read is bounds-checked; `bad` sticks once set
struct Thrift {
    const uint8_t *base;
    int64_t p, end;
    bool bad = false;
    enum { TRUE_ = 1, FALSE_ = 2, BYTE = 3, I16 = 4, I32 = 5, I64 = 6, DOUBLE = 7, BINARY = 8, LIST = 9, SET = 10, MAP = 11, STRUCT = 12 };

    uint8_t byte() {
        if (p >= end) { bad = true; return 0; }
        return base[p++];
    }
    uint64_t uvarint() {
        uint64_t v = 0;
        for (int shift = 0; shift < 70; shift += 7) {
            const uint8_t b = byte();
            if (bad) return 0;
            v |= (uint64_t)(b & 0x7f) << (shift < 64 ? shift : 63);
            if (!(b & 0x80)) return v;
        }
        bad = true;
        return 0;
    }
    int64_t zigzag() {
        const uint64_t u = uvarint();
        return (int64_t)(u >> 1) ^ -(int64_t)(u & 1);
    }
    // a binary / string: position and length inside the buffer
    void binary(int64_t *pos, int64_t *len) {
        const uint64_t n = uvarint();
        if (bad || n > (uint64_t)(end - p)) { bad = true; *pos = 0; *len = 0; return; }
        *pos = p;
        *len = (int64_t)n;
        p += (int64_t)n;
    }
    // next field of a struct: false at the stop byte (or on error). *last_id is the running field id of this struct.
    bool field(int16_t *last_id, int *type) {
        const uint8_t h = byte();
        if (bad || h == 0) return false;
        *type = h & 0x0f;
        const int delta = h >> 4;
        if (delta) *last_id = (int16_t)(*last_id + delta);
        else *last_id = (int16_t)zigzag();
        return !bad;
    }
    void list(int *elem_type, int64_t *n) {
        const uint8_t h = byte();
        *elem_type = h & 0x0f;
        *n = h >> 4;
        if (*n == 15) *n = (int64_t)uvarint();
        if (*n < 0 || *n > end - p) bad = true;   // every element takes at least a byte
        if (bad) *n = 0;
    }
    void skip(int type, int depth = 0) {
        if (bad || depth > 32) { bad = true; return; }
        switch (type) {
        case TRUE_: case FALSE_: return;
        case BYTE: (void)byte(); return;
        case I16: case I32: case I64: (void)uvarint(); return;
        case DOUBLE: if (end - p < 8) bad = true; else p += 8; return;
        case BINARY: { int64_t a, b; binary(&a, &b); return; }
        case LIST: case SET: {
            int et; int64_t n;
            list(&et, &n);
            for (int64_t i = 0; i < n && !bad; i++) {
                if (et == TRUE_ || et == FALSE_) (void)byte();   // a bool inside a list is one byte
                else skip(et, depth + 1);
            }
            return;
        }
        case MAP: {
            const int64_t n = (int64_t)uvarint();
            if (bad || n < 0 || n > end - p) { bad = true; return; }
            if (n == 0) return;
            const uint8_t kv = byte();
            for (int64_t i = 0; i < n && !bad; i++) { skip(kv >> 4, depth + 1); skip(kv & 0x0f, depth + 1); }
            return;
        }
        case STRUCT: {
            int16_t id = 0; int t;
            while (field(&id, &t)) skip(t, depth + 1);
            return;
        }
        default: bad = true;
        }
    }
};

struct Leaf {                       // one leaf column of the schema, in schema order
    int64_t name_pos = 0, name_len = 0;
    int32_t phys = -1, type_length = 0;
    int32_t converted = CT_NONE, scale = 0, precision = 0;
    int32_t logical = 0;            // LogicalType union field: 1 STRING, 5 DECIMAL, 6 DATE, 0 none, others as parquet.thrift numbers them
    int32_t max_def = 0, max_rep = 0;
    int32_t ph_type = 0, ph_scale = 0;   // what the schema maps to (0: no device type)
};

struct Chunk {
    int32_t phys = -1, codec = 0;
    int64_t num_values = 0, total_compressed = 0, data_page_offset = -1, dict_page_offset = -1;
    bool has_meta = false, encrypted = false;
    int64_t start() const { return dict_page_offset > 0 && dict_page_offset < data_page_offset ? dict_page_offset : data_page_offset; }
};

struct RowGroup {
    int64_t num_rows = 0, first_row = 0;
    std::vector<Chunk> chunks;
};

struct FileMeta {
    int64_t num_rows = 0;
    std::vector<Leaf> leaves;
    std::vector<RowGroup> groups;
};

struct Page {
    int32_t row_group = 0, kind = 0, encoding = 0, num_values = 0;
    int64_t first_row = 0, header_pos = 0, data_pos = 0, data_bytes = 0;
    int64_t rep_bytes = 0, def_bytes = 0;   // v2: the level sections' lengths from the header (v1: 0, the length prefix is in the data)
    int32_t codec = 0;                      // the chunk's CompressionCodec
    int32_t compressed = 0;                 // 1: the values (v1 and dictionary pages: all data_bytes) are stored as one compressed stream
    int64_t uncompressed_bytes = 0;         // the header's uncompressed_page_size
    bool v2_is_compressed = true;           // DataPageHeaderV2.is_compressed (default true)
    // a compressed page's stream: where it lies in the file and what it must produce
    int64_t stream_pos() const { return data_pos + rep_bytes + def_bytes; }
    int64_t stream_bytes() const { return data_bytes - rep_bytes - def_bytes; }
    int64_t stream_out() const { return uncompressed_bytes - rep_bytes - def_bytes; }
};

// page_directory's flags: PH_PARQUET_* of planhip.h, and
constexpr uint32_t DIR_LIST_ONLY = 0x80000000u;   // ph_parquet_pages_ex: list the pages of a chunk in any codec, check no stream

// the ph_type a leaf's schema entry maps to (the table of planhip.h)
inline void map_leaf(Leaf &l) {
    l.ph_type = 0;
    l.ph_scale = 0;
    const bool dec = l.converted == CT_DECIMAL || l.logical == 5;
    const bool date = l.converted == CT_DATE || l.logical == 6;
    const bool str = l.converted == CT_UTF8 || l.logical == 1;
    const bool plain = l.converted == CT_NONE && l.logical == 0;
    if (dec) {
        const bool width = l.phys == T_INT32 || l.phys == T_INT64 || (l.phys == T_FLBA && l.type_length >= 1 && l.type_length <= 16);
        if (width && l.scale >= 0 && l.scale <= 18) { l.ph_type = PH_DEC64; l.ph_scale = l.scale; }
        return;
    }
    if (l.phys == T_INT32 && date) l.ph_type = PH_DATE;
    else if (l.phys == T_INT32 && (plain || l.converted == CT_INT_32)) l.ph_type = PH_I32;
    else if (l.phys == T_INT64 && (plain || l.converted == CT_INT_64)) l.ph_type = PH_I64;
    else if (l.phys == T_BYTE_ARRAY && (plain || str)) l.ph_type = PH_STR;
}

namespace detail {

struct Element {
    Leaf leaf;
    int32_t repetition = 0, num_children = 0;
};

inline void parse_logical(Thrift &t, Leaf &l) {
    int16_t id = 0; int ty;
    while (t.field(&id, &ty)) {
        l.logical = id;
        if (id == 5 && ty == Thrift::STRUCT) {   // DecimalType { 1: scale, 2: precision }
            int16_t id2 = 0; int ty2;
            while (t.field(&id2, &ty2)) {
                if (id2 == 1 && ty2 == Thrift::I32) l.scale = (int32_t)t.zigzag();
                else if (id2 == 2 && ty2 == Thrift::I32) l.precision = (int32_t)t.zigzag();
                else t.skip(ty2);
            }
        } else t.skip(ty);
    }
}

inline void parse_element(Thrift &t, Element &e) {
    int16_t id = 0; int ty;
    while (t.field(&id, &ty)) {
        if (id == 1 && ty == Thrift::I32) e.leaf.phys = (int32_t)t.zigzag();
        else if (id == 2 && ty == Thrift::I32) e.leaf.type_length = (int32_t)t.zigzag();
        else if (id == 3 && ty == Thrift::I32) e.repetition = (int32_t)t.zigzag();
        else if (id == 4 && ty == Thrift::BINARY) t.binary(&e.leaf.name_pos, &e.leaf.name_len);
        else if (id == 5 && ty == Thrift::I32) e.num_children = (int32_t)t.zigzag();
        else if (id == 6 && ty == Thrift::I32) e.leaf.converted = (int32_t)t.zigzag();
        else if (id == 7 && ty == Thrift::I32) e.leaf.scale = (int32_t)t.zigzag();
        else if (id == 8 && ty == Thrift::I32) e.leaf.precision = (int32_t)t.zigzag();
        else if (id == 10 && ty == Thrift::STRUCT) parse_logical(t, e.leaf);
        else t.skip(ty);
    }
}

inline void parse_chunk_meta(Thrift &t, Chunk &c) {
    int16_t id = 0; int ty;
    c.has_meta = true;
    while (t.field(&id, &ty)) {
        if (id == 1 && ty == Thrift::I32) c.phys = (int32_t)t.zigzag();
        else if (id == 4 && ty == Thrift::I32) c.codec = (int32_t)t.zigzag();
        else if (id == 5 && ty == Thrift::I64) c.num_values = t.zigzag();
        else if (id == 7 && ty == Thrift::I64) c.total_compressed = t.zigzag();
        else if (id == 9 && ty == Thrift::I64) c.data_page_offset = t.zigzag();
        else if (id == 11 && ty == Thrift::I64) c.dict_page_offset = t.zigzag();
        else t.skip(ty);
    }
}

inline void parse_chunk(Thrift &t, Chunk &c) {
    int16_t id = 0; int ty;
    while (t.field(&id, &ty)) {
        if (id == 3 && ty == Thrift::STRUCT) parse_chunk_meta(t, c);
        else if (id == 8) { c.encrypted = true; t.skip(ty); }
        else t.skip(ty);
    }
}

inline void parse_row_group(Thrift &t, RowGroup &g) {
    int16_t id = 0; int ty;
    while (t.field(&id, &ty)) {
        if (id == 1 && ty == Thrift::LIST) {
            int et; int64_t n;
            t.list(&et, &n);
            if (et != Thrift::STRUCT) { t.bad = true; return; }
            g.chunks.resize((size_t)n);
            for (int64_t i = 0; i < n && !t.bad; i++) parse_chunk(t, g.chunks[(size_t)i]);
        } else if (id == 3 && ty == Thrift::I64) g.num_rows = t.zigzag();
        else t.skip(ty);
    }
}

}  // namespace detail

// the footer: "PAR1" ... FileMetaData, its 4-byte little-endian length, "PAR1"
inline int parse_footer(const uint8_t *file, int64_t nbytes, FileMeta *out, Status *st) {
    if (!file || nbytes < 12) return st->fail(PH_EINVAL, "not a parquet file: %lld bytes, fewer than the two magics and the footer length take", (long long)nbytes);
    if (!memcmp(file + nbytes - 4, "PARE", 4)) return st->fail(PH_EUNSUPPORTED, "the file has an encrypted footer (PARE)");
    if (memcmp(file, "PAR1", 4) || memcmp(file + nbytes - 4, "PAR1", 4)) return st->fail(PH_EINVAL, "not a parquet file: the PAR1 magic is missing at the head or the tail");
    uint32_t flen;
    memcpy(&flen, file + nbytes - 8, 4);
    if ((int64_t)flen > nbytes - 12 || flen == 0) return st->fail(PH_EINVAL, "footer length %u does not fit a file of %lld bytes", flen, (long long)nbytes);
    Thrift t{file, nbytes - 8 - (int64_t)flen, nbytes - 8};
    std::vector<detail::Element> elems;
    bool encrypted = false;
    int16_t id = 0; int ty;
    while (t.field(&id, &ty)) {
        if (id == 2 && ty == Thrift::LIST) {
            int et; int64_t n;
            t.list(&et, &n);
            if (et != Thrift::STRUCT) { t.bad = true; break; }
            elems.resize((size_t)n);
            for (int64_t i = 0; i < n && !t.bad; i++) detail::parse_element(t, elems[(size_t)i]);
        } else if (id == 3 && ty == Thrift::I64) out->num_rows = t.zigzag();
        else if (id == 4 && ty == Thrift::LIST) {
            int et; int64_t n;
            t.list(&et, &n);
            if (et != Thrift::STRUCT) { t.bad = true; break; }
            out->groups.resize((size_t)n);
            for (int64_t i = 0; i < n && !t.bad; i++) detail::parse_row_group(t, out->groups[(size_t)i]);
        } else if (id == 8) { encrypted = true; t.skip(ty); }
        else t.skip(ty);
    }
    if (t.bad) return st->fail(PH_EINVAL, "the footer is not a well-formed FileMetaData (malformed or cut near byte %lld)", (long long)t.p);
    if (encrypted) return st->fail(PH_EUNSUPPORTED, "the file is encrypted");
    if (elems.empty() || out->num_rows < 0) return st->fail(PH_EINVAL, "the footer holds no schema or a negative row count");
    // leaves in schema order with their maximum levels: a depth-first walk that never trusts num_children beyond the list's length
    struct Frame { int64_t left; int32_t def, rep; };
    std::vector<Frame> stack;
    stack.push_back(Frame{elems[0].num_children, 0, 0});
    for (size_t i = 1; i < elems.size(); i++) {
        while (!stack.empty() && stack.back().left == 0) stack.pop_back();
        if (stack.empty()) return st->fail(PH_EINVAL, "the schema tree has more elements than its groups announce");
        stack.back().left--;
        const detail::Element &e = elems[i];
        const int32_t def = stack.back().def + (e.repetition != 0 ? 1 : 0), rep = stack.back().rep + (e.repetition == 2 ? 1 : 0);
        if (e.num_children > 0) { stack.push_back(Frame{e.num_children, def, rep}); continue; }
        Leaf l = e.leaf;
        l.max_def = def;
        l.max_rep = rep;
        map_leaf(l);
        out->leaves.push_back(l);
    }
    int64_t rows = 0;
    for (RowGroup &g : out->groups) {
        if (g.num_rows < 0 || g.chunks.size() != out->leaves.size())
            return st->fail(PH_EINVAL, "a row group holds %zu column chunks for a schema of %zu leaves", g.chunks.size(), out->leaves.size());
        g.first_row = rows;
        rows += g.num_rows;
    }
    if (rows != out->num_rows) return st->fail(PH_EINVAL, "the row groups hold %lld rows, the footer says %lld", (long long)rows, (long long)out->num_rows);
    return PH_OK;
}

inline std::string leaf_name(const uint8_t *file, const Leaf &l) { return std::string((const char *)file + l.name_pos, (size_t)l.name_len); }

// one page header at [pos, end): *hdr_bytes = its length. Fills kind, encoding, num_values, data_bytes and the v2 level lengths.
inline int parse_page_header(const uint8_t *file, int64_t pos, int64_t end, Page *pg, int64_t *hdr_bytes, int32_t *uncompressed, Status *st) {
    Thrift t{file, pos, end};
    int32_t type = -1, csize = -1, usize = -1;
    bool have = false;
    int16_t id = 0; int ty;
    pg->num_values = -1;
    pg->encoding = -1;
    while (t.field(&id, &ty)) {
        if (id == 1 && ty == Thrift::I32) type = (int32_t)t.zigzag();
        else if (id == 2 && ty == Thrift::I32) usize = (int32_t)t.zigzag();
        else if (id == 3 && ty == Thrift::I32) csize = (int32_t)t.zigzag();
        else if ((id == 5 || id == 7) && ty == Thrift::STRUCT) {   // DataPageHeader / DictionaryPageHeader: 1 num_values, 2 encoding
            int16_t id2 = 0; int ty2;
            have = true;
            while (t.field(&id2, &ty2)) {
                if (id2 == 1 && ty2 == Thrift::I32) pg->num_values = (int32_t)t.zigzag();
                else if (id2 == 2 && ty2 == Thrift::I32) pg->encoding = (int32_t)t.zigzag();
                else t.skip(ty2);
            }
        } else if (id == 8 && ty == Thrift::STRUCT) {              // DataPageHeaderV2
            int16_t id2 = 0; int ty2;
            have = true;
            while (t.field(&id2, &ty2)) {
                if (id2 == 1 && ty2 == Thrift::I32) pg->num_values = (int32_t)t.zigzag();
                else if (id2 == 4 && ty2 == Thrift::I32) pg->encoding = (int32_t)t.zigzag();
                else if (id2 == 5 && ty2 == Thrift::I32) pg->def_bytes = (int32_t)t.zigzag();
                else if (id2 == 6 && ty2 == Thrift::I32) pg->rep_bytes = (int32_t)t.zigzag();
                else if (id2 == 7 && (ty2 == Thrift::TRUE_ || ty2 == Thrift::FALSE_)) pg->v2_is_compressed = ty2 == Thrift::TRUE_;   // (a bool lives in the field header)
                else t.skip(ty2);
            }
        } else t.skip(ty);
    }
    if (t.bad || type < 0 || csize < 0) return st->fail(PH_EINVAL, "the page header at byte %lld is malformed or leaves its chunk", (long long)pos);
    pg->kind = type;
    pg->header_pos = pos;
    pg->data_pos = t.p;
    pg->data_bytes = csize;
    *hdr_bytes = t.p - pos;
    *uncompressed = usize;
    if (pg->data_pos + pg->data_bytes > end) return st->fail(PH_EINVAL, "the page at byte %lld (%d data bytes) leaves its chunk", (long long)pos, csize);
    if (type != P_INDEX && (!have || pg->num_values < 0)) return st->fail(PH_EINVAL, "the page header at byte %lld lacks its page-type header", (long long)pos);
    if (type == P_DATA_V2 && (pg->def_bytes < 0 || pg->rep_bytes < 0 || pg->def_bytes + pg->rep_bytes > pg->data_bytes))
        return st->fail(PH_EINVAL, "the v2 page at byte %lld: level sections of %lld + %lld bytes in %d data bytes", (long long)pos, (long long)pg->rep_bytes, (long long)pg->def_bytes, csize);
    return PH_OK;
}

// the page directory of leaf `column` over all row groups (index pages are stepped over). `what` prefixes the messages ("column 3 (name)").
// flags 0: UNCOMPRESSED chunks only. PH_PARQUET_SNAPPY: SNAPPY chunks too; of a compressed page everything the host can see is checked
// here — the sizes against each other and the stream's own length preamble — so what is allocated for it is bounded by the file's size.
// PH_PARQUET_LZ4_RAW: LZ4_RAW chunks (codec 7) too. Such a stream has no preamble: what it must produce comes from the page header alone, at
// most 255 times the stream's bytes, and the decoder's exact-length rule is what catches a lying header. A file may hold chunks in different
// codecs; each is accepted when its flag is set (parquet_codecs.h: the table of flags and names that also words the refusal). Codec 5, the
// deprecated LZ4, is refused whatever the flags (lz4_decode.h says why).
// PH_PARQUET_GZIP: GZIP chunks (codec 2) too. No preamble either: a non-empty stream must hold the 20 bytes of the smallest member, begin
// 1f 8b 08 with no reserved FLG bit, and may be asked for at most 1032 times its bytes (gzip_decode.h); the rest is the decoder's.
// PH_PARQUET_ZSTD: ZSTD chunks (codec 6) too. A non-empty stream must hold the 9 bytes of the smallest frame, begin with the frame magic
// 28 b5 2f fd or a skippable frame's 5? 2a 4d 18, and may be asked for at most 32768 times its bytes (zstd_decode.h derives the bound).
inline int page_directory(const uint8_t *file, int64_t nbytes, const FileMeta &fm, int32_t column, const char *what, std::vector<Page> *out, Status *st,
                          uint32_t flags = 0) {
    for (size_t g = 0; g < fm.groups.size(); g++) {
        const RowGroup &rg = fm.groups[g];
        const Chunk &c = rg.chunks[(size_t)column];
        if (rg.num_rows == 0) continue;   // (nothing to decode; writers leave such a chunk's offsets at 0)
        if (c.encrypted) return st->fail(PH_EUNSUPPORTED, "%s: row group %zu: the column chunk is encrypted", what, g);
        if (!c.has_meta) return st->fail(PH_EINVAL, "%s: row group %zu: the column chunk has no metadata", what, g);
        const bool list_only = (flags & DIR_LIST_ONLY) != 0;
        const int known = codec_row(c.codec);
        if (c.codec != 0 && !list_only && (known < 0 || !(flags & CODECS[known].flag))) {   // the text lists the codecs the given word enables
            const bool note = c.codec == 5 && (flags & (PH_PARQUET_LZ4_RAW | PH_PARQUET_GZIP | PH_PARQUET_ZSTD)) != 0;
            return st->fail(PH_EUNSUPPORTED, "%s: row group %zu: %s pages%s; %s", what, g, codec_name(c.codec),
                            note ? " (codec 5, the deprecated LZ4 whose framing differs from writer to writer; not LZ4_RAW)" : "", decoded_codecs_text(flags).c_str());
        }
        const int64_t start = c.start();
        if (start < 4 || c.total_compressed < 0 || start > nbytes - 8 || c.total_compressed > nbytes - 8 - start)
            return st->fail(PH_EINVAL, "%s: row group %zu: the column chunk [%lld, +%lld) leaves the file", what, g, (long long)start, (long long)c.total_compressed);
        if (c.num_values != rg.num_rows) return st->fail(PH_EINVAL, "%s: row group %zu: %lld values for %lld rows", what, g, (long long)c.num_values, (long long)rg.num_rows);
        const int64_t end = start + c.total_compressed;
        int64_t pos = start, row = rg.first_row;
        bool dict = false;
        while (pos < end) {
            Page pg;
            int64_t hdr = 0;
            int32_t usize = 0;
            pg.row_group = (int32_t)g;
            if (parse_page_header(file, pos, end, &pg, &hdr, &usize, st) != PH_OK) {
                st->msg = std::string(what) + ": row group " + std::to_string(g) + ": " + st->msg;
                return st->code;
            }
            pos = pg.data_pos + pg.data_bytes;
            if (pg.kind == P_INDEX) continue;
            pg.codec = c.codec;
            pg.uncompressed_bytes = usize;
            pg.compressed = c.codec != 0 && (pg.kind != P_DATA_V2 || pg.v2_is_compressed) ? 1 : 0;
            if (pg.kind != P_DATA_V2) pg.rep_bytes = pg.def_bytes = 0;   // (only a v2 header carries them)
            if (list_only) {}
            else if (!pg.compressed) {
                if (usize != pg.data_bytes) return st->fail(PH_EUNSUPPORTED, "%s: row group %zu: a page of %d bytes holds %lld: compressed pages are not decoded", what, g, usize, (long long)pg.data_bytes);
            } else {
                const size_t i = out->size();
                const int64_t sbytes = pg.stream_bytes(), want = pg.stream_out();
                if (usize < 0 || want < 0)
                    return st->fail(PH_EINVAL, "%s: row group %zu, page %zu: an uncompressed size of %d bytes with level sections of %lld", what, g, i, usize, (long long)(pg.rep_bytes + pg.def_bytes));
                if (c.codec == 2) {
                    int sub = gzip::check_sizes(sbytes, want);
                    if (sub == gzip::S_OK && sbytes > 0) sub = gzip::check_header(file + pg.stream_pos());
                    if (sub == gzip::S_EMPTY) return st->fail(PH_EINVAL, "%s: row group %zu, page %zu: an empty GZIP stream for %lld bytes", what, g, i, (long long)want);
                    if (sub == gzip::S_IMPOSSIBLE)
                        return st->fail(PH_EINVAL, "%s: row group %zu, page %zu: %lld bytes from a GZIP stream of %lld: no stream yields more than 1032 to one", what, g, i, (long long)want, (long long)sbytes);
                    if (sub != gzip::S_OK)
                        return st->fail(PH_EINVAL, "%s: row group %zu, page %zu: a corrupt GZIP stream of %lld bytes for %lld: %s", what, g, i, (long long)sbytes, (long long)want, gzip::sub_text(sub));
                } else if (c.codec == 6) {
                    int sub = zstd::check_sizes(sbytes, want);
                    if (sub == zstd::S_OK && sbytes > 0) sub = zstd::check_header(file + pg.stream_pos());
                    if (sub == zstd::S_EMPTY) return st->fail(PH_EINVAL, "%s: row group %zu, page %zu: an empty ZSTD stream for %lld bytes", what, g, i, (long long)want);
                    if (sub == zstd::S_IMPOSSIBLE)
                        return st->fail(PH_EINVAL, "%s: row group %zu, page %zu: %lld bytes from a ZSTD stream of %lld: no stream yields more than 32768 to one", what, g, i, (long long)want, (long long)sbytes);
                    if (sub != zstd::S_OK)
                        return st->fail(PH_EINVAL, "%s: row group %zu, page %zu: a corrupt ZSTD stream of %lld bytes for %lld: %s", what, g, i, (long long)sbytes, (long long)want, zstd::sub_text(sub));
                } else if (c.codec == 7) {
                    const int sub = lz4::check_sizes(sbytes, want);
                    if (sub == lz4::S_EMPTY) return st->fail(PH_EINVAL, "%s: row group %zu, page %zu: an empty LZ4_RAW stream for %lld bytes", what, g, i, (long long)want);
                    if (sub != lz4::S_OK)
                        return st->fail(PH_EINVAL, "%s: row group %zu, page %zu: %lld bytes from an LZ4_RAW stream of %lld: no stream yields more than 255 to one", what, g, i, (long long)want, (long long)sbytes);
                } else if (sbytes == 0) {
                    if (want != 0) return st->fail(PH_EINVAL, "%s: row group %zu, page %zu: an empty SNAPPY stream for %lld bytes", what, g, i, (long long)want);
                } else if (want > snappy::MAX_EXPANSION * sbytes) {
                    return st->fail(PH_EINVAL, "%s: row group %zu, page %zu: %lld bytes from a SNAPPY stream of %lld: no stream yields more than 22 to one", what, g, i, (long long)want, (long long)sbytes);
                } else {
                    int64_t len = 0, body = 0;
                    const int sub = snappy::read_preamble(snappy::HostStream{file}, pg.stream_pos(), pg.stream_pos() + sbytes, want, &len, &body);
                    if (sub != snappy::S_OK)
                        return st->fail(PH_EINVAL, "%s: row group %zu, page %zu: a corrupt SNAPPY stream of %lld bytes for %lld: %s", what, g, i, (long long)sbytes, (long long)want, snappy::sub_text(sub));
                }
            }
            if (pg.kind == P_DICTIONARY) {
                if (dict || row != rg.first_row) return st->fail(PH_EINVAL, "%s: row group %zu: a second or late dictionary page", what, g);
                dict = true;
                pg.first_row = row;
            } else if (pg.kind == P_DATA || pg.kind == P_DATA_V2) {
                pg.first_row = row;
                row += pg.num_values;
                if (row > rg.first_row + rg.num_rows) return st->fail(PH_EINVAL, "%s: row group %zu: the data pages hold more values than the row group has rows", what, g);
            } else return st->fail(PH_EINVAL, "%s: row group %zu: page type %d", what, g, pg.kind);
            out->push_back(pg);
        }
        if (row != rg.first_row + rg.num_rows) return st->fail(PH_EINVAL, "%s: row group %zu: the data pages hold %lld values for %lld rows", what, g, (long long)(row - rg.first_row), (long long)rg.num_rows);
    }
    return PH_OK;
}

}  // namespace pq
}  // namespace ph
