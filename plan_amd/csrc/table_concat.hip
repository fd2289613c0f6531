// ph_table_concat: one resident table from N resident tables, built on the device (the rules are in include/planhip.h).
//
// Tables are immutable after load, so this is no append: the parts are read, and the result is the table ph_table_create would build over
// the same values in the same order. The work per column does not depend on the number of parts in launches or read-backs: ONE device
// table {source pointer, first output row} per part is uploaded for the whole call (parts of 0 rows are left out of it), every array is
// written by ONE launch over tiles of the OUTPUT, a workgroup finds the parts of its tile's first and last row by binary search over the
// starts, and a lane searches only between those two (not at all when they are the same part, which is every tile of a large part).
//
//   concat_fixed_kernel<W>      a lane writes aligned 16-byte units of the output. A unit that lies inside one part is read as the one or
//                               two ALIGNED 16-byte units of the source that cover it and shifted into place (the source of a part starts
//                               at an arbitrary output row: the two are misaligned against each other unless the start is a multiple of
//                               16 / W); a unit that crosses a part boundary or the end of the rows is put together value by value. The
//                               kernel covers the padding too (zeros), so the output needs no memset.
//   concat_fixed_kernel<1,true> the same over dictionary codes, each rewritten through its part's 256-byte table. The tables are read from
//                               global memory and served by L1 (a tile meets one table, or a few): no LDS staging. A NULL row's code is 0.
//   concat_validity_kernel      one lane per 32-bit output word (table_concat.h), every word written once.
//   concat_str_lengths_kernel   per output row the length and the address of its bytes: a PH_STR part's from its offsets, a code part's
//                               from a per-dictionary table over an uploaded blob of the dictionaries; then the context's scan and
//                               str_encode.h's copy_strings_kernel, as the loaders use them.
// Each column is finished by ph::table_finish_column over the new arrays.
#include <map>
#include <string>

#include "ops.h"
#include "str_encode.h"
#include "table_concat.h"

using ph::Temps;
using ph::TableGuard;
namespace cc = ph::concat;

namespace ph {

constexpr int CONCAT_UNITS = 4;                          // 16-byte units a lane writes
constexpr int CONCAT_TILE_UNITS = 256 * CONCAT_UNITS;    // per workgroup: 16 KiB of output

// the parts of rows r_first and r_last (both below the total), found by two lanes for the workgroup
__device__ inline void concat_tile_parts(const cc::Parts &P, int64_t r_first, int64_t r_last, int *s_range, int *plo, int *phi) {
    if (threadIdx.x < 2) s_range[threadIdx.x] = cc::find_part(P.starts, 0, P.np - 1, threadIdx.x ? r_last : r_first);
    __syncthreads();
    *plo = s_range[0];
    *phi = s_range[1];
}

// W = 1, 4, 8 bytes a value; REMAP: codes through their part's table (table_concat.h fixed_unit). nunits: the output's 16-byte units, padding included.
template <int W, bool REMAP>
__global__ __launch_bounds__(256) void concat_fixed_kernel(cc::Parts P, const uint8_t *__restrict__ remap, const int32_t *__restrict__ tab,
                                                           uint4 *__restrict__ out, int64_t nunits) {
    constexpr int R = 16 / W;   // values a unit
    __shared__ int s_range[2];
    const int64_t u0 = (int64_t)blockIdx.x * CONCAT_TILE_UNITS;
    const int64_t total = P.total;
    int plo = 0, phi = 0;
    if (u0 * R < total) {   // (the same for the whole workgroup)
        const int64_t r_end = (u0 + CONCAT_TILE_UNITS) * R;
        concat_tile_parts(P, u0 * R, (r_end < total ? r_end : total) - 1, s_range, &plo, &phi);
    }
#pragma unroll
    for (int i = 0; i < CONCAT_UNITS; i++) {
        const int64_t u = u0 + i * 256 + threadIdx.x;
        if (u < nunits) out[u] = cc::fixed_unit<W, REMAP>(P, remap, tab, u, plo, phi);
    }
}

__global__ __launch_bounds__(256) void concat_validity_kernel(cc::Parts P, uint32_t *__restrict__ out, int64_t nwords) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w < nwords) out[w] = cc::validity_word(w, P.np, P.starts, P.validity);
}

// VARCHAR: per output row its length into len_out and the place of its bytes into sbegin (table_concat.h string_row). The grid covers rows below the total only.
__global__ __launch_bounds__(256) void concat_str_lengths_kernel(cc::Parts P, const unsigned char *const *__restrict__ aux, const int32_t *__restrict__ tab,
                                                                 const int32_t *__restrict__ dlen, const int64_t *__restrict__ dpos,
                                                                 const unsigned char *blob, int32_t *__restrict__ len_out, int64_t *__restrict__ sbegin) {
    __shared__ int s_range[2];
    const int64_t r0 = (int64_t)blockIdx.x * 256, total = P.total;
    int plo, phi;
    concat_tile_parts(P, r0, (r0 + 256 < total ? r0 + 256 : total) - 1, s_range, &plo, &phi);
    const int64_t r = r0 + threadIdx.x;
    if (r >= total) return;
    int32_t len;
    int64_t begin;
    cc::string_row(P, aux, tab, dlen, dpos, blob, r, plo, phi, &len, &begin);
    len_out[r] = len;
    sbegin[r] = begin;
}

// ---------------------------------------------------------------- dictionaries (host)

static std::vector<std::string> split_blob(const char *blob, int64_t bytes) {   // NUL-separated, as table_finish_column reads it
    std::vector<std::string> d;
    const char *p = blob, *end = blob + bytes;
    while (p < end) {
        const size_t len = strnlen(p, (size_t)(end - p));
        d.emplace_back(p, len);
        p += len + 1;
    }
    return d;
}

// the union of the dictionaries' entries (the 256 a code can name) in unsigned byte order
static std::vector<std::string> merge_dicts(const std::vector<const std::vector<std::string> *> &dicts) {
    std::vector<std::string> m;
    for (const auto *d : dicts) m.insert(m.end(), d->begin(), d->begin() + (ptrdiff_t)std::min<size_t>(d->size(), 256));
    std::sort(m.begin(), m.end());   // std::string compares as unsigned bytes
    m.erase(std::unique(m.begin(), m.end()), m.end());
    return m;
}

// code of `dict` -> code of `merged` (at most 256 entries); a code the dictionary does not have -> 0
static void remap_of(const std::vector<std::string> &dict, const std::vector<std::string> &merged, uint8_t *out256) {
    memset(out256, 0, 256);
    for (size_t c = 0; c < dict.size() && c < 256; c++)
        out256[c] = (uint8_t)(std::lower_bound(merged.begin(), merged.end(), dict[c]) - merged.begin());
}

}  // namespace ph

extern "C" int ph_validity_concat_host(int32_t nparts, const uint8_t *const *bitmaps, const int64_t *rows, uint8_t *out, int64_t out_bytes) {
    PH_REQUIRE(nparts >= 0 && (nparts == 0 || rows) && out_bytes >= 0 && (out || out_bytes == 0), "ph_validity_concat_host: bad arguments");
    std::vector<int64_t> starts((size_t)nparts + 1, 0);
    for (int32_t p = 0; p < nparts; p++) {
        PH_REQUIRE(rows[p] >= 0, "ph_validity_concat_host: part %d has %lld rows", p, (long long)rows[p]);
        starts[(size_t)p + 1] = starts[(size_t)p] + rows[p];
    }
    const int64_t total = starts[(size_t)nparts], need = (total + 7) / 8;
    if (out_bytes < need) {
        ph::set_error("ph_validity_concat_host: %lld rows need %lld bytes, the buffer has %lld", (long long)total, (long long)need, (long long)out_bytes);
        return PH_ECAPACITY;
    }
    memset(out, 0, (size_t)out_bytes);
    for (int64_t w = 0; w * 32 < total; w++) {
        const uint32_t word = cc::validity_word(w, nparts, starts.data(), bitmaps);
        for (int b = 0; b < 4 && w * 4 + b < out_bytes; b++) out[w * 4 + b] = (uint8_t)(word >> (8 * b));
    }
    return PH_OK;
}

extern "C" int ph_dict_merge_host(int32_t nparts, const char *const *blobs, const int64_t *blob_bytes, char *merged, int64_t merged_cap,
                                  int64_t *merged_bytes, int32_t *nmerged, uint8_t *remap, int32_t *identical) {
    PH_REQUIRE(nparts >= 1 && blobs && blob_bytes && merged_bytes && nmerged && remap && identical && merged_cap >= 0 && (merged || merged_cap == 0),
               "ph_dict_merge_host: bad arguments");
    std::vector<std::vector<std::string>> dicts((size_t)nparts);
    for (int32_t p = 0; p < nparts; p++) {
        PH_REQUIRE(blob_bytes[p] >= 0 && (blobs[p] || blob_bytes[p] == 0), "ph_dict_merge_host: part %d has no dictionary", p);
        dicts[(size_t)p] = ph::split_blob(blobs[p], blob_bytes[p]);
        PH_REQUIRE(dicts[(size_t)p].size() <= 256, "ph_dict_merge_host: part %d has %lld entries (a code names 256)", p, (long long)dicts[(size_t)p].size());
    }
    bool same = true;
    for (int32_t p = 1; p < nparts && same; p++) same = dicts[(size_t)p] == dicts[0];
    std::vector<std::string> m;
    if (same) {
        m = dicts[0];
    } else {
        std::vector<const std::vector<std::string> *> ptrs;
        for (auto &d : dicts) ptrs.push_back(&d);
        m = ph::merge_dicts(ptrs);
    }
    *identical = same ? 1 : 0;
    *nmerged = (int32_t)m.size();
    int64_t bytes = 0;
    for (auto &s : m) bytes += (int64_t)s.size() + 1;
    *merged_bytes = bytes;
    memset(remap, 0, (size_t)nparts * 256);
    if (m.size() <= 256)   // (beyond that a code cannot name the entry: the column becomes PH_STR, and the tables stay 0)
        for (int32_t p = 0; p < nparts; p++) {
            if (same) for (size_t c = 0; c < m.size(); c++) remap[(size_t)p * 256 + c] = (uint8_t)c;
            else ph::remap_of(dicts[(size_t)p], m, remap + (size_t)p * 256);
        }
    if (bytes > merged_cap) {
        ph::set_error("ph_dict_merge_host: the merged dictionary needs %lld bytes, the buffer has %lld", (long long)bytes, (long long)merged_cap);
        return PH_ECAPACITY;
    }
    char *w = merged;
    for (auto &s : m) {
        memcpy(w, s.c_str(), s.size() + 1);
        w += s.size() + 1;
    }
    return PH_OK;
}

// ---------------------------------------------------------------- the call

namespace {

// what the host decides about one result column before anything is allocated, and where its arrays lie in the uploaded device table
struct ColPlan {
    int32_t type = 0, scale = 0;
    bool validity = false;   // some part has a bitmap
    bool remap = false;      // PH_CODE8 from different dictionaries: codes go through tables
    bool strings = false;    // PH_STR
    std::vector<std::string> dict;                          // PH_CODE8: the result's dictionary
    std::vector<const std::vector<std::string> *> uniq;     // the distinct dictionaries of the code parts
    std::vector<int32_t> tab;                               // per part with rows: its dictionary in uniq, -1 for a PH_STR part
    int64_t src = 0, val = 0, aux = 0, tabs = 0, remaps = 0, dlen = 0, dpos = 0, blob = 0;   // byte positions in the device table
};

struct MetaBuilder {
    std::vector<char> bytes;
    int64_t reserve(int64_t n) {
        const int64_t at = ph::round_up((int64_t)bytes.size(), 16);
        bytes.resize((size_t)(at + n), 0);
        return at;
    }
    template <class T> T *at(int64_t pos) { return (T *)(bytes.data() + pos); }
};

bool is_varchar(int32_t t) { return t == PH_CODE8 || t == PH_STR; }

}  // namespace

extern "C" int ph_table_concat(ph_ctx *ctx, const ph_table *const *parts, int32_t nparts, ph_table **out) {
    PH_REQUIRE(ctx && parts && out, "ph_table_concat: bad arguments");
    PH_REQUIRE(nparts >= 1 && nparts <= 65536, "ph_table_concat: %d parts (1..65536)", nparts);
    int64_t nrows = 0;
    for (int32_t p = 0; p < nparts; p++) {
        PH_REQUIRE(parts[p] != nullptr, "ph_table_concat: part %d is NULL", p);
        PH_REQUIRE(parts[p]->ctx && parts[p]->ctx->device == ctx->device, "ph_table_concat: part %d lives on another device than the context", p);
        nrows += parts[p]->nrows;
    }
    PH_REQUIRE(nrows < (1ll << 31), "ph_table_concat: %lld rows exceed the int32 row-id domain", (long long)nrows);
    const int32_t ncols = (int32_t)parts[0]->cols.size();
    PH_REQUIRE(ncols > 0, "ph_table_concat: part 0 has no columns");
    for (int32_t p = 1; p < nparts; p++)
        PH_REQUIRE((int32_t)parts[p]->cols.size() == ncols, "ph_table_concat: part %d has %d columns, part 0 has %d", p, (int)parts[p]->cols.size(), ncols);

    // ---- the parts that have rows, and their first output rows
    std::vector<const ph_table *> live;
    for (int32_t p = 0; p < nparts; p++)
        if (parts[p]->nrows > 0) live.push_back(parts[p]);
    const int32_t np = (int32_t)live.size();
    std::vector<int32_t> starts((size_t)np + 1, 0);
    for (int32_t p = 0; p < np; p++) starts[(size_t)p + 1] = (int32_t)((int64_t)starts[(size_t)p] + live[(size_t)p]->nrows);

    // ---- per column: the schema rules, the result's type and dictionary (host only)
    std::vector<ColPlan> plan((size_t)ncols);
    MetaBuilder meta;
    const int64_t starts_at = meta.reserve(((int64_t)np + 1) * 4);
    memcpy(meta.at<int32_t>(starts_at), starts.data(), ((size_t)np + 1) * 4);
    for (int32_t c = 0; c < ncols; c++) {
        ColPlan &C = plan[(size_t)c];
        const ph_table::column &first = parts[0]->cols[(size_t)c];
        bool any_str = false;
        for (int32_t p = 0; p < nparts; p++) {
            const ph_table::column &s = parts[p]->cols[(size_t)c];
            const bool same = s.type == first.type || (is_varchar(s.type) && is_varchar(first.type));
            PH_REQUIRE(same, "ph_table_concat: column %d: part %d has type %d, part 0 has type %d", c, p, s.type, first.type);
            PH_REQUIRE(s.scale == first.scale, "ph_table_concat: column %d: part %d has scale %d, part 0 has scale %d", c, p, s.scale, first.scale);
            C.validity = C.validity || s.validity != nullptr;
            any_str = any_str || s.type == PH_STR;
        }
        C.type = first.type;
        C.scale = first.scale;
        PH_REQUIRE(is_varchar(C.type) || ph::type_width(C.type) > 0, "ph_table_concat: column %d has unknown type %d", c, C.type);
        if (is_varchar(C.type)) {
            std::map<std::vector<std::string>, int32_t> seen;   // a dictionary that many parts share is merged, and uploaded, once
            auto dict_id = [&](const ph_table::column &s) {
                auto it = seen.find(s.dict);
                if (it != seen.end()) return it->second;
                const int32_t id = (int32_t)C.uniq.size();
                C.uniq.push_back(&s.dict);
                seen.emplace(s.dict, id);
                return id;
            };
            for (int32_t p = 0; p < nparts; p++)   // (a part of 0 rows contributes no rows, but its entries: the union is over the parts)
                if (parts[p]->cols[(size_t)c].type == PH_CODE8 && parts[p]->nrows == 0) dict_id(parts[p]->cols[(size_t)c]);
            C.tab.resize((size_t)np);
            for (int32_t p = 0; p < np; p++) {
                const ph_table::column &s = live[(size_t)p]->cols[(size_t)c];
                C.tab[(size_t)p] = s.type == PH_CODE8 ? dict_id(s) : -1;
            }
            if (!any_str && C.uniq.size() == 1) {   // the same entries in the same order everywhere: kept as they are, codes copied
                C.type = PH_CODE8;
                C.dict = *C.uniq[0];
            } else {
                std::vector<std::string> merged = any_str ? std::vector<std::string>() : ph::merge_dicts(C.uniq);
                if (!any_str && merged.size() <= 256) {
                    C.type = PH_CODE8;
                    C.remap = true;
                    C.dict = std::move(merged);
                } else {
                    C.type = PH_STR;
                    C.strings = true;
                }
            }
        }
        // the column's share of the device table
        C.src = meta.reserve((int64_t)np * 8);
        for (int32_t p = 0; p < np; p++) meta.at<const void *>(C.src)[p] = live[(size_t)p]->cols[(size_t)c].data;
        if (C.validity) {
            C.val = meta.reserve((int64_t)np * 8);
            for (int32_t p = 0; p < np; p++) meta.at<const uint8_t *>(C.val)[p] = live[(size_t)p]->cols[(size_t)c].validity;
        }
        if (C.remap || C.strings) {
            C.tabs = meta.reserve((int64_t)np * 4);
            if (np) memcpy(meta.at<int32_t>(C.tabs), C.tab.data(), (size_t)np * 4);
        }
        if (C.remap) {
            C.remaps = meta.reserve((int64_t)C.uniq.size() * 256);
            for (size_t u = 0; u < C.uniq.size(); u++) ph::remap_of(*C.uniq[u], C.dict, meta.at<uint8_t>(C.remaps) + u * 256);
        }
        if (C.strings) {
            C.aux = meta.reserve((int64_t)np * 8);
            for (int32_t p = 0; p < np; p++) meta.at<const void *>(C.aux)[p] = live[(size_t)p]->cols[(size_t)c].aux;
            const int64_t nu = (int64_t)C.uniq.size();
            C.dlen = meta.reserve(nu * 256 * 4);
            C.dpos = meta.reserve(nu * 256 * 8);
            int64_t blob_bytes = 0;
            for (const auto *d : C.uniq) for (size_t k = 0; k < d->size() && k < 256; k++) blob_bytes += (int64_t)(*d)[k].size();
            C.blob = meta.reserve(blob_bytes + 1);
            int64_t at = 0;
            for (int64_t u = 0; u < nu; u++) {
                const auto &d = *C.uniq[(size_t)u];
                for (size_t k = 0; k < d.size() && k < 256; k++) {
                    meta.at<int32_t>(C.dlen)[u * 256 + (int64_t)k] = (int32_t)d[k].size();
                    meta.at<int64_t>(C.dpos)[u * 256 + (int64_t)k] = at;
                    memcpy(meta.at<char>(C.blob) + at, d[k].data(), d[k].size());
                    at += (int64_t)d[k].size();
                }
            }
        }
    }

    // ---- the device table, one upload for the call
    PH_HIP(hipSetDevice(ctx->device));
    Temps tmp;
    tmp.who = "ph_table_concat";
    char *meta_dev = nullptr;
    PH_CHECK(tmp.alloc((void **)&meta_dev, (int64_t)meta.bytes.size()));
    PH_CHECK(ph_dev_upload(ctx, meta_dev, meta.bytes.data(), (int64_t)meta.bytes.size()));
    unsigned long long *str_bytes_dev = nullptr;   // one byte total per VARCHAR column, then the scan's total
    PH_CHECK(tmp.alloc((void **)&str_bytes_dev, ((int64_t)ncols + 1) * 8));
    PH_HIP(hipMemsetAsync(str_bytes_dev, 0, ((size_t)ncols + 1) * 8, ctx->stream));
    int64_t *scan_total_dev = (int64_t *)(str_bytes_dev + ncols);

    TableGuard guard;
    ph_table *t = guard.t = new ph_table();
    t->ctx = ctx;
    t->nrows = nrows;
    t->cols.resize((size_t)ncols);
    const int64_t padded = ph::round_up(nrows > 0 ? nrows : 1, PH_ROW_PAD);
    auto no_memory = [&](int c) { (void)hipGetLastError(); ph::set_error("ph_table_concat: no device memory for column %d", c); return PH_EHIP; };
    for (int32_t c = 0; c < ncols; c++) {
        const ColPlan &C = plan[(size_t)c];
        ph_table::column &d = t->cols[(size_t)c];
        d.type = C.type;
        d.scale = C.scale;
        d.dict = C.dict;
        cc::Parts P{(const int32_t *)(meta_dev + starts_at), (const void *const *)(meta_dev + C.src),
                          C.validity ? (const uint8_t *const *)(meta_dev + C.val) : nullptr, np, (int32_t)nrows};
        if (C.validity) {
            if (hipMalloc((void **)&d.validity, (size_t)(padded / 8)) != hipSuccess) return no_memory(c);
            const int64_t nwords = padded / 32;
            ph::concat_validity_kernel<<<(unsigned)((nwords + 255) / 256), 256, 0, ctx->stream>>>(P, (uint32_t *)d.validity, nwords);
            PH_HIP(hipGetLastError());
        }
        if (!C.strings) {
            const int w = ph::type_width(C.type);
            if (hipMalloc(&d.data, (size_t)(padded * w)) != hipSuccess) return no_memory(c);
            const int64_t nunits = padded * w / 16;
            const unsigned grid = (unsigned)((nunits + ph::CONCAT_TILE_UNITS - 1) / ph::CONCAT_TILE_UNITS);
            if (C.remap)
                ph::concat_fixed_kernel<1, true><<<grid, 256, 0, ctx->stream>>>(P, (const uint8_t *)(meta_dev + C.remaps), (const int32_t *)(meta_dev + C.tabs), (uint4 *)d.data, nunits);
            else
                ph::dispatch_int<1, 4, 8>(w, [&](auto W) { ph::concat_fixed_kernel<W(), false><<<grid, 256, 0, ctx->stream>>>(P, nullptr, nullptr, (uint4 *)d.data, nunits); });
            PH_HIP(hipGetLastError());
            continue;
        }
        // VARCHAR: lengths, the byte total (the column's one read-back), offsets by the context's scan, bytes
        if (hipMalloc(&d.data, (size_t)((padded + 1) * 4)) != hipSuccess) return no_memory(c);
        PH_HIP(hipMemsetAsync(d.data, 0, (size_t)((padded + 1) * 4), ctx->stream));
        int64_t *sbegin = nullptr;
        if (nrows > 0) {
            PH_CHECK(tmp.alloc((void **)&sbegin, nrows * 8));
            ph::concat_str_lengths_kernel<<<(unsigned)((nrows + 255) / 256), 256, 0, ctx->stream>>>(
                P, (const unsigned char *const *)(meta_dev + C.aux), (const int32_t *)(meta_dev + C.tabs), (const int32_t *)(meta_dev + C.dlen),
                (const int64_t *)(meta_dev + C.dpos), (const unsigned char *)(meta_dev + C.blob), (int32_t *)d.data, sbegin);
            PH_HIP(hipGetLastError());
            ph::sum_lengths_kernel<<<ph::load_grid_for(ctx, nrows), 256, 0, ctx->stream>>>((const int32_t *)d.data, nrows, str_bytes_dev + c);
            PH_HIP(hipGetLastError());
        }
        unsigned long long str_bytes = 0;
        PH_CHECK(ctx->download(&str_bytes, str_bytes_dev + c, 8));
        PH_REQUIRE(str_bytes < (1ull << 31), "ph_table_concat: column %d holds %llu string bytes (int32 offsets)", c, str_bytes);
        d.aux_bytes = (int64_t)str_bytes;
        if (hipMalloc(&d.aux, (size_t)(d.aux_bytes + 64)) != hipSuccess) return no_memory(c);
        if (nrows > 0) {
            PH_CHECK(ph::exclusive_scan_i32(ctx, (int32_t *)d.data, nrows + 1, scan_total_dev));
            ph::copy_strings_kernel<false><<<(unsigned)((nrows + 255) / 256), 256, 0, ctx->stream>>>(
                (const unsigned char *)(meta_dev + C.blob), sbegin, (const int32_t *)d.data, nrows, (unsigned char *)d.aux);
            PH_HIP(hipGetLastError());
        }
    }

    // ---- the temporaries go (the kernels that read them have run); the shared finishing
    PH_HIP(hipStreamSynchronize(ctx->stream));
    tmp.release();
    for (int32_t c = 0; c < ncols; c++) PH_CHECK(ph::table_finish_column(ctx, t->cols[(size_t)c], nrows, padded, nullptr, 0));
    ph::register_table(t);
    guard.t = nullptr;
    *out = t;
    return PH_OK;
}
