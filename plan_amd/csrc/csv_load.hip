// ph_table_create_csv / ph_table_create_csv_ex: delimited text (dbgen .tbl, CSV with encoding/csv's quoted fields under PH_CSV_QUOTES) ->
// resident table, parsed on the device (see planhip.h).
//
// The reference's text scan (COPY FROM ... (format csv, delimiter '|'): readCsvTable + fieldToValue, pkg/compute/executor_scan.go:107-120,
// 311-408; Vector.SetValue, pkg/chunk/vector.go:195-264) converts ONE value at a time into 24-byte decimals and 12-byte dates. Here the
// text is uploaded once and three passes over it build the columns in their device encodings (DESIGN.md "Text load"):
//   1. csv_rows_kernel   — per 32 KiB tile: count the record starts (flags 0: and look for '"'; PH_CSV_QUOTES: for both parities of the
//                          quotes before the tile, next to the tile's quote count, whose scan picks one), the context's exclusive scan over
//                          the tile counts, then the same kernel again writes every record's int64 start offset;
//   2. csv_fields_kernel — a workgroup stages its tile in LDS with 16-byte loads and walks the records that START in the tile out of
//                          LDS (only the tail of a record that leaves the tile is read from global memory) with csv_parse.h's walk_field,
//                          under PH_CSV_QUOTES never past the next record's start: fixed-width values, validity bits, NULL counts, field
//                          counts, VARCHAR begin / length; the lowest failing (row, column, cause) by atomicMin;
//   3. VARCHAR           — lengths scanned into int32 offsets, bytes copied one output byte per lane (rows with "" or "\r\n" inside
//                          quotes once more by csv_copy_escaped_kernel), distinct strings counted by interning (ph_strdict_build);
//                          <= 256 of them -> PH_CODE8 + dictionary in byte order (csv_remap_kernel).
// Every column is then finished by ph::table_finish_column, exactly as ph_table_create finishes an uploaded one.
#include <algorithm>
#include <numeric>

#include "common.h"
#include "csv_parse.h"
#include "ops.h"
#include "str_encode.h"

namespace ph {

constexpr int CSV_TILE = 32768;                    // bytes of text per workgroup (rows kernel: 8 x 16 bytes a thread; fields kernel: the LDS tile):
                                                   // about one lineitem record (~125 bytes) per thread of the fields kernel
constexpr int CSV_THREADS = 256;                   // rows kernel
constexpr int CSV_FIELD_THREADS = 512;             // fields kernel: a tile of ~125-byte records holds about 260, one round of the record loop
constexpr int CSV_PIECES = CSV_TILE / 16;          // 16-byte pieces of a tile
constexpr int CSV_PER = CSV_PIECES / CSV_THREADS;  // pieces per thread
constexpr int CSV_PAD = 16;                        // '\n' bytes in front of the text and (at least) behind it

// The text on the device is [16 x '\n'][text][ '\n' up to a multiple of CSV_TILE, at least one ][16 x '\n']: every record ends in '\n' (a final
// record without one, and a lone '\r' at the end of input, become ordinary lines), position -1 reads as a line end, and 16-byte loads of
// whole tiles stay inside the allocation.
//
// A position p starts a record when it follows a '\n' and the line beginning there is not empty ("\n" or "\r\n": encoding/csv skips those).
__device__ __forceinline__ bool record_start(unsigned prev, unsigned c, unsigned next) {
    return prev == '\n' && c != '\n' && !(c == '\r' && next == '\n');
}

// exclusive prefix over the tile's pieces of the per-piece counts in s_cnt (written, and a barrier passed, by the caller): thread t owns
// pieces CSV_PER t .. CSV_PER t + CSV_PER - 1. c4: its pieces' counts, mine: their sum, off: the count before its first piece.
__device__ __forceinline__ void tile_prefix(const unsigned short *s_cnt, int *s_wave, int (&c4)[CSV_PER], int &off, int &mine) {
    mine = 0;
#pragma unroll
    for (int q = 0; q < CSV_PER; q++) { c4[q] = s_cnt[threadIdx.x * CSV_PER + q]; mine += c4[q]; }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    if (lane == 63) s_wave[wv] = incl;
    __syncthreads();
    off = incl - mine;
    for (int k = 0; k < wv; k++) off += s_wave[k];
}

// QUOTES (PH_CSV_QUOTES): a '\n' inside a quoted field is data. In a text that is well-formed up to a position, "inside a quoted field" there
// equals "an odd number of '"' bytes before it" (every '"' is an opener, a closer or half of a "" pair), so a position starts a record when
// record_start holds AND the quotes before it are even in number. Within a tile that parity is a prefix XOR: inside a 16-byte piece by the
// shift-XOR cascade over the piece's quote bitmask, across pieces as the low bit of the same prefix sum (wave shuffle + LDS step) that places
// the starts. The tile's own incoming parity is not known while the tiles are counted: the counting pass counts the starts for BOTH incoming
// parities in its one pass over the text (tile_rows: even, tile_rows_odd: odd) next to the tile's quote count; the low bit of the exclusive
// scan of the quote counts then picks one (csv_pick_rows_kernel), and the WRITE pass reads the same bit. With QUOTES = false none of this is
// compiled in.
template <bool WRITE, bool QUOTES>
__global__ __launch_bounds__(CSV_THREADS) void csv_rows_kernel(const unsigned char *__restrict__ text, int32_t *__restrict__ tile_rows,
                                                               int64_t *__restrict__ starts, unsigned *__restrict__ quote_flag,
                                                               int32_t *__restrict__ tile_quotes, int32_t *__restrict__ tile_rows_odd) {
    __shared__ unsigned short s_cnt[CSV_PIECES];   // record starts per 16-byte piece, then their exclusive prefix within the tile
    __shared__ int s_wave[(QUOTES ? 2 : 1) * (CSV_THREADS / 64)];
    const int64_t base = (int64_t)blockIdx.x * CSV_TILE;
    unsigned mask[CSV_PER], qmask[QUOTES ? CSV_PER : 1];
    bool quote = false;
#pragma unroll
    for (int k = 0; k < CSV_PER; k++) {
        const int piece = k * CSV_THREADS + threadIdx.x;     // lane i of a wave loads bytes 16 i .. 16 i + 15: 1 KiB per wave instruction
        const int64_t pos = base + (int64_t)piece * 16;
        const uint4 v = *reinterpret_cast<const uint4 *>(text + pos);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
        unsigned prev = text[pos - 1];
        const unsigned last_next = text[pos + 16];
        unsigned m = 0, qm = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const unsigned c = (w[j >> 2] >> ((j & 3) * 8)) & 0xffu;
            const unsigned next = j < 15 ? (w[(j + 1) >> 2] >> (((j + 1) & 3) * 8)) & 0xffu : last_next;
            if constexpr (QUOTES) qm |= (c == '"' ? 1u : 0u) << j;
            else quote |= c == '"';
            m |= (record_start(prev, c, next) ? 1u : 0u) << j;
            prev = c;
        }
        mask[k] = m;
        if constexpr (QUOTES) { qmask[k] = qm; s_cnt[piece] = (unsigned short)__popc(qm); }
        else s_cnt[piece] = (unsigned short)__popc(m);
    }
    if (!QUOTES && !WRITE && quote) atomicOr(quote_flag, 1u);
    __syncthreads();
    int c4[CSV_PER], mine, off;
    if constexpr (QUOTES) {
        tile_prefix(s_cnt, s_wave, c4, off, mine);          // the quotes before every piece of the tile
        if (!WRITE && threadIdx.x == CSV_THREADS - 1) tile_quotes[blockIdx.x] = off + mine;
#pragma unroll
        for (int q = 0; q < CSV_PER; q++) { s_cnt[threadIdx.x * CSV_PER + q] = (unsigned short)off; off += c4[q]; }
        __syncthreads();
        const unsigned tile_odd = WRITE ? (unsigned)tile_quotes[blockIdx.x] & 1u : 0u;   // scanned: the quotes before this tile
        int odd_starts = 0;
#pragma unroll
        for (int k = 0; k < CSV_PER; k++) {
            unsigned x = qmask[k];
            x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8;      // bit j: the parity of the piece's quotes in bytes 0 .. j
            unsigned inside = (x << 1) & 0xffffu;                    // bit j: an odd number of quotes in the piece before byte j
            if ((s_cnt[k * CSV_THREADS + threadIdx.x] ^ tile_odd) & 1u) inside ^= 0xffffu;
            if (!WRITE) odd_starts += __popc(mask[k] & inside);      // the starts if the tile begins inside a quoted field
            mask[k] &= ~inside;
        }
        __syncthreads();                                             // (every thread has read its pieces' prefixes)
#pragma unroll
        for (int k = 0; k < CSV_PER; k++) s_cnt[k * CSV_THREADS + threadIdx.x] = (unsigned short)__popc(mask[k]);
        if (!WRITE) {
            for (int o = 32; o > 0; o >>= 1) odd_starts += __shfl_xor(odd_starts, o);
            if ((threadIdx.x & 63) == 0) s_wave[CSV_THREADS / 64 + (threadIdx.x >> 6)] = odd_starts;
        }
        __syncthreads();
    }
    tile_prefix(s_cnt, s_wave, c4, off, mine);
    if (!WRITE) {
        if (threadIdx.x == CSV_THREADS - 1) {
            tile_rows[blockIdx.x] = off + mine;
            if constexpr (QUOTES) {
                int odd = 0;
                for (int k = 0; k < CSV_THREADS / 64; k++) odd += s_wave[CSV_THREADS / 64 + k];
                tile_rows_odd[blockIdx.x] = odd;
            }
        }
        return;
    }
#pragma unroll
    for (int q = 0; q < CSV_PER; q++) { s_cnt[threadIdx.x * CSV_PER + q] = (unsigned short)off; off += c4[q]; }
    __syncthreads();
    const int64_t row0 = tile_rows[blockIdx.x];   // scanned: the first record that starts in this tile
#pragma unroll
    for (int k = 0; k < CSV_PER; k++) {
        const int piece = k * CSV_THREADS + threadIdx.x;
        int64_t r = row0 + s_cnt[piece];
        for (unsigned m = mask[k]; m; m &= m - 1) starts[r++] = base + (int64_t)piece * 16 + (__ffs(m) - 1);
    }
}

// PH_CSV_QUOTES: a tile that begins inside a quoted field (an odd number of quotes before it) takes its other start count
__global__ __launch_bounds__(256) void csv_pick_rows_kernel(const int32_t *__restrict__ tile_quotes, const int32_t *__restrict__ tile_rows_odd,
                                                            int32_t *__restrict__ tile_rows, int64_t ntiles) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < ntiles && (tile_quotes[i] & 1)) tile_rows[i] = tile_rows_odd[i];
}

// one requested column, as the fields kernel sees it; the array is sorted by field so that a record is walked once
struct CsvColDev {
    int32_t field, type, scale, orig;   // orig: the column's index in the caller's list (error order, NULL counters)
    void *data;                         // fixed width: the values; PH_STR: int32 lengths (scanned into offsets afterwards)
    unsigned *validity;                 // all ones on entry; a NULL clears its bit (and sets the column's flag)
    int64_t *sbegin;                    // PH_STR: where the field's bytes begin in the text
};

// bytes of the text for a workgroup whose tile [base, end) sits in LDS: the tail of a record that leaves the tile comes from global memory
struct TileBytes {
    const unsigned char *lds, *text;
    int64_t base, end;
    __device__ __forceinline__ unsigned char operator()(int64_t p) const { return p < end ? lds[p - base] : text[p]; }
};

// the error key: the lowest wins. Within a row a quoting error (col1 = 0, bit 31 clear) sorts below everything else, as encoding/csv returns
// its parse error before it compares field counts and before any value is looked at; then the field-count check (col1 = 0), then the columns
constexpr unsigned long long CSV_ERR_NOT_QUOTE = 1ull << 31;
__device__ __forceinline__ void csv_report(unsigned long long *err, int64_t row, int col1, int cause) {
    atomicMin(err, ((unsigned long long)row << 32) | CSV_ERR_NOT_QUOTE | ((unsigned long long)(unsigned)col1 << 8) | (unsigned)cause);
}

// QUOTES: row r is walked from starts[r] and no byte at or past starts[r + 1] (the last row: text_end, the end of the padded text) is read.
// Up to the first malformed record the parity of csv_rows_kernel IS the state of encoding/csv, so every earlier row and that row's own start
// are exact and its thread meets the error where Go does; rows behind it may be cut anywhere and report anything, under a higher row number
// that atomicMin drops. The bound keeps the work of a malformed text at one walk over the text in all.
// A quoted fixed-width field is parsed over the RAW bytes between its quotes: an escape leaves a '"' or a '\r' there, which the value
// parsers refuse with the cause the unescaped byte ('"' or '\n') would get at the same place, and everything before it is the same bytes.
template <bool QUOTES>
__global__ __launch_bounds__(CSV_FIELD_THREADS) void csv_fields_kernel(const unsigned char *__restrict__ text, const int32_t *__restrict__ tile_rows,
                                                                 const int64_t *__restrict__ starts, const CsvColDev *__restrict__ cols, int ncols,
                                                                 int delim, int nfields0, unsigned long long *__restrict__ err,
                                                                 unsigned *__restrict__ nulls, unsigned *__restrict__ escapes, int64_t nrows,
                                                                 int64_t text_end) {
    __shared__ __attribute__((aligned(16))) unsigned char s_text[CSV_TILE];
    const int64_t r0 = tile_rows[blockIdx.x], r1 = tile_rows[blockIdx.x + 1];
    if (r0 == r1) return;                                   // (the whole workgroup: no record starts here, e.g. inside a long record)
    const int64_t base = (int64_t)blockIdx.x * CSV_TILE;
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(text + base);
        uint4 *dst = reinterpret_cast<uint4 *>(s_text);
        for (int i = threadIdx.x; i < CSV_PIECES; i += CSV_FIELD_THREADS) dst[i] = src[i];
    }
    __syncthreads();
    const TileBytes g{s_text, text, base, base + CSV_TILE};
    for (int64_t row = r0 + threadIdx.x; row < r1; row += CSV_FIELD_THREADS) {
        const int64_t p = starts[row];
        int64_t lim = 0;
        if constexpr (QUOTES) lim = row + 1 < nrows ? starts[row + 1] : text_end;
        int f = 0, k = 0, walk = csv::C_OK;
        int64_t q = p;
        for (;;) {
            csv::Field F;
            int64_t next;
            walk = csv::walk_field<QUOTES>(g, (unsigned)delim, q, lim, &F, &next);
            if (QUOTES && walk != csv::C_OK) break;
            const int64_t fb = F.b, fe = F.e;
            for (; k < ncols && cols[k].field == f; k++) {
                const CsvColDev &C = cols[k];
                if (C.type == PH_STR) {
                    const int64_t len = QUOTES ? fe - fb - F.drop : fe - fb;      // the unescaped length
                    C.sbegin[row] = QUOTES && F.drop ? fb | INT64_MIN : fb;       // the sign bit marks a row that csv_copy_escaped_kernel copies
                    if (QUOTES && F.drop) escapes[C.orig] = 1u;
                    ((int32_t *)C.data)[row] = (int32_t)(len > INT32_MAX ? INT32_MAX : len);
                    continue;
                }
                int64_t v = 0;
                int is_null = 0;
                const int cause = csv::parse_field(C.type, C.scale, g, fb, fe, &v, &is_null);
                if (cause != csv::C_OK) { csv_report(err, row, C.orig + 1, cause); v = 0; }
                if (is_null) {
                    atomicAnd(&C.validity[row >> 5], ~(1u << (row & 31)));
                    nulls[C.orig] = 1u;   // a flag (the host only asks whether the column has a NULL): a plain store, no contended counter
                }
                if (C.type == PH_I32 || C.type == PH_DATE) ((int32_t *)C.data)[row] = (int32_t)v;
                else ((int64_t *)C.data)[row] = v;
            }
            f++;
            q = next;
            if (F.last) break;
        }
        if constexpr (QUOTES) {
            // what lies between the record's line end and the next record's start is empty lines only (always so behind a true start)
            for (; walk == csv::C_OK && q < lim; q++)
                if (!csv::empty_line(g, q, lim)) walk = csv::C_QUOTE;
            if (walk != csv::C_OK) {
                atomicMin(err, ((unsigned long long)row << 32) | (unsigned)walk);
                continue;
            }
        }
        if (f != nfields0) csv_report(err, row, 0, csv::C_FIELD_COUNT);
        for (; k < ncols; k++) csv_report(err, row, cols[k].orig + 1, csv::C_NO_FIELD);
    }
}

// PH_CSV_QUOTES, a VARCHAR column that has a field with "" or "\r\n" inside its quotes: one thread per marked row walks the field's content
// and writes its unescaped bytes (the second '"' of a pair and the '\r' of a pair dropped; the walker has checked the content, whose every
// '"' begins a pair). Such rows are few and short in what real exporters write; the other rows keep the coalesced copy above.
__global__ __launch_bounds__(256) void csv_copy_escaped_kernel(const unsigned char *__restrict__ text, const int64_t *__restrict__ sbegin,
                                                               const int32_t *__restrict__ off, int64_t n, unsigned char *__restrict__ out) {
    for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < n; row += (int64_t)gridDim.x * 256) {
        const int64_t b = sbegin[row];
        if (b >= 0) continue;
        const unsigned char *src = text + (b & INT64_MAX);
        const int64_t end = off[row + 1];
        for (int64_t o = off[row]; o < end; o++) {
            const unsigned char c = *src;
            const bool pair = c == '"' || (c == '\r' && src[1] == '\n');
            out[o] = c == '\r' && pair ? (unsigned char)'\n' : c;
            src += pair ? 2 : 1;
        }
    }
}

// interning codes -> the representatives (rows whose code is their own row id): their number, and the first 256 of them
// skip_empty (a column with NULL rows none of whose valid rows is the empty string): the empty string's group is the NULL rows alone and
// is no distinct value, so its representative is left out
__global__ __launch_bounds__(256) void csv_reps_kernel(const int32_t *__restrict__ codes, int64_t n, unsigned *__restrict__ count, int32_t *__restrict__ reps,
                                                       const int32_t *__restrict__ off, int skip_empty) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (codes[i] != (int32_t)i) continue;
        if (skip_empty && off[i + 1] == off[i]) continue;
        const unsigned at = atomicAdd(count, 1u);
        if (at < 256u) reps[at] = (int32_t)i;
    }
}

// does a VALID row hold the empty string? (flag[1]; the rows are NULL where the bitmap's bit is clear)
__global__ __launch_bounds__(256) void csv_valid_empty_kernel(const int32_t *__restrict__ off, const uint8_t *__restrict__ validity, int64_t n, unsigned *__restrict__ flag) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        if (off[i + 1] == off[i] && ((validity[i >> 3] >> (i & 7)) & 1)) flag[1] = 1u;
}

__global__ __launch_bounds__(256) void csv_rep_lengths_kernel(const int32_t *__restrict__ off, const int32_t *__restrict__ reps, int nd, int32_t *__restrict__ len) {
    if ((int)threadIdx.x < nd) len[threadIdx.x] = off[reps[threadIdx.x] + 1] - off[reps[threadIdx.x]];
}

// representative row id -> dictionary code: reps ascending, rank[i] = the code of reps[i]
__global__ __launch_bounds__(256) void csv_remap_kernel(const int32_t *__restrict__ codes, int64_t n, const int32_t *__restrict__ reps,
                                                        const uint8_t *__restrict__ rank, int nd, uint8_t *__restrict__ out,
                                                        const uint8_t *__restrict__ validity) {
    __shared__ int32_t s_rep[256];
    __shared__ uint8_t s_rank[256];
    if ((int)threadIdx.x < nd) { s_rep[threadIdx.x] = reps[threadIdx.x]; s_rank[threadIdx.x] = rank[threadIdx.x]; }
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (validity && !((validity[i >> 3] >> (i & 7)) & 1)) { out[i] = 0; continue; }   // a NULL row's code is 0
        const int32_t c = codes[i];
        int a = 0, b = nd;                                  // s_rep[a] <= c (c IS one of them)
        while (b - a > 1) {
            const int m = (a + b) >> 1;
            if (s_rep[m] <= c) a = m; else b = m;
        }
        out[i] = s_rank[a];
    }
}

}  // namespace ph

namespace {

struct HostBytes {
    const char *s;
    unsigned char operator()(int64_t p) const { return (unsigned char)s[p]; }
};

// control block of a call on the device: what the kernels report and the host reads back in one copy
struct CsvControl {
    unsigned long long err;        // lowest (row << 32 | not a quoting error << 31 | column + 1 << 8 | cause), see csv_report; all ones = none
    unsigned long long scan_total; // the scans' totals (their int32 domain: the 64-bit sums below are what the host trusts)
    unsigned long long rows;       // 64-bit sum of the tiles' record counts
    unsigned quote, distinct;
    unsigned long long str_bytes[1];   // per requested column, then unsigned nulls[ncols], then unsigned escapes[ncols]
};

using ph::Temps;
using ph::TableGuard;
int grid_for(ph_ctx *ctx, int64_t n) { return ph::load_grid_for(ctx, n); }

// the host's text as the kernels see theirs: behind the input every byte reads as '\n'
struct HostText {
    const char *s;
    int64_t n;
    unsigned char operator()(int64_t p) const { return p < n ? (unsigned char)s[p] : (unsigned char)'\n'; }
};

// one record from `pos` on with the kernel's walker (empty lines skipped first): calls on_field(index, Field) per field.
// *nfields = fields walked, *next = behind the record's line end (at most n). Returns the walker's cause.
template <bool QUOTES, class F>
int host_walk_record(const char *s, int64_t n, int delim, int64_t pos, int32_t *nfields, int64_t *next, F on_field) {
    const HostText g{s, n};
    const int64_t lim = n + 1;
    *nfields = 0;
    for (int e; pos < n && (e = ph::csv::empty_line(g, pos, lim)) != 0;) pos += e;
    *next = std::min(pos, n);
    if (pos >= n) return ph::csv::C_OK;
    for (;;) {
        ph::csv::Field fld;
        int64_t nx = pos;
        const int cause = ph::csv::walk_field<QUOTES>(g, (unsigned)delim, pos, lim, &fld, &nx);
        if (cause != ph::csv::C_OK) return cause;
        on_field(*nfields, fld);
        ++*nfields;
        pos = nx;
        *next = std::min(pos, n);
        if (fld.last) return ph::csv::C_OK;
    }
}

// field count of the first record (the host reads a few hundred bytes of the text it still holds), under the grammar of the load
int first_record_fields(const char *s, int64_t n, int delim, bool quotes) {
    int32_t nf = 0;
    int64_t next = 0;
    auto none = [](int32_t, const ph::csv::Field &) {};
    if (quotes) (void)host_walk_record<true>(s, n, delim, 0, &nf, &next, none);   // (a quoting error in row 0 is the fields kernel's to report)
    else (void)host_walk_record<false>(s, n, delim, 0, &nf, &next, none);
    return nf;
}

}  // namespace

// a VARCHAR column whose offsets (d.data) and bytes (d.aux) are in place: <= 256 distinct strings -> PH_CODE8 + dictionary in byte order
// (str_encode.h; shared with the Parquet load path, whose columns may hold NULL rows)
int ph::encode_strings(ph_ctx *ctx, ph_table::column &d, int64_t nrows, int64_t padded, unsigned *count_dev, Temps &tmp, const uint8_t *validity) {
    if (nrows >= (1ll << 30)) return PH_OK;   // beyond the interning primitive's domain: stays PH_STR
    int32_t *codes = nullptr, *reps = nullptr, *lens = nullptr;
    const int64_t head = 65536;
    PH_CHECK(tmp.alloc((void **)&codes, std::min(nrows, head) * 4));
    PH_CHECK(tmp.alloc((void **)&reps, 256 * 4));
    PH_CHECK(tmp.alloc((void **)&lens, 256 * 4));
    ph_col v{};
    v.type = PH_STR; v.data = d.data; v.aux = d.aux; v.aux_bytes = d.aux_bytes;
    unsigned nd = 0;
    int skip_empty = 0;
    if (validity) {   // the NULL rows' empty string counts only when a valid row holds it too
        unsigned flag[2] = {0, 0};
        PH_HIP(hipMemsetAsync(count_dev, 0, 8, ctx->stream));
        ph::csv_valid_empty_kernel<<<grid_for(ctx, nrows), 256, 0, ctx->stream>>>((const int32_t *)d.data, validity, nrows, count_dev);
        PH_HIP(hipGetLastError());
        PH_CHECK(ctx->download(flag, count_dev, 8));
        skip_empty = flag[1] ? 0 : 1;
    }
    // the distinct strings of the first `n` rows. A column that cannot be a dictionary (a comment column) shows it within its first rows:
    // those are interned alone first, so that the interning table over ALL rows (2 x rows slots, the largest temporary of a load) is only built
    // for a column that may qualify
    auto count_distinct = [&](int64_t n) -> int {
        ph_strdict *sd = nullptr;
        PH_CHECK(ph_strdict_build(ctx, &v, nullptr, n, codes, &sd));
        ph_strdict_free(sd);   // (stream-ordered: the table goes back to the pool behind the interning kernel)
        PH_HIP(hipMemsetAsync(count_dev, 0, 4, ctx->stream));
        ph::csv_reps_kernel<<<grid_for(ctx, n), 256, 0, ctx->stream>>>(codes, n, count_dev, reps, (const int32_t *)d.data, skip_empty);
        PH_HIP(hipGetLastError());
        return ctx->download(&nd, count_dev, 4);
    };
    if (nrows > head) {
        PH_CHECK(count_distinct(head));
        if (nd > 256u) return PH_OK;
        PH_CHECK(tmp.alloc((void **)&codes, nrows * 4));
    }
    PH_CHECK(count_distinct(nrows));
    if (nd > 256u) return PH_OK;
    std::vector<int32_t> rep((size_t)nd), len((size_t)nd), soff((size_t)nd + 1);
    if (nd > 0) {   // (0: every row is NULL; the column is PH_CODE8 with an empty dictionary)
        PH_CHECK(ctx->download(rep.data(), reps, nd * 4));
        std::sort(rep.begin(), rep.end());
        PH_CHECK(ph_dev_upload(ctx, reps, rep.data(), nd * 4));
        ph::csv_rep_lengths_kernel<<<1, 256, 0, ctx->stream>>>((const int32_t *)d.data, reps, (int)nd, lens);
        PH_HIP(hipGetLastError());
        PH_CHECK(ctx->download(len.data(), lens, nd * 4));
    }
    int64_t total = 0;
    for (int32_t l : len) total += l;
    int32_t *soff_dev = nullptr;
    uint8_t *sbytes_dev = nullptr;
    PH_CHECK(tmp.alloc((void **)&soff_dev, (nd + 1) * 4));
    PH_CHECK(tmp.alloc((void **)&sbytes_dev, total + 64));
    int64_t nb = 0;
    if (nd > 0) PH_CHECK(ph_substring(ctx, &v, 1, INT64_MAX, reps, nd, soff_dev, sbytes_dev, std::max<int64_t>(total, 1), &nb));
    std::string bytes((size_t)total, '\0');
    if (nd > 0) PH_CHECK(ctx->download(soff.data(), soff_dev, (nd + 1) * 4));
    if (total > 0) PH_CHECK(ctx->download(&bytes[0], sbytes_dev, total));
    if (bytes.find('\0') != std::string::npos) return PH_OK;   // a dictionary entry is a C string (ph_table_dict_entry): a value with a NUL byte keeps the column PH_STR
    std::vector<std::string> strs((size_t)nd);
    for (unsigned i = 0; i < nd; i++) strs[i] = bytes.substr((size_t)soff[i], (size_t)(soff[i + 1] - soff[i]));
    std::vector<int> order((size_t)nd);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return strs[(size_t)a] < strs[(size_t)b]; });   // std::string compares as unsigned bytes
    std::vector<uint8_t> rank((size_t)std::max(nd, 1u));
    d.dict.clear();
    for (unsigned k = 0; k < nd; k++) { rank[(size_t)order[k]] = (uint8_t)k; d.dict.push_back(strs[(size_t)order[k]]); }
    uint8_t *rank_dev = nullptr;
    PH_CHECK(tmp.alloc((void **)&rank_dev, 256));
    if (nd > 0) PH_CHECK(ph_dev_upload(ctx, rank_dev, rank.data(), nd));
    void *code8 = nullptr;
    PH_HIP(hipMalloc(&code8, (size_t)padded));
    if (hipMemsetAsync((char *)code8 + nrows, 0, (size_t)(padded - nrows), ctx->stream) != hipSuccess) { (void)hipFree(code8); ph::set_error("encode_strings: memset failed"); return PH_EHIP; }
    ph::csv_remap_kernel<<<grid_for(ctx, nrows), 256, 0, ctx->stream>>>(codes, nrows, reps, rank_dev, (int)nd, (uint8_t *)code8, validity);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) { (void)hipFree(code8); ph::set_error("encode_strings: csv_remap_kernel failed"); return PH_EHIP; }
    (void)hipFree(d.data);
    (void)hipFree(d.aux);
    d.type = PH_CODE8;
    d.data = code8;
    d.aux = nullptr;
    d.aux_bytes = 0;
    return PH_OK;
}

extern "C" int ph_csv_parse_field(int32_t type, int32_t scale, const char *s, int64_t len, int64_t *value, int32_t *is_null) {
    PH_REQUIRE(value && is_null && len >= 0 && (s || len == 0), "ph_csv_parse_field: bad arguments");
    PH_REQUIRE(type == PH_I32 || type == PH_I64 || type == PH_DATE || type == PH_DEC64, "ph_csv_parse_field: type %d has no fixed-width text form", type);
    PH_REQUIRE(type != PH_DEC64 || (scale >= 0 && scale <= 18), "ph_csv_parse_field: scale %d", scale);
    int null = 0;
    const int cause = ph::csv::parse_field(type, scale, HostBytes{s}, 0, len, value, &null);
    *is_null = null;
    if (cause != ph::csv::C_OK) { *value = 0; ph::set_error("ph_csv_parse_field: %s", ph::csv::cause_text(cause)); }
    return ph::csv::cause_code(cause);
}

extern "C" int ph_csv_split_record(const char *text, int64_t nbytes, int32_t delimiter, uint32_t flags, int64_t pos, int64_t *begin,
                                   int64_t *end, int32_t *fflags, int32_t cap, int32_t *nfields, int64_t *next) {
    PH_REQUIRE(nfields && next && nbytes >= 0 && (text || nbytes == 0) && pos >= 0 && pos <= nbytes && cap >= 0 && (cap == 0 || (begin && end && fflags)),
               "ph_csv_split_record: bad arguments");
    PH_REQUIRE((flags & ~PH_CSV_QUOTES) == 0, "ph_csv_split_record: unknown flags 0x%x", flags);
    PH_REQUIRE(delimiter > 0 && delimiter < 128 && delimiter != '"' && delimiter != '\r' && delimiter != '\n',
               "ph_csv_split_record: the delimiter is one byte (1..127), not '\"', '\r' or '\n' (got %d)", delimiter);
    auto keep = [&](int32_t i, const ph::csv::Field &f) {
        if (i >= cap) return;
        begin[i] = f.b;
        end[i] = f.e;
        fflags[i] = (f.quoted ? ph::csv::F_QUOTED : 0) | (f.drop ? ph::csv::F_ESCAPED : 0);
    };
    const int cause = flags & PH_CSV_QUOTES ? host_walk_record<true>(text, nbytes, delimiter, pos, nfields, next, keep)
                                            : host_walk_record<false>(text, nbytes, delimiter, pos, nfields, next, keep);
    if (cause != ph::csv::C_OK) ph::set_error("ph_csv_split_record: field %d of the record at byte %lld: %s", *nfields, (long long)pos, ph::csv::cause_text(cause));
    return ph::csv::cause_code(cause);
}

extern "C" int ph_table_create_csv(ph_ctx *ctx, const void *text, int64_t nbytes, int32_t delimiter, const ph_csv_col *cols, int32_t ncols,
                                   ph_table **out) {
    return ph_table_create_csv_ex(ctx, text, nbytes, delimiter, cols, ncols, 0, out);
}

extern "C" int ph_table_create_csv_ex(ph_ctx *ctx, const void *text, int64_t nbytes, int32_t delimiter, const ph_csv_col *cols, int32_t ncols,
                                      uint32_t flags, ph_table **out) {
    PH_REQUIRE(ctx && out && cols && ncols > 0 && ncols < 65535 && nbytes >= 0 && (text || nbytes == 0), "ph_table_create_csv: bad arguments");
    PH_REQUIRE((flags & ~PH_CSV_QUOTES) == 0, "ph_table_create_csv: unknown flags 0x%x", flags);
    const bool quotes = (flags & PH_CSV_QUOTES) != 0;
    PH_REQUIRE(delimiter > 0 && delimiter < 128 && delimiter != '"' && delimiter != '\r' && delimiter != '\n',
               "ph_table_create_csv: the delimiter is one byte (1..127), not '\"', '\r' or '\n' (got %d)", delimiter);
    for (int32_t k = 0; k < ncols; k++) {
        const int32_t t = cols[k].type;
        PH_REQUIRE(cols[k].field >= 0, "ph_table_create_csv: column %d: field %d", k, cols[k].field);
        PH_REQUIRE(t == PH_I32 || t == PH_I64 || t == PH_DATE || t == PH_DEC64 || t == PH_STR, "ph_table_create_csv: column %d: type %d has no text form", k, t);
        PH_REQUIRE(t != PH_DEC64 || (cols[k].scale >= 0 && cols[k].scale <= 18), "ph_table_create_csv: column %d: scale %d", k, cols[k].scale);
    }
    PH_HIP(hipSetDevice(ctx->device));
    const int64_t T = ph::CSV_TILE;
    Temps tmp;

    // ---- the text, padded with line ends (see csv_rows_kernel)
    const int64_t L = ph::round_up(nbytes + 1, T), ntiles = L / T;
    unsigned char *buf = nullptr;
    PH_CHECK(tmp.alloc((void **)&buf, ph::CSV_PAD + L + ph::CSV_PAD));
    unsigned char *dtext = buf + ph::CSV_PAD;
    PH_HIP(hipMemsetAsync(buf, '\n', ph::CSV_PAD, ctx->stream));
    PH_HIP(hipMemsetAsync(dtext + nbytes, '\n', (size_t)(L - nbytes + ph::CSV_PAD), ctx->stream));
    PH_CHECK(ph_dev_upload(ctx, dtext, text, nbytes));

    const int64_t ctl_bytes = ph::round_up((int64_t)offsetof(CsvControl, str_bytes) + (int64_t)ncols * 8 + (int64_t)ncols * 4 * 2, 8);
    std::vector<char> ctl_host((size_t)ctl_bytes, 0);
    CsvControl *ctl = (CsvControl *)ctl_host.data();
    ctl->err = ~0ull;
    char *ctl_dev = nullptr;
    PH_CHECK(tmp.alloc((void **)&ctl_dev, ctl_bytes));
    PH_CHECK(ph_dev_upload(ctx, ctl_dev, ctl_host.data(), ctl_bytes));
    unsigned long long *err_dev = (unsigned long long *)(ctl_dev + offsetof(CsvControl, err));
    int64_t *total_dev = (int64_t *)(ctl_dev + offsetof(CsvControl, scan_total));
    unsigned long long *str_bytes_dev = (unsigned long long *)(ctl_dev + offsetof(CsvControl, str_bytes));
    unsigned *nulls_dev = (unsigned *)(str_bytes_dev + ncols);
    unsigned *escapes_dev = nulls_dev + ncols;   // PH_CSV_QUOTES: the column has a field with "" or "\r\n" inside its quotes

    // ---- 1. row boundaries
    int32_t *tile_rows = nullptr;
    PH_CHECK(tmp.alloc((void **)&tile_rows, (ntiles + 1) * 4));
    PH_HIP(hipMemsetAsync(tile_rows + ntiles, 0, 4, ctx->stream));
    int32_t *tile_quotes = nullptr, *tile_rows_odd = nullptr;
    unsigned *quote_dev = (unsigned *)(ctl_dev + offsetof(CsvControl, quote));
    if (quotes) {   // starts by quote parity: counts for both incoming parities, the scan of the quote counts picks (see csv_rows_kernel)
        PH_CHECK(tmp.alloc((void **)&tile_quotes, ntiles * 4));
        PH_CHECK(tmp.alloc((void **)&tile_rows_odd, ntiles * 4));
        ph::csv_rows_kernel<false, true><<<(unsigned)ntiles, ph::CSV_THREADS, 0, ctx->stream>>>(dtext, tile_rows, nullptr, nullptr, tile_quotes, tile_rows_odd);
        PH_HIP(hipGetLastError());
        PH_CHECK(ph::exclusive_scan_i32(ctx, tile_quotes, ntiles, total_dev));   // (a wrapped sum keeps its low bit)
        ph::csv_pick_rows_kernel<<<(unsigned)((ntiles + 255) / 256), 256, 0, ctx->stream>>>(tile_quotes, tile_rows_odd, tile_rows, ntiles);
        PH_HIP(hipGetLastError());
    } else {
        ph::csv_rows_kernel<false, false><<<(unsigned)ntiles, ph::CSV_THREADS, 0, ctx->stream>>>(dtext, tile_rows, nullptr, quote_dev, nullptr, nullptr);
        PH_HIP(hipGetLastError());
    }
    ph::sum_lengths_kernel<<<grid_for(ctx, ntiles), 256, 0, ctx->stream>>>(tile_rows, ntiles, (unsigned long long *)(ctl_dev + offsetof(CsvControl, rows)));
    PH_HIP(hipGetLastError());
    PH_CHECK(ph::exclusive_scan_i32(ctx, tile_rows, ntiles + 1, total_dev));
    PH_CHECK(ctx->download(ctl_host.data(), ctl_dev, (int64_t)offsetof(CsvControl, str_bytes)));
    if (ctl->quote) {
        ph::set_error("ph_table_create_csv: the text holds a '\"' byte; quoted fields are not parsed on the device");
        return PH_EUNSUPPORTED;
    }
    const int64_t nrows = (int64_t)ctl->rows;   // (not the scan's total: above 2^31 record starts its int32 prefixes wrap)
    PH_REQUIRE(nrows >= 0 && nrows < (1ll << 31), "ph_table_create_csv: %lld rows exceed the int32 row-id domain", (long long)nrows);
    if (nrows == 0) {   // empty text / only empty lines: an empty table, as ph_table_create builds it
        const int64_t zero[2] = {0, 0};
        std::vector<ph_col> hc((size_t)ncols);
        for (int32_t k = 0; k < ncols; k++) {
            hc[(size_t)k] = ph_col{};
            hc[(size_t)k].type = cols[k].type == PH_STR ? PH_CODE8 : cols[k].type;
            hc[(size_t)k].scale = cols[k].type == PH_DEC64 ? cols[k].scale : 0;
            hc[(size_t)k].data = zero;
            if (cols[k].type == PH_STR) hc[(size_t)k].aux = "";
        }
        return ph_table_create(ctx, ncols, hc.data(), 0, out);
    }
    int64_t *starts = nullptr;
    PH_CHECK(tmp.alloc((void **)&starts, nrows * 8));
    if (quotes) ph::csv_rows_kernel<true, true><<<(unsigned)ntiles, ph::CSV_THREADS, 0, ctx->stream>>>(dtext, tile_rows, starts, nullptr, tile_quotes, nullptr);
    else ph::csv_rows_kernel<true, false><<<(unsigned)ntiles, ph::CSV_THREADS, 0, ctx->stream>>>(dtext, tile_rows, starts, nullptr, nullptr, nullptr);
    PH_HIP(hipGetLastError());

    // ---- the table's columns, and what the fields kernel needs of them
    TableGuard guard;
    ph_table *t = guard.t = new ph_table();
    t->ctx = ctx;
    t->nrows = nrows;
    t->cols.resize((size_t)ncols);
    const int64_t padded = ph::round_up(nrows, PH_ROW_PAD);
    std::vector<ph::CsvColDev> dc((size_t)ncols);
    for (int32_t k = 0; k < ncols; k++) {
        ph_table::column &d = t->cols[(size_t)k];
        d.type = cols[k].type;
        d.scale = cols[k].type == PH_DEC64 ? cols[k].scale : 0;
        ph::CsvColDev &C = dc[(size_t)k];
        C = ph::CsvColDev{cols[k].field, d.type, d.scale, k, nullptr, nullptr, nullptr};
        if (d.type == PH_STR) {
            PH_HIP(hipMalloc(&d.data, (size_t)((padded + 1) * 4)));
            PH_HIP(hipMemsetAsync(d.data, 0, (size_t)((padded + 1) * 4), ctx->stream));
            PH_CHECK(tmp.alloc((void **)&C.sbegin, nrows * 8));
        } else {
            const int w = ph::type_width(d.type);
            PH_HIP(hipMalloc(&d.data, (size_t)(padded * w)));
            PH_HIP(hipMemsetAsync((char *)d.data + nrows * w, 0, (size_t)((padded - nrows) * w), ctx->stream));
            if (d.type != PH_DEC64) {   // may hold NULLs: all rows valid until the kernel meets an empty field; the padding's bits are 0
                PH_HIP(hipMalloc((void **)&d.validity, (size_t)(padded / 8)));
                PH_HIP(hipMemsetAsync(d.validity, 0, (size_t)(padded / 8), ctx->stream));
                if (nrows / 8) PH_HIP(hipMemsetAsync(d.validity, 0xff, (size_t)(nrows / 8), ctx->stream));
                if (nrows % 8) PH_HIP(hipMemsetAsync(d.validity + nrows / 8, (1 << (nrows % 8)) - 1, 1, ctx->stream));
                C.validity = (unsigned *)d.validity;
            }
        }
        C.data = d.data;
    }
    std::stable_sort(dc.begin(), dc.end(), [](const ph::CsvColDev &a, const ph::CsvColDev &b) { return a.field < b.field; });
    ph::CsvColDev *dc_dev = nullptr;
    PH_CHECK(tmp.alloc((void **)&dc_dev, (int64_t)ncols * (int64_t)sizeof(ph::CsvColDev)));
    PH_CHECK(ph_dev_upload(ctx, dc_dev, dc.data(), (int64_t)ncols * (int64_t)sizeof(ph::CsvColDev)));

    // ---- 2. fields
    const int nfields0 = first_record_fields((const char *)text, nbytes, delimiter, quotes);
    if (quotes)
        ph::csv_fields_kernel<true><<<(unsigned)ntiles, ph::CSV_FIELD_THREADS, 0, ctx->stream>>>(dtext, tile_rows, starts, dc_dev, ncols, delimiter, nfields0, err_dev, nulls_dev, escapes_dev, nrows, L);
    else
        ph::csv_fields_kernel<false><<<(unsigned)ntiles, ph::CSV_FIELD_THREADS, 0, ctx->stream>>>(dtext, tile_rows, starts, dc_dev, ncols, delimiter, nfields0, err_dev, nulls_dev, escapes_dev, nrows, L);
    PH_HIP(hipGetLastError());
    for (int32_t k = 0; k < ncols; k++)
        if (cols[k].type == PH_STR) {
            ph::sum_lengths_kernel<<<grid_for(ctx, nrows), 256, 0, ctx->stream>>>((const int32_t *)t->cols[(size_t)k].data, nrows, str_bytes_dev + k);
            PH_HIP(hipGetLastError());
        }
    PH_CHECK(ctx->download(ctl_host.data(), ctl_dev, ctl_bytes));
    if (ctl->err != ~0ull) {
        const long long row = (long long)(ctl->err >> 32);
        const int col1 = (int)((ctl->err >> 8) & 0xffff), cause = (int)(ctl->err & 0xff);
        if (cause == ph::csv::C_BARE_QUOTE || cause == ph::csv::C_QUOTE) ph::set_error("ph_table_create_csv: row %lld: %s", row, ph::csv::cause_text(cause));
        else if (col1 == 0) ph::set_error("ph_table_create_csv: row %lld: %s (%d fields)", row, ph::csv::cause_text(cause), nfields0);
        else ph::set_error("ph_table_create_csv: row %lld, field %d (column %d): %s", row, cols[col1 - 1].field, col1 - 1, ph::csv::cause_text(cause));
        return ph::csv::cause_code(cause);
    }
    const unsigned long long *str_bytes = ctl->str_bytes;
    const unsigned *nulls = (const unsigned *)(ctl->str_bytes + ncols);
    const unsigned *escapes = nulls + ncols;
    for (int32_t k = 0; k < ncols; k++)
        PH_REQUIRE(cols[k].type != PH_STR || str_bytes[k] < (1ull << 31), "ph_table_create_csv: column %d holds %llu string bytes (int32 offsets)", k, str_bytes[k]);

    // ---- 3. VARCHAR: offsets, bytes, encoding
    for (int32_t k = 0; k < ncols; k++) {
        ph_table::column &d = t->cols[(size_t)k];
        if (d.type != PH_STR) continue;
        int64_t *sbegin = nullptr;
        for (auto &C : dc) if (C.orig == k) sbegin = C.sbegin;
        PH_CHECK(ph::exclusive_scan_i32(ctx, (int32_t *)d.data, nrows + 1, total_dev));
        d.aux_bytes = (int64_t)str_bytes[k];
        PH_HIP(hipMalloc(&d.aux, (size_t)(d.aux_bytes + 64)));
        if (quotes) ph::copy_strings_kernel<true><<<(unsigned)((nrows + 255) / 256), 256, 0, ctx->stream>>>(dtext, sbegin, (const int32_t *)d.data, nrows, (unsigned char *)d.aux);
        else ph::copy_strings_kernel<false><<<(unsigned)((nrows + 255) / 256), 256, 0, ctx->stream>>>(dtext, sbegin, (const int32_t *)d.data, nrows, (unsigned char *)d.aux);
        PH_HIP(hipGetLastError());
        if (escapes[k]) {   // only a column that has such a row pays for the second kernel
            ph::csv_copy_escaped_kernel<<<grid_for(ctx, nrows), 256, 0, ctx->stream>>>(dtext, sbegin, (const int32_t *)d.data, nrows, (unsigned char *)d.aux);
            PH_HIP(hipGetLastError());
        }
        PH_CHECK(ph::encode_strings(ctx, d, nrows, padded, (unsigned *)(ctl_dev + offsetof(CsvControl, scan_total)), tmp, nullptr));
    }

    // ---- 4. the text and the temporaries go; a column without a NULL has no bitmap; the shared finishing
    PH_HIP(hipStreamSynchronize(ctx->stream));
    tmp.release();
    for (int32_t k = 0; k < ncols; k++) {
        ph_table::column &d = t->cols[(size_t)k];
        if (d.validity && !nulls[k]) { (void)hipFree(d.validity); d.validity = nullptr; }
        PH_CHECK(ph::table_finish_column(ctx, d, nrows, padded, nullptr, 0));
    }
    ph::register_table(t);
    guard.t = nullptr;
    *out = t;
    return PH_OK;
}
