/*
 * planhip.h — C ABI of libplanhip.so, the MI355X (gfx950) execution backend for the hot path of
 * daviszhen/plan:  PhysicalScan -> Filter -> HashJoin build/probe -> HashAggregate
 * (pkg/compute executors over pkg/chunk vectors).
 *
 * This is the boundary a cgo shim binds (INTEGRATION.md shows the Go side). It replaces, inside
 * the reference's `buildOperatorExec` switch (pkg/compute/executor.go:305-350), the bodies of
 *   scanExecutor.Execute / runFilterExec        pkg/compute/executor_scan.go:144-241
 *   filterExecutor.Execute                      pkg/compute/executor_filter.go:27-114
 *   joinExecutor.Execute (build + probe)        pkg/compute/executor_join.go:54-264
 *   aggExecutor.Execute (sink + finalize)       pkg/compute/executor_aggr.go:106-265
 * while the OperatorExec interface itself (executor_operator.go:52-56) and pkg/chunk stay as they
 * are. Plain pointers and sizes only; no C++ or torch types cross it.
 *
 * Conventions
 *  - Every function returns 0 (PH_OK) or a negative PH_E* code; ph_last_error() gives the
 *    thread-local message. Nothing aborts: the shim turns a code into a Go `error`, which is how
 *    the reference reports operator failures (panic -> recover -> error, executor_bench.go:184-204).
 *  - A ph_ctx is bound to one HIP device and one stream. Calls on one ctx are stream-ordered and
 *    must come from one thread at a time (the reference drives a query from one goroutine).
 *    Separate ctxs are independent (concurrent queries of the psql server path).
 *  - Column encodings on the device = what the reference's loader reads from
 *    parquet (executor_scan.go:410-466): INTEGER int32, BIGINT int64, DATE int32 days since
 *    1970-01-01, DECIMAL int64 unscaled (+ scale), VARCHAR with <=256 distinct values as uint8
 *    dictionary codes, other VARCHAR as int32 offsets + bytes.
 *  - Validity is pkg/util/bitmap.go's: 1 bit per row, LSB first, NULL pointer = all valid.
 *  - Row ids / selection vectors on the device are int32 (a device batch is < 2^31 rows); the
 *    shim widens them to pkg/chunk's `[]int` (select_vector.go:7-9) when it hands them back.
 *  - "dev" pointers are HIP device pointers owned by the caller unless stated otherwise.
 */
#ifndef PLANHIP_H
#define PLANHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PH_OK 0
#define PH_EINVAL (-1)      /* bad argument */
#define PH_EHIP (-2)        /* a HIP runtime call failed */
#define PH_EUNSUPPORTED (-3)/* expression / type shape outside the device path: caller falls back */
#define PH_EOVERFLOW (-4)   /* decimal arithmetic would leave the exact int64/int128 domain */
#define PH_ECAPACITY (-5)   /* an output buffer supplied by the caller is too small */
#define PH_ECONSTRAINT (-6) /* a strict lookup met a probe row without exactly one build row */

typedef struct ph_ctx ph_ctx;

const char *ph_last_error(void);
const char *ph_version(void);

int ph_ctx_create(int device, ph_ctx **out);
/* Use an existing stream (e.g. the caller's torch stream) for all later calls; NULL = own stream */
int ph_ctx_set_stream(ph_ctx *ctx, void *hip_stream);
int ph_ctx_sync(ph_ctx *ctx);
/* Deferred errors. A call that only reads a FLAG back (ph_expr_eval's overflow flag) stalls the
 * stream for a host round trip (~25-45 us of idle GPU) although the flag is almost never set. With
 * `on` != 0 such flags stay on the device and the NEXT call on this ctx that reads anything back
 * (a count, a result download, ph_ctx_check_deferred) fetches them in the same synchronisation and
 * returns the deferred error (PH_EOVERFLOW / PH_ECONSTRAINT, ph_last_error names the origin)
 * instead of its own success: everything computed since the failing call must be discarded, which
 * is what a query does with PH_EOVERFLOW anyway (it falls back as a whole). Off by default: every
 * call then reports its own errors, like the reference's operators do per chunk.
 * `on` == 2 HOLDS deferred errors: no ordinary read-back reports them, only ph_ctx_check_deferred does.
 * That is the mode of a query that runs over several ranks: a rank must not leave the sequence of
 * collectives in the middle because of an error only it has seen (its peers would block in the next
 * collective) — it runs to the end, checks, and the ranks agree on the outcome (one small all-reduce)
 * before any of them reruns the query. The ph_comm_* calls never report a deferred error. */
int ph_ctx_set_deferred_errors(ph_ctx *ctx, int32_t on);
/* Asynchronous counts. With `on` != 0 the calls that hand a row count back to the host
 * (ph_filter_select's *n_out, ph_join_probe_inner*'s *n_out) return as soon as their kernels and an
 * 8-byte copy are queued, with *n_out = -1; ph_ctx_wait_counts fills every pending count in (waiting
 * for the last of those copies, not for the stream) and reports PH_ECAPACITY for a pair list that
 * overflowed. The count variables must stay alive until then. Independent work queued in between —
 * another join's build, a probe that needs the table but not the count — keeps the GPU busy while
 * the host wakes up and prepares the launches that depend on the count (~25 us per round trip).
 * Switching it off waits first. */
int ph_ctx_set_async_counts(ph_ctx *ctx, int32_t on);
int ph_ctx_wait_counts(ph_ctx *ctx);
/* synchronise and report a pending deferred error (PH_OK when none is pending) */
int ph_ctx_check_deferred(ph_ctx *ctx);
/* How often this context's exclusive scan of block counts (the step that places the rows of every count / scan / write operator) took each of
 * its forms, counted on the host since the context was created: out[0] the one-workgroup loop (up to 1024 counts), out[1] the one-step form (up to
 * 16384), out[2] the single-pass look-back, out[3] the three-pass form (PH_SCAN_THREE_PASS, once per level of its recursion). Like ph_join_kind and
 * ph_scan_plan_kind it says which path ran: a test takes the difference around a call. */
int ph_ctx_scan_forms(ph_ctx *ctx, int64_t out[4]);
void ph_ctx_destroy(ph_ctx *ctx);

/* ------------------------------------------------------------------ columns */
typedef enum {
    PH_I32 = 1,
    PH_I64 = 2,
    PH_DATE = 3,  /* int32 days since epoch */
    PH_DEC64 = 4, /* int64 unscaled, `scale` fractional digits */
    PH_CODE8 = 5, /* uint8 dictionary code */
    PH_F32 = 6,
    PH_F64 = 7,
    PH_STR = 8,   /* int32 offsets[n+1] in `data`, bytes in `aux` */
    PH_COLREF = 9 /* ph_const only (resident plans): the right operand is another column, ph_const.i = its index */
} ph_type;

typedef struct {
    int32_t type;
    int32_t scale;
    const void *data;       /* host or device pointer, depending on the call */
    const uint8_t *validity;/* bitmap or NULL */
    const void *aux;        /* PH_STR: bytes */
    int64_t aux_bytes;
} ph_col;

/* ------------------------------------------------------------------ table residency
 * Replaces DataTable.Scan's per-chunk materialisation (pkg/storage/table.go:418-428 feeding
 * scanRows, executor_scan.go:158-241): the pruned columns of a table are loaded once into HBM
 * (pinned staging + hipMemcpyAsync) and stay resident across queries. */
typedef struct ph_table ph_table;

int ph_table_create(ph_ctx *ctx, int32_t ncols, const ph_col *host_cols, int64_t nrows,
                    ph_table **out);
int64_t ph_table_rows(const ph_table *t);
int32_t ph_table_ncols(const ph_table *t);
/* device view of column c (data/validity/aux are device pointers) */
int ph_table_col(const ph_table *t, int32_t c, ph_col *out);
/* per-column min/max gathered at load (int64 domain; used for overflow proofs). The range of a NULL-able column covers every stored
 * slot, the NULL slots included (whatever the caller stored there), so it bounds what a kernel can read from the column. */
int ph_table_col_range(const ph_table *t, int32_t c, int64_t *min, int64_t *max);
/* ---- Arrow C data interface (the stable ABI of https://arrow.apache.org/docs/format/CDataInterface.html; the two
 * structs are declared here exactly as the specification prints them, under its own include guard) */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
struct ArrowSchema {
    const char *format;
    const char *name;
    const char *metadata;
    int64_t flags;
    int64_t n_children;
    struct ArrowSchema **children;
    struct ArrowSchema *dictionary;
    void (*release)(struct ArrowSchema *);
    void *private_data;
};
struct ArrowArray {
    int64_t length;
    int64_t null_count;
    int64_t offset;
    int64_t n_buffers;
    int64_t n_children;
    const void **buffers;
    struct ArrowArray **children;
    struct ArrowArray *dictionary;
    void (*release)(struct ArrowArray *);
    void *private_data;
};
#endif
/* The column load path through the C-ABI: a record batch — a struct array ("+s") whose children
 * are the columns, as parquet readers, Arrow Flight and Go's arrow/cdata hand it over — becomes a resident table in the
 * device encodings, whole columns at a time. Replaces COPY FROM parquet + the scan's materialisation
 * (pkg/compute/executor_scan.go:272-309 readers, :410-466 parquetColToValue + Vector.SetValue: one VALUE at a time into
 * 24-byte Decimal / 12-byte Date / malloc'd String cells). Arrow's buffers already hold the narrow encodings:
 *   int32 "i" -> PH_I32, int64 "l" -> PH_I64, date32 "tdD" -> PH_DATE (days since 1970-01-01, the same number),
 *   decimal128 "d:p,s" -> PH_DEC64 (the low word; PH_EOVERFLOW when a value needs more than 64 bits),
 *   utf8 "u" / large_utf8 "U" -> PH_CODE8 + dictionary in byte order when the column has <= 256 distinct strings
 *   (also dictionary-encoded arrays of such strings), else PH_STR offsets + bytes;
 * validity bitmaps have pkg/util/bitmap.go's convention (1 bit per row, LSB first, 1 = valid) and pass through (re-packed
 * when the array's offset is not a multiple of 8). The buffers are read during the call only; the caller keeps
 * ownership and releases the batch as usual. `cols` (optional, ncols entries) selects and orders the children, else all. */
int ph_table_create_arrow(ph_ctx *ctx, const struct ArrowSchema *schema, const struct ArrowArray *batch, const int32_t *cols,
                          int32_t ncols, ph_table **out);
/* ---- delimited text (dbgen .tbl, CSV with encoding/csv's quoting), parsed on the device
 * The reference's own load path: COPY FROM ... (format csv, delimiter '|') read by scanExecutor through encoding/csv
 * (pkg/compute/executor_scan.go:107-120), readCsvTable + fieldToValue (:311-408) and Vector.SetValue
 * (pkg/chunk/vector.go:195-264), one VALUE at a time into 24-byte decimals and 12-byte dates. Here the text is uploaded
 * once (pinned staging, 64-bit byte positions) and kernels find the records, parse the requested fields into the device
 * encodings and build the columns where they stay; the table is the one ph_table_create builds over the same values
 * (padding and NULL slots zeroed, a validity bitmap only for a column that has a NULL, min / max, order and run
 * statistics, narrowed copies).
 *
 * Records — encoding/csv with only Comma set: a record ends at '\n', "\r\n" counts as '\n', the final record needs no
 * newline, ONE trailing '\r' at the end of input is dropped, empty lines are skipped and are no rows. Every record has as
 * many fields as the first (PH_EINVAL otherwise), and at least cols[k].field + 1 of them (PH_EINVAL, "no enough fields in
 * the line"); a trailing delimiter, as dbgen writes one, is one more (empty) field. Without PH_CSV_QUOTES (flags 0,
 * ph_table_create_csv) quoting is NOT parsed: a '"' byte anywhere in the text -> PH_EUNSUPPORTED (found by the pass that
 * counts the rows). For PH_EINVAL / PH_EOVERFLOW / PH_EUNSUPPORTED of a value, ph_last_error names the LOWEST failing row
 * (0-based, empty lines not counted), the field and the cause. Empty text or only empty lines: a table of 0 rows.
 *
 * Quoted fields — ph_table_create_csv_ex with PH_CSV_QUOTES: encoding/csv's readRecord, strict (the reference sets none of
 * LazyQuotes, TrimLeadingSpace and Comment; they are NOT offered). The quote character is '"', always.
 *   - A field is quoted only when its FIRST byte is '"'. A '"' anywhere else in an unquoted field (a"b, or _"x" behind a
 *     leading space) is an error: "bare quote" (Go's ErrBareQuote).
 *   - Inside a quoted field "" is one '"'; '"' followed by the delimiter ends the field; '"' followed by '\n' or "\r\n"
 *     (or the end of input, or one '\r' and the end of input) ends the field and the record; '"' followed by anything
 *     else — a lone '\r' before more text included — is an error: "extraneous or missing quote" (Go's ErrQuote), and so
 *     is the end of input inside a quoted field. The delimiter and '\n' are data; "\r\n" is the ONE byte '\n' (Go
 *     normalises every physical line), a lone '\r' stays, empty lines inside a quoted field are data.
 *   - Outside quotes the record rules above are unchanged.
 *   - Both errors are PH_EINVAL; ph_last_error names the row and which of the two it was. A row with a quoting error
 *     reports THAT error whatever else is wrong with it (Go returns the parse error before it compares field counts and
 *     before any value is looked at); the lowest failing row still wins across all causes.
 *   - Values are taken from the unescaped content: "" is the empty field (NULL for PH_I32 / PH_I64 / PH_DATE, 0 for
 *     PH_DEC64, the empty string for VARCHAR), "12" is the integer 12. The field count ("as many as the first record")
 *     counts fields under this grammar.
 *
 * Values — fieldToValue + SetValue:
 *   PH_I32 / PH_I64  strconv.ParseInt(s, 10, 64): [+-] and one or more digits, nothing else (leading zeros are fine); the
 *                    empty field is NULL; outside int64 -> PH_EOVERFLOW. PH_I32: outside int32 -> PH_EOVERFLOW — a
 *                    DELIBERATE deviation: the reference truncates silently (int32(val.I64)).
 *   PH_DATE          time.Parse("2006-01-02"): exactly dddd-dd-dd, month 1..12, a day that month has (Gregorian leap
 *                    years); the empty field is NULL, anything else PH_EINVAL. Stored as days since 1970-01-01 (negative
 *                    before).
 *   PH_DEC64, scale  ParseExact(field, scale): [+-]digits[.digits] with at most `scale` fractional digits, padded to
 *                    `scale`; the sign survives a zero integer part ("-0.05"). The EMPTY field is the value 0, NOT NULL
 *                    (the reference takes NewFromInt64(0, 0, scale) for it). More fractional digits -> PH_EUNSUPPORTED
 *                    (the reference would widen that one value's scale); a digit missing before or after the point, an
 *                    exponent or any other byte -> PH_EUNSUPPORTED; an unscaled value outside int64 -> PH_EOVERFLOW.
 *   PH_STR (VARCHAR) the field's bytes; the empty field is the empty string, not NULL. Encoded as ph_table_create_arrow
 *                    encodes strings: <= 256 distinct -> PH_CODE8 + dictionary in unsigned byte order (ph_table_dict_*),
 *                    else PH_STR offsets + bytes (also when a value holds a NUL byte: dictionary entries are C strings);
 *                    2^31 string bytes or more in one column -> PH_EINVAL. */
typedef struct {
    int32_t field;   /* 0-based field of the record this column is read from (any order, fields may be skipped) */
    int32_t type;    /* PH_I32, PH_I64, PH_DATE, PH_DEC64, or PH_STR = VARCHAR */
    int32_t scale;   /* PH_DEC64: the column's scale (0..18) */
} ph_csv_col;
/* text: host bytes, read during the call only. delimiter: one byte (1..127), not '"', '\r' or '\n' (PH_EINVAL). */
int ph_table_create_csv(ph_ctx *ctx, const void *text, int64_t nbytes, int32_t delimiter, const ph_csv_col *cols, int32_t ncols,
                        ph_table **out);
/* the same with flags: 0 is ph_table_create_csv; unknown bits -> PH_EINVAL */
#define PH_CSV_QUOTES 1u   /* parse '"'-quoted fields as encoding/csv does (strict: LazyQuotes off) */
int ph_table_create_csv_ex(ph_ctx *ctx, const void *text, int64_t nbytes, int32_t delimiter, const ph_csv_col *cols, int32_t ncols,
                           uint32_t flags, ph_table **out);
/* host only, no device: the value of ONE field exactly as the device parser computes it (the same __host__ __device__
 * function), so the parsing rules can be tested on a machine without a GPU. type as above except PH_STR. *value: int32 /
 * int64 / days / unscaled, widened to int64. *is_null: 1 for a NULL. Returns PH_OK or the error code above. */
int ph_csv_parse_field(int32_t type, int32_t scale, const char *s, int64_t len, int64_t *value, int32_t *is_null);
/* host only: walk ONE record that starts at text[pos] with the same __host__ __device__ walker the kernel uses (empty
 * lines at pos are skipped first, as readRecord skips them). Fills up to cap fields: begin / end of the field's content
 * (inside the quotes for a quoted field) and flags (bit 0 quoted, bit 1 content holds "" or "\r\n" that the value drops).
 * *nfields = fields seen (0: only empty lines were left), *next = first byte behind the record's line end (at most
 * nbytes). flags: 0 or PH_CSV_QUOTES. Returns PH_OK or PH_EINVAL (ph_last_error: bare quote / extraneous or missing
 * quote; *nfields then counts the fields before the failing one). */
int ph_csv_split_record(const char *text, int64_t nbytes, int32_t delimiter, uint32_t flags, int64_t pos, int64_t *begin,
                        int64_t *end, int32_t *fflags, int32_t cap, int32_t *nfields, int64_t *next);
/* ---- Parquet column chunks, decoded on the device
 * The reference's other COPY FROM format (format parquet: pkg/compute/executor_scan.go:96-123, readers :272-309,
 * parquetColToValue :410-466, one VALUE at a time). Here the host parses only the metadata — the Thrift footer and the page
 * headers, O(pages) — uploads the byte ranges of the REQUESTED columns' chunks (pruned columns never cross PCIe) and kernels
 * decode levels, dictionary indices and values into the columns where they stay. The table is the one
 * ph_table_create_arrow builds over the same file read into Arrow: NULL slots and padding zeroed, a validity bitmap only for
 * a column that has a NULL, a NULL string of length 0 that is no distinct value, min / max, order and run statistics and
 * narrowed copies. Rows < 2^31; a file of 0 rows is a table of 0 rows.
 *
 * The subset. Anything outside it -> PH_EUNSUPPORTED, ph_last_error names the column and what it met; only the requested
 * columns are judged.
 *   Schema       flat: a requested leaf has max repetition level 0 and max definition level 0 or 1.
 *   Types        INT32 -> PH_I32; INT32 (Date) -> PH_DATE; INT64 -> PH_I64; INT32 / INT64 / FIXED_LEN_BYTE_ARRAY(1..16) with
 *                Decimal(p, s), 0 <= s <= 18 -> PH_DEC64 scale s (FIXED_LEN_BYTE_ARRAY: big-endian two's complement; a valid
 *                value outside int64 -> PH_EOVERFLOW, ph_table_create_arrow's rule for decimal128); BYTE_ARRAY (String or
 *                unannotated) -> VARCHAR, encoded as the other loaders encode it: <= 256 distinct non-NULL strings ->
 *                PH_CODE8 + dictionary in unsigned byte order, else PH_STR (also when a value holds a NUL byte); 2^31 or more
 *                string bytes in one column -> PH_EINVAL. BOOLEAN, INT96, FLOAT, DOUBLE: unsupported.
 *   Overrides    ph_parquet_col.type: 0 = what the schema says. The table's declared type may decide instead, as in
 *                parquetColToValue: PH_I64 over INT32 widens; PH_I32 over INT64 narrows, PH_EOVERFLOW outside int32 (the
 *                same DELIBERATE deviation as the text path: the reference truncates); PH_DEC64 + scale over a plain INT32 /
 *                INT64 takes the integer as the unscaled value. Naming the schema's own type is no override. Any other
 *                combination -> PH_EINVAL.
 *   Pages        dictionary pages (PLAIN), data pages v1 and v2, values PLAIN or RLE_DICTIONARY / PLAIN_DICTIONARY,
 *                definition levels in the RLE / bit-packed hybrid (both run kinds; bit widths 0..32 for indices); a chunk
 *                may change encoding from page to page; several row groups. DELTA_BINARY_PACKED (INT32 / INT64) and
 *                DELTA_LENGTH_BYTE_ARRAY (BYTE_ARRAY) only through the _ex entry points with PH_PARQUET_DELTA (below),
 *                without the flag they are refused, as is DELTA_BYTE_ARRAY (BYTE_ARRAY) without PH_PARQUET_DELTA_BYTE_ARRAY
 *                (further below). BYTE_STREAM_SPLIT always is.
 *   Compression  UNCOMPRESSED; SNAPPY only through the _ex entry points with PH_PARQUET_SNAPPY, LZ4_RAW (codec 7, the bare
 *                LZ4 block format, what pyarrow writes for compression="LZ4") only through them with PH_PARQUET_LZ4_RAW, and
 *                GZIP (codec 2) only through them with PH_PARQUET_GZIP, and ZSTD (codec 6) only through them with PH_PARQUET_ZSTD
 *                (all below). Without its flag each is refused like
 *                BROTLI, LZO and the deprecated LZ4 (codec 5), which always are: PH_EUNSUPPORTED naming the codec. A file may hold chunks in different codecs; each chunk is
 *                judged by its own. Encrypted files are refused likewise.
 *
 * Malformed files never read out of range. Every position and length taken from the file (footer length, chunk offsets,
 * page sizes, level section lengths) is checked on the host against the file's size and the enclosing chunk or page before
 * a kernel sees it: PH_EINVAL (bad magic and a file shorter than 12 bytes included). What only decoding can see — a hybrid
 * run past its section, a BYTE_ARRAY length past its page, a dictionary index at or above the dictionary's size, fewer or
 * more values than num_values — is bounded by the page's own byte range inside the decoders: PH_EINVAL, and ph_last_error
 * names the column, row group and page of the LOWEST failing page (page = its index in ph_parquet_pages' directory). */
typedef struct {
    int32_t column;  /* leaf column of the file's schema, 0-based, schema order */
    int32_t type;    /* 0 = what the file's schema says (above); or PH_I32 / PH_I64 / PH_DEC64 as an override */
    int32_t scale;   /* override PH_DEC64 only */
} ph_parquet_col;
typedef struct {
    int64_t name_pos;       /* the leaf's name: position and length inside the file's bytes (not NUL-terminated) */
    int32_t name_len;
    int32_t physical_type;  /* parquet.thrift Type: 0 BOOLEAN 1 INT32 2 INT64 3 INT96 4 FLOAT 5 DOUBLE 6 BYTE_ARRAY 7 FIXED_LEN_BYTE_ARRAY */
    int32_t type_length;    /* FIXED_LEN_BYTE_ARRAY */
    int32_t type;           /* the ph_type the schema maps to (PH_STR = VARCHAR), 0 if none (or the leaf is not flat) */
    int32_t scale;
    int32_t nullable;       /* max definition level > 0 */
} ph_parquet_colinfo;
#define PH_PARQUET_PAGE_DATA 0
#define PH_PARQUET_PAGE_DICTIONARY 2
#define PH_PARQUET_PAGE_DATA_V2 3
typedef struct {
    int32_t row_group;
    int32_t kind;           /* PH_PARQUET_PAGE_* (parquet.thrift PageType) */
    int32_t encoding;       /* parquet.thrift Encoding of the values: 0 PLAIN, 2 PLAIN_DICTIONARY, 8 RLE_DICTIONARY, ... */
    int32_t num_values;
    int64_t first_row;      /* data pages: the table row of the page's first value (a dictionary page: of its chunk's) */
    int64_t header_pos, data_pos, data_bytes;   /* the page header, and the page's data behind it */
    int64_t rep_levels_bytes, def_levels_bytes; /* v2: the level sections' lengths (v1: 0, a 4-byte length leads the section) */
} ph_parquet_page;
/* file: the whole file's bytes on the host, read during the call only. cols NULL / ncols 0: every column. A column may be
 * named twice. */
int ph_table_create_parquet(ph_ctx *ctx, const void *file, int64_t nbytes, const ph_parquet_col *cols, int32_t ncols, ph_table **out);
/* host only, no device: the leaves of the schema (up to cap are filled, *ncols = how many there are), rows and row groups */
int ph_parquet_schema(const void *file, int64_t nbytes, int64_t *nrows, int32_t *nrow_groups, ph_parquet_colinfo *info, int32_t cap,
                      int32_t *ncols);
/* host only: the page directory of one leaf column, the one the device path itself works from (index pages left out) */
int ph_parquet_pages(const void *file, int64_t nbytes, int32_t column, ph_parquet_page *pages, int32_t cap, int32_t *npages);
/* host only: ONE column decoded with the same __host__ __device__ decoders the kernels instantiate (the slow twin, as
 * ph_csv_parse_field is for text). Fixed types: values[nrows] widened to int64, NULL slots 0. VARCHAR: str_offsets[nrows + 1]
 * and the bytes (str_cap = room in str_bytes; *str_total = bytes the column holds; PH_ECAPACITY when they do not fit — call
 * with str_bytes NULL to learn the size). valid[nrows]: one BYTE per row, 1 = not NULL. Pointers a column does not need may
 * be NULL. Same codes and messages as ph_table_create_parquet. */
int ph_parquet_read_column_host(const void *file, int64_t nbytes, const ph_parquet_col *col, int64_t *values, uint8_t *valid,
                                int32_t *str_offsets, char *str_bytes, int64_t str_cap, int64_t *str_total);
/* ---- SNAPPY pages, decompressed on the device (opt-in)
 * The _ex forms take a flags word: 0 makes each its plain twin above (the plain entry points call them with 0), any bit
 * outside the defined set -> PH_EINVAL. With PH_PARQUET_SNAPPY a chunk whose codec is SNAPPY is decoded instead of refused,
 * and everything promised above for uncompressed files holds for it: the same table, subset, overrides, codes and "lowest
 * failing page" rule. Chunks in any other codec stay PH_EUNSUPPORTED naming the codec (LZ4_RAW, GZIP, ZSTD: unless its own flag is set, below).
 *   The host still reads metadata only. Per compressed page it checks what it can see: a v1 or dictionary page is ONE stream
 * that must produce uncompressed_page_size bytes; a v2 page keeps its level sections raw and the rest is one stream that
 * must produce uncompressed_page_size minus the level bytes (a v2 page whose header says is_compressed = false is stored raw
 * and decoded in place, as are all pages of an UNCOMPRESSED chunk). The stream's own length preamble (a varint of at most
 * 5 bytes and 32 bits) must equal that length, the length may not exceed 22 times the stream's bytes (no element yields more
 * than 64 bytes from fewer than 3), and a stream of 0 bytes is valid only for a length of 0: PH_EINVAL before anything is
 * allocated, so device memory is bounded by the file's size, never by a number in the file. The chunks are uploaded as
 * stored; one kernel launch in front of the first column's kernels decompresses every compressed section of the call (one
 * workgroup a section) into a region behind the upload, and the decoders then run on it unchanged. A corrupt stream —
 * offset 0, an offset beyond the bytes produced, a literal or copy operand past the input, an element past the expected
 * length, input that ends early or is left over — is PH_EINVAL naming column, row group and page. A v1 page's level-section
 * length lies inside the stream and is checked after decompression (same message as for a raw page).
 *   Which page is "the lowest failing page" when several fail: pages are ordered as the decoders meet them, on the device and in
 * the host twin alike — per column the BYTE_ARRAY dictionary pages, then the data pages, then the dictionary pages of fixed-width
 * columns (whose streams are the last thing judged). So a corrupt fixed-width dictionary page and a corrupt data page of the same
 * column name the DATA page; in every other combination the page that comes first in that order is named. */
#define PH_PARQUET_SNAPPY 1u   /* decode SNAPPY pages instead of refusing them */
int ph_table_create_parquet_ex(ph_ctx *ctx, const void *file, int64_t nbytes, const ph_parquet_col *cols, int32_t ncols,
                               uint32_t flags, ph_table **out);
/* host only: the twin decompresses the requested column's pages with the function the kernel instantiates, then decodes them */
int ph_parquet_read_column_host_ex(const void *file, int64_t nbytes, const ph_parquet_col *col, uint32_t flags, int64_t *values,
                                   uint8_t *valid, int32_t *str_offsets, char *str_bytes, int64_t str_cap, int64_t *str_total);
/* host only: the page directory of ph_parquet_pages, also for chunks in ANY codec (data_bytes = the bytes as stored; nothing
 * is decompressed or checked beyond the headers), plus per page what codecs[i] holds. codecs may be NULL. */
typedef struct {
    int32_t codec;              /* parquet.thrift CompressionCodec of the chunk: 0 UNCOMPRESSED, 1 SNAPPY, 2 GZIP, ... 6 ZSTD, 7 LZ4_RAW */
    int32_t compressed;         /* 1: this page's values (v1 and dictionary pages: the whole page) are stored compressed */
    int64_t uncompressed_bytes; /* the header's uncompressed_page_size */
} ph_parquet_page_codec;
int ph_parquet_pages_ex(const void *file, int64_t nbytes, int32_t column, ph_parquet_page *pages, ph_parquet_page_codec *codecs,
                        int32_t cap, int32_t *npages);
/* host only: one raw Snappy stream (the block format: a varint length, then elements), decoded by the host twin of the
 * device decoder. *dst_bytes = the length the preamble states (set whenever the preamble itself is readable). dst NULL: only
 * that length is wanted. PH_ECAPACITY when dst_cap is smaller; PH_EINVAL for a corrupt stream (ph_last_error says what is
 * wrong with it) or a preamble above 22 times src_bytes. Nothing outside dst[0, *dst_bytes) is written. */
int ph_snappy_decompress_host(const void *src, int64_t src_bytes, void *dst, int64_t dst_cap, int64_t *dst_bytes);
/* n independent streams on the device, by the kernel the Parquet load uses. src_dev / dst_dev are device buffers; the position
 * and length arrays are host arrays. Stream i lies at src_dev + src_pos[i], src_bytes[i] long (preamble included), and is
 * expected to produce exactly dst_bytes[i] at dst_dev + dst_pos[i]; only those bytes of dst_dev are written (a refused stream
 * leaves zeros there). The kernel READS src_dev in whole aligned 16-byte units: up to 15 bytes in front of a stream and behind
 * it are read (never used), so src_dev + src_pos[i] rounded down to 16 and the stream's end rounded up to 16 must lie inside
 * the allocation — true of any stream inside a hipMalloc'd buffer, whose size the runtime rounds up beyond that. status[i] (host) = PH_OK or PH_EINVAL. The call returns PH_OK when it ran, whatever the streams
 * held. */
int ph_snappy_decompress(ph_ctx *ctx, const void *src_dev, const int64_t *src_pos, const int64_t *src_bytes, void *dst_dev,
                         const int64_t *dst_pos, const int64_t *dst_bytes, int32_t n, int32_t *status);
/* ---- LZ4_RAW pages, decompressed on the device (opt-in)
 * With PH_PARQUET_LZ4_RAW a chunk whose codec is LZ4_RAW (parquet.thrift CompressionCodec 7: one bare LZ4 block per stream, no
 * frame, no length preamble) is decoded instead of refused, by the plumbing SNAPPY chunks take: the same per-page streams (a v1
 * or dictionary page whole, a v2 page behind its raw level sections, a v2 page with is_compressed = false raw), one kernel
 * launch per codec present in front of the first column's kernels, the same region behind the upload, the same "lowest
 * failing page" order. The flag composes with PH_PARQUET_SNAPPY (a file whose columns are SNAPPY, LZ4_RAW and UNCOMPRESSED
 * loads with 1 | 16) and with PH_PARQUET_DELTA. Bits 1 and 3 of the flags word are not defined: the valid words are every OR
 * of 1, 4 and 16. Without the flag every code and message is what it was. Codec 5, the deprecated LZ4, stays
 * PH_EUNSUPPORTED with or without the flag: three incompatible framings exist under that number.
 *   The block has no preamble, so what a stream must produce comes from the page header alone: uncompressed_page_size (v2:
 * minus the level bytes; negative -> PH_EINVAL). The host refuses, before anything is allocated, a length above 255 times the
 * stream's bytes (no byte of a block yields more) and a stream of 0 bytes for more than 0 bytes: PH_EINVAL. Everything else
 * is the decoder's: lengths are summed in 64 bits and refused as soon as they pass what is left of the input or the output;
 * a match needs 1 <= offset <= bytes produced (offset 0 is refused; liblz4 accepts it); the stream must produce exactly
 * the expected bytes and consume exactly its input, so a header that lies about the size is caught here. A corrupt stream
 * is PH_EINVAL "a corrupt LZ4_RAW stream" naming column, row group and page. The format's end-of-block restrictions (the
 * last 5 bytes are literals, the last match starts 12 bytes before the end) bind compressors and are NOT enforced: a stream
 * that breaks them decodes to exactly one byte string (liblz4 refuses it). */
#define PH_PARQUET_LZ4_RAW 16u /* decode LZ4_RAW pages instead of refusing them */
/* host only: one bare LZ4 block, decoded by the host twin of the device decoder. The format has no
 * preamble, so the caller states expected; dst has room for expected. *produced is set to the bytes
 * written (== expected on PH_OK). PH_EINVAL: a corrupt stream (ph_last_error names the sub-case), or
 * expected > 255 * src_bytes. */
int ph_lz4_decompress_host(const void *src, int64_t src_bytes, void *dst, int64_t expected, int64_t *produced);
/* n independent blocks on the device, by the kernel the Parquet load uses; same contract as ph_snappy_decompress
 * (host position / length arrays, 16-byte-unit reads, status[i], zeros for a refused block). */
int ph_lz4_decompress(ph_ctx *ctx, const void *src_dev, const int64_t *src_pos, const int64_t *src_bytes, void *dst_dev,
                      const int64_t *dst_pos, const int64_t *dst_bytes, int32_t n, int32_t *status);
/* ---- GZIP pages, inflated on the device (opt-in)
 * With PH_PARQUET_GZIP a chunk whose codec is GZIP (parquet.thrift CompressionCodec 2: RFC 1952 members around RFC 1951 DEFLATE)
 * is decoded instead of refused, by the plumbing SNAPPY and LZ4_RAW chunks take: the same per-page streams (a v1 or dictionary
 * page whole, a v2 page behind its raw level sections, a v2 page with is_compressed = false raw), one kernel launch per codec
 * present in front of the first column's kernels, the same region behind the upload, the same "lowest failing page" order.
 * The flag composes with the other three (a file whose columns are GZIP, SNAPPY, LZ4_RAW and UNCOMPRESSED loads with
 * 1 | 16 | 64; delta pages inside GZIP chunks are inflated first). Bits 0, 2, 4, 6 and (below) 8 of the flags word are defined and no other: the
 * valid words are every OR of 1, 4, 16, 64 and 256. Without the flag every code and message is what it was; with it, a codec that
 * is still refused (ZSTD without its own flag, BROTLI, LZO, codec 5) reads GZIP among the codecs that are decoded.
 *   What a stream must produce comes from the page header alone: uncompressed_page_size (v2: minus the level bytes). The
 * host refuses, before anything is allocated: a stream of 0 bytes for more than 0 bytes; a non-empty stream of fewer than 20
 * bytes (a 10-byte header, the 2 bytes of an empty fixed block, an 8-byte trailer); one that does not begin 1f 8b 08 or
 * has a reserved FLG bit set; a length above 1032 times the stream's bytes (a match of 258 bytes costs at least two bits):
 * PH_EINVAL. Everything else is the decoder's. A stream is one or more members back to back; FEXTRA, FNAME, FCOMMENT and
 * FHCRC are parsed and checked against the stream's end, FHCRC against the header's bytes; every member's CRC-32 and ISIZE are
 * verified against the bytes it produced, on the device too; stored, fixed and dynamic blocks are taken, with zlib's rules
 * for code lengths (over-subscribed and incomplete sets refused, but for a set whose only code has length 1 and a distance
 * set without codes); a match needs 1 <= distance <= bytes produced by its member; all members together must produce exactly
 * the expected bytes and consume exactly the input. A corrupt stream is PH_EINVAL "a corrupt GZIP stream" naming column,
 * row group and page. Stricter than pyarrow's codec on purpose: zlib framing (RFC 1950) and raw DEFLATE are refused, and so is
 * output short of the expected length. */
#define PH_PARQUET_GZIP 64u /* inflate GZIP pages instead of refusing them */
/* host only: one GZIP stream (one or more members), decoded by the host twin of the device decoder. The caller states
 * expected; dst has room for expected. *produced is set to the bytes written (== expected on PH_OK). PH_EINVAL: a corrupt
 * stream (ph_last_error names the sub-case), fewer than 20 bytes, or expected > 1032 * src_bytes. */
int ph_gzip_decompress_host(const void *src, int64_t src_bytes, void *dst, int64_t expected, int64_t *produced);
/* n independent streams on the device, by the kernel the Parquet load uses; same contract as ph_snappy_decompress
 * (host position / length arrays, 16-byte-unit reads, status[i], zeros for a refused stream; a stream that fails only
 * its CRC-32 is refused like any other). */
int ph_gzip_decompress(ph_ctx *ctx, const void *src_dev, const int64_t *src_pos, const int64_t *src_bytes, void *dst_dev,
                       const int64_t *dst_pos, const int64_t *dst_bytes, int32_t n, int32_t *status);
/* ---- ZSTD pages, decompressed on the device (opt-in)
 * With PH_PARQUET_ZSTD a chunk whose codec is ZSTD (parquet.thrift CompressionCodec 6: RFC 8878 frames) is decoded instead of
 * refused, by the plumbing the other three codecs take: the same per-page streams, one kernel launch per codec present, the
 * same region behind the upload, the same "lowest failing page" order. The flag composes with the other four (a file whose
 * columns are ZSTD, GZIP, SNAPPY, LZ4_RAW and UNCOMPRESSED loads with 1 | 16 | 64 | 256; delta pages inside ZSTD chunks are
 * decompressed first). The valid words are every OR of 1, 4, 16, 64 and 256 (and of 1024, PH_PARQUET_DELTA_BYTE_ARRAY below). Without the flag every code and message is what
 * it was; with it, a codec that is still refused (BROTLI, LZO, codec 5) reads ZSTD among the codecs that are decoded.
 *   What a stream must produce comes from the page header alone. The host refuses, before anything is allocated: a stream of
 * 0 bytes for more than 0 bytes; a non-empty stream of fewer than 9 bytes (magic, descriptor, one more header byte, a last
 * block's 3-byte header); one that begins with neither the frame magic 28 b5 2f fd nor a skippable frame's 5? 2a 4d 18; a
 * length above 32768 times the stream's bytes (an RLE block makes 128 KiB from 4 bytes): PH_EINVAL. Everything else is the
 * decoder's, all of RFC 8878 but dictionaries: one or more frames, skippable frames stepped over; every header field and
 * content-size width, a Frame_Content_Size checked against what its frame produced, a Content_Checksum (XXH64) verified, on
 * the device too; raw, RLE and compressed blocks; literals of every type and size format, Huffman weights direct and
 * FSE-compressed; sequences in every mode with the repeat-offset rules. A non-zero Dictionary_ID, a reserved bit, block type
 * 3, a missing final-bit marker and a bitstream that is not consumed exactly are refused; a match needs 1 <= offset <= bytes
 * produced by its frame (the window size is not enforced beyond that, as in libzstd's one-shot decoder); all frames together
 * must produce exactly the expected bytes and consume exactly the input. A corrupt stream is PH_EINVAL "a corrupt ZSTD
 * stream" naming column, row group and page. Stricter than libzstd's one-shot decoder on purpose: Huffman codes of 12 bits (RFC 8878 allows 11) and
 * blocks above Block_Maximum_Size (a Block_Size, or what a compressed block regenerates) are refused. */
#define PH_PARQUET_ZSTD 256u /* decompress ZSTD pages instead of refusing them */
/* host only: one ZSTD stream (one or more frames), decoded by the host twin of the device decoder. The caller states
 * expected; dst has room for expected. *produced is set to the bytes written (== expected on PH_OK). PH_EINVAL: a corrupt
 * stream (ph_last_error names the sub-case), fewer than 9 bytes, or expected > 32768 * src_bytes. */
int ph_zstd_decompress_host(const void *src, int64_t src_bytes, void *dst, int64_t expected, int64_t *produced);
/* host only: what one ZSTD stream is made of, counted by the host twin: stats[0] = literal bytes (raw and RLE blocks
 * included), [1] = sequences, [2] = match bytes, [3] = match bytes whose offset is above far_limit. */
int ph_zstd_stream_stats_host(const void *src, int64_t src_bytes, int64_t expected, int64_t far_limit, int64_t *stats);
/* n independent streams on the device, by the kernel the Parquet load uses; same contract as ph_snappy_decompress
 * (host position / length arrays, 16-byte-unit reads, status[i], zeros for a refused stream; a stream that fails only
 * its checksum is refused like any other). */
int ph_zstd_decompress(ph_ctx *ctx, const void *src_dev, const int64_t *src_pos, const int64_t *src_bytes, void *dst_dev,
                       const int64_t *dst_pos, const int64_t *dst_bytes, int32_t n, int32_t *status);
/* ---- delta-encoded pages, decoded on the device (opt-in)
 * With PH_PARQUET_DELTA a data page (v1 or v2) whose values are DELTA_BINARY_PACKED is decoded when the column's physical type
 * is INT32 or INT64 — into every type those map to above, overrides and the PH_I32-over-INT64 range rule included — and a
 * page whose values are DELTA_LENGTH_BYTE_ARRAY when it is BYTE_ARRAY. Everything promised above holds for such pages: the
 * same table, zeroed NULL slots and padding, statistics and narrowed copies, the "lowest failing page" rule; a chunk may mix
 * dictionary, PLAIN and delta pages; the flag composes with PH_PARQUET_SNAPPY (compressed delta pages are decompressed first,
 * like any other). DELTA_BYTE_ARRAY (it has a flag of its own, PH_PARQUET_DELTA_BYTE_ARRAY below, and this one does not enable
 * it), BYTE_STREAM_SPLIT and a delta encoding over a type it is not defined for stay
 * PH_EUNSUPPORTED naming the encoding. Without the flag every code and message is what it was. Bit 1 of the flags word is
 * not defined: of bits 0..2 the valid words are 0, 1, 4 and 5.
 *   The stream (parquet-format, Encodings.md): block_size, miniblocks per block, total_count as ULEB128 and first_value as
 * zigzag ULEB128 (64 bits, up to 10 bytes); per block min_delta (zigzag ULEB128), one width byte per miniblock, and the
 * miniblocks, block_size / miniblocks values of `width` bits each, LSB first. value[i] = value[i-1] + min_delta + delta modulo
 * 2^64; an INT32 column keeps the low 32 bits. A miniblock of the last block that holds no value has no bytes and its width
 * byte is ignored; the last one that holds a value is stored whole. PH_EINVAL: block_size 0 or no multiple of 128, 0
 * miniblocks, values per miniblock no multiple of 32, a varint above 10 bytes / 64 bits, a needed miniblock's width above
 * the type's bits (32 / 64), a varint, width array or needed miniblock that leaves the values section ("a malformed
 * DELTA_BINARY_PACKED header or miniblock"); total_count other than the page's count of non-NULL values, or bytes left
 * behind the last needed miniblock of an integer page (the count message PLAIN pages have). A page without a non-NULL value
 * may have an empty values section. PH_EUNSUPPORTED: block_size above 65536 or more than 512 miniblocks — a block's header
 * is staged whole on the device, and those are its limits (writers use 128 or 256 values and 4 miniblocks).
 *   DELTA_LENGTH_BYTE_ARRAY: one such stream of INT32 lengths, then the bytes of all values back to back. A negative length or
 * lengths that sum past the page's end -> the BYTE_ARRAY length message; a sum short of the page's end -> the count message. */
#define PH_PARQUET_DELTA 4u    /* decode DELTA_BINARY_PACKED / DELTA_LENGTH_BYTE_ARRAY pages instead of refusing them */
/* One raw DELTA_BINARY_PACKED stream, for tests and tools: in, the stream and what is expected of it; out, what it held. */
typedef struct {
    int64_t src_pos, src_bytes; /* in: the stream inside the source buffer */
    int32_t bits;               /* in: 32 or 64, the column type's bits (the widest legal miniblock; 32 wraps and sign-extends) */
    int32_t exact;              /* in: 1 = the stream must end at src_bytes as an integer page's does (else PH_EINVAL) */
    int64_t expected;           /* in: the count the header must state (else PH_EINVAL); -1 = any count up to dst_cap */
    int64_t dst_pos, dst_cap;   /* in: where the values go in the destination, in VALUES, and the room there */
    int64_t count;              /* out: the count the header states (0 when the header is unreadable) */
    int64_t consumed;           /* out: bytes from src_pos to behind the last needed miniblock (valid streams) */
    int32_t status;             /* out: PH_OK; PH_EINVAL; PH_EUNSUPPORTED (the two limits); PH_ECAPACITY (count > dst_cap) */
    int32_t sub;                /* out: which rule the stream broke (ph_delta_decode_host's message names it) */
} ph_delta_stream;
/* host only: ONE stream, src + s->src_pos, decoded by the host twin of the device decoder into dst[dst_pos ..) (int64 each).
 * dst may be NULL when dst_cap is 0. Returns s->status; ph_last_error names the sub-case. Only dst[dst_pos, + count) is
 * written, and only for a stream that is PH_OK or is refused behind its header (values in front of the fault may be there). */
int ph_delta_decode_host(const void *src, int64_t *dst, ph_delta_stream *s);
/* n independent streams on the device, one workgroup each, by the device function the page kernels run. src_dev / dst_dev
 * (int64 values) are device buffers, streams a host array. Returns PH_OK when it ran, whatever the streams held. */
int ph_delta_decode(ph_ctx *ctx, const void *src_dev, void *dst_dev, ph_delta_stream *streams, int32_t n);
/* ---- DELTA_BYTE_ARRAY pages (front coding), decoded on the device (opt-in)
 * With PH_PARQUET_DELTA_BYTE_ARRAY (bit 10 of the flags word; bit 9, 512, stays undefined) a data page (v1 or v2) whose values
 * are DELTA_BYTE_ARRAY is decoded when the column's physical type is BYTE_ARRAY. The flag stands alone: it does not enable
 * DELTA_BINARY_PACKED or DELTA_LENGTH_BYTE_ARRAY pages (PH_PARQUET_DELTA does, and the two compose), it composes with every
 * codec flag (a compressed page is decompressed first, like any other), and a chunk may mix dictionary, PLAIN, delta and
 * front-coded pages. The valid words are every OR of 1, 4, 16, 64, 256 and 1024. DELTA_BYTE_ARRAY over FIXED_LEN_BYTE_ARRAY or
 * any other type stays PH_EUNSUPPORTED naming the encoding and the physical type, BYTE_STREAM_SPLIT stays PH_EUNSUPPORTED
 * naming the encoding: both are out of scope. Without the flag every code and message is what it was.
 *   The stream (parquet-format, Encodings.md): the values section is one DELTA_BINARY_PACKED stream of INT32 prefix lengths,
 * and behind it a DELTA_LENGTH_BYTE_ARRAY section of the suffixes (a DELTA_BINARY_PACKED stream of INT32 suffix lengths, then
 * the suffixes' bytes back to back, which end at the page's end). value[k] = value[k-1][0 .. prefix[k]) + suffix[k]; the value
 * in front of value[0] is the empty string, so pages are independent of each other.
 *   Rules, each failure naming column, row group and page by the "lowest failing page" rule, judged in this order on the host
 * twin and on the device alike: the prefix stream (its total_count must equal the page's count of non-NULL values: the count
 * message; a malformed header or miniblock keeps PH_PARQUET_DELTA's causes and limits; a negative prefix is the prefix
 * message); the suffix-length stream (likewise; a negative suffix length is the BYTE_ARRAY length message); prefix[k] above
 * the length of value[k-1] -> PH_EINVAL "a DELTA_BYTE_ARRAY prefix longer than the value in front of it" (a non-zero
 * prefix[0] is this case); suffix lengths that sum past the page's end -> the BYTE_ARRAY length message, a sum short of it ->
 * the count message. Lengths are summed in 64 bits, and a column whose values reach 2^31 bytes is the PH_EINVAL of every
 * VARCHAR column, judged from the lengths alone BEFORE the byte buffer is allocated or a byte is moved. A page without a
 * non-NULL value may have an empty values section.
 *   Front coding is the one encoding where a small page legitimately expands by orders of magnitude (70 000 values whose
 * prefixes are 0, 1, 2, ... take a few kilobytes and state 2.4 GB). So for such columns "device memory is bounded by the
 * file's size" reads "bounded by the 2^31 column rule": the per-value temporaries are sized by the file's ROWS, the bytes by
 * the lengths the first pass has summed and checked. */
#define PH_PARQUET_DELTA_BYTE_ARRAY 1024u /* decode DELTA_BYTE_ARRAY pages of BYTE_ARRAY columns instead of refusing them */
/* One raw DELTA_BYTE_ARRAY values section, for tests and tools: in, the section and the rooms; out, what it held. */
typedef struct {
    int64_t src_pos, src_bytes; /* in: the section inside the source buffer; it must end where its suffix bytes end */
    int64_t expected;           /* in: the count both streams must state (else PH_EINVAL); -1 = any count up to len_cap */
    int64_t len_pos, len_cap;   /* in: where the int32 lengths go in the lengths destination, in VALUES, and the room there */
    int64_t byte_pos, byte_cap; /* in: where the values' bytes go in the bytes destination, in BYTES, and the room there */
    int64_t count;              /* out: the count the prefix stream's header states (0 when it is unreadable) */
    int64_t total_bytes;        /* out: the bytes all values hold, summed in 64 bits; known once every rule but the rooms holds,
                                 * so also with PH_ECAPACITY for the bytes and with the 2^31 PH_EINVAL; else 0 */
    int64_t consumed;           /* out: src_bytes for a section that is PH_OK, else 0 */
    int32_t status;             /* out: PH_OK; PH_EINVAL; PH_EUNSUPPORTED (the delta limits); PH_ECAPACITY (count > len_cap or
                                 * total_bytes > byte_cap: nothing outside the rooms is written, and no byte at all) */
    int32_t sub;                /* out: which rule was broken (ph_delta_byte_array_decode_host's message names it): 0 none;
                                 * 1..12 ph_delta_stream's sub-case in the prefix stream, 32 + that in the suffix-length stream;
                                 * 64 a prefix above the value in front of it or negative, 65 a negative suffix length, 66 suffix
                                 * bytes past the section's end, 67 short of it, 68 byte_cap too small, 69 2^31 bytes or more */
} ph_dba_stream;
/* host only: ONE section, src + s->src_pos, decoded by the host twin of the device decoder: lens[len_pos, + count) and
 * bytes[byte_pos, + total_bytes), the values back to back. Either destination may be NULL when its room is 0. The per-value
 * temporaries are sized by len_cap, never by a number of the stream, so count > len_cap reports count and no total_bytes.
 * Returns s->status; ph_last_error names the sub-case. */
int ph_delta_byte_array_decode_host(const void *src, int32_t *lens, char *bytes, ph_dba_stream *s);
/* n independent sections on the device, by the device functions the load itself runs: the lengths pass of the page kernel (one
 * workgroup a section), then the reconstruction kernel (one wave a section) over the sections that passed. src_dev, lens_dev
 * (int32) and bytes_dev are device buffers, streams a host array. src_dev is read in whole aligned 16-byte units, as
 * ph_snappy_decompress reads it. Returns PH_OK when it ran, whatever the sections held. */
int ph_delta_byte_array_decode(ph_ctx *ctx, const void *src_dev, void *lens_dev, void *bytes_dev, ph_dba_stream *streams, int32_t n);
/* dictionary of a PH_CODE8 column (code -> string), for callers that did not build it themselves */
int32_t ph_table_dict_size(const ph_table *t, int32_t c);
const char *ph_table_dict_entry(const ph_table *t, int32_t c, int32_t code);

/* Order statistics gathered at load like min / max (one pass per integer column without NULLs), and what the
 * catalog declares. They are what a planner's choice of table form rests on (ph_plan below; ph_join_build_ex's
 * hints): PH_STAT_ASCENDING = values non-decreasing in storage order (a clustering column: lineitem by
 * l_orderkey), PH_STAT_STRICT = strictly ascending (a primary key stored in key order),
 * PH_STAT_DECLARED_UNIQUE = ph_table_declare_unique named this single column. */
#define PH_STAT_ASCENDING 1
#define PH_STAT_STRICT 2
#define PH_STAT_DECLARED_UNIQUE 4
int ph_table_col_stats(const ph_table *t, int32_t c, int32_t *flags);
/* > 0: the column is ascending in runs of this ONE length over consecutive values — row i holds min + i / run_len (PARTSUPP by ps_partkey: four
 * suppliers per part) — so the rows of a key are found by arithmetic (ph_join_run_lookup). Measured at load like the order; 0 = not that shape.
 * Only run lengths 2..64 are reported: a strictly ascending column (runs of one row) and runs longer than 64 rows report 0. */
int32_t ph_table_col_run_len(const ph_table *t, int32_t c);
/* Frame-of-reference narrowed copies, built at load beside the columns: a NULL-free PH_I32 / PH_DATE / PH_I64 /
 * PH_DEC64 column whose max - min fits in fewer bytes than its width also gets code = value - min as uint8 / uint16 / uint32. The
 * fused scans (ph_scan_plan_bytes_per_row) read the copies; every other call reads the column itself. PH_NARROW=0 in the
 * environment builds none and plans ignore them. ph_table_col_narrow: 1 with *width (1, 2 or 4) and *base (the column minimum) set
 * when column c has a copy, 0 when it has none. ph_table_narrow_bytes: device bytes the copies of the table hold. */
int ph_table_col_narrow(const ph_table *t, int32_t c, int32_t *width, int64_t *base);
int64_t ph_table_narrow_bytes(const ph_table *t);
/* the catalog's PRIMARY KEY / UNIQUE constraint over 1..4 columns of the table (cases/tpch/query/ddl.sql: every
 * TPC-H table declares one). A join whose build key covers a declared-unique set is N:1. Trusted, like the
 * reference trusts its catalog; a lookup that meets two build rows for one key reports it (PH_ECONSTRAINT). */
int ph_table_declare_unique(ph_table *t, int32_t ncols, const int32_t *cols);
/* A co-located copy of 2..8 fixed-width columns without NULLs: row r of the copy holds the columns' values of row r side
 * by side (widest first, the row padded to a power of two up to 64 bytes), beside the column arrays, which stay. It serves
 * ph_gather_multi (and with it the late materialisation of ph_plan): the reference's row-format TupleDataCollection
 * (join_collection.go:268-529) for exactly the columns that are fetched together by row id. A host that knows such a set
 * (the planner: the probe-side columns that survive a selective join) calls this at load; without it the library builds
 * the copy itself the SECOND time the same set of three or more columns of a table is gathered at no more than an eighth of
 * its rows (PH_COLOCATE=0 switches both off). Costs stride x rows bytes of HBM and one pass. */
int ph_table_colocate(ph_table *t, int32_t ncols, const int32_t *cols);
/* 1 when a co-located copy covers the given columns */
int32_t ph_table_colocated(const ph_table *t, int32_t ncols, const int32_t *cols);
/* What the library may spend ON ITS OWN on copies of this table's columns — ONE budget for both kinds it builds by itself, the co-located
 * copies above and the packed scan groups below: `bytes` of HBM in all, default 4 GiB; 0 = never (the host's veto; copies asked for by
 * name with ph_table_colocate / ph_table_pack_scan_group are the host's decision and not limited). A build that would exceed the budget
 * is skipped and the consumer reads the column arrays. ph_table_colocate_bytes: what the co-located copies hold now. */
int ph_table_set_colocate_budget(ph_table *t, int64_t bytes);
int64_t ph_table_colocate_bytes(const ph_table *t);
/* A packed scan group: for the seven columns a lowcard_chain plan reads — cols = the predicate column, then q, e, d, t,
 * then the two group columns — one uint64 per row (8 bytes a row, padded like the columns) that holds the narrowed copies' codes
 * (value - min, bitlen(max - min) bits each, at least 1) and the dense group slot k0 nk1 + k1, placed first fit, largest first, into
 * the word's two dwords so that no field straddles them. A plan that takes the lean instance ("narrow32_lean") reads the word instead
 * of the seven arrays once the group exists ("packed64", 8 instead of 11 bytes a row for TPC-H Q1); results are the same integers.
 * PH_EUNSUPPORTED (the reason in ph_last_error) when a column is NULL-able, of another type or without a narrowed copy of the lean
 * instance's width (2, 1, 4, 1, 1 bytes), when the group columns are not NULL-free codes inside their dictionaries with at most 12
 * slots, or when the fields do not fit. Without this call the library builds the group itself when lean plans have scanned the set
 * twice the table's rows (the second full scan), provided the set's narrowed columns exceed the device's last-level cache (256 MiB;
 * below it back-to-back scans are served on-die; PH_SCAN_PACK_MIN_BYTES in the environment, read at every run, overrides the
 * threshold) and the copy fits ph_table_set_colocate_budget. PH_SCAN_PACK=0 (read once per process) switches the automatic build and
 * the plans' use of any group off. Over a group in TPC-H lineitem's layout the scan bins the price codes by (slot, tax, discount)
 * instead of multiplying per row (ph_scan_plan_row_body; PH_SCAN_HIST=0, read at every run, switches that off). Built by one kernel
 * on the calling ctx's stream under the table's mutex, ordered against other consumers by an event, like a co-located copy.
 * ph_table_scan_group_bytes: what the groups hold now (not part of ph_table_narrow_bytes or ph_table_colocate_bytes). */
int ph_table_pack_scan_group(ph_table *t, int32_t ncols, const int32_t *cols);
int64_t ph_table_scan_group_bytes(const ph_table *t);
/* The same with the group's form named: PH_SCAN_GROUP_WORD64 is ph_table_pack_scan_group; PH_SCAN_GROUP_SPLIT56 (TPC-H lineitem's
 * layout only, else PH_EUNSUPPORTED) stores the word's low dword and the 24 used bits of its high dword apart, in blocks of 1024 rows:
 * 7 bytes a row ("split56"), the same integers. A column set has one group: asking for one form where the other exists is
 * PH_EUNSUPPORTED. The library's own build takes the split form when the layout is lineitem's, PH_SCAN_PACK_GENERIC is off and the
 * 64-bit group would exceed the last-level cache (PH_SCAN_SPLIT_MIN_BYTES, read at every run, overrides the 256 MiB). PH_SCAN_SPLIT=0
 * (read at every run): a split group is neither built nor bound by a plan. */
#define PH_SCAN_GROUP_WORD64 0
#define PH_SCAN_GROUP_SPLIT56 1
int ph_table_pack_scan_group_ex(ph_table *t, int32_t ncols, const int32_t *cols, int32_t form);
/* The layout rule of the packed scan groups, without a device: shifts[i] (0..63) for nfields fields of widths[i] bits (1..32), or
 * PH_EUNSUPPORTED when they do not fit two dwords by first fit, largest first. ph_pack_scan_bits: the bits of a field for codes 0..span. */
int ph_pack_scan_layout(int32_t nfields, const int32_t *widths, int32_t *shifts);
int32_t ph_pack_scan_bits(uint64_t span);
/* ---- concatenation of resident tables, on the device
 * A table usually arrives in pieces: a directory of Parquet files or of dbgen .tbl chunks, a file larger than the host wants to
 * hold at once, the reference's tables that grow by INSERT and by repeated COPY. Each piece is loaded by any of the loaders
 * above; ph_table_concat then builds ONE new table from the N resident pieces without the host seeing a row again. Tables are
 * immutable after load (see Sharing below), so this is no in-place append. The result is the table ph_table_create would build
 * over the same values in the same order: data, zeroed padding, validity bits, dictionary, offsets and bytes, min / max, order
 * and run statistics, narrowed copies.
 *
 * Parts — 1 <= nparts <= 65536 (PH_EINVAL otherwise). Every part is non-NULL and lives on ctx's device (PH_EINVAL); a part
 * created on another ctx of that device is fine. A part may be named more than once. Parts are only read: they stay valid and
 * unchanged. The result belongs to ctx, is registered like any table and is complete when the call returns. Row order: all
 * rows of parts[0], then parts[1], and so on; a part of 0 rows contributes no rows, all parts empty gives a table of 0 rows.
 * 2^31 rows or more in all -> PH_EINVAL "rows exceed the int32 row-id domain", judged before anything is allocated.
 *
 * Schema — every part has the same number of columns, and per column the parts have the same type and scale, with ONE
 * exception: PH_CODE8 and PH_STR are both VARCHAR and may mix. Anything else is PH_EINVAL; ph_last_error names the column, the
 * part and the two types (or scales).
 *
 * Fixed-width columns (PH_I32, PH_I64, PH_DATE, PH_DEC64, PH_F32, PH_F64): the values laid end to end, the padding zeroed.
 * Validity: the result column has a bitmap if and only if at least one part has one; parts without one contribute ones; bits
 *   at and beyond the total row count are 0.
 * All parts PH_CODE8: when every part's dictionary has the same entries in the same order, the dictionary is kept as it is and
 *   the codes are copied (a caller's own order survives). Otherwise the merged dictionary is the union of the parts' entries in
 *   unsigned byte order, the loaders' order (a duplicate inside one part's dictionary maps to the one merged entry; a part of 0
 *   rows still contributes its entries). Up to 256 merged entries the column stays PH_CODE8 and each code is rewritten through
 *   its part's 256-entry table; a NULL row's code is 0 whatever the part stored. More than 256 merged entries make the column
 *   PH_STR: every row becomes its dictionary entry, a NULL row the empty string (not entry 0).
 * Any part PH_STR: the result is PH_STR, code parts expanded as above. Lengths are taken per row (off[i + 1] - off[i]), so a
 *   part's offsets need not start at 0 nor be dense; the result's offsets are dense and start at 0. 2^31 string bytes or more in
 *   one column -> PH_EINVAL.
 * Statistics: each column is finished over the NEW arrays exactly as ph_table_create finishes one, so range, ascending /
 *   strict, run length and the narrowed copy are the concatenation's own. NOT carried over from the parts: declared unique keys
 *   (two unique parts need not be unique together), co-located copies, packed scan groups, the replicated flag and the
 *   co-location budget. The caller declares them again on the result.
 * Failures: PH_EHIP when device memory runs out. On any failure no table is returned, the parts are untouched and the context
 * stays usable.
 *
 * The work does not depend on the number of parts in launches or read-backs: one launch per array over tiles of the output,
 * which find their parts by binary search in a small device table of {source, first output row}; one read-back per VARCHAR
 * column that becomes PH_STR (its byte total), none for the others beyond what the finishing does. */
int ph_table_concat(ph_ctx *ctx, const ph_table *const *parts, int32_t nparts, ph_table **out);
/* host only, no device: the concatenation of nparts validity bitmaps (LSB first, 1 = valid) of rows[p] rows each, by the same
 * __host__ __device__ function that computes one 32-bit word of the result in the kernel. bitmaps[p] = NULL: every row of part p
 * is valid; rows[p] = 0 is allowed. Writes (total + 7) / 8 bytes with the last byte's unused bits 0, and zeroes the rest of
 * out up to out_bytes. PH_ECAPACITY when out_bytes is smaller than that. */
int ph_validity_concat_host(int32_t nparts, const uint8_t *const *bitmaps, const int64_t *rows, uint8_t *out, int64_t out_bytes);
/* host only: ph_table_concat's dictionary rule over nparts dictionaries given as ph_col.aux of PH_CODE8 gives them (NUL-separated
 * entries, at most 256 each; blob_bytes[p] = 0 is the empty dictionary). *identical = 1: all parts have the same entries in the
 * same order, merged is that dictionary and the tables are the identity. Else merged is the union in unsigned byte order.
 * *nmerged entries, *merged_bytes bytes (each entry with its NUL), written to merged when they fit merged_cap (else
 * PH_ECAPACITY, the counts still set). remap: nparts x 256 bytes, remap[p * 256 + code] = the merged code of part p's `code`
 * (0 for a code the part's dictionary does not have) — all 0 when *nmerged > 256, where no code can name the entries and
 * ph_table_concat makes the column PH_STR. */
int ph_dict_merge_host(int32_t nparts, const char *const *blobs, const int64_t *blob_bytes, char *merged, int64_t merged_cap,
                       int64_t *merged_bytes, int32_t *nmerged, uint8_t *remap, int32_t *identical);
/* Sharing (SURVEY.md §8(b) "threading"; the psql server path, cmd/main/main.go:71-122: every connection plans and runs its own query
 * over the same storage). A resident table may be read by plans and operator calls on ANY ctx of its device, from several threads at
 * once: columns, statistics and declared keys are immutable once loading is done (ph_table_create* / ph_table_declare_unique /
 * ph_table_colocate / ph_table_pack_scan_group belong to the load phase, one thread); the only state a query may add — an automatic
 * co-located copy or packed scan group, and the counts that trigger them — is guarded by a mutex inside the table, built on the calling ctx's stream and ordered against every other consumer's stream by an event. The
 * ctx rule stands: ONE thread at a time per ctx; concurrent queries take a ctx each. ph_table_free: when no plan reads the table. */
void ph_table_free(ph_table *t);

/* plain device buffers for callers without their own allocator */
int ph_dev_alloc(ph_ctx *ctx, int64_t bytes, void **dev);
int ph_dev_free(ph_ctx *ctx, void *dev);
/* n buffers in one call (the end of a query plan frees dozens of intermediates: one FFI crossing) */
int ph_dev_free_many(ph_ctx *ctx, void *const *devs, int64_t n);
int ph_dev_upload(ph_ctx *ctx, void *dev, const void *host, int64_t bytes);
int ph_dev_download(ph_ctx *ctx, void *host, const void *dev, int64_t bytes);
int ph_dev_memset(ph_ctx *ctx, void *dev, int value, int64_t bytes);

/* ------------------------------------------------------------------ filter
 * ExprExec.executeSelect / selectOperation / selectFlatLoop
 * (pkg/compute/expr_exec.go:342-486, function_operator_boolean.go:393-521, 780-868):
 * one comparison `col OP const`, optionally narrowing an input selection (the AND chain of
 * execSelectAnd). Output: ascending row ids, wavefront-ballot compacted.
 * The (type, op) pairs the reference does not implement select nothing, as there. */
typedef enum { PH_EQ = 1, PH_NE, PH_LT, PH_LE, PH_GT, PH_GE, PH_LIKE, PH_NOTLIKE } ph_cmp;

/* A dictionary-code column (PH_CODE8) takes the CODE of a string literal as a PH_I32 constant ('=' / '!='), or — type
 * PH_CODE8, op PH_EQ — a RUN of codes i .. scale: what `LIKE 'prefix%'` or a sorted IN list is over a dictionary in
 * byte order. */
typedef struct {
    int32_t type;  /* PH_I32, PH_DATE, PH_F32 (decimal column vs float literal), PH_DEC64, PH_STR */
    int32_t scale;
    int64_t i;
    double f;
    const char *s; /* host string: '=' operand or LIKE pattern */
} ph_const;

/* col: device column of n rows. sel_in (dev, may be NULL = identity over n rows), n_in rows.
 * sel_out: dev buffer of >= n_in int32. *n_out (host) receives the count (synchronises). */
int ph_filter_select(ph_ctx *ctx, const ph_col *col, int64_t n, int32_t op, const ph_const *k,
                     const int32_t *sel_in, int64_t n_in, int32_t *sel_out, int64_t *n_out);

/* Two conjuncts `col OP1 k1 AND col OP2 k2` over ONE column in one pass (a date range: execSelectAnd, expr_exec.go:430-486, runs the second over
 * the first's selection). Both must lower to value ranges of one kind (integer / date / decimal orderings, '=', a dictionary code);
 * PH_EUNSUPPORTED otherwise — run them one after the other with ph_filter_select. Same outputs as ph_filter_select. */
int ph_filter_select_and(ph_ctx *ctx, const ph_col *col, int64_t n, int32_t op1, const ph_const *k1, int32_t op2, const ph_const *k2,
                         const int32_t *sel_in, int64_t n_in, int32_t *sel_out, int64_t *n_out);

/* `col IN (v1 .. vk)` in one pass (InExpr = an OR of equalities: execSelectOr, expr_exec.go:488-530, runs k passes and a union). INTEGER columns and
 * (k <= 16) and dictionary-code columns (values = codes, any number: what a LIKE over a dictionary selects); PH_EUNSUPPORTED otherwise (the
 * caller unites ph_filter_select results with ph_sel_union). */
int ph_filter_select_in(ph_ctx *ctx, const ph_col *col, int64_t n, const int64_t *values, int32_t nvalues, const int32_t *sel_in, int64_t n_in,
                        int32_t *sel_out, int64_t *n_out);

/* column OP column over the same rows (selectBinary with two FLAT vectors, function_operator_boolean.go:506-521),
 * e.g. Q4 / Q12's l_commitdate < l_receiptdate. The (type, op) pairs are selectOperation's: INTEGER all six, DATE
 * the four orderings, DECIMAL (one scale) '>' only; the pairs the reference does not implement select nothing. */
int ph_filter_select_cols(ph_ctx *ctx, const ph_col *a, const ph_col *b, int64_t n, int32_t op, const int32_t *sel_in,
                          int64_t n_in, int32_t *sel_out, int64_t *n_out);

/* out_dev[i] = i for i < n; marks_dev[sel_dev[i]] = 1 for i < n (bytes; the caller clears them first): the two small device helpers a shim needs to
 * turn a filtered pair list into marks of its probe rows (a join with a residual condition, as ph_plan does it) */
int ph_dev_iota(ph_ctx *ctx, int32_t *out_dev, int64_t n);
int ph_sel_mark(ph_ctx *ctx, const int32_t *sel_dev, int64_t n, uint8_t *marks_dev);
/* The operators' own exclusive scan, in place: dev[i] = dev[0] + .. + dev[i - 1] for i < n, *total_dev (device, 8 bytes) = the sum of all n.
 * The values are counts: none negative, their total below 2^31. */
int ph_dev_exclusive_scan_i32(ph_ctx *ctx, int32_t *dev, int64_t n, int64_t *total_dev);

/* OR of predicates = union of their selections: execSelectOr (expr_exec.go:488-530), which is
 * also how `a IN (x, y, ...)` runs (in(a,x) OR in(a,y) ..., `in` selecting like `=`,
 * function_operator_boolean.go:419-429). sels_dev[i] (device, counts[i] ascending row ids < n_rows)
 * are the children's selections, each produced by ph_filter_select over the same input; the
 * output is their union in ascending order (the reference emits it child by child; the row set
 * is the same). out_sel_dev: >= min(n_rows, sum counts) int32. */
int ph_sel_union(ph_ctx *ctx, const int32_t *const *sels_dev, const int64_t *counts, int32_t k,
                 int64_t n_rows, int32_t *out_sel_dev, int64_t *n_out);

/* falseSel of a predicate: the rows of the parent selection (NULL = identity over n_rows) that
 * the child selection does not contain, ascending — what execSelectExpr hands back next to the
 * true rows and executeCase continues with (expr_exec.go:144-246: curSel = curFalseSel). */
int ph_sel_difference(ph_ctx *ctx, const int32_t *parent_dev, int64_t n_parent, const int32_t *child_dev,
                      int64_t n_child, int64_t n_rows, int32_t *out_sel_dev, int64_t *n_out);
/* FillSwitch / TemplatedFillLoop (expr_exec.go:559-606): out[sel[i]] = values[i] for a positional
 * value column (PH_I32 or PH_DEC64 — the two result types FillSwitch handles; n rows), i.e. a CASE branch's THEN/ELSE results written
 * back at the rows the branch selected. out_validity_dev (optional bitmap, zeroed by the caller
 * before the first branch) gets the bit of every row whose value is non-NULL. CASE on the device
 * = ph_filter_select (WHEN) -> ph_expr_eval over the true rows -> ph_scatter, then the same for
 * the next WHEN / the ELSE over ph_sel_difference's rows. */
int ph_scatter(ph_ctx *ctx, const ph_col *values, const int32_t *sel_dev, int64_t n, void *out_data_dev,
               uint8_t *out_validity_dev);

/* ------------------------------------------------------------------ hash
 * Chunk.Hash / HashTypeSwitch / CombineHashTypeSwitch (pkg/chunk/chunk.go:160-166,
 * hash.go:26-41, 182-413; util.HashBytes pkg/util/hash.go:13-65) — bit-identical values.
 * PH_CODE8 columns need `dict_hashes` (dev uint64 per code = HashBytes of the string). */
int ph_hash(ph_ctx *ctx, const ph_col *cols, const uint64_t *const *dict_hashes, int32_t ncols,
            int64_t n, uint64_t *out_dev);
/* host helper: HashBytes of one string (for building dict_hashes) */
uint64_t ph_hash_bytes(const void *p, uint64_t len);

/* ------------------------------------------------------------------ decimal expressions
 * ExprExec.executeExprs over DECIMAL/INTEGER operands (expr_exec.go:85-340;
 * function_operator_binary.go:134-207). Values are exact unscaled int64 at a scale fixed by the
 * binder's typing rules (Mul: sum of scales, Add/Sub: max; function_scalar.go:37-84, 429-475).
 * Program = RPN over columns and literals. */
typedef enum { PH_X_COL = 1, PH_X_CONST, PH_X_ADD, PH_X_SUB, PH_X_MUL,
               PH_X_DIV, PH_X_LT, PH_X_LE, PH_X_GT, PH_X_GE /* ph_float_eval only */ } ph_xop;

typedef struct {
    int32_t op;
    int32_t col;   /* PH_X_COL: index into cols (PH_DEC64 or PH_I32/PH_I64 = scale 0) */
    int64_t ival;  /* PH_X_CONST: unscaled value */
    int32_t scale; /* PH_X_CONST: its scale */
} ph_rpn;

/* FLOAT / DOUBLE arithmetic and comparisons (the FLOAT and DOUBLE overloads of + - * / and of the comparison operators: function_scalar.go:476-512,
 * 960-1025, 1335-1470): the program per row in float32 — every operation rounded to it — or, wide != 0, in float64. PH_X_COL casts the column as the
 * binder does (INTEGER -> float, DECIMAL -> float64 -> float32; a HUGEINT travels as a scale-0 decimal), PH_X_CONST is a FLOAT literal (its float32
 * bits in ival; widened for DOUBLE arithmetic). Comparisons give 1 / 0 and follow selectOperation: FLOAT has > >= <=, DOUBLE has < — the others are
 * never true. out_type PH_I32: the truth value of a program that ends in a comparison (a NULL operand: 0); PH_F32: the value of a float32 program;
 * PH_F64: the value of a float64 program (wide != 0), 8 bytes a row. An integer column (PH_I32, PH_DATE, PH_I64) reaches float32 in one
 * rounding; only a decimal goes through the double.
 * out_validity_dev (value modes; required there when a column carries validity, ignored in truth mode): bit i = every operand of row i is
 * valid. The kernel stores one 64-bit word per 64 rows, so the buffer must be 8-byte aligned and hold (n + 63) / 64 * 8 bytes — more than
 * the (n + 7) / 8 of a column's bitmap; exactly that many bytes are written, and the bits past row n - 1 of the last word are 0. */
int ph_float_eval(ph_ctx *ctx, const ph_col *cols, int32_t ncols, const ph_rpn *prog, int32_t nprog, int32_t wide, const int32_t *sel, int64_t n,
                  int32_t out_type, void *out_dev, uint8_t *out_validity_dev);
/* result scale of a program (host side, no device work); PH_EUNSUPPORTED if malformed */
int ph_expr_scale(const ph_col *cols, const ph_rpn *prog, int32_t nprog, int32_t *scale);
/* out_dev[i] = value of row sel[i] (or i), unscaled at ph_expr_scale's scale. Every add/sub/mul
 * is overflow-checked on the device; if any row leaves the int64 domain the call returns
 * PH_EOVERFLOW (the reference's govalues arithmetic would start rounding there, so the caller
 * must fall back; with ph_ctx_set_deferred_errors the error is reported by the next call that
 * reads back instead). NULL inputs give a NULL result: out_validity_dev (bitmap, may be NULL when no
 * input column has validity) receives the result validity. */
int ph_expr_eval(ph_ctx *ctx, const ph_col *cols, int32_t ncols, const ph_rpn *prog,
                 int32_t nprog, const int32_t *sel, int64_t n, int64_t *out_dev,
                 uint8_t *out_validity_dev);

/* Build check without a device of the generated expression kernels (ph_expr_eval compiles the RPN
 * of batches >= 2^18 rows into straight-line code with hiprtc, cached per expression shape;
 * PH_EXPR_JIT=0 keeps the interpreter): canned shape `which` (0..2) compiles for gfx950. */
int ph_expr_jit_selfcheck(int32_t which);

/* extract(year|month|day from date) — ExtractFunc (pkg/compute/function_scalar.go:1509-1563) over a
 * PH_DATE column: out_dev[i] (int32) for row sel[i] (or i). Every int32 day count is a date (proleptic Gregorian, years -5877641 ..
 * 5881580). */
typedef enum { PH_PART_YEAR = 1, PH_PART_MONTH = 2, PH_PART_DAY = 3 } ph_datepart;
int ph_date_extract(ph_ctx *ctx, int32_t part, const ph_col *col, const int32_t *sel, int64_t n,
                    int32_t *out_dev);

/* substring(s FROM offset FOR length) — substringFunc / substringStartEnd
 * (pkg/compute/function_operator_binary.go:553-625; SubstringFunc function_scalar.go:1530-1563): byte
 * positions, 1-based, a negative offset counts from the end, a negative length reads leftwards,
 * offset 0 shortens the length by one; NULL rows give the empty string (and stay NULL through the
 * column's validity). `length` = INT64_MAX is the two-argument form: from every offset it reads to
 * the row's end (the reference passes 2^32 - 1 there, which is the same for rows below 2^31 bytes).
 * Every other int64 offset and length is accepted too and means what substringStartEnd's arithmetic
 * gives in unbounded integers — the reference itself refuses arguments beyond +-2^32 (isValidRange):
 * an offset past either end of the row is clamped to that end, a length that reaches past an end
 * stops there, and offset 0 with a length <= 1 (INT64_MIN included) reads nothing. Result: a PH_STR column over
 * rows sel[0..n) (or 0..n): out_offsets_dev (n+1 int32) and out_bytes_dev; *out_bytes = bytes
 * written (PH_ECAPACITY when out_bytes_capacity is too small; the source's aux_bytes always is
 * enough for lengths >= 0 without repeated rows). */
int ph_substring(ph_ctx *ctx, const ph_col *col, int64_t offset, int64_t length, const int32_t *sel, int64_t n,
                 int32_t *out_offsets_dev, uint8_t *out_bytes_dev, int64_t out_bytes_capacity, int64_t *out_bytes);
/* Host only: the byte range [*start, *end) ph_substring takes from a row of slen bytes; returns 0 (and 0, 0) when it is empty. */
int ph_substring_range(int64_t slen, int64_t offset, int64_t length, int64_t *start, int64_t *end);

/* ------------------------------------------------------------------ string keys
 * VARCHAR group-by / join keys that are not <= 256-value dictionaries (PH_STR columns). The reference hashes them with
 * util.HashBytes (pkg/chunk/hash.go:182-207, pkg/util/hash.go:13-65) and compares candidates byte by byte (Match,
 * pkg/compute/util_match.go:25-301) inside its group table and its join table. On the device both steps are ONE
 * primitive, string interning: every row's string is looked up in an open-addressing table keyed by the same hash and
 * verified by the same byte compare; the first row to claim a slot becomes the string's representative, and every row
 * gets the representative's ROW ID as its int32 code. Equal strings have equal codes, different strings different
 * codes (colliding hashes included: the compare decides), so ph_agg_* and ph_join_* run unchanged on the codes
 * (PH_I32 columns carrying the string column's validity), and a code leads back to the bytes (ph_table_strings).
 * ph_strdict_build: codes of rows sel[0..n) / 0..n of `col` (which must outlive the dictionary); NULL rows get -1.
 * ph_strdict_lookup: codes of another column's rows in that dictionary; absent strings and NULL rows get -2. */
typedef struct ph_strdict ph_strdict;
int ph_strdict_build(ph_ctx *ctx, const ph_col *col, const int32_t *sel, int64_t n, int32_t *codes_out_dev, ph_strdict **out);
int ph_strdict_lookup(ph_strdict *d, const ph_col *col, const int32_t *sel, int64_t n, int32_t *codes_out_dev);
void ph_strdict_free(ph_strdict *d);
/* strings of rows rows_host[0..n) of PH_STR column c of a resident table (group keys that came back as codes):
 * out_offsets n+1 int32 into out_bytes */
int ph_table_strings(ph_ctx *ctx, const ph_table *t, int32_t c, const int64_t *rows_host, int64_t n, int32_t *out_offsets, char *out_bytes,
                     int64_t out_capacity);

/* ------------------------------------------------------------------ hash aggregate
 * GroupedAggrHashTable.AddChunk/FindOrCreateGroups + UpdateStates + FinalizeStates
 * (pkg/compute/aggregate_hash.go:136-391, aggregate_exec.go:456-475,
 * function_aggr.go:420-1365). Device form: open-addressing table in HBM keyed by the packed
 * group key, LDS-staged per workgroup, 128-bit integer sums, counts, min/max; first-seen row id
 * per group so that groups come back in the reference's insertion order. */
typedef enum { PH_A_SUM = 1, PH_A_AVG, PH_A_COUNT, PH_A_MIN, PH_A_MAX, PH_A_COUNT_STAR,
               PH_A_COUNT_DISTINCT /* resident plans only (ph_plan_agg.kind): count(distinct x) — the distinct (group keys, x) rows of a side
                                      table feed the aggregate, as SinkDistinctGrouping / DistinctGrouping do (aggregate_exec.go:76-105,
                                      201-304); at the operator level the same is ph_agg_sink_masked + ph_agg_keys_dev */
} ph_aggkind;

typedef struct {
    int32_t kind;
    int32_t arg; /* index into the args given to sink; ignored for COUNT_STAR */
} ph_aggspec;

typedef struct ph_agg ph_agg;

/* key_types: PH_I32/PH_I64/PH_DATE/PH_DEC64/PH_CODE8 per key column (<= 4 keys).
 * expected_groups sizes the table initially; it is doubled when `capacity - groups <= incoming
 * rows`, the reference's own Resize rule (aggregate_hash.go:214-217). */
int ph_agg_create(ph_ctx *ctx, int32_t nkeys, const int32_t *key_types, int32_t naggs,
                  const ph_aggspec *aggs, int64_t expected_groups, ph_agg **out);
/* keys/args: device columns addressed by row id; rows = sel[0..n) or 0..n. args are PH_I32 /
 * PH_I64 / PH_DEC64 columns (validity honoured: NULL inputs are skipped, NULL keys group together).
 * `positional` != 0: args are addressed by position i instead of row id sel[i] (expression
 * results from ph_expr_eval). The first-seen row recorded for a group is row_base + the row id
 * (sel[i], or i without a selection); give row_base the rows consumed by earlier sinks. */
int ph_agg_sink(ph_agg *a, const ph_col *keys, const ph_col *args, int32_t nargs,
                const int32_t *sel, int64_t n, int32_t positional, int64_t row_base);
/* Same, but only the aggregates whose bit is set in agg_mask are updated (groups are still found
 * or created for every row) — AddChunk's `filter []int` (aggregate_hash.go:155-199), which the
 * reference uses to feed non-DISTINCT aggregates from the raw rows and each DISTINCT aggregate
 * from its own (group keys + argument) table (aggregate_exec.go:74-99, 201-304). */
int ph_agg_sink_masked(ph_agg *a, const ph_col *keys, const ph_col *args, int32_t nargs,
                       const int32_t *sel, int64_t n, int32_t positional, int64_t row_base,
                       uint32_t agg_mask);
/* Key column `key_index` of all current groups, in group-id order, as a dense DEVICE column of
 * the key's own element width (4 B for PH_I32/PH_DATE, 1 B for PH_CODE8, else 8 B) plus an
 * optional validity bitmap (1 bit per group, LSB first, at least (ngroups+7)/8 bytes; NULL keys
 * clear their bit). This is RadixPartitionedHashTable.GetData for the DISTINCT tables
 * (aggregate_exec.go:266-279): the distinct (group keys, argument) rows, re-sunk into the main
 * table with ph_agg_sink_masked. Returns the group count through *ngroups. */
int ph_agg_keys_dev(ph_agg *a, int32_t key_index, void *out_data_dev, uint8_t *out_validity_dev,
                    int64_t capacity, int64_t *ngroups);
/* Aggregate `agg_index` of all current groups, in group-id order, as a dense DEVICE column of int64 (SUM: the sum, PH_EOVERFLOW
 * when one exceeds int64; COUNT / COUNT_STAR: the count; MIN / MAX: the value) plus a validity bitmap (a group no input
 * reached is NULL, as SumOp / CountOp / MinMaxOp.Finalize make it, function_aggr.go:813-823, 950-962). Together with
 * ph_agg_keys_dev this turns an aggregate into a device-resident relation: an aggregate BELOW other operators (a
 * subquery's GROUP BY .. HAVING under a join) never travels through the host. AVG: PH_EUNSUPPORTED. */
int ph_agg_values_dev(ph_agg *a, int32_t agg_index, int64_t *out_dev, uint8_t *out_validity_dev, int64_t capacity, int64_t *ngroups);
/* Streaming aggregate (the planner's StreamAggregate): the FIRST sink into an empty table whose n rows
 * (positions 0..n of keys and args: no selection) arrive ordered by the group-key tuple — e.g. the
 * output of a join whose probe side is clustered by the key. Every group is then one run of adjacent
 * rows: run heads are marked, counted and scanned, and each head's thread reduces its run and writes
 * the group's record, in first-seen order by construction; no hash table, so no later ph_agg_sink into
 * the same table (PH_EUNSUPPORTED). Results are those of ph_agg_sink (exact 128-bit sums, NULL inputs
 * skipped). The order is verified on the device: a key tuple lexicographically below its predecessor's
 * is a DEFERRED PH_ECONSTRAINT of the ctx, reported by the next call that reads back, and the caller
 * aggregates again with ph_agg_sink. Runs may be of any length: a 1024-row tile is reduced as a segmented scan and the pieces of a run that
 * crosses tiles are joined one step per TILE (a table clustered by a low-cardinality key included). NULL-able keys: PH_EUNSUPPORTED. */
int ph_agg_sink_sorted(ph_agg *a, const ph_col *keys, const ph_col *args, int32_t nargs, int64_t n, int64_t row_base);
int ph_agg_group_count(ph_agg *a, int64_t *ngroups);
/* Build check without a device of the plan-specialised sink: ph_agg_sink calls of >= 2^20 rows run
 * the sink kernel compiled (hiprtc, cached per shape) with the key types / aggregate kinds /
 * argument types / NULL-ability of THIS call as constants instead of interpreting them per row
 * (PH_AGG_JIT=0 switches it off). Compiles canned shape `which` (0, 1) for gfx950. */
int ph_agg_jit_selfcheck(int32_t which);
/* Host outputs, groups in first-seen order:
 *   first_row[g]; keys[g*nkeys+c] (int64-widened), key_null[g*nkeys+c];
 *   sum_lo/sum_hi[g*naggs+a] = 128-bit sum (SUM/AVG) or min/max value in sum_lo;
 *   count[g*naggs+a] = non-NULL inputs seen (COUNT_STAR: rows). */
int ph_agg_finalize(ph_agg *a, int64_t max_groups, int64_t *first_row, int64_t *keys,
                    uint8_t *key_null, uint64_t *sum_lo, int64_t *sum_hi, uint64_t *count);
/* ph_agg_finalize that also reports the group count, so a caller with room for max_groups groups
 * needs no ph_agg_group_count first: ONE host round trip for the whole result when header + records
 * fit 64 KiB (the records are packed on the device, which reads the count there). *ngroups is set
 * even when it exceeds max_groups (PH_ECAPACITY: call again with room). */
int ph_agg_fetch(ph_agg *a, int64_t max_groups, int64_t *ngroups, int64_t *first_row, int64_t *keys,
                 uint8_t *key_null, uint64_t *sum_lo, int64_t *sum_hi, uint64_t *count);
/* ph_agg_fetch restricted to the groups whose aggregates satisfy `value OP k` for every conjunct (the HAVING of aggExecutor's output phase,
 * executor_aggr.go:143-263, evaluated on the device: the values as columns, ph_filter_select over the group ids, the survivors packed):
 * agg_index[c] names the aggregate (SUM / MIN / MAX / COUNT: a value that fits int64; AVG is PH_EUNSUPPORTED), value_scale[c] the scale its
 * values carry (ph_agg_result.scale), k[c] a PH_I32 / PH_DEC64 / PH_F32 constant — a DECIMAL value against a FLOAT literal compares in
 * float32, as everywhere. NULL aggregates (no input reached them) fail every comparison. The values are compared as int64: when the SUM
 * a conjunct names does not fit int64 in ANY group (whatever the other groups hold) the call returns PH_EOVERFLOW and no groups, as
 * ph_agg_topk does — fetch with ph_agg_fetch and filter the 128-bit sums on the host. MIN / MAX / COUNT always fit. */
int ph_agg_fetch_where(ph_agg *a, int32_t nconj, const int32_t *agg_index, const int32_t *op, const ph_const *k, const int32_t *value_scale,
                       int64_t max_groups, int64_t *ngroups, int64_t *first_row, int64_t *keys, uint8_t *key_null, uint64_t *sum_lo,
                       int64_t *sum_hi, uint64_t *count);
/* Top-N pre-selection for an `ORDER BY <aggregate> [DESC] ... LIMIT k` tail (the reference's
 * orderExecutor + limit, executor_order.go:56-138, executor_limit.go:105-238, sort over all group
 * rows on the host). A one-workgroup radix select finds the k-th best value
 * of aggregate `agg_index` on the device and only the groups at least that good come back
 * (>= k of them when ties exist, fewer when there are fewer groups), in first-seen order, in the
 * same layout as ph_agg_finalize. The caller applies the full ORDER BY (tie-breaks) and LIMIT to
 * those few rows. Sums must fit int64 (PH_EOVERFLOW otherwise: use ph_agg_finalize). SUM / MIN / MAX rank by their value, COUNT / COUNT(*)
 * by their count; AVG and COUNT(DISTINCT) are refused (PH_EUNSUPPORTED). NULL aggregates sort first in either direction and share
 * their key with the best possible live value (INT64_MIN ascending, INT64_MAX descending): when the k-th best is a NULL, groups of
 * that value may come back as well — a superset, like every tie. */
int ph_agg_topk(ph_agg *a, int32_t agg_index, int32_t descending, int64_t k, int64_t max_groups,
                int64_t *n_out, int64_t *first_row, int64_t *keys, uint8_t *key_null,
                uint64_t *sum_lo, int64_t *sum_hi, uint64_t *count);
void ph_agg_free(ph_agg *a);

/* ------------------------------------------------------------------ hash join
 * JoinHashTable.Build/Finalize/Probe + Scan.NextInnerJoin (pkg/compute/join_table.go:85-336,
 * join_scan.go:30-300, util_match.go:25-301). Device form: bucket-head table + next[] chains
 * (the reference's layout: head insertion with the previous head kept per row), built with
 * atomic exchange; rows with a NULL key are dropped on both sides. */
typedef struct ph_join ph_join;

int ph_join_build(ph_ctx *ctx, const ph_col *keys, int32_t nkeys, const int32_t *sel, int64_t n,
                  ph_join **out);
/* ph_join_build with the value range of the (single, integer) key column, as column statistics
 * give it (ph_table_col_range; any superset of the build keys' range). When the build side fills
 * the range densely (at most 8 slots per build row: a primary-key column, possibly filtered) the
 * table is a DIRECT table addressed by key - key_lo: no hashing, no key compares, one 4-byte read
 * per probe, and probes in key order read it front to back. The reference has no counterpart (it
 * always hashes, join_table.go:197-288); every probe call returns what it returns for
 * ph_join_build's tables. Sparse ranges, several key columns and 1-byte keys fall back to
 * ph_join_build. A build key outside [key_lo, key_hi] is an error, reported by ph_join_count
 * (-1 + ph_last_error) — the build itself makes no host round trip. */
int ph_join_build_range(ph_ctx *ctx, const ph_col *keys, int32_t nkeys, const int32_t *sel, int64_t n,
                        int64_t key_lo, int64_t key_hi, ph_join **out);
/* ph_join_build with what the planner knows about the join:
 *   PH_JOIN_KEY_RANGE  key_lo / key_hi hold the key column's value range (as ph_join_build_range)
 *   PH_JOIN_FK_PROBES  the probe side is a foreign key into this side's key: nearly every probe row
 *                      matches, so a Bloom bitmap would reject nothing. Build sides of >= 32 K rows with
 *                      one key column or two 4-byte ones then take the NODE table (16-byte {key, row,
 *                      next} records: a chain step is one read instead of next + one per key column)
 *                      at every size, not only above 4 M rows.
 * Every probe call works on every table form; the flags only pick the faster one. */
#define PH_JOIN_KEY_RANGE 1
#define PH_JOIN_FK_PROBES 2
/*   PH_JOIN_KEYS_SORTED_UNIQUE  column statistics say the build keys are strictly ascending (a primary key in
 *                      storage order). With PH_JOIN_KEY_RANGE and a dense range the direct table is then ONE
 *                      kernel: the sorted fill, which still verifies the claim, but reports a violation as a
 *                      DEFERRED PH_ECONSTRAINT of the ctx (see ph_ctx_set_deferred_errors: the next call that
 *                      reads back fails, whether or not that option is on) instead of launching the general
 *                      passes behind itself. The caller then builds again without the flag. Ignored where the
 *                      sorted fill does not apply (selections, NULL-able keys, small or sparse tables). */
#define PH_JOIN_KEYS_SORTED_UNIQUE 4
/*   PH_JOIN_EXISTS_ONLY  the table will only be asked WHETHER a key has a build row (ph_join_probe_mark / _mark_where: SEMI, ANTI and mark
 *                      joins). With a key range of at most 64 M values and a big build side it is then a flag table — one byte per key value,
 *                      one pass of plain byte stores, duplicates and row ids never materialised (ph_join_kind "bitmap"); every other probe is
 *                      PH_EUNSUPPORTED on it. Ignored where it does not apply. */
#define PH_JOIN_EXISTS_ONLY 8
int ph_join_build_ex(ph_ctx *ctx, const ph_col *keys, int32_t nkeys, const int32_t *sel, int64_t n, int32_t flags,
                     int64_t key_lo, int64_t key_hi, ph_join **out);
/* Filter -> HashJoin build in one pass (filterExecutor under joinExecutor's build child): the rows
 * sel[0..n) / 0..n that pass the comparison are built, without a selection vector and WITHOUT a
 * host read of how many pass — possible because a direct table is sized by the key range, not by
 * the row count. Only where ph_join_build_range picks a direct table (the test uses n, an upper
 * bound of the rows built) and the comparison lowers to an integer range over a column without
 * NULLs; PH_EUNSUPPORTED otherwise, and the caller runs ph_filter_select + ph_join_build_range.
 * Build row ids reported by probes are positions in the UNFILTERED input (sel[i] or i). */
int ph_join_build_where(ph_ctx *ctx, const ph_col *keys, int32_t nkeys, const ph_col *where_col, int32_t where_op,
                        const ph_const *where_k, const int32_t *sel, int64_t n, int64_t key_lo, int64_t key_hi,
                        ph_join **out);
/* ... with the planner hints of ph_join_build_ex (PH_JOIN_KEY_RANGE is implied). With
 * PH_JOIN_KEYS_SORTED_UNIQUE the Filter rides along in the verified one-pass sorted fill, which also
 * writes the table's occupancy bitmap (ranges up to 128 M slots): the candidate pass of a later inner probe
 * tests the bitmap and reads the slot array only for keys that are present — Q3's orders build after the
 * customer semi-join flags (the planner's Filter over executor_join.go:54-264's build child). */
int ph_join_build_where_ex(ph_ctx *ctx, const ph_col *keys, int32_t nkeys, const ph_col *where_col, int32_t where_op,
                           const ph_const *where_k, const int32_t *sel, int64_t n, int32_t flags, int64_t key_lo,
                           int64_t key_hi, ph_join **out);
/* the table form a build chose: "direct", "radix", "nodes", "chained+bloom" or "chained".
 * ph_join_build WITHOUT a range, over a million build rows or more, reads the key range off the column and takes the
 * direct table when the keys are dense in it; build sides above 4 M rows whose keys are not (and at most 29 M rows)
 * take the "radix" form: both sides partitioned by key hash, open-addressing tables built in LDS and kept as images
 * that the probes of one partition find on chip (joinExecutor's chained table, join_table.go:85-288, for build sides
 * that no cache holds). It answers inner probes itself; lookups and marks build the node table on first use. */
const char *ph_join_kind(const ph_join *j);
/* the form that sank the most recent rows into an aggregate's table — after a fallback the one that did the work: "" before any sink,
 * "generic" / "spec" (the incremental kernel, its generic or hiprtc-specialised body), "bulk1" (first bulk build), "bulk2" / "bulk2_spec"
 * (second bulk build, generic or specialised partial build), "two_level" (its variant above 512 bins), "sorted" (ph_agg_sink_sorted).
 * A specialised body whose compile failed reports the generic one. */
const char *ph_agg_sink_kind(const ph_agg *a);
/* The form (a string of ph_agg_sink_kind's) and sizes ph_agg_sink WOULD choose, without a device: for `rows` rows into a table that took
 * rows_sunk rows before and was created for expected_groups groups, nkeys key columns, naggs aggregates that read used_args argument
 * columns, any_nulls: a key or used argument has a validity bitmap, need_cnt: an aggregate over a NULL-able argument. It reads the
 * PH_AGG_* switches as a sink does and knows nothing of what happens at run time (a voided bulk build, a failed compile).
 * sizing: [0] LDS table entries of a bulk build, [1] partitions of the (first) scatter, [2] build bins, [3] shift, [4] slices (1 where a form has none),
 * [5] chunks of 256 rows a scatter workgroup stages, [6] its threads, [7] its LDS bytes, [8] the build's LDS bytes, [9] rows per scatter
 * workgroup, [10] LDS table entries and [11] threads of the incremental kernel; what a form does not use is 0. */
int ph_agg_sink_choice(int64_t rows, int64_t rows_sunk, int64_t expected_groups, int32_t nkeys, int32_t naggs, int32_t used_args,
                       int32_t any_nulls, int32_t need_cnt, const char **kind, int64_t sizing[12]);
/* 1 when ph_join_probe_inner* emit their pairs in probe-row order (every form except "radix", whose pairs come out
 * partition by partition — the same SET of pairs; a caller that relies on the order asks here) */
int ph_join_pairs_ordered(const ph_join *j);
int64_t ph_join_count(const ph_join *j);
/* Inner probe: writes (probe row id, build row id) pairs to dev buffers of `cap` entries.
 * *n_out (host) = number of matches (may exceed cap -> PH_ECAPACITY, nothing lost but the tail). */
int ph_join_probe_inner(ph_join *j, const ph_col *keys, const int32_t *sel, int64_t n,
                        int32_t *out_probe_dev, int32_t *out_build_dev, int64_t cap,
                        int64_t *n_out);
/* Filter -> HashJoin probe in one pass: the same pairs as ph_filter_select(where) followed by
 * ph_join_probe_inner over its selection (filterExecutor under joinExecutor's probe child,
 * executor_filter.go:27-114 + executor_join.go:54-264), without materialising the selection: the
 * kernel that streams the probe keys tests the comparison first. Only comparisons that lower to
 * an integer range (INTEGER / DATE / DECIMAL-vs-integer / dictionary-code columns, not `!=`) and
 * tables that carry a Bloom bitmap (build side <= 4 M keys) or are direct tables; PH_EUNSUPPORTED
 * otherwise, and the caller runs the two calls. `sel` narrows the probe rows first, as in ph_join_probe_inner. */
int ph_join_probe_inner_where(ph_join *j, const ph_col *keys, const ph_col *where_col, int32_t where_op,
                              const ph_const *where_k, const int32_t *sel, int64_t n,
                              int32_t *out_probe_dev, int32_t *out_build_dev, int64_t cap,
                              int64_t *n_out);
/* ph_join_probe_inner[_where] with a RESIDUAL predicate on the build row: only pairs whose build row r
 * has build_flags_dev[r] != 0 (a byte per row of the build-side table, e.g. from
 * ph_join_probe_mark_where). This is the form a join takes whose build child is Filter / SemiJoin(T): T
 * itself is built — whole, so a primary key in storage order builds in one pass and the filter's
 * row count never reaches the host — and the filter becomes a flag per row of T that the probe tests
 * on the row it found (Q3: lineitem JOIN (orders SEMI JOIN customer WHERE o_orderdate < ..)).
 * where_col may be NULL (no probe-side filter). Direct tables built without a selection only;
 * PH_EUNSUPPORTED otherwise. */
int ph_join_probe_inner_residual(ph_join *j, const ph_col *keys, const ph_col *where_col, int32_t where_op,
                                 const ph_const *where_k, const uint8_t *build_flags_dev, const int32_t *sel, int64_t n,
                                 int32_t *out_probe_dev, int32_t *out_build_dev, int64_t cap, int64_t *n_out);
/* Filter -> semi-join mark in one pass over rows 0..n: found_dev[i] = the comparison holds for row i
 * AND its key is in the table (0 / 1). Direct tables, integer-range comparisons, 16-byte aligned
 * columns without NULLs; PH_EUNSUPPORTED otherwise (ph_filter_select + ph_join_probe_mark). */
int ph_join_probe_mark_where(ph_join *j, const ph_col *keys, const ph_col *where_col, int32_t where_op,
                             const ph_const *where_k, int64_t n, uint8_t *found_dev);
/* Semi/anti/mark: found_dev[i] = 1 when probe row sel[i] (or i) has a match */
int ph_join_probe_mark(ph_join *j, const ph_col *keys, const int32_t *sel, int64_t n,
                       uint8_t *found_dev);
/* Lookup probe for N:1 joins (unique build keys: a primary key — the shape of every join of Q9 and of
 * the foreign-key joins generally): out_build_dev[i] = the build row matching probe row sel[i] (or
 * i), or -1. One kernel and no compaction, so a chain of such joins keeps ONE row-id array for the
 * probe side (late materialisation: columns are gathered once, after the last join, instead of
 * after every join as Scan.gatherResult does per chunk, join_scan.go:250-278). When a build key is
 * not unique the LAST row of its chain that matches is reported; stats_dev (optional, 2 int32 the
 * caller zeroes) receives the number of probe rows without a match and with more than one, so a
 * caller can verify the uniqueness it assumed with one read at the end of a pipeline. */
int ph_join_lookup(ph_join *j, const ph_col *keys, const int32_t *sel, int64_t n, int32_t *out_build_dev,
                   int32_t *stats_dev);
/* ph_join_lookup for foreign keys the plan trusts (every probe row has exactly one build row): no
 * statistics buffer and no host read. A probe row without a match (out = -1) or with several is a
 * DEFERRED error: the next call on this ctx that reads anything back from the device (a count, a
 * result download, ph_ctx_check_deferred) fails with PH_ECONSTRAINT instead, and the caller reruns
 * the stage with ph_join_lookup / ph_join_probe_inner. ph_gather, ph_gather_multi and ph_date_extract
 * read row 0 for a negative row id, so the positional pipeline behind a strict lookup stays in
 * bounds until the error is seen. */
int ph_join_lookup_strict(ph_join *j, const ph_col *keys, const int32_t *sel, int64_t n, int32_t *out_build_dev);
void ph_join_free(ph_join *j);

/* Merge-style N:1 lookup, no table: build_key is a unique key column in ascending order (a primary key stored in
 * key order), the probe rows sel[0..n) / 0..n arrive ordered by the key too (a clustered table behind
 * order-preserving operators). out[i] = build row whose key equals probe row i's, or -1. A block of probe rows
 * finds the slice of build keys it spans with two searches, streams it through LDS once and searches there:
 * the build column is read once and nothing is written — where the reference builds one hash table whatever
 * its children's order (executor_join.go:54-264). Both orders are checked on the device as the rows stream by
 * (blocks of very sparse probes search the column directly and check the probe order only); a violation is the
 * ctx's deferred PH_ECONSTRAINT and the caller joins again with ph_join_build + ph_join_lookup. strict != 0:
 * a probe row without a match is a deferred PH_ECONSTRAINT as in ph_join_lookup_strict. */
int ph_merge_lookup(ph_ctx *ctx, const ph_col *build_key, int64_t n_build, const ph_col *probe_key, const int32_t *sel,
                    int64_t n, int32_t strict, int32_t *out_build_dev);

/* Inner pairs against a CLUSTERED build key column, no table: build_key is a key column in ascending order WITH duplicates (lineitem by
 * l_orderkey; PH_STAT_ASCENDING), the probe rows sel[0..n) / 0..n come in any order. Every probe row finds the run of its key with a binary
 * search over the column; the pairs are (probe row id, each row of the run), in probe order. For a probe side far smaller than the build
 * side this replaces every pass a table build makes over ALL build rows (JoinHashTable.Build / Finalize, join_table.go:85-288) by
 * ~log2(n_build) reads per probe row. Same outputs and capacity protocol as ph_join_probe_inner. The column's order is the caller's claim
 * (ph_table_col_stats reports what the library measured at load). */
int ph_join_sorted_pairs(ph_ctx *ctx, const ph_col *build_key, int64_t n_build, const ph_col *probe_key, const int32_t *sel, int64_t n,
                         int32_t *out_probe_dev, int32_t *out_build_dev, int64_t cap, int64_t *n_out);

/* N:1 lookup on a two-column unique key into a table stored in runs of one length by the FIRST key column (ph_table_col_run_len > 0; key1_min =
 * that column's minimum, ph_table_col_range), no table: the candidate rows of probe row i are (probe_keys[0][i] - key1_min) * run_len .. + run_len,
 * the one whose build_key2 equals probe_keys[1][i] is the match (out_build_dev[i], -1 = none). Replaces JoinHashTable.Build + Probe
 * (join_table.go:85-288, join_scan.go:67-165) for a composite foreign key into such a table (Q9's lineitem -> partsupp). strict != 0: a probe row
 * without a match, or with several, is a deferred PH_ECONSTRAINT as in ph_join_lookup_strict. The run structure is the caller's claim. */
int ph_join_run_lookup(ph_ctx *ctx, const ph_col *build_key2, int64_t n_build, int64_t key1_min, int32_t run_len, const ph_col *probe_keys,
                       const int32_t *sel, int64_t n, int32_t strict, int32_t *out_build_dev);

/* Children per parent: what Agg(parent key; count(child column)) <- LEFT JOIN(parent, child ON parent key = child key) computes when the parent
 * key is unique (Q13: orders per customer) without the pair list (NextLeftJoin, join_scan.go) and the second fold (AddChunk, aggregate_hash.go):
 * the child rows child_sel[0..n_child) / 0..n_child are counted by key into an array over [key_min, key_min + key_range), parent row i receives
 * out_counts_dev[i] = the count of its key and bit i of out_valid_dev = count > 0 (a group without a non-NULL input finalises as NULL: CountOp,
 * aggr_ops.go). out_valid_dev: (n_parent + 63) / 64 * 8 bytes. Child rows with a NULL key or a key outside the range match nothing. */
int ph_count_by_key(ph_ctx *ctx, const ph_col *child_key, const int32_t *child_sel, int64_t n_child, int64_t key_min, int64_t key_range,
                    const ph_col *parent_key, const int32_t *parent_sel, int64_t n_parent, int64_t *out_counts_dev, uint8_t *out_valid_dev);

/* Cross product (CrossProduct / CrossProductExec, pkg/compute/join_cross.go:34-230) as row-id pairs:
 * for every right row, all left rows in order — the order the reference emits (one output chunk
 * per (left chunk, right row)) — so that both sides materialise with ph_gather like a join's
 * output. n_left * n_right must stay below 2^31. */
int ph_cross_pairs(ph_ctx *ctx, int64_t n_left, int64_t n_right, int32_t *out_left_dev, int32_t *out_right_dev);

/* gather: out[i] = col[idx[i]] for fixed-width columns (join payload materialisation,
 * TupleDataTemplatedGather join_collection.go:501-529) */
int ph_gather(ph_ctx *ctx, const ph_col *col, const int32_t *idx_dev, int64_t n, void *out_dev);

/* Validity of a row-id vector: bit i of bitmap_dev (pkg/util/bitmap.go's layout, (n + 7) / 8 bytes) = ids_dev[i] >= 0. The build side of a
 * LEFT OUTER join reports row id -1 for a probe row without a match (NextLeftJoin, join_scan.go:67-88: the build side's vectors are constant
 * NULL for those rows); values gathered through such ids (ph_gather* read row 0 for a negative id) carry this bitmap as their validity. */
int ph_rowid_validity(ph_ctx *ctx, const int32_t *ids_dev, int64_t n, uint8_t *bitmap_dev);
/* dictionary codes (PH_CODE8) of rows sel[0..n) / 0..n as INTEGERs: out_dev[i] = code (a code column as a 4-byte group-key part) */
int ph_widen_codes(ph_ctx *ctx, const ph_col *col, const int32_t *sel, int64_t n, int32_t *out_dev);

/* the same for up to 8 columns through one row-id array, in one pass: the late materialisation of a
 * join chain's probe side (all column reads of a row are in flight together, the index is read
 * once). out_dev[c]: n elements of column c's width. */
/* When the views are columns of ONE resident table and the table holds a co-located copy of them (below), the gather
 * reads it instead: one 64-byte sector per row id where the column arrays cost one per column (Q9's five lineitem
 * columns at 5 % of the rows: 1.27 GB of traffic for 0.1 GB of values). */
int ph_gather_multi(ph_ctx *ctx, int32_t ncols, const ph_col *cols, const int32_t *idx_dev, int64_t n,
                    void *const *out_dev);

/* ------------------------------------------------------------------ fused pipelines
 * The measured mode: Agg <- Scan(filter) collapsed into one pass over the resident table, which
 * is what `gpuScanAggExecutor` calls when the sub-plan matches. */
typedef struct {
    int32_t col;  /* table column */
    int32_t op;   /* ph_cmp */
    ph_const k;
} ph_pred; /* conjuncts, AND-ed in order */

typedef struct {
    int32_t kind;      /* ph_aggkind */
    int32_t nprog;     /* 0 for COUNT_STAR */
    ph_rpn prog[12];   /* argument expression over table columns */
} ph_aggexpr;

typedef struct {
    int64_t ngroups;
    /* arrays owned by the result, groups in first-seen order */
    int64_t *first_row;
    int64_t *keys;      /* ngroups * nkeys */
    uint64_t *sum_lo;   /* ngroups * naggs */
    int64_t *sum_hi;
    uint64_t *count;
    int32_t *scale;     /* naggs: scale of each aggregate's argument */
    int32_t nkeys, naggs;
    uint8_t *key_null;  /* ngroups * nkeys, 1 = the key is NULL (the NULL group; keys[] holds 0 there); NULL pointer = no NULL-able key */
} ph_agg_result;

/* group_cols: table columns to group by (0 columns = one global group, the reference's
 * constant-key ungrouped aggregate, executor_aggr.go:37-48).
 * rows [row_begin,row_end) of the table are scanned. */
int ph_scan_filter_agg(ph_ctx *ctx, const ph_table *t, int64_t row_begin, int64_t row_end,
                       const ph_pred *preds, int32_t npreds, const int32_t *group_cols,
                       int32_t ngroup_cols, const ph_aggexpr *aggs, int32_t naggs,
                       ph_agg_result **out);
/* the same launch sequence without the final download (bench inner loop); result stays on device
 * until ph_scan_filter_agg_fetch */
typedef struct ph_scan_plan ph_scan_plan;
int ph_scan_plan_create(ph_ctx *ctx, const ph_table *t, const ph_pred *preds, int32_t npreds,
                        const int32_t *group_cols, int32_t ngroup_cols, const ph_aggexpr *aggs,
                        int32_t naggs, ph_scan_plan **out);
/* rows [row_begin, row_end): row_begin a multiple of 4, or any row when the plan reads narrowed copies (ph_scan_plan_variant "narrow...") */
int ph_scan_plan_run(ph_scan_plan *p, int64_t row_begin, int64_t row_end);
int ph_scan_plan_fetch(ph_scan_plan *p, ph_agg_result **out);
/* Multi-GPU merge of fused plans (row-range sharded tables, no data-path collective): the raw
 * partial result of the last run is 2*nacc 64-bit words on the device (ph_scan_plan_partials_dev);
 * the ranks all-gather those few hundred bytes and any rank turns the concatenation of all ranks'
 * words (host memory, rank-major) into the merged result: 128-bit sums and counts add, the
 * first-seen row of a group is the one of the lowest rank that saw it. */
int ph_scan_plan_partials_dev(ph_scan_plan *p, void **dev, int32_t *nwords);
int ph_scan_plan_fetch_merged(ph_scan_plan *p, const uint64_t *words, int32_t nranks,
                              ph_agg_result **out);
/* Build check of the plan-specialised path without a device: generates the kernel source of canned
 * shape `which` (0 Q1, 1 Q6, 2 three keys + MIN/MAX + `!=`, 3 predicate-only COUNT) and compiles it
 * with hiprtc for gfx950; src_out (optional, cap bytes) receives the source. */
int ph_scan_jit_selfcheck(int32_t which, char *src_out, int64_t cap);
/* name of the kernel family the plan dispatches to: "lowcard_chain" / "filter_sumprod" (the two
 * precompiled fused kernels), "jit" (a kernel generated from the plan's shape and compiled with
 * hiprtc at plan creation: any range / != conjunction over NULL-free columns, <= 4 dictionary-code
 * group columns whose slots fit LDS, SUM/AVG/COUNT of products of affine column factors, MIN/MAX of
 * a column), "generic" (the operator chain: filter -> expression -> aggregate sink) */
const char *ph_scan_plan_kind(const ph_scan_plan *p);
/* bytes per row the plan's scan kernel loads: the fused kinds read the narrowed copies of their columns when every column they read
 * has one (ph_table_col_narrow; Q1 at 11 instead of 34, Q6 at 8 instead of 24), 8 once the plan has bound a packed scan group
 * (ph_table_pack_scan_group); 0 for "generic". This and ph_scan_plan_variant describe the NEXT launch: a lean plan binds the table's
 * group at the start of a ph_scan_plan_run, when it exists or when that run triggers its build, and keeps it from then on. */
int32_t ph_scan_plan_bytes_per_row(const ph_scan_plan *p);
/* the kernel instance the plan launches, a constant string: "wide" (the columns themselves); over the narrowed copies "narrow64" (64-bit
 * products), "narrow_rt" (32-bit products, code widths read at run time), "narrow32" (32-bit products, the code widths of TPC-H lineitem
 * fixed at compile time), "narrow32_lean" (the same with the lean row body: factors computed on the codes, sums of values, unmasked
 * interior tiles, every load of a wave reading consecutive bytes; PH_SCAN_LEAN=0 in the environment keeps plans off it),
 * "packed64" (the lean row body over the table's packed scan group, once the plan has bound one);
 * ph_scan_plan_kind's string for "jit" and "generic" */
const char *ph_scan_plan_variant(const ph_scan_plan *p);
/* the row body of a "packed64" plan's launches, a constant string: "bins" (lowcard_chain_kernel_group's BinsBody: a passing row adds its price code
 * and a count to a bin named by (slot, tax, discount) and its quantity code to a column; the products with the two factors are formed
 * once per workgroup from the bins; the same integers) when the group has TPC-H lineitem's layout and at most 6 slots, "columns" (sums
 * of per-row products in per-lane columns) for every other plan. PH_SCAN_HIST=0 in the environment, read at every run and by this call,
 * keeps plans on "columns". The bins body folds at most 1023 tiles of 4096 rows per workgroup: a run with more raises its grid, and
 * takes "columns" where it cannot; the answer is for the next launch over the rows of the last one ("columns" before the plan has bound
 * a group). */
const char *ph_scan_plan_row_body(const ph_scan_plan *p);
void ph_scan_plan_free(ph_scan_plan *p);
void ph_agg_result_free(ph_agg_result *r);

/* ------------------------------------------------------------------ resident plans
 * The join analogue of ph_scan_plan: a whole operator SUBTREE over resident tables,
 *     Agg <- [Project] <- [Filter] <- HashJoin* <- Scan(filter)
 * exactly as buildOperatorExec (pkg/compute/executor.go:305-350) receives it from the planner, handed to the
 * library as a flat array of node descriptors and run there without a chunk crossing the boundary:
 * joinExecutor.Execute's build + probe (executor_join.go:54-264), filterExecutor (executor_filter.go:27-114),
 * projectExecutor (executor_project.go:39-78) and aggExecutor's sink + finalize (executor_aggr.go:106-265).
 * The shim's gpuResidentPlanExecutor translates a PhysicalOperator subtree whose leaves are
 * resident tables into this descriptor, else the tree falls through to the per-operator executors.
 *
 * The library is the physical planner below the operator interface. Per join it picks, from the tables'
 * STATISTICS (ph_table_col_range, ph_table_col_stats, ph_table_declare_unique) — never from hints of the caller:
 *   - the table form: direct table over a dense integer key range, the one-pass sorted fill for a key in
 *     storage order, the gated fill when a filter or a semi-join's marks sit under the build child, node table
 *     for composite foreign keys, chained + Bloom otherwise (ph_join_build_ex / ph_join_build_where_ex);
 *   - the probe form: N:1 lookup when the build key is unique (no pair list; the intermediate stays aligned
 *     with the probe side), a merge lookup without any table when both sides are ordered by the key, marks
 *     instead of pairs for a join that only tests existence (SEMI, or INNER with a unique build key none of
 *     whose columns is used above) and feeds another build, the fused Filter -> probe otherwise;
 *   - sideways information passing: a big build side whose key the probe side has already joined against a
 *     small table is first reduced to the rows that can match (a mark probe against that table);
 *   - late materialisation: intermediates are row-id vectors per base table; columns are gathered once, when an
 *     expression, a key or the aggregate needs them;
 *   - the aggregate form: the fused scan kernels for Agg <- Scan, the streaming aggregate when the rows reach
 *     the aggregate ordered by the first group key, the LDS hash aggregate otherwise, a top-k preselection
 *     when the caller announces ORDER BY <aggregate> LIMIT k (ph_plan_set_topk).
 * Claims derived from statistics (sorted, unique, every foreign key has its row) are verified on the device
 * while the data streams by; a broken claim is the deferred PH_ECONSTRAINT, and ph_plan_fetch then runs the
 * plan again in its conservative forms (general builds, counted lookups, hash aggregate) — results never
 * depend on a statistic being right. ph_plan_explain names the forms the last run chose. */
typedef enum { PH_PN_SCAN = 1, PH_PN_FILTER, PH_PN_JOIN, PH_PN_PROJECT, PH_PN_AGG } ph_plan_kind;
typedef enum { PH_JT_INNER = 1, PH_JT_SEMI, PH_JT_ANTI,
               PH_JT_LEFT   /* LEFT OUTER (NextLeftJoin, join_scan.go:67-88): the inner matches, then every probe row without one with the build
                               side's columns NULL. Those columns carry a validity bitmap from then on: aggregates skip the NULLs (count(x) of a
                               customer without orders is 0 and finalises to NULL, function_aggr.go:950-962), operators that cannot take a
                               NULL-able column answer PH_EUNSUPPORTED. Rows come out matches first, then the unmatched probe rows. */
} ph_plan_join_type;   /* LOT_JoinType* of join_scan.go:47-165 */
typedef enum {
    PH_PE_COL = 1,    /* column reference (executeColumnRef: zero copy) */
    PH_PE_DECIMAL,    /* decimal / integer arithmetic, RPN over the child's output columns (executeFunc) */
    PH_PE_YEAR,       /* extract(year from <DATE column>)  (ExtractFunc, function_scalar.go:1509-1563) */
    PH_PE_CASE,       /* CASE WHEN <when> THEN <prog> ELSE <else_prog> END (executeCase, expr_exec.go:144-246):
                         the WHEN is a select, THEN is evaluated on its true rows and ELSE on the others
                         (FillSwitch, :559-606). Both branches are DECIMAL programs of ONE result scale (an integer
                         constant in a branch — `ELSE 0` — is cast to it), or — result_int != 0 — both INTEGER
                         constants. */
    PH_PE_SUBSTR,     /* substring(<VARCHAR table column col> FROM sub_offset FOR sub_length) (substringFunc,
                         function_operator_binary.go:553-625; ph_substring). The value is VARCHAR computed inside the plan:
                         it may be compared with VARCHAR constants by = / <> in a PH_PN_FILTER above (an IN list is their OR),
                         be a group key or pass through joins; as a group key it is reported as PH_STR by ph_plan_key_info,
                         whose table is then a one-column relation the PLAN owns (valid until the plan runs again or is
                         freed): the key values are its rows, ph_table_strings reads them. */
    PH_PE_FLOAT       /* FLOAT (float_wide = 0) or DOUBLE (float_wide != 0) arithmetic over the child's columns, as ph_float_eval: `prog` with
                         PH_X_DIV and the comparison steps allowed. result_int != 0: the program ends in a comparison and the value is its truth
                         (an INTEGER 1 / 0 column: a PH_PN_FILTER above keeps `column = 1` — Q17's `l_quantity < 0.2 * avg`, Q20's
                         `ps_availqty > 0.5 * sum`); else FLOAT values (float32 only). */
} ph_plan_expr_kind;

/* A boolean expression over a node's input columns as a flat tree (node 0 = the root): what ExprExec.executeSelect
 * walks (execSelectExpr / And / Or / Compare, expr_exec.go:342-530). AND narrows the selection child by child, OR
 * evaluates every child on the parent's rows and unites the true rows (`a IN (x, y)` is in(a,x) OR in(a,y)).
 * A comparison's right operand is a constant or — k.type = PH_COLREF — the column k.i. */
typedef enum { PH_B_CMP = 1, PH_B_AND, PH_B_OR } ph_bool_kind;
typedef struct {
    int32_t kind;          /* ph_bool_kind */
    int32_t col, op;       /* PH_B_CMP: column OP k  (ph_cmp; PH_LIKE / PH_NOTLIKE also over dictionary-code columns) */
    ph_const k;
    int32_t first_child;   /* PH_B_AND / PH_B_OR: children are nodes first_child .. first_child + nchildren - 1 */
    int32_t nchildren;
} ph_bool;

typedef struct {
    int32_t kind;     /* ph_plan_expr_kind */
    int32_t col;      /* PH_PE_COL / PH_PE_YEAR: child output column */
    int32_t nprog;
    ph_rpn prog[12];  /* PH_PE_DECIMAL: ph_rpn.col indexes the child's output columns. PH_PE_CASE: the THEN branch */
    /* PH_PE_CASE */
    int32_t nwhen;
    const ph_bool *when;   /* the WHEN condition over the child's output columns */
    int32_t nelse;
    ph_rpn else_prog[12];
    int32_t result_int;    /* != 0: THEN / ELSE are single PH_X_CONST programs of scale 0 and the result is INTEGER */
    /* PH_PE_SUBSTR */
    int64_t sub_offset, sub_length;   /* as ph_substring's; sub_length = INT64_MAX is the two-argument form */
    /* PH_PE_FLOAT */
    int32_t float_wide;               /* != 0: DOUBLE arithmetic */
} ph_plan_expr;

typedef struct {
    int32_t kind;     /* ph_aggkind */
    ph_plan_expr arg; /* over the child's output columns; ignored for PH_A_COUNT_STAR */
} ph_plan_agg;

typedef struct {
    int32_t kind;                /* ph_plan_kind */
    int32_t child[2];            /* node indexes (children precede their parent), -1 = none.
                                    PH_PN_JOIN: child[0] probes, child[1] is built (executor_join.go:237-264) */
    /* PH_PN_SCAN: the pruned columns of a resident table + the conjuncts pushed into the scan
       (scanExecutor.runFilterExec, executor_scan.go:225). ph_pred.col is a TABLE column. */
    const ph_table *table;
    int32_t ncols;
    const int32_t *cols;         /* table columns the scan emits, in output order */
    /* PH_PN_SCAN / PH_PN_FILTER: conjuncts, AND-ed in order (PH_PN_FILTER: ph_pred.col = child output column) */
    int32_t npreds;
    const ph_pred *preds;
    /* ... and one more conjunct of any shape (OR / IN lists, column-vs-column comparisons), AND-ed behind them.
       Simple `column OP constant` conjuncts belong in preds: those are the ones a build or a probe can absorb. */
    int32_t nbools;
    const ph_bool *bools;
    /* PH_PN_JOIN: equi-join on nkeys column pairs; the output picks from [probe child's columns | build
       child's columns] (SEMI / ANTI: probe columns only). A join's `bools` is its RESIDUAL condition — the non-equi
       conjuncts of the ON clause (Q21's `l2.l_suppkey <> l1.l_suppkey` inside EXISTS: the reference's HashJoin keeps them
       as join conditions beside the keys), a tree over [probe columns | build columns]: an INNER join keeps the pairs that
       satisfy it, a SEMI (ANTI) join the probe rows with at least one (without any) such pair. Not with PH_JT_LEFT. */
    int32_t join_type;           /* ph_plan_join_type */
    int32_t nkeys;
    const int32_t *probe_keys;   /* probe child's output columns */
    const int32_t *build_keys;   /* build child's output columns */
    int32_t nout;
    const int32_t *out;          /* indexes into the concatenation [probe columns | build columns] */
    /* PH_PN_PROJECT */
    int32_t nexprs;
    const ph_plan_expr *exprs;
    /* PH_PN_AGG (the root): group-by expressions and aggregates over the child's output columns; no group
       expression = one global group (executor_aggr.go:37-48) */
    int32_t ngroups;
    const ph_plan_expr *groups;
    int32_t naggs;
    const ph_plan_agg *aggs;
} ph_plan_node;

typedef struct ph_plan ph_plan;
typedef struct ph_comm ph_comm;   /* the multi-GPU communicator (declared with its entry points further down) */
/* nodes[nnodes-1] is the root: a PH_PN_AGG (the groups come back through ph_plan_fetch) or a join / filter / project (its rows through
 * ph_plan_fetch_rows). The descriptor (and the strings of its predicates) is
 * copied; the tables must outlive the plan. PH_EUNSUPPORTED for a shape outside the device path (the caller
 * keeps its per-operator executors). */
int ph_plan_create(ph_ctx *ctx, const ph_plan_node *nodes, int32_t nnodes, ph_plan **out);
/* ORDER BY <aggregate agg_index> [DESC] ... LIMIT k sits above the aggregate: only the groups at least as good
 * as the k-th come back (>= k with ties), as ph_agg_topk; the caller applies the full ORDER BY and the LIMIT. PH_EUNSUPPORTED beside
 * ph_plan_set_having: HAVING runs in the aggregate's output phase, before Order and Limit (executor_aggr.go:143-263) — the k best groups
 * could fail it while later ones pass — so a plan carries one or the other, and with a HAVING the caller sorts the survivors. */
int ph_plan_set_topk(ph_plan *p, int32_t agg_index, int32_t descending, int64_t k);
/* The same announcement for a JOIN-rooted plan (ph_plan_fetch_rows) under `ORDER BY <column col of the rows> [DESC] ... LIMIT k` (orderExecutor +
 * limit above the join, executor_order.go:56-138, executor_limit.go:105-238): only the rows whose key is at least as good as the k-th best come
 * back (>= k with ties; all rows when the key can be NULL, is a VARCHAR / BIGINT, or a DECIMAL in ascending order or of a scale above 2 — the
 * orderings the reference's selection and sort encoder do not share). The caller applies the full ORDER BY and the LIMIT to those rows. */
int ph_plan_set_rows_topk(ph_plan *p, int32_t col, int32_t descending, int64_t k);
/* HAVING conjuncts `result column OP constant` over the root's AGGREGATE columns (ph_pred.col counts the result's columns: group keys first,
 * then the aggregates), applied on the device when the groups are fetched (ph_agg_fetch_where): only the surviving groups come back.
 * PH_EUNSUPPORTED — and the caller filters the fetched rows itself — for a conjunct over a key column or an AVG, for Agg <- Scan plans
 * (a fused scan: few groups) and beside ph_plan_set_topk. */
int ph_plan_set_having(ph_plan *p, int32_t nconj, const ph_pred *conj);
/* 1 when the last ph_plan_fetch applied the conjuncts of ph_plan_set_having. The device compares the aggregates as int64 values: when
 * a sum of the run exceeds that range every group comes back with its exact 128-bit sums instead (0 here; likewise a top-k
 * preselection is then skipped) and the caller applies its HAVING to the fetched rows, as without ph_plan_set_having. */
int32_t ph_plan_having_applied(const ph_plan *p);
/* enqueue one execution of the whole subtree (host round trips only where a row count sizes the next step) */
int ph_plan_run(ph_plan *p);
/* the group rows of the last run, in first-seen order (ph_agg_result_free releases them). If the run's
 * optimistic forms met a broken statistic (deferred PH_ECONSTRAINT), the plan is run again conservatively
 * first; later runs of this plan then start conservatively. An aggregate without group expressions has its ONE group whatever its
 * input: over no input row every count is 0 and every other aggregate NULL (count 0) — at the root, whether it runs as a fused scan
 * (Agg <- Scan) or over joins, and below other operators alike. A HAVING (ph_plan_set_having) judges that group like any other: a
 * conjunct over a count compares 0 with its constant, a conjunct over a NULL aggregate fails. Single rank only: across ranks a plan
 * without input rows still returns no group. */
int ph_plan_fetch(ph_plan *p, ph_agg_result **out);
/* A plan whose root is NOT an aggregate — a join, filter or project (Q15's final Join(supplier, revenue = max)) — returns the root
 * relation's rows: every fixed-width column as nrows values widened to 64 bits (type[c] / scale[c] say what they are; NULL-able
 * columns are PH_EUNSUPPORTED), every VARCHAR column — a table column behind row ids, or a value computed in the plan — as
 * offsets[c] (nrows + 1) and bytes[c], gathered on the device. Row order is the root relation's (probe order for joins the
 * library ran in probe order; apply the query's ORDER BY above). */
typedef struct {
    int64_t nrows;
    int32_t ncols;
    int32_t *type, *scale;
    int64_t **values;    /* [ncols]: NULL for VARCHAR columns */
    int32_t **offsets;   /* [ncols]: NULL for fixed-width columns */
    char **bytes;
} ph_rows_result;
int ph_plan_fetch_rows(ph_plan *p, ph_rows_result **out);
void ph_rows_result_free(ph_rows_result *r);
/* group key k of the result: device type and scale, and — when it is a table column carried through unchanged
 * (dictionary codes need their dictionary) — the table and column it comes from (else *table = NULL) */
int ph_plan_key_info(const ph_plan *p, int32_t k, int32_t *type, int32_t *scale, const ph_table **table, int32_t *col);
/* type (PH_I32 / PH_I64 / PH_DEC64 ...) of aggregate a's argument; its scale is ph_agg_result.scale[a] */
int ph_plan_agg_arg_type(const ph_plan *p, int32_t a, int32_t *type);
/* one line per operator of the last run: the forms chosen and the row counts seen */
const char *ph_plan_explain(const ph_plan *p);
/* Multi-rank execution (no reference counterpart: the reference runs one goroutine). Every rank creates the SAME plan over its shard
 * of the sharded tables (row ranges: the default) and its copy of the replicated ones (ph_table_set_replicated: NATION, REGION, any small table),
 * announces the communicator, and runs and fetches like a single rank; every rank receives the complete result. The library inserts the exchanges:
 *   join: build side replicated -> local; both sides co-located by key RANGE (the ranks' column statistics: a database split by order ranges)
 *         -> local; build side small (ph_plan_set_broadcast_rows, default 4 Mi rows in all) -> all-gathered (VARCHAR columns included) into a
 *         replicated temporary table; otherwise both sides hash-partitioned by the first key (ph_partition_dev) and exchanged all-to-all;
 *   aggregate below other operators: whole groups per rank — by disjoint key ranges, else its input hash-partitioned by a group key;
 *   root aggregate: local, the ranks' partial states (128-bit sums, counts, min / max) merged at ph_plan_fetch; with a top-k, a HAVING or a
 *         DISTINCT aggregate its input is hash-partitioned first and the ranks' whole groups are concatenated;
 *   join-rooted plans: the root relation's rows all-gathered.
 * Every decision is taken from all-reduced values, so all ranks walk the same sequence of collectives; a broken statistic on any rank is agreed on at
 * the end of the run and all ranks rerun conservatively, together. Works over RCCL (ph_comm_init) and the in-process transport alike. */
int ph_plan_set_comm(ph_plan *p, ph_comm *comm);
int ph_plan_set_broadcast_rows(ph_plan *p, int64_t rows);
/* this rank holds ALL rows of the table (every rank loaded the same rows) — the default is a shard (a row range) */
int ph_table_set_replicated(ph_table *t, int32_t on);
void ph_plan_free(ph_plan *p);

/* ------------------------------------------------------------------ multi-GPU partitioning
 * No reference counterpart (the reference is single-threaded): hash-partition
 * rows by key so that join build/probe sides and group-by keys co-locate per GPU.
 * dest = mix64(key) % nparts. Writes per-partition counts and a permutation of row ids grouped
 * by destination, input order kept inside every partition (reproducible); the caller gathers
 * columns with ph_gather and exchanges them (ph_comm_* below). */
int ph_partition(ph_ctx *ctx, const ph_col *key, const int32_t *sel, int64_t n, int32_t nparts,
                 int64_t *counts_host, int32_t *perm_dev);
/* Same, with the nparts counts left on the device (int64 each) and no host round trip: what the
 * exchange below consumes (ph_comm_exchange_counts reads them there). */
int ph_partition_dev(ph_ctx *ctx, const ph_col *key, const int32_t *sel, int64_t n, int32_t nparts,
                     int64_t *counts_dev, int32_t *perm_dev);

/* ------------------------------------------------------------------ multi-GPU exchange (RCCL over xGMI)
 * One process (or goroutine-pinned OS thread) per GPU; SURVEY.md §8(e). No reference counterpart.
 * The plug point that drives it is the same one that builds the executors (buildOperatorExec,
 * pkg/compute/executor.go:305-350): a partitioned gpuJoinExecutor partitions its build and probe
 * batches with ph_partition_dev, gathers the needed columns (ph_gather) and exchanges them.
 * Everything is stream-ordered on the ctx stream; a stage makes ONE host round trip (the count
 * matrix), none between the partition, the gathers and the all-to-all. */
#define PH_COMM_ID_BYTES 128
typedef struct ph_comm ph_comm;
typedef enum { PH_RED_SUM = 1, PH_RED_MAX = 2, PH_RED_MIN = 3 } ph_redop;
/* rank 0 creates the id (ncclGetUniqueId) and ships its 128 bytes to the other ranks by any host
 * channel (the Go side: the coordinator's RPC; the tests: a file / torch.distributed store) */
int ph_comm_unique_id(void *id_out);
int ph_comm_init(ph_ctx *ctx, int32_t nranks, int32_t rank, const void *id, ph_comm **out);
/* The in-process transport: the ranks are THREADS of one process, each with a ctx of its own — on different devices (a host that drives every
 * GPU of a node from one process) or on one (the single-GPU test box: RCCL refuses two ranks on one device). ph_local_group_create makes the
 * rendezvous object the threads share; every thread calls ph_comm_init_local with its rank. Every ph_comm_* call below then works as over
 * RCCL (same arguments, same results); the copies are device-to-device on the calling ctx's stream between host barriers. */
typedef struct ph_local_group ph_local_group;
int ph_local_group_create(int32_t nranks, ph_local_group **out);
void ph_local_group_free(ph_local_group *g);
int ph_comm_init_local(ph_ctx *ctx, ph_local_group *g, int32_t rank, ph_comm **out);
int32_t ph_comm_nranks(const ph_comm *c);
int32_t ph_comm_rank(const ph_comm *c);
void ph_comm_destroy(ph_comm *c);
/* every rank contributes `bytes` from send_dev; recv_dev gets nranks*bytes, rank-major. async != 0:
 * the collective runs on the communicator's own stream behind everything already queued on the ctx
 * stream, so later kernels on the ctx stream overlap it; ph_comm_wait makes the ctx stream wait for
 * it (stream-side, no host block). Used for the per-step merge of fused-plan partials. */
int ph_comm_allgather(ph_comm *c, const void *send_dev, void *recv_dev, int64_t bytes, int32_t async);
int ph_comm_wait(ph_comm *c);
/* same, except that the newest `keep` (0..3) asynchronous collectives may still be running: with
 * two alternating result buffers, `keep` = 1 before a step lets the previous step's collective
 * overlap this step's kernels while the buffer about to be overwritten is safe */
int ph_comm_wait_keep(ph_comm *c, int32_t keep);
/* n <= 64 host values reduced over all ranks, result on every rank (timings, row totals, flags) */
int ph_comm_allreduce_i64(ph_comm *c, int64_t *host_vals, int32_t n, int32_t op);
int ph_comm_barrier(ph_comm *c);
/* send_counts_dev: this rank's nranks per-destination row counts (ph_partition_dev's output).
 * matrix_host[s*nranks + d] = rows rank s sends to rank d, on every rank: one all-gather and the
 * stage's one device->host copy. */
int ph_comm_exchange_counts(ph_comm *c, const int64_t *send_counts_dev, int64_t *matrix_host);
/* host-only (no device, no RCCL): offsets of every peer's rows in this rank's send buffers (rows
 * ordered by destination, as ph_partition orders them) and receive buffers (ordered by source rank).
 * send_off / recv_off: nranks+1 entries; recv_off[nranks] = rows this rank ends up with. */
int ph_exchange_layout(const int64_t *matrix, int32_t nranks, int32_t rank, int64_t *send_off, int64_t *recv_off);
/* all-to-all of ncols column buffers (elem_bytes[k] bytes per row) as one group of
 * ncclSend/ncclRecv pairs: every peer pair and every column concurrently. recv_dev[k] needs
 * recv_off[nranks]*elem_bytes[k] bytes. */
int ph_comm_exchange_columns(ph_comm *c, int32_t ncols, const void *const *send_dev, void *const *recv_dev,
                             const int32_t *elem_bytes, const int64_t *matrix_host);
/* variable-length all-gather of one column (broadcast of a small build side): counts_host[r] =
 * rows of rank r, recv_dev = all rows in rank order (PH_ECAPACITY when recv_capacity is too small;
 * counts_host is valid then) */
int ph_comm_allgather_rows(ph_comm *c, const void *send_dev, int64_t count, int32_t elem_bytes, void *recv_dev,
                           int64_t recv_capacity, int64_t *counts_host);
/* The capacity test above is collective: the ranks exchange (count, capacity) pairs and either ALL return
 * PH_ECAPACITY (the total exceeds the smallest capacity) or all exchange — no rank leaves alone. This form needs
 * no capacity at all: the library allocates exactly the total (*recv_dev_out, from ph_dev_alloc's pool; free it
 * with ph_dev_free). */
int ph_comm_allgather_rows_alloc(ph_comm *c, const void *send_dev, int64_t count, int32_t elem_bytes, void **recv_dev_out,
                                 int64_t *counts_host);

/* ------------------------------------------------------------------ measurement
 * streaming-read ceiling: a read-only reduce over `bytes` of device memory with the fused scan
 * kernels' access pattern (grid workgroups of 256 threads, 16-byte non-temporal loads); one word
 * per workgroup is written to out_words_dev. The caller times it (HIP events on the ctx stream). */
int ph_dev_read_reduce(ph_ctx *ctx, const void *dev, int64_t bytes, uint64_t *out_words_dev, int32_t grid);

/* ------------------------------------------------------------------ ORDER BY
 * LocalSort (sort_local.go:64-250; key layout sort_layout.go:29-88; encoders
 * sort_encoder.go:33-114; RadixScatter sort_radix.go:242-380): rows sel[0..n) (or 0..n) ordered
 * by the ORDER BY columns `keys` (first = most significant), descending[c] != 0 for DESC.
 * As in the reference NULLs always sort first (sort_layout.go:46), DECIMAL keys compare by their
 * value rounded half-even to two decimals (decimalEncoder: dec.Int64(2)), DATE by (year, month,
 * day), INTEGER as int32; PH_CODE8 keys compare by code and therefore need a dictionary in
 * ascending byte order (the loader's dictionaries are). PH_STR keys (VARCHAR: data = int32
 * offsets[rows+1], aux = bytes, aux_bytes < 2^31 or PH_EINVAL) compare as Go's bytes.Compare, bytes
 * unsigned, a proper prefix first: the reference keys an 11-byte zero-padded prefix, inverted for
 * DESC (RadixScatterStringVector sort_radix.go:728-805, sort_layout.go:55-66) and re-sorts tied
 * prefixes by the whole string, times -1 for DESC (sort_radix.go:180-230, CompareVal :898-933,
 * common/string.go:37-41); DESC is the exact reverse. Strings under 11 bytes that differ only by
 * trailing NUL bytes tie in the reference's prefix; bytes.Compare is a valid refinement there.
 * BIGINT / DOUBLE keys: PH_EUNSUPPORTED (the reference's RadixScatter has no case for them either).
 * Rows with equal keys keep their input order (the reference leaves their order undefined).
 * out_rows_dev: n int32 row ids, sorted. */
int ph_sort_rows(ph_ctx *ctx, const ph_col *keys, const int32_t *descending, int32_t nkeys,
                 const int32_t *sel, int64_t n, int32_t *out_rows_dev);

#ifdef __cplusplus
}
#endif
#endif
