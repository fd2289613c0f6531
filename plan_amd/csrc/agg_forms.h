// Which form sinks rows into a ph_agg, and with what sizes (DESIGN.md "sink forms"): the forms, the switches and the pure rule that chooses.
// Host only, no HIP: ph_agg_sink_choice answers without a device.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace ph {

// The form that sank a table's most recent rows (ph_agg::form, ph_agg_sink_kind). Incremental and Bulk2 run a generic or a
// hiprtc-specialised body (ph_agg::spec_body); a Sorted table has no hash slots and takes no further sinks.
enum class AggSinkForm { None, Incremental, Bulk1, Bulk2, TwoLevel, Sorted };

// The switches that turn a form off or force one, read once per sink call (tests compare forms over the same rows in one process).
struct AggKnobs {
    bool jit;                                // PH_AGG_JIT=0: generic bodies only
    bool no_bulk, bulk_v1, one_level;        // PH_AGG_NO_BULK, PH_AGG_BULK_V1, PH_AGG_BULK_ONE_LEVEL
    bool stream_one_pass, stream_two_pass;   // PH_STREAM_AGG_ONE_PASS, PH_STREAM_AGG_TWO_PASS
    static AggKnobs read() {
        auto set = [](const char *name) { return getenv(name) != nullptr; };
        const char *jit = getenv("PH_AGG_JIT");
        return {!(jit && atoi(jit) == 0), set("PH_AGG_NO_BULK"), set("PH_AGG_BULK_V1"), set("PH_AGG_BULK_ONE_LEVEL"),
                set("PH_STREAM_AGG_ONE_PASS"), set("PH_STREAM_AGG_TWO_PASS")};
    }
};

constexpr int AGG_BULK_MAX_ARGS = 4;   // BK_MAX_ARGS of agg_sink.inc (ops_agg.hip asserts the two agree)

// what the choice depends on
struct AggSinkQuery {
    int64_t n, rows_sunk, hint;   // rows of this sink, rows the table already took, ph_agg_create's expected groups
    int nkeys, naggs, nused;      // nused: argument columns some aggregate of the call reads
    bool nulls;                   // some key or used argument carries a validity bitmap
    bool need_cnt;                // some aggregate counts its own non-NULL inputs (agg_spec_need_cnt)
};

struct AggSinkChoice {
    AggSinkForm form = AggSinkForm::Incremental;
    bool spec = false;   // Incremental, Bulk2: the specialised body is wanted (a failed compile still lands on the generic one)
    // Bulk1, Bulk2, TwoLevel
    int T = 0;           // entries of a build workgroup's LDS table
    int nparts = 0;      // partitions of the (first) scatter
    int bins = 0;        // build bins: nparts, or all bins of the two levels
    int shift = 0;       // hash bits below the partition number
    int slices = 1;      // Bulk2: workgroups that share a partition
    int bu = 0, tpb = 0; // Bulk2, TwoLevel: the scatter stages 256 x bu rows per chunk in a workgroup of tpb threads
    int64_t lds_scatter = 0, lds_build = 0, rows_per_wg = 0;
    // Incremental
    int slots = 0, threads = 0;   // LDS table entries, workgroup size
    int entry_bytes = 0;          // of one LDS entry
    int64_t lds_budget = 0;       // the LDS size the table was fitted to
};

// entry of the specialised incremental kernel's LDS table
inline int agg_spec_entry_bytes(int nkeys, int naggs, bool need_cnt) { return 12 + 8 * nkeys + 8 * naggs + (need_cnt ? 4 * naggs : 0); }
// entry of a bulk build's LDS table, and the largest power-of-two table (256..4096 entries) that fits 120 KiB
inline int agg_bulk_entry_bytes(int nkeys, int naggs) { return 4 + 8 * nkeys + 8 + 20 * naggs; }
inline int agg_bulk_table(int per_entry) {
    int T = 256;
    while (T * 2 * per_entry <= 120 * 1024 && T < 4096) T *= 2;
    return T;
}

inline AggSinkChoice incremental_choice(const AggSinkQuery &q, bool spec) {
    AggSinkChoice c;
    c.form = AggSinkForm::Incremental;
    c.spec = spec;
    if (!spec) {
        // LDS table: as many entries as fit 32 KiB (at most 1024): state 4 B, first row 8 B, 8 B per key column, 12 B per aggregate
        c.entry_bytes = 12 + 8 * q.nkeys + 12 * q.naggs;
        c.slots = 64;
        while (c.slots * 2 * c.entry_bytes <= 32 * 1024 && c.slots < 1024) c.slots *= 2;
        c.threads = 256;
        c.lds_budget = 32 * 1024;
        return c;
    }
    // 512-thread workgroups share one LDS table among 8 waves: half of the flushes (every workgroup pays one find-or-create + state
    // update of device-scope atomics per group it saw: 800 workgroups x 175 groups cost more than the 3.3 M rows of Q9's aggregate
    // themselves). Measured, two int32 keys / 175 groups / one sum: 3.3 M rows 100 -> 78 us, 32 M rows 370 -> 309 us; 1024 threads
    // (one workgroup per CU by registers) 74 / 409 us.
    c.threads = 512;
    // The specialised kernel's table is static, so it may pass 64 KiB: when the creator expects more groups than half of the 32 KiB
    // table holds, the table grows (up to 128 KiB: one 1024-thread workgroup per CU) — rows whose group finds no room in LDS go to
    // the global table one by one (1000 groups in a 256-entry table: 4.3 ms per 32 M rows).
    c.entry_bytes = agg_spec_entry_bytes(q.nkeys, q.naggs, q.need_cnt);
    auto fit = [&](size_t b) { int t = 64; while ((size_t)t * 2 * c.entry_bytes <= b && t < 8192) t *= 2; return t; };
    size_t budget = 32 * 1024;
    c.slots = fit(budget);
    for (size_t b = budget; b <= 144 * 1024; b = b < 128 * 1024 ? b * 2 : b + 16 * 1024)   // the smallest table the expected groups fill to 70 % at most
        if ((int64_t)fit(b) * 7 / 10 >= q.hint) { budget = b; c.slots = fit(b); break; }
    if (budget > 64 * 1024) c.threads = 1024;
    c.lds_budget = (int64_t)budget;
    return c;
}
// sinks large enough to repay a one-time compile (~0.5 s per shape and process) run the kernel specialised for this shape;
// small ones, and everything when hiprtc is unavailable, the generic one
inline AggSinkChoice incremental_choice(const AggSinkQuery &q, const AggKnobs &k) { return incremental_choice(q, k.jit && q.n >= (1 << 20)); }

// the first bulk build; Incremental when the shape is not one it handles
inline AggSinkChoice bulk1_choice(const AggSinkQuery &q, const AggKnobs &k) {
    const int per_entry = agg_bulk_entry_bytes(q.nkeys, q.naggs);
    const int T = agg_bulk_table(per_entry);
    if (q.nused > AGG_BULK_MAX_ARGS || T * per_entry > 120 * 1024) return incremental_choice(q, k);
    AggSinkChoice c;
    c.form = AggSinkForm::Bulk1;
    c.T = T;
    const int64_t want_parts = (q.hint + T / 4 - 1) / (T / 4);
    // one 1024-thread workgroup builds one partition: big inputs get at least two partitions per CU
    // (65 k groups from 32 M rows used 64 partitions = a quarter of the CUs: build 1.09 -> 0.51 ms)
    c.nparts = q.n >= (4ll << 20) ? 512 : 8;
    while (c.nparts < want_parts && c.nparts < 4096) c.nparts *= 2;
    c.bins = c.nparts;
    c.shift = 40;
    c.rows_per_wg = std::max<int64_t>(1024, ((q.n + 511) / 512 + 255) / 256 * 256);
    c.lds_build = (int64_t)T * per_entry;
    return c;
}

// The rule. Bulk builds serve a first sink of at least 65536 rows whose hint reaches bulk_min; the second form (Bulk2, or TwoLevel
// above 512 bins) 4 Mi rows and more with at most 8192 bins; everything else is incremental, with the specialised body from 2^20 rows.
inline AggSinkChoice choose_sink_form(const AggSinkQuery &q, const AggKnobs &k) {
    // bulk_min: hints from which the bulk build pays, lowered for big first sinks whose expected groups overflow the largest LDS table the incremental kernel can have (144 KiB at
    // 70 %): their rows would update the global table one by one with device-scope atomics (3000 groups / 32 M rows: 4.9 ms
    // against 1.5 ms for the bulk build)
    int64_t bulk_min = 32768;
    if (q.n >= (4ll << 20)) {
        const int sper = agg_spec_entry_bytes(q.nkeys, q.naggs, q.need_cnt);
        int t = 64;
        while ((size_t)t * 2 * sper <= 144 * 1024 && t < 8192) t *= 2;
        bulk_min = std::min<int64_t>(bulk_min, (int64_t)t * 7 / 10 + 1);
    }
    if (k.no_bulk || q.rows_sunk != 0 || q.hint < bulk_min || q.n < 65536) return incremental_choice(q, k);
    const AggSinkChoice first = bulk1_choice(q, k);
    if (first.form != AggSinkForm::Bulk1 || k.bulk_v1 || q.n < (4ll << 20) || q.n >= (1ll << 31)) return first;
    // big inputs, up to ~4 M expected groups: the staged, sliced form
    AggSinkChoice c;
    const int T = first.T;
    c.T = T;
    // partitions: a quarter-full LDS table per partition (every slice of a partition sees all of its groups)
    const int64_t want_parts = (q.hint + T / 4 - 1) / (T / 4);
    int nparts = 16;
    while (nparts < want_parts && nparts <= 8192) nparts *= 2;
    const bool two_level = nparts > 512;   // more bins than one staged scatter serves in runs: a first level of 64 partitions, then all bins
    if (nparts > 8192 || (two_level && k.one_level)) return first;
    c.form = two_level ? AggSinkForm::TwoLevel : AggSinkForm::Bulk2;
    c.spec = !two_level && k.jit;
    c.bins = nparts;
    int log_bins = 0;
    while ((1 << log_bins) < c.bins) log_bins++;
    if (two_level) nparts = 64;
    c.nparts = nparts;
    c.shift = two_level ? 40 + (log_bins - 6) : 40;
    while (!two_level && nparts * c.slices < 512 && c.slices < 64) c.slices *= 2;   // two workgroups per CU in all: every slice pays a table initialisation and a write-out
    // chunk of the scatter: what fits 64 KiB of LDS beside the three partition tables (two workgroups per CU)
    const int W = q.nkeys + q.nused;
    const int row_bytes = 8 * W + 8 + (q.nulls ? 4 : 0);
    const size_t tables = (size_t)(3 * nparts + (nparts & 1)) * 4;
    int bu = 8;
    while (bu > 2 && tables + (size_t)256 * bu * row_bytes > 64 * 1024) bu /= 2;
    c.tpb = 1024;
    if (bu < 4) bu = 4;   // at least a row per thread
    // one 1024-thread workgroup per CU can stage 4096 rows: runs twice as long per partition (fewer partial lines written)
    if (bu == 8 && tables + (size_t)256 * 16 * row_bytes <= 120 * 1024) bu = 16;
    c.bu = bu;
    c.lds_scatter = (int64_t)(tables + (size_t)256 * bu * row_bytes);
    if (c.lds_scatter > 124 * 1024) return first;
    const int ch = 256 * bu;
    c.rows_per_wg = std::max<int64_t>(ch, ((q.n + 511) / 512 + ch - 1) / ch * ch);
    c.lds_build = (int64_t)T * agg_bulk_entry_bytes(q.nkeys, q.naggs);
    return c;
}

inline const char *agg_sink_kind_name(AggSinkForm form, bool spec) {
    switch (form) {
    case AggSinkForm::None: return "";
    case AggSinkForm::Incremental: return spec ? "spec" : "generic";
    case AggSinkForm::Bulk1: return "bulk1";
    case AggSinkForm::Bulk2: return spec ? "bulk2_spec" : "bulk2";
    case AggSinkForm::TwoLevel: return "two_level";
    case AggSinkForm::Sorted: return "sorted";
    }
    return "";
}

}  // namespace ph
