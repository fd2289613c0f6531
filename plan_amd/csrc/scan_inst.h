// Which kernel instance a fused scan launches, as a value chosen by one pure function of the plan's facts and the process's switches
// (DESIGN.md §4.1 "Which instance runs"), and the grid geometry of a run. No HIP in it: scan_plan.hip and the launches of scan_kernels.hip
// go through these, tests/test_scan_inst.py runs them from a g++ program.
#pragma once
#include <algorithm>
#include <cstdint>

namespace ph {

// How a fused scan reads its columns: the wide columns, or their narrowed copies (the kernels *_for: a lane owns 16 consecutive rows,
// predicates compare codes against bounds rewritten into the code domain), optionally with 32-bit products (operand and product bounds
// proven at plan creation).
enum ScanForm : int32_t { FORM_WIDE = 0, FORM_NARROW = 1, FORM_NARROW32 = 2 };

// the bins body of the packed lowcard_chain scan (BinsBody of lowcard_chain_kernel_group): slots its tables hold, and the tiles one workgroup may fold
// into them before a bin's packed count and sum could carry (scan_kernels.hip states the field widths)
constexpr int LC_BINS_MAX_SLOTS = 6;
constexpr int LC_BINS_MAX_TILES = 1023;

// The environment switches of the fused scans, as the value the choices below take. Read once per process: nt
// (PH_SCAN_NT), narrow_generic (PH_SCAN_NARROW_GENERIC), pack_generic (PH_SCAN_PACK_GENERIC), lean (PH_SCAN_LEAN), tail (PH_SCAN_TAIL).
// Read at every run: hist (PH_SCAN_HIST), unroll (PH_SCAN_UNROLL), grid (PH_SCAN_GRID, 0 = none).
struct ScanSwitches {
    bool nt = true, narrow_generic = false, pack_generic = false, lean = true, tail = true, hist = true;
    int unroll = 1, grid = 0;
};

enum FsInst { FSI_WIDE, FSI_NARROW_RT64, FSI_NARROW_RT32, FSI_NARROW_FIXED32 };
enum LcInst { LCI_WIDE, LCI_NARROW_RT64, LCI_NARROW_RT32, LCI_NARROW_FIXED32, LCI_LEAN, LCI_PACKED_RT, LCI_PACKED_FIXED, LCI_BINS, LCI_SPLIT_COLUMNS, LCI_SPLIT_BINS };

// the narrow kernels' instances: 64-bit products and every width tuple other than lineitem's read the code widths at run time; so does
// every plan under PH_SCAN_NT=0 or PH_SCAN_NARROW_GENERIC=1 (the fixed-width instances exist with non-temporal loads only)
inline FsInst narrow_inst(int32_t form, bool lineitem_widths, const ScanSwitches &s) {
    if (form == FORM_NARROW) return FSI_NARROW_RT64;
    return !s.nt || s.narrow_generic || !lineitem_widths ? FSI_NARROW_RT32 : FSI_NARROW_FIXED32;
}

// filter_sumprod: the code widths of p0, p2, b, a (Q6 over lineitem: shipdate 2, quantity 1, discount 1, extendedprice 4). No lean
// instance: built and measured, it was not clearly faster
struct FsFacts {
    int32_t form = FORM_WIDE;
    int32_t w[4] = {0, 0, 0, 0};
};
inline FsInst fs_choose(const FsFacts &f, const ScanSwitches &s) {
    if (f.form == FORM_WIDE) return FSI_WIDE;
    return narrow_inst(f.form, f.w[0] == 2 && f.w[1] == 1 && f.w[2] == 1 && f.w[3] == 4, s);
}
inline const char *fs_variant_name(FsInst i) {
    return i == FSI_WIDE ? "wide" : i == FSI_NARROW_RT64 ? "narrow64" : i == FSI_NARROW_RT32 ? "narrow_rt" : "narrow32";
}

// lowcard_chain: the code widths of p, q, e, d, t (Q1 over lineitem: shipdate 2, quantity 1, extendedprice 4, discount 1, tax 1), whether
// the plan's factors admit the lean row body, the packed scan group once one is bound and whether its layout is lineitem's, and whether
// this run's tiles per workgroup stay within LC_BINS_MAX_TILES; group_split: the bound group is in the 7-byte split form (pack_layout.h;
// lineitem's layout only), which has the two row bodies of the fixed 64-bit instances and no run-time layout
struct LcFacts {
    int32_t form = FORM_WIDE;
    int32_t w[5] = {0, 0, 0, 0, 0};
    bool lean = false, group_bound = false, group_lineitem = false;
    int32_t nslots = 0;
    bool tiles_fit = true;
    bool group_split = false;
};
inline LcInst lc_choose(const LcFacts &f, const ScanSwitches &s) {
    if (f.group_bound) {
        const bool fixed = f.group_lineitem && !s.pack_generic;
        const bool bins = fixed && s.hist && f.nslots <= LC_BINS_MAX_SLOTS && f.tiles_fit;
        if (f.group_split) return bins ? LCI_SPLIT_BINS : LCI_SPLIT_COLUMNS;
        if (bins) return LCI_BINS;
        return fixed ? LCI_PACKED_FIXED : LCI_PACKED_RT;
    }
    if (f.form == FORM_WIDE) return LCI_WIDE;
    const FsInst n = narrow_inst(f.form, f.w[0] == 2 && f.w[1] == 1 && f.w[2] == 4 && f.w[3] == 1 && f.w[4] == 1, s);
    return n == FSI_NARROW_RT64 ? LCI_NARROW_RT64 : n == FSI_NARROW_RT32 ? LCI_NARROW_RT32 : f.lean ? LCI_LEAN : LCI_NARROW_FIXED32;
}
// the plans that count towards, and bind, a packed scan group: the choice with the group ignored
inline bool lc_takes_lean(LcFacts f, const ScanSwitches &s) {
    f.group_bound = false;
    return lc_choose(f, s) == LCI_LEAN;
}
inline bool lc_takes_bins(LcInst i) { return i == LCI_BINS || i == LCI_SPLIT_BINS; }
inline bool lc_takes_split(LcInst i) { return i == LCI_SPLIT_COLUMNS || i == LCI_SPLIT_BINS; }
inline const char *lc_variant_name(LcInst i) {
    return i == LCI_WIDE ? "wide" : i == LCI_NARROW_RT64 ? "narrow64" : i == LCI_NARROW_RT32 ? "narrow_rt" : i == LCI_NARROW_FIXED32 ? "narrow32"
         : i == LCI_LEAN ? "narrow32_lean" : lc_takes_split(i) ? "split56" : "packed64";
}
inline const char *lc_row_body_name(LcInst i) { return lc_takes_bins(i) ? "bins" : "columns"; }

// A run's tiles and grid. The narrow kernels: a lane owns 16 rows, a workgroup tile is 4096 rows from row_begin rounded down to a multiple
// of 16 (rows below row_begin are masked); every other kernel loads 4-row vectors, 1024 rows a tile, from row_begin on. grid_override
// (PH_SCAN_GRID, 0 = none) replaces max_grid, clamped to partials_cap, the workgroups the plan's partials were allocated for. The bins
// body folds at most LC_BINS_MAX_TILES tiles per workgroup: a longer share raises the grid, as far as partials_cap goes; beyond that the
// columns body runs (bins = false). anchor: what a narrow run's first tile is rounded down to — 16 rows, or 4096 over a split group, whose
// blocks lie at absolute multiples of 1024 rows.
struct ScanGeometry {
    int64_t tile_rows, tiles;
    int grid;
    bool bins;
};
inline ScanGeometry scan_geometry(int64_t row_begin, int64_t rows, bool narrow, int max_grid, int grid_override, bool bins_eligible, int partials_cap,
                                   int64_t anchor = 16) {
    ScanGeometry g;
    g.tile_rows = narrow ? 4096 : 1024;
    const int64_t span = rows > 0 && narrow ? rows + (row_begin & (anchor - 1)) : rows;
    g.tiles = (span + g.tile_rows - 1) / g.tile_rows;
    if (grid_override > 0) max_grid = std::min(grid_override, partials_cap);
    g.grid = (int)std::min<int64_t>(max_grid, std::max<int64_t>(g.tiles, 1));
    g.bins = bins_eligible;
    if (g.bins && (g.tiles + g.grid - 1) / g.grid > LC_BINS_MAX_TILES) {
        const int64_t need = (g.tiles + LC_BINS_MAX_TILES - 1) / LC_BINS_MAX_TILES;
        if (need <= partials_cap) g.grid = (int)need;
        else g.bins = false;
    }
    return g;
}

}  // namespace ph
