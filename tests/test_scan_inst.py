"""plan_amd/csrc/scan_inst.h on the host: which kernel instance a fused scan launches, and a run's grid geometry.

The header has no HIP in it, so a plain g++ program checks it, as tests/test_dispatch.py does for dispatch.h:
 * lc_choose and fs_choose over the full product of their inputs against the table of DESIGN.md §4.1 "Which instance runs", restated
   below row by row (first matching row wins);
 * the variant and row-body name of every instance, "takes lean" (the choice with the group ignored) and "takes bins";
 * scan_geometry at the bins body's bound of 1023 tiles a workgroup, beyond the partials' capacity, at an unaligned row_begin, over no
   rows, and under a grid override on both sides of the capacity."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]

PROGRAM = r"""
#include "scan_inst.h"
#include <cstdio>
#include <cstring>
#include <initializer_list>

using namespace ph;
static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); fails++; } } while (0)

// DESIGN.md §4.1, "Which instance runs": lowcard_chain
static LcInst lc_table(int form, bool lineitem_widths, bool lean, bool group, bool group_lineitem, int nslots, bool tiles_fit, const ScanSwitches &s) {
    if (group && group_lineitem && !s.pack_generic && s.hist && nslots <= 6 && tiles_fit) return LCI_BINS;
    if (group && group_lineitem && !s.pack_generic) return LCI_PACKED_FIXED;
    if (group) return LCI_PACKED_RT;
    if (form == FORM_WIDE) return LCI_WIDE;
    if (form == FORM_NARROW) return LCI_NARROW_RT64;
    if (!lineitem_widths || !s.nt || s.narrow_generic) return LCI_NARROW_RT32;
    if (lean) return LCI_LEAN;
    return LCI_NARROW_FIXED32;
}
// and filter_sumprod
static FsInst fs_table(int form, bool lineitem_widths, const ScanSwitches &s) {
    if (form == FORM_WIDE) return FSI_WIDE;
    if (form == FORM_NARROW) return FSI_NARROW_RT64;
    if (!lineitem_widths || !s.nt || s.narrow_generic) return FSI_NARROW_RT32;
    return FSI_NARROW_FIXED32;
}

static bool geo(int64_t row_begin, int64_t rows, bool narrow, int max_grid, int override_, bool bins, int cap, int64_t tiles, int grid, bool want_bins) {
    const ScanGeometry g = scan_geometry(row_begin, rows, narrow, max_grid, override_, bins, cap);
    if (g.tiles == tiles && g.grid == grid && g.bins == want_bins && g.tile_rows == (narrow ? 4096 : 1024)) return true;
    std::printf("  got tiles %lld grid %d bins %d\n", (long long)g.tiles, g.grid, (int)g.bins);
    return false;
}

int main() {
    const int LC_W[5] = {2, 1, 4, 1, 1}, FS_W[4] = {2, 1, 1, 4};
    long n = 0;
    for (int bits = 0; bits < 64; bits++) {
        ScanSwitches s;
        s.nt = bits & 1; s.narrow_generic = bits & 2; s.pack_generic = bits & 4; s.lean = bits & 8; s.tail = bits & 16; s.hist = bits & 32;
        for (int form : {FORM_WIDE, FORM_NARROW, FORM_NARROW32})
            for (int odd = -1; odd < 5; odd++)   // -1: lineitem's widths; else that width differs
                for (int lean = 0; lean < 2; lean++) for (int group = 0; group < 2; group++) for (int gl = 0; gl < 2; gl++)
                    for (int nslots : {1, 6, 7, 12}) for (int fit = 0; fit < 2; fit++) {
                        LcFacts f;
                        f.form = form;
                        for (int i = 0; i < 5; i++) f.w[i] = LC_W[i] == 4 && i == odd ? 2 : i == odd ? LC_W[i] + 1 : LC_W[i];
                        f.lean = lean; f.group_bound = group; f.group_lineitem = gl; f.nslots = nslots; f.tiles_fit = fit;
                        const LcInst got = lc_choose(f, s), want = lc_table(form, odd < 0, lean, group, gl, nslots, fit, s);
                        if (got != want) { std::printf("lc_choose: bits %d form %d odd %d lean %d group %d/%d slots %d fit %d: %d, expected %d\n", bits, form, odd, lean, group, gl, nslots, fit, got, want); fails++; }
                        // "takes lean" ignores the group; "takes bins" is the chosen instance
                        CHECK(lc_takes_lean(f, s) == (lc_table(form, odd < 0, lean, false, false, nslots, fit, s) == LCI_LEAN));
                        CHECK(lc_takes_bins(got) == (want == LCI_BINS));
                        n++;
                    }
        for (int form : {FORM_WIDE, FORM_NARROW, FORM_NARROW32})
            for (int odd = -1; odd < 4; odd++) {
                FsFacts f;
                f.form = form;
                for (int i = 0; i < 4; i++) f.w[i] = FS_W[i] == 4 && i == odd ? 2 : i == odd ? FS_W[i] + 1 : FS_W[i];
                CHECK(fs_choose(f, s) == fs_table(form, odd < 0, s));
            }
    }
    CHECK(n == 64 * 3 * 6 * 2 * 2 * 2 * 4 * 2);
    // ---- names
    const char *lc_variant[8] = {"wide", "narrow64", "narrow_rt", "narrow32", "narrow32_lean", "packed64", "packed64", "packed64"};
    const LcInst lc_all[8] = {LCI_WIDE, LCI_NARROW_RT64, LCI_NARROW_RT32, LCI_NARROW_FIXED32, LCI_LEAN, LCI_PACKED_RT, LCI_PACKED_FIXED, LCI_BINS};
    for (int i = 0; i < 8; i++) {
        CHECK(!std::strcmp(lc_variant_name(lc_all[i]), lc_variant[i]));
        CHECK(!std::strcmp(lc_row_body_name(lc_all[i]), lc_all[i] == LCI_BINS ? "bins" : "columns"));
    }
    const char *fs_variant[4] = {"wide", "narrow64", "narrow_rt", "narrow32"};
    const FsInst fs_all[4] = {FSI_WIDE, FSI_NARROW_RT64, FSI_NARROW_RT32, FSI_NARROW_FIXED32};
    for (int i = 0; i < 4; i++) CHECK(!std::strcmp(fs_variant_name(fs_all[i]), fs_variant[i]));
    // ---- geometry: (row_begin, rows, narrow, max_grid, override, bins eligible, partials' capacity) -> tiles, grid, bins
    const int64_t T = 4096;
    CHECK(geo(0, 512 * 1023 * T, true, 512, 0, true, 8192, 512 * 1023, 512, true));               // exactly 1023 tiles a workgroup: as it is
    CHECK(geo(0, 512 * 1023 * T + 1, true, 512, 0, true, 8192, 512 * 1023 + 1, 513, true));        // 1024 for one: ceil(tiles / 1023) workgroups
    CHECK(geo(0, 512 * 1024 * T, true, 512, 0, true, 8192, 512 * 1024, 513, true));                // 1024 for all: ceil(524288 / 1023) = 513
    CHECK(geo(0, 512 * 1024 * T, true, 512, 0, false, 8192, 512 * 1024, 512, false));              // not eligible: the grid stays
    CHECK(geo(0, 8192ll * 1023 * T, true, 8, 0, true, 8192, 8192 * 1023, 8192, true));             // the last span the capacity serves
    CHECK(geo(0, 8192ll * 1023 * T + 1, true, 8, 0, true, 8192, 8192 * 1023 + 1, 8, false));       // beyond it: the columns body, the grid stays
    CHECK(geo(0, 9000ll * 1023 * T, true, 512, 0, true, 16384, 9000 * 1023, 9000, true));          // a larger capacity serves a longer span
    CHECK(geo(16, 2 * T, true, 512, 0, true, 8192, 2, 2, true));                                   // row_begin on a lane boundary
    CHECK(geo(17, 2 * T, true, 512, 0, true, 8192, 3, 3, true));                                   // row_begin & 15 != 0: the span grows by it
    CHECK(geo(15, 2 * T - 15, true, 512, 0, true, 8192, 2, 2, true));
    CHECK(geo(4, 2 * 1024, false, 512, 0, false, 8192, 2, 2, false));                              // the 4-row-vector kernels: 1024 rows a tile, no rounding
    CHECK(geo(4, 2 * 1024 + 1, false, 512, 0, false, 8192, 3, 3, false));
    CHECK(geo(7, 0, true, 512, 0, true, 8192, 0, 1, true));                                        // no rows: one workgroup
    CHECK(geo(0, 0, false, 512, 0, false, 8192, 0, 1, false));
    CHECK(geo(0, 100000 * T, true, 512, 10000, false, 8192, 100000, 8192, false));                 // an override above the capacity: clamped
    CHECK(geo(0, 100000 * T, true, 512, 4000, false, 8192, 100000, 4000, false));                  // below: taken
    CHECK(geo(0, 100000 * T, true, 512, 1, true, 8192, 100000, 98, true));                         // bins under PH_SCAN_GRID=1: ceil(100000 / 1023)
    CHECK(geo(0, 100 * T, true, 512, 1, true, 8192, 100, 1, true));
    CHECK(geo(0, 100000 * T, true, 512, -3, false, 8192, 100000, 512, false));                     // not positive: no override
    CHECK(geo(0, 3 * T, true, 512, 0, false, 8192, 3, 3, false));                                  // fewer tiles than workgroups
    if (!fails) std::printf("scan_inst ok\n");
    return fails ? 1 : 0;
}
"""


def test_scan_inst_on_the_host(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the host-only check of scan_inst.h needs a C++17 host compiler")
    src = tmp_path / "scan_inst_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "scan_inst_check"
    cc = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'plan_amd' / 'csrc'}", str(src), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "scan_inst ok"
