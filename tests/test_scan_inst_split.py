"""plan_amd/csrc/scan_inst.h on the host, with a split scan group bound (LcFacts::group_split): which instance runs, and the geometry of
a run whose tiles are anchored at multiples of 4096 rows. A plain g++ program, as tests/test_scan_inst.py:
 * lc_choose over the full product of its inputs with group_split set, against the table of DESIGN.md §4.1 restated below (split
   bins under exactly the conditions of the 64-bit bins instance, otherwise split columns; without a bound group the flag is ignored);
 * the names of the two instances, "takes bins" and "takes split";
 * scan_geometry with anchor 4096 at row_begin 0, 1, 4095, 4096, 4097, and at the bins body's bound of 1023 tiles a workgroup."""
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

// DESIGN.md §4.1, "Which instance runs": lowcard_chain with a split group
static LcInst lc_table(int form, bool lineitem_widths, bool lean, bool group, bool group_lineitem, int nslots, bool tiles_fit, const ScanSwitches &s) {
    if (group && group_lineitem && !s.pack_generic && s.hist && nslots <= 6 && tiles_fit) return LCI_SPLIT_BINS;
    if (group) return LCI_SPLIT_COLUMNS;
    if (form == FORM_WIDE) return LCI_WIDE;
    if (form == FORM_NARROW) return LCI_NARROW_RT64;
    if (!lineitem_widths || !s.nt || s.narrow_generic) return LCI_NARROW_RT32;
    if (lean) return LCI_LEAN;
    return LCI_NARROW_FIXED32;
}

static bool geo(int64_t row_begin, int64_t rows, int max_grid, int override_, bool bins, int cap, int64_t tiles, int grid, bool want_bins) {
    const ScanGeometry g = scan_geometry(row_begin, rows, true, max_grid, override_, bins, cap, 4096);
    if (g.tiles == tiles && g.grid == grid && g.bins == want_bins && g.tile_rows == 4096) return true;
    std::printf("  got tiles %lld grid %d bins %d\n", (long long)g.tiles, g.grid, (int)g.bins);
    return false;
}

int main() {
    const int LC_W[5] = {2, 1, 4, 1, 1};
    static_assert(LCI_SPLIT_COLUMNS == LCI_BINS + 1 && LCI_SPLIT_BINS == LCI_BINS + 2, "appended");
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
                        f.group_split = true;
                        const LcInst got = lc_choose(f, s), want = lc_table(form, odd < 0, lean, group, gl, nslots, fit, s);
                        if (got != want) { std::printf("lc_choose: bits %d form %d odd %d lean %d group %d/%d slots %d fit %d: %d, expected %d\n", bits, form, odd, lean, group, gl, nslots, fit, got, want); fails++; }
                        // the same facts without the flag: the 64-bit instance with the same row body, or the same instance without a group
                        f.group_split = false;
                        const LcInst word = lc_choose(f, s);
                        CHECK(lc_takes_bins(got) == lc_takes_bins(word) && lc_takes_bins(got) == (want == LCI_SPLIT_BINS));
                        CHECK(lc_takes_split(got) == (group != 0) && !lc_takes_split(word));
                        CHECK(group || got == word);
                        f.group_split = true;
                        CHECK(lc_takes_lean(f, s) == (lc_table(form, odd < 0, lean, false, false, nslots, fit, s) == LCI_LEAN));
                        n++;
                    }
    }
    CHECK(n == 64 * 3 * 6 * 2 * 2 * 2 * 4 * 2);
    // ---- names
    for (LcInst i : {LCI_SPLIT_COLUMNS, LCI_SPLIT_BINS}) {
        CHECK(!std::strcmp(lc_variant_name(i), "split56"));
        CHECK(!std::strcmp(lc_row_body_name(i), i == LCI_SPLIT_BINS ? "bins" : "columns"));
        CHECK(lc_takes_split(i));
    }
    CHECK(!lc_takes_split(LCI_BINS) && !lc_takes_split(LCI_PACKED_FIXED) && !lc_takes_split(LCI_LEAN));
    CHECK(lc_takes_bins(LCI_BINS) && lc_takes_bins(LCI_SPLIT_BINS) && !lc_takes_bins(LCI_SPLIT_COLUMNS));
    // ---- geometry with tiles anchored at multiples of 4096: (row_begin, rows, max_grid, override, bins eligible, capacity) -> tiles, grid, bins
    const int64_t T = 4096;
    CHECK(geo(0, 2 * T, 512, 0, true, 8192, 2, 2, true));
    CHECK(geo(1, 2 * T, 512, 0, true, 8192, 3, 3, true));                 // the span grows by row_begin & 4095
    CHECK(geo(1, 2 * T - 1, 512, 0, true, 8192, 2, 2, true));
    CHECK(geo(4095, 1, 512, 0, true, 8192, 1, 1, true));                  // the last row of the first tile
    CHECK(geo(4095, 2, 512, 0, true, 8192, 2, 2, true));                  // ... and the first of the second
    CHECK(geo(4096, T, 512, 0, true, 8192, 1, 1, true));                  // on the anchor: nothing to mask
    CHECK(geo(4097, T, 512, 0, true, 8192, 2, 2, true));
    CHECK(geo(4097, T - 1, 512, 0, true, 8192, 1, 1, true));
    CHECK(geo(4097, 0, 512, 0, true, 8192, 0, 1, true));                  // no rows: one workgroup
    CHECK(geo(17, 2 * T, 512, 0, true, 8192, 3, 3, true) && scan_geometry(17, 2 * T - 17, true, 512, 0, true, 8192).tiles == 2);   // (anchor 16: 2 tiles)
    CHECK(geo(0, 512 * 1023 * T, 512, 0, true, 8192, 512 * 1023, 512, true));            // exactly 1023 tiles a workgroup
    CHECK(geo(1, 512 * 1023 * T, 512, 0, true, 8192, 512 * 1023 + 1, 513, true));        // one row further down: one tile more, one workgroup more
    CHECK(geo(4095, 512 * 1023 * T - 4095, 512, 0, true, 8192, 512 * 1023, 512, true));
    CHECK(geo(0, 1023 * T, 512, 1, true, 8192, 1023, 1, true));                          // PH_SCAN_GRID=1: 1023 tiles in one workgroup
    CHECK(geo(0, 1024 * T, 512, 1, true, 8192, 1024, 2, true));                          // one tile more: two workgroups
    CHECK(geo(4095, 1023 * T - 4094, 512, 1, true, 8192, 1024, 2, true));
    CHECK(geo(0, 8192ll * 1023 * T + 1, 8, 0, true, 8192, 8192 * 1023 + 1, 8, false));   // beyond the capacity: the columns body
    if (!fails) std::printf("scan_inst split ok\n");
    return fails ? 1 : 0;
}
"""


def test_scan_inst_with_a_split_group_on_the_host(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the host-only check of scan_inst.h needs a C++17 host compiler")
    src = tmp_path / "scan_inst_split_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "scan_inst_split_check"
    cc = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'plan_amd' / 'csrc'}", str(src), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "scan_inst split ok"
