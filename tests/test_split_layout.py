"""plan_amd/csrc/pack_layout.h on the host: the 7-byte split form of lineitem's scan group (DESIGN.md §3 "The split form").

A g++ program prints what the header's functions give for every row of a block and for a set of quads; numpy restates the layout from
the issue's words and compares:
 * the row -> low dword and (row, r3) -> high dword maps are bijections onto a block's 1792 dwords;
 * a lane's loads 4..6 (dwords 1024 + 256 m + 4 l + c) hold exactly the twelve high dwords of the quads of its loads 0..3;
 * split_quad_encode / split_quad_decode round-trip, rows 0..2 are the low 24 bits of A, B, C, and row 3 comes out of the three top
   bytes in the right order: its values have three distinct bytes, so a wrong byte selector cannot pass."""
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]

# h3 values: the edges the issue names, then values whose three bytes differ
H3 = [0x000000, 0x7FFFFF, 0x0000FF, 0x00FF00, 0x7F0000, 0x123456, 0x7EDCBA, 0x010203, 0x6500FE, 0x00A17C]
H012 = [(0x000000, 0x000000, 0x000000), (0x7FFFFF, 0x7FFFFF, 0x7FFFFF), (0x0000FF, 0x00FF00, 0x7F0000), (0x654321, 0x0ABCDE, 0x7F00F1)]

PROGRAM = r"""
#include "pack_layout.h"
#include <cstdio>
#include <cstdlib>

using namespace ph;
static_assert(SPLIT_BLOCK_ROWS == 1024 && SPLIT_BLOCK_DWORDS == 1792 && SPLIT_BLOCK_BYTES == 7168 && SPLIT_LOW_DWORDS == 1024, "");
static_assert(split_group_bytes(8192) == 8192 * 7, "");
// constexpr through and through: a quad that round-trips at compile time
constexpr uint32_t round_trip_h3(uint32_t a, uint32_t b, uint32_t c, uint32_t h3) {
    uint32_t h[4] = {a, b, c, h3}, d[3] = {}, g[4] = {};
    split_quad_encode(h, d);
    split_quad_decode(d, g);
    return g[0] == a && g[1] == b && g[2] == c ? g[3] : 0xffffffffu;
}
static_assert(round_trip_h3(1, 2, 3, 0x123456) == 0x123456, "");

int main(int argc, char **argv) {
    for (int r = 0; r < SPLIT_BLOCK_ROWS; r++)
        std::printf("row %d %d %d %d %d %d %d %d\n", r, split_lane(r), split_load(r), split_role(r), split_low_dword(r), split_high_dword(r, 0),
                    split_high_dword(r, 1), split_high_dword(r, 2));
    for (int l = 0; l < 64; l++)
        for (int i = 0; i < 12; i++) std::printf("lane %d %d %d\n", l, i, split_lane_high_dword(l, i));
    for (int a = 1; a + 3 < argc; a += 4) {
        uint32_t h[4], d[3], g[4];
        for (int k = 0; k < 4; k++) h[k] = (uint32_t)std::strtoul(argv[a + k], nullptr, 0);
        split_quad_encode(h, d);
        split_quad_decode(d, g);
        std::printf("quad %u %u %u %u %u %u %u %u %u %u %u\n", h[0], h[1], h[2], h[3], d[0], d[1], d[2], g[0], g[1], g[2], g[3]);
    }
    std::printf("lineitem %d %d\n", (int)LCP_LINEITEM.ok, (int)split_layout_fits(LCP_LINEITEM));
    return 0;
}
"""


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the host-only check of pack_layout.h needs a C++17 host compiler")
    tmp = tmp_path_factory.mktemp("split_layout")
    src = tmp / "split_layout_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp / "split_layout_check"
    cc = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'plan_amd' / 'csrc'}", str(src), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    args = [hex(v) for h012 in H012 for h3 in H3 for v in (*h012, h3)]
    run = subprocess.run([str(exe)] + args, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    out = {"row": [], "lane": [], "quad": [], "lineitem": []}
    for line in run.stdout.split("\n"):
        if line:
            out[line.split()[0]].append([int(x) for x in line.split()[1:]])
    return {k: np.array(v, dtype=np.int64) for k, v in out.items()}


def test_row_maps_are_bijections_onto_the_block(printed):
    rows = printed["row"]
    assert rows.shape == (1024, 8) and list(rows[:, 0]) == list(range(1024))
    r = rows[:, 0]
    # the restated maps: a lane's load j is the quad of rows 256 j + 4 l + k
    assert (rows[:, 1] == (r >> 2) % 64).all() and (rows[:, 2] == r // 256).all() and (rows[:, 3] == r % 4).all()
    assert (r == 256 * rows[:, 2] + 4 * rows[:, 1] + rows[:, 3]).all()
    assert (rows[:, 4] == r).all()                                     # low dwords in row order
    low = set(rows[:, 4])
    assert low == set(range(1024))
    # the three high dwords of a quad are the same for its four rows, and all quads' together fill dwords 1024..1791 once
    quads = rows.reshape(256, 4, 8)
    assert (quads[:, :, 5:] == quads[:, :1, 5:]).all()
    high = quads[:, 0, 5:].reshape(-1)
    assert len(high) == 768 and set(high) == set(range(1024, 1792))
    assert low | set(high) == set(range(1792))


def test_a_lanes_high_loads_hold_its_own_quads(printed):
    lanes = printed["lane"]
    assert lanes.shape == (64 * 12, 3)
    l, i, dw = lanes[:, 0], lanes[:, 1], lanes[:, 2]
    # dword 1024 + 256 m + 4 l + c holds D[4 m + c]: component c of the lane's 16-byte load 4 + m at byte 4096 + 1024 m + 16 l
    assert (dw == 1024 + 256 * (i // 4) + 4 * l + i % 4).all()
    assert (dw * 4 == 4096 + 1024 * (i // 4) + 16 * l + 4 * (i % 4)).all()
    by_lane = {(int(a), int(b)): int(c) for a, b, c in lanes}
    for row in printed["row"]:
        r, lane, j = int(row[0]), int(row[1]), int(row[2])
        # the lane that loads the row's low dword (load j at byte 1024 j + 16 l) also loads its quad's dwords D[3 j + r3]
        assert r * 4 // 1024 == j and (r * 4 % 1024) // 16 == lane
        assert [int(x) for x in row[5:]] == [by_lane[(lane, 3 * j + r3)] for r3 in range(3)]
    assert sorted(by_lane.values()) == list(range(1024, 1792))


def test_quad_encode_and_decode(printed):
    quads = printed["quad"]
    assert len(quads) == len(H3) * len(H012)
    assert {int(h) for h in quads[:, 3]} == set(H3)
    for h3 in H3[5:]:
        assert len({h3 & 0xFF, h3 >> 8 & 0xFF, h3 >> 16}) == 3
    for h0, h1, h2, h3, a, b, c, g0, g1, g2, g3 in (map(int, q) for q in quads):
        assert (a, b, c) == (h0 | (h3 & 0xFF) << 24, h1 | (h3 >> 8 & 0xFF) << 24, h2 | (h3 >> 16) << 24)
        assert a < 2 ** 32 and b < 2 ** 32 and c < 2 ** 32
        assert (a & 0xFFFFFF, b & 0xFFFFFF, c & 0xFFFFFF) == (h0, h1, h2)          # rows 0..2: read in place
        assert (g0, g1, g2, g3) == (h0, h1, h2, h3)
        assert g3 == (a >> 24) | (b >> 24) << 8 | (c >> 24) << 16                   # row 3: the three top bytes, A's lowest


def test_lineitems_layout_admits_the_split(printed):
    assert [int(x) for x in printed["lineitem"][0]] == [1, 1]
