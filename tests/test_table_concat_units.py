"""plan_amd/csrc/table_concat.h on the host: the __host__ __device__ functions ph_table_concat's kernels run per 16-byte output unit
(fixed_unit: aligned loads shifted into place, value by value across part boundaries, codes through their part's table) and per VARCHAR
row (string_row), driven tile by tile exactly as the kernels drive them, against a plain concatenation.

The program is compiled for the host only with AddressSanitizer, and every part's array is allocated at its row count rounded up to 16
bytes, tighter than a column's PH_ROW_PAD padding: a read behind the unit of a part's last value, or in front of its first, ends the
run. No GPU is involved."""
import os
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "plan_amd" / "csrc"

PROGRAM = r"""
#include "table_concat.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

namespace cc = ph::concat;
static int fails = 0;
static std::mt19937_64 rng(12345);

static void *tight(size_t bytes) { return aligned_alloc(16, (bytes + 15) / 16 * 16 + (bytes == 0 ? 16 : 0)); }

struct Case {
    std::vector<int32_t> rows, starts;
    std::vector<void *> data;
    std::vector<uint8_t *> bitmap;
    std::vector<const void *> src;
    std::vector<const uint8_t *> val;
    int64_t total = 0;
    ~Case() { for (void *p : data) free(p); for (uint8_t *p : bitmap) free(p); }
};

// parts of `rows` rows (all > 0) of W random bytes a value; with_validity: every second part has a bitmap
static void build(Case &c, const std::vector<int32_t> &rows, int W, bool with_validity) {
    c.rows = rows;
    c.starts.assign(1, 0);
    for (size_t p = 0; p < rows.size(); p++) {
        const size_t bytes = (size_t)rows[p] * W;
        unsigned char *d = (unsigned char *)tight(bytes);
        for (size_t i = 0; i < bytes; i++) d[i] = (unsigned char)rng();
        c.data.push_back(d);
        c.src.push_back(d);
        uint8_t *bm = nullptr;
        if (with_validity && p % 2 == 0) {
            const size_t vb = ((size_t)rows[p] + 7) / 8;
            bm = (uint8_t *)malloc(vb);
            for (size_t i = 0; i < vb; i++) bm[i] = (uint8_t)rng();
        }
        c.bitmap.push_back(bm);
        c.val.push_back(bm);
        c.starts.push_back(c.starts.back() + rows[p]);
    }
    c.total = c.starts.back();
}

template <int W, bool REMAP>
static void check_fixed(const std::vector<int32_t> &rows, int tile_units) {
    Case c;
    build(c, rows, W, REMAP);
    const int np = (int)rows.size();
    std::vector<uint8_t> remap((size_t)np * 256);
    std::vector<int32_t> tab((size_t)np);
    for (auto &b : remap) b = (uint8_t)rng();
    for (int p = 0; p < np; p++) tab[(size_t)p] = np - 1 - p;
    cc::Parts P{c.starts.data(), c.src.data(), REMAP ? c.val.data() : nullptr, np, (int32_t)c.total};
    constexpr int R = 16 / W;
    const int64_t padded = (c.total + 63) / 64 * 64 + 64, nunits = padded * W / 16;
    // the plain concatenation
    std::vector<unsigned char> want((size_t)(padded * W), 0);
    for (int p = 0; p < np; p++)
        for (int64_t i = 0; i < rows[(size_t)p]; i++)
            for (int b = 0; b < W; b++) {
                unsigned char x = ((const unsigned char *)c.src[(size_t)p])[i * W + b];
                if (REMAP) {
                    const bool ok = !c.val[(size_t)p] || (c.val[(size_t)p][i >> 3] >> (i & 7) & 1);
                    x = ok ? remap[(size_t)tab[(size_t)p] * 256 + x] : 0;
                }
                want[(size_t)((c.starts[(size_t)p] + i) * W + b)] = x;
            }
    for (int64_t u0 = 0; u0 < nunits; u0 += tile_units) {
        int plo = 0, phi = 0;
        if (u0 * R < c.total) {
            const int64_t r_end = (u0 + tile_units) * R;
            plo = cc::find_part(P.starts, 0, np - 1, u0 * R);
            phi = cc::find_part(P.starts, 0, np - 1, (r_end < c.total ? r_end : c.total) - 1);
        }
        for (int64_t u = u0; u < u0 + tile_units && u < nunits; u++) {
            const uint4 v = cc::fixed_unit<W, REMAP>(P, remap.data(), tab.data(), u, plo, phi);
            if (memcmp(&v, want.data() + u * 16, 16) != 0) {
                if (fails++ < 10) std::printf("W=%d REMAP=%d parts=%d tile=%d: unit %lld differs\n", W, (int)REMAP, np, tile_units, (long long)u);
            }
        }
    }
}

static void check_strings(const std::vector<int32_t> &rows) {
    // even parts are PH_STR with offsets that start above 0 and leave gaps; odd parts are codes over two dictionaries
    const int np = (int)rows.size();
    Case c;
    build(c, rows, 1, true);
    std::vector<std::vector<int32_t>> offs((size_t)np);
    std::vector<std::vector<unsigned char>> bytes((size_t)np);
    std::vector<const unsigned char *> aux((size_t)np, nullptr);
    std::vector<int32_t> tab((size_t)np);
    std::vector<int32_t> dlen(2 * 256);
    std::vector<int64_t> dpos(2 * 256);
    std::vector<unsigned char> blob;
    for (int e = 0; e < 512; e++) {
        dlen[(size_t)e] = (int32_t)(rng() % 5);
        dpos[(size_t)e] = (int64_t)blob.size();
        for (int k = 0; k < dlen[(size_t)e]; k++) blob.push_back((unsigned char)rng());
    }
    blob.push_back(0);
    for (int p = 0; p < np; p++) {
        tab[(size_t)p] = p % 2 == 0 ? -1 : (p / 2) % 2;
        if (p % 2) continue;
        auto &o = offs[(size_t)p];
        int32_t at = 3 + p;
        for (int i = 0; i < rows[(size_t)p]; i++) { o.push_back(at); at += (int32_t)(rng() % 4); }
        o.push_back(at);
        bytes[(size_t)p].resize((size_t)at + 1);
        for (auto &b : bytes[(size_t)p]) b = (unsigned char)rng();
        aux[(size_t)p] = bytes[(size_t)p].data();
        c.src[(size_t)p] = o.data();
    }
    cc::Parts P{c.starts.data(), c.src.data(), c.val.data(), np, (int32_t)c.total};
    for (int64_t r0 = 0; r0 < c.total; r0 += 256) {
        const int plo = cc::find_part(P.starts, 0, np - 1, r0);
        const int phi = cc::find_part(P.starts, 0, np - 1, (r0 + 256 < c.total ? r0 + 256 : c.total) - 1);
        for (int64_t r = r0; r < r0 + 256 && r < c.total; r++) {
            int32_t len = -1;
            int64_t begin = 0;
            cc::string_row(P, aux.data(), tab.data(), dlen.data(), dpos.data(), blob.data(), r, plo, phi, &len, &begin);
            int p = 0;
            while (c.starts[(size_t)p + 1] <= r) p++;
            const int64_t s = r - c.starts[(size_t)p];
            int32_t wlen;
            const unsigned char *wsrc;
            if (p % 2 == 0) {
                wlen = offs[(size_t)p][(size_t)s + 1] - offs[(size_t)p][(size_t)s];
                wsrc = aux[(size_t)p] + offs[(size_t)p][(size_t)s];
            } else {
                const unsigned code = ((const uint8_t *)c.src[(size_t)p])[s];
                const bool ok = !c.val[(size_t)p] || (c.val[(size_t)p][s >> 3] >> (s & 7) & 1);
                wlen = ok ? dlen[(size_t)tab[(size_t)p] * 256 + code] : 0;
                wsrc = blob.data() + dpos[(size_t)tab[(size_t)p] * 256 + code];
            }
            if (len != wlen || (wlen > 0 && blob.data() + begin != wsrc)) {
                if (fails++ < 10) std::printf("string row %lld (part %d): length %d, expected %d\n", (long long)r, p, len, wlen);
            }
        }
    }
}

template <int W>
static void both(const std::vector<int32_t> &rows, int tile) {
    check_fixed<W, false>(rows, tile);
    if (W == 1) check_fixed<1, true>(rows, tile);
}

int main() {
    const std::vector<std::vector<int32_t>> shapes = {
        {1, 7, 8, 9, 31, 33, 63, 64, 65, 2047, 8192, 8193},
        {5000},
        {16, 16, 16, 32},
        {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1},
        {3, 4099, 2, 1, 4093, 17},
    };
    for (const auto &rows : shapes)
        for (int tile : {1024, 64, 1}) {
            both<1>(rows, tile);
            both<4>(rows, tile);
            both<8>(rows, tile);
        }
    for (int k = 0; k < 40; k++) {
        std::vector<int32_t> rows((size_t)(1 + rng() % 9));
        for (auto &r : rows) r = (int32_t)(1 + rng() % (k % 2 ? 40 : 3000));
        both<1>(rows, 1024);
        both<4>(rows, 1024);
        both<8>(rows, 1024);
        check_strings(rows);
    }
    for (const auto &rows : shapes) check_strings(rows);
    if (!fails) std::printf("table_concat units ok\n");
    return fails ? 1 : 0;
}
"""


def test_units_and_string_rows_on_the_host_under_asan(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the host-only check of table_concat.h needs the HIP headers and compiler")
    src = tmp_path / "table_concat_units.hip"
    src.write_text(PROGRAM)
    exe = tmp_path / "table_concat_units"
    cc = subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address", f"-I{CSRC}",
                         f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr[-4000:]
    assert run.stdout.strip() == "table_concat units ok"
