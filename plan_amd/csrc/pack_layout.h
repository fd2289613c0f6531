// Where the fields of a packed scan group lie in its 64-bit word, and where the word's parts lie in a group of the split form
// (ph_table::scangroup). Host only, no device needed.
#pragma once
#include <cstdint>

namespace ph {

// the fields of a lowcard_chain scan group: the codes of p, q, e, d, t (value - min, as in the narrowed copies) and the dense group slot
constexpr int PACK_NFIELDS = 6;
enum PackField { PF_P = 0, PF_Q, PF_E, PF_D, PF_T, PF_SLOT };

// bits a field needs for codes 0 .. span: the length of span in bits, at least 1
constexpr int pack_bits(uint64_t span) {
    int b = 1;
    while (b < 64 && (span >> b) != 0) b++;
    return b;
}

// First fit, largest first (ties in the order given), into the two dwords of the word: no field straddles the dword boundary, so a field is
// one 32-bit extract. shift[i] = position of field i in the word (0..63; bit 5 names the dword). false: a field is wider than a dword or
// has no bits, or the fields do not fit (more than 64 bits, or no placement without a straddle by this rule).
constexpr bool pack_layout(int n, const int32_t *width, int32_t *shift) {
    if (n < 1 || n > 64) return false;
    bool placed[64] = {};
    int used[2] = {0, 0};
    for (int i = 0; i < n; i++)
        if (width[i] < 1 || width[i] > 32) return false;
    for (int k = 0; k < n; k++) {
        int best = -1;
        for (int i = 0; i < n; i++)
            if (!placed[i] && (best < 0 || width[i] > width[best])) best = i;
        const int dw = used[0] + width[best] <= 32 ? 0 : used[1] + width[best] <= 32 ? 1 : -1;
        if (dw < 0) return false;
        shift[best] = 32 * dw + used[dw];
        used[dw] += width[best];
        placed[best] = true;
    }
    return true;
}

// the layout of TPC-H lineitem's Q1 columns (the bits of shipdate, quantity, extendedprice, discount, tax and of six slots; the same at
// every scale factor): the packed kernels have an instance with these field positions fixed at compile time
struct PackLayout {
    int32_t width[PACK_NFIELDS], shift[PACK_NFIELDS];
    bool ok;
};
constexpr PackLayout lineitem_pack_layout() {
    PackLayout L = {{12, 6, 24, 4, 4, 3}, {}, false};
    L.ok = pack_layout(PACK_NFIELDS, L.width, L.shift);
    return L;
}
constexpr PackLayout LCP_LINEITEM = lineitem_pack_layout();
static_assert(LCP_LINEITEM.ok, "lineitem's 53 bits fit one word");

template <class T> inline bool is_lineitem_layout(const T *shift, const T *width) {
    for (int f = 0; f < PACK_NFIELDS; f++)
        if (shift[f] != LCP_LINEITEM.shift[f] || width[f] != LCP_LINEITEM.width[f]) return false;
    return true;
}

// ---- the split form of lineitem's group (DESIGN.md §3 "The split form"): 7 bytes a row instead of 8
// The form of a scan group: one 64-bit word a row, or — lineitem's layout only — the word's low dword and the 24 bits of its high dword
// that hold fields, stored apart in blocks of 1024 rows.
enum ScanGroupForm : int32_t { SG_WORD64 = 0, SG_SPLIT56 = 1 };

// fields of the high dword end below this bit
constexpr int SPLIT_HIGH_BITS = 24;
constexpr bool split_layout_fits(const PackLayout &L) {
    int low = 0;
    for (int f = 0; f < PACK_NFIELDS; f++) {
        if (L.shift[f] >= 32 && L.shift[f] - 32 + L.width[f] > SPLIT_HIGH_BITS) return false;
        if (L.shift[f] < 32) low += L.width[f];
    }
    return low <= 32;
}
static_assert(split_layout_fits(LCP_LINEITEM), "lineitem's high-dword fields end below bit 24 and its low-dword fields fill no more than 32 bits");

// A split group is a sequence of blocks, one per SPLIT_BLOCK_ROWS rows: block c covers rows 1024 c .. 1024 c + 1023 and is
// SPLIT_BLOCK_DWORDS dwords long. The table is padded to a multiple of 4096 rows and the padding zero-filled, so the four blocks of a
// 4096-row tile that starts inside the padded table lie inside the allocation.
//   dwords 0 .. 1023     the rows' low dwords in row order. A wave's lane l loads four of them at once, load j (0..3) at dword 256 j + 4 l:
//                        rows 256 j + 4 l + k (k = 0..3) of the block, a "quad"
//   dwords 1024 .. 1791  the 24-bit high parts h0..h3 of every quad as three dwords (split_quad_encode): the lane's four quads give twelve
//                        dwords D[3 j + r] (r = 0..2); dword 1024 + 256 m + 4 l + c holds D[4 m + c], so the lane's loads 4 + m (m = 0..2)
//                        at dword 1024 + 256 m + 4 l are exactly its own rows' high parts
// Every wave-instruction of the seven reads 1024 consecutive bytes and a wave's seven cover its block end to end.
constexpr int SPLIT_BLOCK_ROWS = 1024, SPLIT_LOW_DWORDS = 1024, SPLIT_BLOCK_DWORDS = 1792, SPLIT_BLOCK_BYTES = SPLIT_BLOCK_DWORDS * 4;
constexpr int64_t split_group_bytes(int64_t padded_rows) { return padded_rows / SPLIT_BLOCK_ROWS * SPLIT_BLOCK_BYTES; }

// row r of a block (0..1023): the lane that reads it, which of the lane's four low loads, and its place in the quad
constexpr int split_lane(int r) { return (r >> 2) & 63; }
constexpr int split_load(int r) { return r >> 8; }
constexpr int split_role(int r) { return r & 3; }
// its low dword's index in the block
constexpr int split_low_dword(int r) { return r; }
// the index in the block of dword i (0..11) of lane l's twelve high dwords
constexpr int split_lane_high_dword(int l, int i) { return SPLIT_LOW_DWORDS + 256 * (i >> 2) + 4 * l + (i & 3); }
// the index in the block of dword r3 (0..2: A, B, C) of row r's quad. A row of role 0..2 has its high part in the low 24 bits of dword
// `role`; a row of role 3 has one byte of it in the top byte of each of the three.
constexpr int split_high_dword(int r, int r3) { return split_lane_high_dword(split_lane(r), 3 * split_load(r) + r3); }

// a quad's three dwords from its rows' 24-bit high parts, and back
constexpr void split_quad_encode(const uint32_t h[4], uint32_t d[3]) {
    d[0] = h[0] | (h[3] & 0xffu) << 24;
    d[1] = h[1] | (h[3] >> 8 & 0xffu) << 24;
    d[2] = h[2] | (h[3] >> 16) << 24;
}
constexpr void split_quad_decode(const uint32_t d[3], uint32_t h[4]) {
    h[0] = d[0] & 0xffffffu;
    h[1] = d[1] & 0xffffffu;
    h[2] = d[2] & 0xffffffu;
    h[3] = d[0] >> 24 | d[1] >> 24 << 8 | d[2] >> 24 << 16;
}

}  // namespace ph
