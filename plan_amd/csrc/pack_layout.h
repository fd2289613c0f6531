// Where the fields of a packed scan group lie in its 64-bit word (ph_table::scangroup). Host only, no device needed.
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

inline bool is_lineitem_layout(const uint8_t *shift, const uint8_t *width) {
    for (int f = 0; f < PACK_NFIELDS; f++)
        if (shift[f] != LCP_LINEITEM.shift[f] || width[f] != LCP_LINEITEM.width[f]) return false;
    return true;
}

}  // namespace ph
