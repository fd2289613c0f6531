// What ph_table_concat's kernels (table_concat.hip) and their sequential twin ph_validity_concat_host share: where an output row lies among
// the parts, and one 32-bit word of the concatenated validity bitmap. __host__ __device__, so the bit rules are tested without a GPU.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace ph {
namespace concat {

// The part that holds output row r: the largest p in [lo, hi] with starts[p] <= r (starts: first output row per part, starts[np] = all rows).
// A part of 0 rows shares its start with the part behind it and is never the answer for a row below the total.
template <class S>
__host__ __device__ inline int find_part(const S *starts, int lo, int hi, int64_t r) {
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int64_t)starts[mid] <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// k bits (1..32) of a bitmap from bit s on, LSB first. Reads bytes s / 8 .. (s + k - 1) / 8 only: never behind the byte of the last bit asked for.
__host__ __device__ inline uint32_t take_bits(const uint8_t *bm, int64_t s, int k) {
    const int64_t b0 = s >> 3, b1 = (s + k - 1) >> 3;   // at most 5 bytes
    uint64_t acc = 0;
    for (int64_t b = b0; b <= b1; b++) acc |= (uint64_t)bm[b] << (8 * (int)(b - b0));
    const uint32_t mask = k == 32 ? 0xffffffffu : (1u << k) - 1u;
    return (uint32_t)(acc >> (s & 7)) & mask;
}

// Word w (rows 32 w .. 32 w + 31) of the concatenation's bitmap. bitmaps: per part a bitmap or NULL = every row valid (the array itself may be
// NULL: no part has one). The word's rows may span many parts, parts of 0 rows included, and start at any bit of a source byte. Bits at and
// beyond the total are 0.
template <class S>
__host__ __device__ inline uint32_t validity_word(int64_t w, int np, const S *starts, const uint8_t *const *bitmaps) {
    const int64_t total = (int64_t)starts[np];
    int64_t r = w * 32;
    if (r >= total) return 0;
    const int64_t end = r + 32 < total ? r + 32 : total;
    int p = find_part(starts, 0, np - 1, r);
    uint32_t word = 0;
    while (r < end) {
        while ((int64_t)starts[p + 1] <= r) p++;
        const int64_t pe = (int64_t)starts[p + 1] < end ? (int64_t)starts[p + 1] : end;
        const int k = (int)(pe - r);
        const uint8_t *bm = bitmaps ? bitmaps[p] : nullptr;
        const uint32_t bits = bm ? take_bits(bm, r - (int64_t)starts[p], k) : (k == 32 ? 0xffffffffu : (1u << k) - 1u);
        word |= bits << (int)(r - w * 32);
        r = pe;
    }
    return word;
}

// one column's parts as the kernels see them (np parts of at least one row each; starts[np] = total rows)
struct Parts {
    const int32_t *starts;
    const void *const *src;            // the part's `data`
    const uint8_t *const *validity;    // per part a bitmap or NULL; NULL itself when no part has one
    int32_t np;
    int32_t total;
};

// 16 bytes from an address of any alignment, through aligned 16-byte loads of the one or two units that hold them. The second unit is
// read only when the bytes reach into it, so nothing behind the unit of the last byte is touched: with a 16-byte aligned allocation
// whose size is a multiple of 16 (every column array: PH_ROW_PAD rows) the loads stay inside it.
__host__ __device__ inline uint4 load16_any(const unsigned char *a) {
    const unsigned k = (unsigned)((uintptr_t)a & 15);
    const uint4 *base = (const uint4 *)(a - k);
    const uint4 lo = base[0];
    if (k == 0) return lo;
    const uint4 hi = base[1];
    const uint64_t q0 = (uint64_t)lo.x | (uint64_t)lo.y << 32, q1 = (uint64_t)lo.z | (uint64_t)lo.w << 32;
    const uint64_t q2 = (uint64_t)hi.x | (uint64_t)hi.y << 32, q3 = (uint64_t)hi.z | (uint64_t)hi.w << 32;
    uint64_t o0, o1;
    if (k < 8) {
        const int s = 8 * (int)k;
        o0 = q0 >> s | q1 << (64 - s);
        o1 = q1 >> s | q2 << (64 - s);
    } else if (k == 8) {
        o0 = q1;
        o1 = q2;
    } else {
        const int s = 8 * (int)(k - 8);
        o0 = q1 >> s | q2 << (64 - s);
        o1 = q2 >> s | q3 << (64 - s);
    }
    return make_uint4((unsigned)o0, (unsigned)(o0 >> 32), (unsigned)o1, (unsigned)(o1 >> 32));
}

// Unit u (16 aligned bytes: rows u R .. u R + R - 1, R = 16 / W) of a fixed-width output column; zeros at and beyond the total. plo, phi: parts
// known to hold the unit's rows between them (the tile's first and last). W = 1, 4, 8 bytes a value. REMAP (W = 1, dictionary codes): tab[p]
// names part p's 256-byte table in `remap`, and a NULL row's code is 0.
template <int W, bool REMAP>
__host__ __device__ inline uint4 fixed_unit(const Parts &P, const uint8_t *remap, const int32_t *tab, int64_t u, int plo, int phi) {
    static_assert(!REMAP || W == 1, "codes are bytes");
    constexpr int R = 16 / W;
    const int64_t r = u * R, total = P.total;
    uint32_t d[4] = {0, 0, 0, 0};
    if (r >= total) return make_uint4(0, 0, 0, 0);
    int p = plo == phi ? plo : find_part(P.starts, plo, phi, r);
    const int64_t ps = P.starts[p];
    if (r + R <= (int64_t)P.starts[p + 1]) {   // the unit lies inside part p
        const uint4 v = load16_any((const unsigned char *)P.src[p] + (r - ps) * W);
        if (!REMAP) return v;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        const uint8_t *t = remap + (int64_t)tab[p] * 256;
        const uint8_t *bm = P.validity ? P.validity[p] : nullptr;
        const uint32_t ok = bm ? take_bits(bm, r - ps, 16) : 0xffffu;
        uint32_t m[4] = {0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 16; e++)
            if (ok >> e & 1) m[e >> 2] |= (uint32_t)t[(d[e >> 2] >> (8 * (e & 3))) & 255u] << (8 * (e & 3));
        return make_uint4(m[0], m[1], m[2], m[3]);
    }
    // the unit crosses a part boundary or the end of the rows: value by value
#pragma unroll
    for (int e = 0; e < R; e++) {
        const int64_t re = r + e;
        if (re >= total) continue;
        while ((int64_t)P.starts[p + 1] <= re) p++;
        const int64_t s = re - (int64_t)P.starts[p];
        if (W == 8) {
            const uint64_t x = ((const uint64_t *)P.src[p])[s];
            d[(2 * e) & 3] = (uint32_t)x;
            d[(2 * e + 1) & 3] = (uint32_t)(x >> 32);
        } else if (W == 4) {
            d[e & 3] = ((const uint32_t *)P.src[p])[s];
        } else {
            uint32_t x = ((const uint8_t *)P.src[p])[s];
            if (REMAP) {
                const uint8_t *bm = P.validity ? P.validity[p] : nullptr;
                x = (bm && !(bm[s >> 3] >> (s & 7) & 1)) ? 0u : remap[(int64_t)tab[p] * 256 + x];
            }
            d[(e >> 2) & 3] |= x << (8 * (e & 3));
        }
    }
    return make_uint4(d[0], d[1], d[2], d[3]);
}

// VARCHAR, output row r (below the total): its length, and where its bytes lie as a distance from `blob` (what copy_strings_kernel adds to its
// text pointer). tab[p] < 0: part p is PH_STR (offsets in src, bytes in aux[p]: the length is off[i + 1] - off[i], whatever the offsets start
// at). Else part p holds codes and dlen / dpos[tab[p] * 256 + code] are the entry's length and position in the blob; a NULL row is empty.
__host__ __device__ inline void string_row(const Parts &P, const unsigned char *const *aux, const int32_t *tab, const int32_t *dlen, const int64_t *dpos,
                                           const unsigned char *blob, int64_t r, int plo, int phi, int32_t *len, int64_t *begin) {
    const int p = plo == phi ? plo : find_part(P.starts, plo, phi, r);
    const int64_t s = r - (int64_t)P.starts[p];
    if (tab[p] < 0) {
        const int32_t *off = (const int32_t *)P.src[p];
        const int32_t b = off[s];
        *len = off[s + 1] - b;
        *begin = (int64_t)((uintptr_t)aux[p] + (uintptr_t)(int64_t)b - (uintptr_t)blob);
    } else {
        const uint32_t code = ((const uint8_t *)P.src[p])[s];
        const uint8_t *bm = P.validity ? P.validity[p] : nullptr;
        const bool null = bm && !(bm[s >> 3] >> (s & 7) & 1);
        const int64_t e = (int64_t)tab[p] * 256 + code;
        *len = null ? 0 : dlen[e];
        *begin = dpos[e];
    }
}

}  // namespace concat
}  // namespace ph
