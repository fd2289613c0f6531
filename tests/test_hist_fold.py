"""The fold of the bins row body of the packed Q1 scan (lch_fold in scan_kernels.hip, DESIGN.md §4.1 "Bins by (slot, discount, tax)"),
restated in Python with the kernel's word formats and 64-bit wrapping arithmetic, against sums of per-row products in Python integers.
No GPU: this pins the algebra and the field widths; tests/test_gpu_hist_scan.py pins the kernel."""
import random

M64 = (1 << 64) - 1
CNT_SHIFT = 44
MAX_TILES = 1023          # LC_BINS_MAX_TILES
ROWS_PER_WAVE_TILE = 1024


def s64(x):
    """a 64-bit word as the signed integer the partials hold"""
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def fold(bins, qsum, ns, A1c, B1c, A2c, B2c, e_base, q_base, d_base):
    """bins[wave][slot * 256 + (t << 4 | d)]: packed words; qsum[slot]: the lanes' Σ q code. Returns per slot
    [Σq, Σe, Σe·f1, Σe·f1·f2, Σd, count] as lch_fold forms them: every step modulo 2^64"""
    out = []
    for s in range(ns):
        v = [0] * 6
        for j in range(256):
            d, t = j & 15, j >> 4
            n = sum(w[s * 256 + j] >> CNT_SHIFT for w in bins)
            E = sum(w[s * 256 + j] & ((1 << CNT_SHIFT) - 1) for w in bins)
            f1, f2 = (A1c + B1c * d) & M64, (A2c + B2c * t) & M64
            ev = ((e_base & M64) * n + E) & M64
            dp = (f1 * ev) & M64
            ch = (f2 * dp) & M64
            for a, x in enumerate((((q_base & M64) * n) & M64, ev, dp, ch, (((d_base + d) & M64) * n) & M64, n)):
                v[a] = (v[a] + x) & M64
        v[0] = (v[0] + qsum[s]) & M64
        out.append([s64(x) for x in v])
    return out


def run_case(rows, ns, A1c, B1c, A2c, B2c, e_base, q_base, d_base):
    """rows: (slot, d code, t code, e code, q code, multiplicity, wave); the multiplicity stands for that many equal rows"""
    bins = [[0] * (ns * 256) for _ in range(4)]
    qsum = [0] * ns
    want = [[0] * 6 for _ in range(ns)]
    for slot, d, t, e, q, mult, wave in rows:
        idx = slot << 8 | t << 4 | d
        bins[wave][idx] = (bins[wave][idx] + mult * ((1 << CNT_SHIFT) | e)) & M64   # the same word as mult atomic adds
        qsum[slot] += mult * q
        ev, f1, f2 = e_base + e, A1c + B1c * d, A2c + B2c * t
        for a, x in enumerate((q_base + q, ev, ev * f1, ev * f1 * f2, d_base + d, 1)):
            want[slot][a] += x * mult
    assert all(-(1 << 63) <= x < (1 << 63) for w in want for x in w), "the case must fit the partials"
    assert fold(bins, qsum, ns, A1c, B1c, A2c, B2c, e_base, q_base, d_base) == want
    return want


def test_field_widths_hold_the_bound():
    rows_per_table = MAX_TILES * ROWS_PER_WAVE_TILE
    assert rows_per_table < 1 << (64 - CNT_SHIFT)
    assert rows_per_table * ((1 << 24) - 1) < 1 << CNT_SHIFT
    assert MAX_TILES * 16 * 63 < 1 << 32
    assert (MAX_TILES + 1) * ROWS_PER_WAVE_TILE >= 1 << (64 - CNT_SHIFT)   # one tile more could carry out of the count


def test_random_bins_factors_of_both_signs():
    rng = random.Random(7)
    for case in range(40):
        ns = rng.randint(1, 6)
        A1c, B1c = rng.randint(-200, 200), rng.choice([-1, 1]) * rng.randint(1, 40)
        A2c, B2c = rng.randint(-200, 200), rng.choice([-1, 1]) * rng.randint(1, 40)
        e_base, q_base, d_base = rng.randint(-(1 << 23), 1 << 23), rng.randint(-50, 50), rng.randint(-8, 100)
        rows = [(rng.randrange(ns), rng.randrange(16), rng.randrange(16), rng.randrange(1 << 24), rng.randrange(64), rng.randint(1, 3), rng.randrange(4))
                for _ in range(rng.randint(0, 600))]
        rows += [(ns - 1, 15, 15, (1 << 24) - 1, 63, 1, 3), (0, 0, 0, 0, 0, 1, 0)]   # the last and the first bin, the largest and the smallest codes
        run_case(rows, ns, A1c, B1c, A2c, B2c, e_base, q_base, d_base)


def test_full_bins_near_the_partials_bound():
    """every wave's table at its row bound, all in one bin or spread over a slot, with the largest codes and factors whose products take a
    workgroup's Σ e·f1·f2 to about ±4e18 (the plan's overflow proof admits nothing larger) and Σ e·f1 of the other sign"""
    full = MAX_TILES * ROWS_PER_WAVE_TILE
    emax = (1 << 24) - 1
    for sign1, sign2 in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
        # |f1 f2| e n = 4e18 with n = 4 full tables of e = emax: f1 f2 of about 56900
        A1c, B1c, A2c, B2c = sign1 * 100, sign1 * 9, sign2 * 100, sign2 * 9     # f1(15) = ±235, f2(15) = ±235: 55 225
        one_bin = [(5, 15, 15, emax, 63, full, w) for w in range(4)]
        want = run_case(one_bin, 6, A1c, B1c, A2c, B2c, 0, 1, 0)
        assert abs(want[5][3]) > 3.8e18 and want[5][5] == 4 * full
        spread = [(2, d, t, emax - d - t, 63, full // 256, w) for w in range(4) for d in range(16) for t in range(16)]
        run_case(spread, 6, A1c, -B1c, A2c, -B2c, -5, -3, 90)   # f1, f2 shrink towards d, t = 15 and cross zero for neither
        crossing = [(1, d, t, emax, 0, full // 256, w) for w in range(4) for d in range(16) for t in range(16)]
        run_case(crossing, 6, sign1 * 8, -sign1, sign2 * 7, -sign2, -(1 << 23), 0, 93)   # f1 = ±(8 - d), f2 = ±(7 - t): both cross zero
