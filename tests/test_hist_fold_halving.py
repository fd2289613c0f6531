"""The exchange schedule of the bins body's fold (lch_halve and lch_fold in scan_kernels.hip, DESIGN.md §4.1 "The halving fold and the residency probe"),
restated in Python over the 64 lanes of a wave: 36 sum words and 6 minima per lane, wrapping 64-bit adds. No GPU: this pins which lane
ends with which word, that the lane's (base, end) bookkeeping says so, and how many exchanges a lane makes;
tests/test_gpu_hist_fold.py pins the kernel."""
import random

M64 = (1 << 64) - 1
LANES = 64
NACC, SLOTS = 6, 6                       # LC_NACC, LC_BINS_MAX_SLOTS
WORDS = SLOTS * NACC                     # LCH_FOLD_WORDS
SUM_STEPS = [(36, 1), (18, 2), (9, 4), (5, 8), (3, 16), (2, 32)]      # lch_halve<N, O, FoldSum>, in the kernel's order
MIN_STEPS = [(6, 1), (3, 2), (2, 4), (1, 8), (1, 16), (1, 32)]        # lch_halve<N, O, FoldMin>
U32_MAX = 0xFFFFFFFF


def halve(v, base, end, n, o, op, ident):
    """one lch_halve<n, o> of every lane: v[lane] is the lane's array, base / end its bookkeeping. Returns the exchanges a lane made."""
    h = (n + 1) // 2
    new = []
    for lane in range(LANES):
        up = bool(lane & o)
        mine, partner = v[lane], v[lane ^ o]
        row = []
        for i in range(h):
            lo, hi = mine[i], (mine[i + h] if i + h < n else ident)
            plo, phi = partner[i], (partner[i + h] if i + h < n else ident)
            keep = hi if up else lo
            received = phi if up else plo        # the partner sends what it does not keep: its upper half to an upper lane
            row.append(op(keep, received))
        new.append(row)
        if up:
            base[lane] += h
        else:
            end[lane] = min(end[lane], base[lane] + h)
    for lane in range(LANES):
        v[lane] = new[lane]
    return h


def fold(words, steps, op, ident):
    """the whole schedule: ({word index: (lane, value)}, exchanges per lane)"""
    n0 = steps[0][0]
    v = [list(w) for w in words]
    base, end = [0] * LANES, [n0] * LANES
    exchanges = sum(halve(v, base, end, n, o, op, ident) for n, o in steps)
    out = {}
    for lane in range(LANES):
        if base[lane] < end[lane]:               # the kernel's condition for the store
            assert base[lane] not in out, "two lanes answer for one word"
            out[base[lane]] = (lane, v[lane][0])
    return out, exchanges


def add64(a, b):
    return (a + b) & M64


def test_sum_words_land_once_each_in_38_exchanges():
    rng = random.Random(3)
    words = [[rng.getrandbits(64) for _ in range(WORDS)] for _ in range(LANES)]
    out, exchanges = fold(words, SUM_STEPS, add64, 0)
    assert exchanges == 18 + 9 + 5 + 3 + 2 + 1 == 38
    assert sorted(out) == list(range(WORDS))
    for k, (lane, total) in out.items():
        assert total == sum(w[k] for w in words) & M64, k
    assert len({lane for lane, _ in out.values()}) == WORDS      # one word a lane


def test_minima_land_once_each_in_9_exchanges():
    rng = random.Random(4)
    rows = [[rng.getrandbits(32) for _ in range(SLOTS)] for _ in range(LANES)]
    for s in range(SLOTS):
        rows[rng.randrange(LANES)][s] = s        # a known minimum somewhere
    rows[63][5], rows[0][0] = 0, U32_MAX         # the last lane holds a minimum, the first an identity
    out, exchanges = fold(rows, MIN_STEPS, min, U32_MAX)
    assert exchanges == 3 + 2 + 1 + 1 + 1 + 1 == 9
    assert sorted(out) == list(range(SLOTS))
    for s, (lane, m) in out.items():
        assert m == min(r[s] for r in rows), s


def test_the_lane_of_a_word_is_the_bits_of_its_path():
    """where the kernel stores from: word k's lane has bit O set exactly at the steps where k lay in the upper half, and the red word it
    adds to is [k // 6][k % 6] of its wave"""
    words = [[(lane << 8) | k for k in range(WORDS)] for lane in range(LANES)]
    out, _ = fold(words, SUM_STEPS, add64, 0)
    for k in range(WORDS):
        lane, lo, n = 0, 0, None
        for n, o in SUM_STEPS:
            h = (n + 1) // 2
            if k - lo >= h:
                lane |= o
                lo += h
        assert out[k][0] == lane, k
        assert out[k][1] == sum((l << 8) | k for l in range(LANES))
    # slots 0..2 end in even lanes, slots 3..5 in odd ones: the first exchange pairs slot s with slot s + 3
    assert all((out[k][0] & 1) == (k >= WORDS // 2) for k in range(WORDS))


def test_fewer_slots_fold_identities():
    """ns < 6: the words of the absent slots are zeros and their minima the identity; the kernel stores only words of slots below ns"""
    rng = random.Random(5)
    for ns in range(1, SLOTS):
        words = [[rng.getrandbits(64) if k // NACC < ns else 0 for k in range(WORDS)] for _ in range(LANES)]
        out, _ = fold(words, SUM_STEPS, add64, 0)
        for k, (lane, total) in out.items():
            assert total == (sum(w[k] for w in words) & M64 if k // NACC < ns else 0)
        mins = [[rng.getrandbits(32) if s < ns else U32_MAX for s in range(SLOTS)] for _ in range(LANES)]
        mout, _ = fold(mins, MIN_STEPS, min, U32_MAX)
        for s, (lane, m) in mout.items():
            assert m == (min(r[s] for r in mins) if s < ns else U32_MAX)
