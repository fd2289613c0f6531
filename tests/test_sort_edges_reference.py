"""The inputs, the reference and the structural model of the ORDER BY edge tests (sort_edges.py), checked without a device: the two
statements of `order` against each other and against a table written out by hand, `order` against the oracle's ORDER BY on every numeric
corpus and selection, and every corpus against the edge of ops_sort.hip it is named for (tile / wave / chunk seams, the passes that run,
candidates and segments per refinement round, the load path of a word). A GPU test over a corpus that lost its edge would still pass; this
file is what fails."""
import numpy as np
import pytest

import oracle_lib as O
import sort_edges as S

OT = {"I32": O.OT_INT32, "DATE": O.OT_DATE, "CODE8": O.OT_CODE8, "DEC64": O.OT_DECIMAL}


def oracle_order(cols, desc, sel, n):
    """oracle_sort_rows over NumCols, or None where the oracle reports an error (dec.Int64's `ok`: a DECIMAL whose cents leave int64)"""
    ocols = [O.col(OT[c.type], c.values, c.scale, validity=None if c.valid is None else np.packbits(c.valid, bitorder="little")) for c in cols]
    arr = (O.OCol * len(ocols))(*ocols)
    d = (O.i32 * len(ocols))(*[1 if x else 0 for x in desc])
    s = None if sel is None else np.ascontiguousarray(sel, dtype=np.int64)
    m = n if sel is None else len(sel)
    rows = np.empty(max(m, 1), np.int64)
    rc = O.lib().oracle_sort_rows(arr, d, O.i32(len(ocols)), O.ptr(s), O.i64(m), O.ptr(rows), None, None)
    return rows[:m].tolist() if rc == 0 else None


def check_against_oracle(name, cols, desc):
    """`order` = the oracle for every selection kind, over the numeric keys (the oracle has no VARCHAR case); the number of comparisons made"""
    keep = [i for i, c in enumerate(cols) if isinstance(c, S.NumCol)]
    cols, desc = [cols[i] for i in keep], [desc[i] for i in keep]
    n = len(cols[0].values)
    keys = [S.pykeys(c) for c in cols]
    made = 0
    for kind, sel in S.selections(n).items():
        want = oracle_order(cols, desc, sel, n)
        if want is None:
            continue
        made += 1
        got = S.order(range(n) if sel is None else sel, keys, desc)
        assert got == want, (name, kind)
    return made


# ------------------------------------------------------------------ the reference

A, B = b"a", b"b"
HAND = [
    # (rows, keys, desc, expected)
    ([0, 1, 2], [[3, 1, 2]], [False], [1, 2, 0]),
    ([0, 1, 2], [[3, 1, 2]], [True], [0, 2, 1]),
    ([0, 1, 2], [[3, None, 2]], [False], [1, 2, 0]),                                     # NULL first ascending
    ([0, 1, 2], [[3, None, 2]], [True], [1, 0, 2]),                                      # and descending
    ([0, 1, 2, 3], [[None, 5, None, 5]], [True], [0, 2, 1, 3]),                          # NULLs and ties keep their positions
    ([0, 1, 2], [[b"ab", b"a", b"abc"]], [False], [1, 0, 2]),                            # a prefix before its extension
    ([0, 1, 2], [[b"ab", b"a", b"abc"]], [True], [2, 0, 1]),                             # the reverse descending
    ([0, 1, 2], [[b"a\x00\x00", b"a", b"a\x00"]], [False], [1, 2, 0]),                   # a < a\0 < a\0\0
    ([0, 1, 2], [[b"a\x00\x00", b"a", b"a\x00"]], [True], [0, 2, 1]),
    ([0, 1, 2, 3], [[b"", None, b"\x00", b""]], [False], [1, 0, 3, 2]),                  # NULL, then the empty strings, then NUL
    ([0, 1, 2, 3], [[b"", None, b"\x00", b""]], [True], [1, 2, 0, 3]),
    ([0, 1, 2], [[b"\x7f", b"\x80", b"\xff"]], [True], [2, 1, 0]),                       # bytes are unsigned
    ([0, 1, 2], [[b"\x80", b"\x7f\xff", b"\x7f"]], [False], [2, 1, 0]),
    ([0, 1, 2, 3], [[None, b"\xff" * 8, None, b"\xff" * 9]], [True], [0, 2, 3, 1]),      # 0xFF strings next to NULLs, descending
    ([2, 0, 2, 1, 0], [[7, 7, 1]], [False], [2, 2, 0, 1, 0]),                            # a repeated selection: ties by position, not row id
    ([2, 0, 2, 1, 0], [[7, 7, 1]], [True], [0, 1, 0, 2, 2]),
    ([3, 2, 1, 0], [[5, 5, 5, 5]], [False], [3, 2, 1, 0]),                               # a descending selection, all tied
    ([3, 2, 1, 0], [[1, 2, 1, 2]], [False], [2, 0, 3, 1]),                               # a descending selection with ties
    ([3, 2, 1, 0], [[1, 2, 1, 2]], [True], [3, 1, 2, 0]),
    ([0, 1, 2, 3], [[1, 1, 0, 0], [A, B, B, A]], [False, True], [2, 3, 1, 0]),           # two keys, the second descending
    ([0, 1, 2, 3], [[1, 1, 0, 0], [A, None, B, None]], [True, False], [1, 0, 3, 2]),     # NULL first inside a descending outer key
    ([1, 3, 5], [[9, 2, 9, 1, 9, 3]], [False], [3, 1, 5]),                               # only selected rows are read
    ([0, 1, 2, 3, 4, 5], [[b"abcdefgh", b"abcdefgh\x00", b"abcdefg", b"abcdefgh", b"abcdefghi", b"abcdefg\xff"]], [False],
     [2, 0, 3, 1, 4, 5]),                                                                # equal first words decided past them; 0xFF above 'h'
    ([0, 1, 2, 3, 4, 5], [[b"abcdefgh", b"abcdefgh\x00", b"abcdefg", b"abcdefgh", b"abcdefghi", b"abcdefg\xff"]], [True],
     [5, 4, 1, 0, 3, 2]),
    ([], [[1, 2]], [False], []),
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_order_on_the_hand_written_table(case):
    rows, keys, desc, expected = HAND[case]
    assert len(rows) <= 6
    assert S.order(rows, keys, desc) == expected
    assert S.order_by_comparator(rows, keys, desc) == expected


def test_the_table_is_large_enough():
    assert len(HAND) >= 20


@pytest.mark.parametrize("name", S.VARCHAR_NAMES)
def test_both_statements_of_order_agree_on_the_varchar_corpora(name):
    col = S.varchar_corpus(name)
    n = len(col.strings)
    for label, cols, desc, sel in S.varchar_runs(col):
        keys = [S.pykeys(c) for c in cols]
        rows = list(range(n)) if sel is None else sel
        if n <= 20_000:
            assert S.order(rows, keys, desc) == S.order_by_comparator(rows, keys, desc), (name, label)
        else:
            # the same statement in n comparisons instead of n log n: a permutation of the positions in which the comparator (a total order,
            # the position last) puts every entry strictly before the next is the sorted one
            pos, cmp = S.order_positions(rows, keys, desc), S.comparator(rows, keys, desc)
            assert sorted(pos) == list(range(len(rows))), (name, label)
            assert all(cmp(p, q) < 0 for p, q in zip(pos, pos[1:])), (name, label)
            # and the two statements sorted independently over 10 000 of the entries, kept in their input order
            some = [rows[p] for p in sorted(np.random.default_rng(len(rows)).choice(len(rows), 10_000, replace=False).tolist())]
            assert S.order(some, keys, desc) == S.order_by_comparator(some, keys, desc), (name, label)


def test_packed_columns_hold_their_strings():
    """offsets and bytes of every VARCHAR corpus give back the strings `order` sees; every offset lies inside the buffer"""
    assert len(S.VARCHAR_NAMES) == 24
    for name in S.VARCHAR_NAMES:
        col = S.varchar_corpus(name)
        b, off = col.data.tobytes(), col.off.tolist()
        assert 0 <= off[0] and off[-1] <= len(b) and all(x <= y for x, y in zip(off, off[1:])), name
        assert len(off) == len(col.strings) + 1
        for r, s in enumerate(col.strings):
            assert (col.valid is None or col.valid[r]) == (s is not None), (name, r)
            if s is not None:
                assert b[off[r]:off[r + 1]] == s, (name, r)


# ------------------------------------------------------------------ numeric corpora

def test_seam_sizes_sit_on_the_seams():
    assert S.SEAM_SIZES == (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 12289)
    for seam in (64, S.SORT_TILE, S.SORT_CHUNK, 2 * S.SORT_CHUNK):
        assert {seam - 1, seam, seam + 1} <= set(S.SEAM_SIZES)
    assert 3 * S.SORT_CHUNK + 1 in S.SEAM_SIZES     # four workgroups, the last with one row


@pytest.mark.parametrize("kind", S.LAYOUTS)
def test_digit_layouts_have_their_shape(kind):
    """lane by lane: what each layout promises, at every seam size that can hold it; one pass (byte 0) runs, none for (f)"""
    sizes = [n for n in S.SEAM_SIZES if n >= S.layout_min_rows(kind)]
    assert sizes and sizes[-1] == S.SEAM_SIZES[-1]
    names = [c[0] for c in S.digit_cases(kind)]
    for n in sizes:
        d = S.digit_layout(kind, n)
        assert len(d) == n and d.dtype == np.int32 and d.min() >= 0 and d.max() <= 255
        assert f"layout {kind} n={n}" in names and (kind == "f" or f"layout {kind} n={n} + tie key" in names)
        tiles = [d[t:t + 256] for t in range(0, n, 256)]
        waves = [d[w:w + 64] for w in range(0, n, 64)]
        for desc in (False, True):
            assert S.radix_plan(S.num("I32", d), desc) == (set() if kind == "f" else {0}, False)
        if kind == "a":
            assert all(sorted(t.tolist()) == list(range(256)) for t in tiles if len(t) == 256)
            assert all(len(set(t.tolist())) == len(t) for t in tiles)
            assert any(t.tolist() != sorted(t.tolist()) for t in tiles)
        elif kind == "b":
            assert all(len(set(w.tolist())) == 1 for w in waves)
            for t in tiles:
                heads = t[::64].tolist()
                assert len(set(heads)) == len(heads)
            heads = d[::64].tolist()
            assert n < 255 or any(x > y for x, y in zip(heads, heads[1:]))                                      # a later wave sorts before an earlier one
            assert n < 8 * 64 or any(heads[w] == heads[w + 7] and w // 4 != (w + 7) // 4 for w in range(len(heads) - 7))   # a digit returns in another tile
        elif kind == "c":
            assert set(d[0::2].tolist()) == {200} and set(d[1::2].tolist()) == {3}
        elif kind == "d":
            assert set(d.tolist()) == {0x00, 0xFF}
        elif kind == "e":
            assert set(d[:n - 3].tolist()) == {S.E_BASE} and tuple(d[n - 3:].tolist()) == S.E_ODD
            last_tile = (n - 1) // 256 * 256
            assert n - 1 >= last_tile
            assert (n - 3 >= last_tile) == (n - last_tile >= 3)      # all three in the last tile where it has three rows, across its seam otherwise
        else:
            assert len(set(d.tolist())) == 1
    if kind == "e":   # both placements occur
        assert any(n - (n - 1) // 256 * 256 >= 3 and n % 256 for n in sizes) and any(n - (n - 1) // 256 * 256 < 3 for n in sizes)


@pytest.mark.parametrize("kind", S.LAYOUTS)
def test_order_matches_the_oracle_on_the_digit_layouts(kind):
    made = 0
    for name, cols, desc in S.digit_cases(kind):
        n = len(cols[0].values)
        got = check_against_oracle(name, cols, desc)
        assert got == len(S.selections(n)), name          # small I32 keys: the oracle never reports an error
        made += got
        if len(cols) == 2:                                 # the tie key has its three values and leaves ties
            assert n < 63 or len(set(cols[1].values.tolist())) == 3
    assert made > 0


def test_tie_keys_decide_something():
    """with the tie key behind a layout the order differs from the order without it: stability across the seams decides the result"""
    for kind in "abcde":
        for name, cols, desc in S.digit_cases(kind):
            n = len(cols[0].values)
            digits = cols[0].values.tolist()
            assert n < 63 or len(set(digits)) < n or (kind == "a" and n <= 256)   # the first key leaves ties, but for one tile of 256 digits
            if len(cols) == 2 and n >= 63 and len(set(digits)) < n:
                rows = range(n)
                assert S.order(rows, [S.pykeys(c) for c in cols], desc) != S.order(rows, [S.pykeys(cols[0])], desc[:1]), name


def test_selection_kinds():
    for n in S.SEAM_SIZES + (S.N_BYTES,):
        sels = S.selections(n)
        assert set(sels) == set(S.SEL_KINDS) - (set() if n // 3 >= 2 else {"repeated"})
        assert sels["none"] is None
        asc = sels["ascending"]
        assert asc == sorted(set(asc)) and len(asc) == max(1, n // 2) and sels["descending"] == asc[::-1]
        assert sorted(sels["shuffled"]) == list(range(n)) and (n < 63 or sels["shuffled"] != list(range(n)))
        if "repeated" in sels:
            rep = sels["repeated"]
            assert len(rep) == 2 * (n // 3)
            assert np.bincount(rep).max() == 2 and set(np.bincount(rep).tolist()) <= {0, 2}
            assert all(x != y for x, y in zip(rep, rep[1:]))
        for sel in sels.values():
            assert sel is None or all(0 <= r < n for r in sel)


def test_varying_byte_columns_run_the_passes_they_name():
    cases = S.byte_cases()
    names = [c[0] for c in cases]
    for b in range(8):
        assert f"byte {b} only" in names
    for want in ("bytes 0 and 5", "mixed sign", "only row 0 differs", "row 0 NULL, constant otherwise"):
        assert want in names
    for kind in ("constant", "constant with NULLs", "NULL flag only", "NULL flag only desc"):
        for where in ("first", "middle", "last"):
            assert f"{kind} as {where} key" in names
    for name, cols, desc, exp in cases:
        assert all(len(c.values) == S.N_BYTES == 4097 for c in cols), name
        if exp is not None:
            at, byts, null_varies = exp
            assert S.radix_plan(cols[at], desc[at]) == (byts, null_varies), name
    by_name = {c[0]: c for c in cases}
    c = by_name["constant with NULLs as first key"][1][0]
    assert 0.05 < 1 - c.valid.mean() < 0.15 and S.radix_plan(c)[1]           # 10 % NULLs
    c = by_name["NULL flag only as first key"][1][0]
    assert 0.05 < 1 - c.valid.mean() < 0.15 and c.valid[0]
    c = by_name["only row 0 differs"][1][0]
    assert len(set(c.values[1:].tolist())) == 1 and c.values[0] != c.values[1]
    c = by_name["row 0 NULL, constant otherwise"][1][0]
    assert not c.valid[0] and c.valid[1:].all() and len(set(c.values.tolist())) == 1
    # with row 0 first in the selection keys[0] is 0; a selection that starts elsewhere sees only the bytes that differ from 0 as well
    assert S.radix_plan(c, False, [5, 0, 7]) == ({0, 2, 7}, True)


def test_order_matches_the_oracle_on_the_varying_byte_columns():
    """every case under every selection kind, but the three whose DECIMAL key is INT64_MIN: its cents leave int64 and the oracle reports
    dec.Int64's error for them, whatever the selection. No other case may go uncompared."""
    uncompared = set()
    for name, cols, desc, _ in S.byte_cases():
        made = check_against_oracle(name, cols, desc)
        assert made in (0, len(S.selections(S.N_BYTES))), name
        if made == 0:
            uncompared.add(name)
    assert uncompared == {f"NULL flag only as {where} key" for where in ("first", "middle", "last")}


def test_eight_keys_each_break_a_tie():
    cols, desc = S.eight_keys()
    assert len(cols) == len(desc) == 8 and 0 < sum(desc) < 8
    kinds = [(c.type, c.scale) if isinstance(c, S.NumCol) else ("STR", 0) for c in cols]
    assert {("I32", 0), ("DATE", 0), ("CODE8", 0), ("DEC64", 0), ("DEC64", 4), ("STR", 0)} <= set(kinds)
    keys = [S.pykeys(c) for c in cols]
    n = S.N_BYTES
    assert all(len(k) == n for k in keys)
    groups = 1
    for c in range(8):
        assert 2 <= len(set(keys[c])) <= 4
        now = len({tuple(k[r] for k in keys[:c + 1]) for r in range(n)})
        assert now > groups, c          # key c separates rows that keys 0..c-1 left tied
        groups = now
    assert groups < n                    # and ties remain for the position to decide
    assert check_against_oracle("eight keys", cols, desc) == len(S.selections(n))


# ------------------------------------------------------------------ VARCHAR corpora

def plans(col):
    return {d: S.refine_plan(col.strings, d) for d in (False, True)}


@pytest.mark.parametrize("nseg, seg_bytes", [(300, {0, 1}), (1000, {0, 1}), (70_000, {0, 1, 2})])
def test_many_segments_reach_the_upper_segment_id_bytes(nseg, seg_bytes):
    col = S.many_segments(nseg)
    assert len(col.strings) == 2 * nseg and len({s[:8] for s in col.strings}) == nseg
    assert all(9 <= len(s) <= 16 for s in col.strings)
    for d, plan in plans(col).items():
        r = plan[0]
        assert len(plan) == 1 and r["m"] == 2 * nseg and r["segments"] == nseg and not r["skipped"]
        assert r["seg_bytes"] == seg_bytes                           # the bytes of the segment id that vary: byte b is the pass at shift 72 + 8 b
        assert r["word_bytes"] == set(range(8)) and r["e_varies"]
    words = [S.word_of(s, 0) for s in col.strings]
    assert words != sorted(words)


@pytest.mark.parametrize("base_len", [21, 5])
def test_trailing_nul_is_ordered_by_length_alone(base_len):
    col = S.trailing_nul(base_len)
    assert len(col.strings) == 82 and sorted(len(s) - base_len for s in col.strings) == sorted(list(range(41)) * 2)
    assert all(s[:base_len] == col.strings[0][:base_len] and 0 not in s[:base_len] and set(s[base_len:]) <= {0} for s in col.strings)
    for d, plan in plans(col).items():
        assert all(r["word_bytes"] == set() and r["segments"] == 1 for r in plan)
        if base_len == 21:
            assert len(plan) >= 6 and plan[0]["skipped"] and plan[0]["m"] == 82
            assert all(r["e_varies"] and not r["skipped"] for r in plan[1:])
        else:
            assert len({S.word_of(s, 0) for s in col.strings}) == 1          # the family ties inside the first word
            assert len(plan) >= 4 and all(r["e_varies"] and not r["skipped"] for r in plan)


def test_deep_prefix_skips_thirty_rounds():
    col = S.deep_prefix()
    assert len(col.strings) == 600 and len({s[:256] for s in col.strings}) == 1
    tails = [len(s) - 256 for s in col.strings]
    assert min(tails) == 0 and max(tails) == 19 and tails.count(0) >= 2
    for d, plan in plans(col).items():
        assert len(plan) >= 32
        assert all(r["skipped"] and r["m"] == 600 for r in plan[:30])                    # rounds 1..30
        r31, r32 = plan[30], plan[31]
        assert r31["m"] == 600 and r31["word_bytes"] == set() and r31["e_varies"] and not r31["skipped"]
        assert r32["m"] == 600 - tails.count(0) and r32["word_bytes"] == set(range(8)) and not r32["skipped"]


def test_deep_prefix_two_groups_meet_in_one_round():
    col, equal_rows = S.deep_prefix_two_groups()
    assert len(col.strings) == 600 and len(equal_rows) == 300 and len({col.strings[r] for r in equal_rows}) == 1
    assert len({s[:8] for s in col.strings}) == 1 and len({s[:16] for s in col.strings}) == 2
    others = [s for r, s in enumerate(col.strings) if r not in set(equal_rows)]
    assert len({s[:64] for s in others}) == 1 and len({s[64:72] for s in others}) > 100
    for d, plan in plans(col).items():
        assert all(r["m"] == 600 for r in plan[:8])
        for r in plan[1:7]:                                                              # rounds 2..7: each group equal in itself, the two apart
            assert r["segments"] == 2 and not r["skipped"] and len(set(zip(r["words"], r["e"]))) == 2
        r8 = plan[7]                                                                     # word 8 = bytes 64..71
        assert r8["segments"] == 2 and not r8["skipped"] and r8["word_bytes"]
        eq = {(w, e) for r, w, e in zip(r8["rows"], r8["words"], r8["e"]) if r in set(equal_rows)}
        var = {(w, e) for r, w, e in zip(r8["rows"], r8["words"], r8["e"]) if r not in set(equal_rows)}
        assert len(eq) == 1 and len(var) > 100
        assert plan[8]["m"] >= 300 and len(plan) == 12                                   # the equal group goes on to its end


@pytest.mark.parametrize("m", S.ROUND_M)
def test_round_sizes_plant_m_candidates(m):
    assert S.ROUND_M == (2, 255, 256, 257, 4096, 4097)
    col = S.round_sizes(m)
    assert len(col.strings) == 6000 + m
    assert len({s[:8] for s in col.strings}) == 6001
    for d, plan in plans(col).items():
        assert [r["m"] for r in plan] == [m, m]
        assert plan[0]["skipped"] and plan[0]["segments"] == 1
        assert not plan[1]["skipped"] and plan[1]["word_bytes"] and not plan[1]["e_varies"] and plan[1]["segments"] == 1
        assert len(set(plan[1]["words"])) == m
        assert plan[1]["rows"] == sorted(plan[1]["rows"]) and plan[1]["rows"][-1] - plan[1]["rows"][0] > m   # spread over the larger n


def test_lone_survivor_drops_single_rows():
    col = S.lone_survivor()
    lens = [len(s) for s in col.strings]
    for k in (0, 1, 8, 16, 17, 24):
        assert max(col.strings.count(s) for s in set(col.strings) if len(s) == k) == 5
    assert {7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 40} <= set(lens)
    for d, plan in plans(col).items():
        assert len(plan) == 4
        assert sum(r["lone"] for r in plan) >= 4 and plan[0]["lone"] and plan[1]["lone"] and plan[2]["lone"]
        assert all(not r["skipped"] for r in plan)


def test_null_neighbours():
    col = S.null_neighbours()
    kinds = [None, b"", b"\x00", b"\x00" * 8, b"\xff" * 8, b"\xff" * 9, b"\xff" * 16]
    assert len(col.strings) == 140 and all(col.strings.count(k) == 20 for k in kinds)
    zero_asc = {r for r, (k, f) in enumerate(S.key_words(col, False)) if k == 0}
    zero_desc = {r for r, (k, f) in enumerate(S.key_words(col, True)) if k == 0}
    assert {col.strings[r] for r in zero_asc} == {None, b"", b"\x00", b"\x00" * 8}       # key word 0 like a NULL's
    assert {col.strings[r] for r in zero_desc} == {None, b"\xff" * 8, b"\xff" * 9, b"\xff" * 16}
    assert S.radix_plan(col, False)[1] and S.radix_plan(col, True)[1]
    first = col.strings[S.order(range(140), [col.strings], [False])[19]], col.strings[S.order(range(140), [col.strings], [True])[19]]
    assert first == (None, None)


def test_alignment_sweep_takes_every_shift_and_rest():
    seen = set()
    for part, (lo, hi) in enumerate(S.SWEEP_PARTS):
        col, pairs = S.alignment_sweep(part)
        nbytes, off = len(col.data), col.off
        assert {(a, L) for a, L, _, _ in pairs} == {(a, L) for a in range(8) for L in range(lo, hi + 1)}
        firsts = [s[0] for r, s in enumerate(col.strings) if r % 2 == 0]                 # the fillers
        assert len(set(firsts)) == len(firsts) == len(pairs) * 2 and max(firsts) < 0xA0
        for a, L, x, y in pairs:
            sx, sy = col.strings[x], col.strings[y]
            assert off[x] % 8 == a and off[y] % 8 == a and len(sx) == len(sy) == L
            assert sx[:-1] == sy[:-1] and (L == 0 or (sx[-1] != sy[-1] and sx[0] >= 0xA0))
            assert L == 0 or col.data[off[x] + L] != 0                                   # a non-zero byte behind the string
            for r in (x, y):
                for j in range(3):
                    path, sh, rest = S.word_path(off, nbytes, 0, r, j)
                    if path == "aligned":
                        seen.add((sh, min(rest, 17)))
        # the final pair
        a, L, x, y = pairs[-1]
        if part == 0:
            assert (a, L) == (3, 4) and off[x] >= nbytes - 16 and off[y + 1] == nbytes
            assert S.word_path(off, nbytes, 0, x, 0)[0] == S.word_path(off, nbytes, 0, y, 0)[0] == "bytes"
        else:
            assert off[y + 1] == nbytes and S.word_path(off, nbytes, 0, y, (L - 1) // 8) == ("bytes", 56, 1)   # the deciding byte is the buffer's last
        # behind a misaligned base every load is a byte load
        assert {S.word_path(off, nbytes, k, r, 0)[0] for k in (1, 3, 7) for r in range(len(col.strings)) if col.strings[r]} == {"bytes"}
    assert seen == {(8 * a, rest) for a in range(8) for rest in range(1, 18)}


@pytest.mark.parametrize("total", S.TINY_BYTES)
def test_tiny_buffers(total):
    assert S.TINY_BYTES == (1, 7, 8, 15, 16, 17)
    col = S.tiny_buffer(total)
    assert len(col.data) == total
    paths = {S.word_path(col.off, total, 0, r, j)[0] for r in range(len(col.strings)) for j in range(2)} - {None}
    assert paths == ({"bytes"} if total < 16 else {"aligned", "bytes"})


def test_null_with_bytes_hides_order_changing_bytes():
    col = S.null_with_bytes()
    off, b = col.off.tolist(), col.data.tobytes()
    assert off[0] == 5 and b[:5] == b"\xff" * 5 and off[-1] == len(b)
    hidden = {b[off[r]:off[r + 1]] for r, s in enumerate(col.strings) if s is None}
    assert all(hidden) and any(set(h) == {0xFF} for h in hidden) and any(set(h) == {0x00} for h in hidden)
    # read as values the NULL rows' bytes would move them: the order over the raw ranges differs from the order with NULLs
    raw = [b[off[r]:off[r + 1]] for r in range(len(col.strings))]
    for d in (False, True):
        assert S.order(range(len(raw)), [raw], [d]) != S.order(range(len(raw)), [col.strings], [d])
    assert sum(s is None for s in col.strings) == 80
