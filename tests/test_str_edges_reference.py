"""The references and corpora of the VARCHAR edge tests, checked without a device: the byte-wise LIKE agrees with the find-based check, with
the oracle and with a truth table written by hand; every placement corpus really holds every placement class where its arithmetic says
(asserted, not measured: no case is skipped); the wrap corpus really wraps the table's end; the Python substring agrees with the oracle and
with the library's own host-compiled range over every int64 argument of the tests."""
import numpy as np
import pytest

import oracle_lib as O
import str_edges as S
from plan_amd import hip

PLACEMENT_LITS = [(a, None) for a in S.LITERALS] + S.PAIRS


def all_corpora():
    out = [S.random_corpus(), S.stage_boundary_corpus()[0]] + S.degenerate_corpora()
    out += [S.like_placement_corpus(a, b, off0) for a, b in (PLACEMENT_LITS[1], PLACEMENT_LITS[4], PLACEMENT_LITS[12]) for off0 in (0, 37)]
    return out


CORPORA = all_corpora()


def oracle_column(c):
    data = c.data if len(c.data) else np.zeros(1, np.uint8)
    return O.col(O.OT_VARCHAR, c.off, validity=c.packed_validity(), dictionary=data)


def test_like_truth_table():
    table = [(b"", b"", True), (b"", b"a", False), (b"%", b"", True), (b"%%", b"", True), (b"%%%", b"\x00", True), (b"_", b"", False),
             (b"_", b"\xff", True), (b"_", b"ab", False), (b"%_", b"", False), (b"%_", b"\x00", True), (b"_%", b"p", True), (b"_%", b"", False),
             (b"%_%", b"", False), (b"%_%", b"\x80", True), (b"p%", b"pink", True), (b"p%", b"ip", False), (b"%p", b"ip", True),
             (b"%p", b"pi", False), (b"p_%_k", b"pink", True), (b"p_%_k", b"pik", False), (b"p_%_k", b"pi_k", True), (b"p_%_k", b"pinkk", True),
             (b"%\\%", b"a\\b", True), (b"%\\%", b"ab", False), (b"%\\%", b"%", False), (b"\\%", b"\\anything", True), (b"\\_", b"\\x", True),
             (b"\\_", b"_", False), (b"%\xff%", b"p\xffk", True), (b"%\xff%", b"p\x7fk", False), (b"%\x80\xfe%", b"\x80\x80\xfe", True),
             (b"%in%k%", b"pink", True), (b"%in%n%", b"pink", False), (b"%nk%pi%", b"pink", False), (b"%p%p%", b"p", False),
             (b"%p%p%", b"pp", True), (b"%pi%in%", b"pin", False), (b"%pi%in%", b"piin", True), (b"pink", b"pink", True), (b"pink", b"pinkx", False),
             (b"%a%b", b"ab", True), (b"%a%b", b"abab", True), (b"%a%b", b"aba", False), (b"a%a", b"a", False), (b"a%a", b"aa", True)]
    for pat, s, want in table:
        assert S.like(pat, s) is want, (pat, s)


def test_like_equals_the_find_based_check_on_every_literal_pattern_and_corpus():
    seen = 0
    for c in CORPORA:
        for pat in S.LITERAL_PATTERNS + S.PAIR_PATTERNS + [b"%" + S.LITERALS[-1] + b"%"] + ([S.placement_pattern(c)] if c.plants else []):
            lits = S.literal_shape(pat)
            assert lits is not None, pat
            got = [S.like(pat, s) for s in c.strings]
            assert got == [S.like_literals(lits, s) for s in c.strings], (c.name, pat)
            seen += sum(got)
    assert seen > 1000
    assert S.literal_shape(b"%a_%") is None and S.literal_shape(b"%%") is None and S.literal_shape(b"%a%b%c%") is None and S.literal_shape(b"a%") is None
    assert S.literal_shape(b"%\\%") == (b"\\",) and S.literal_shape(b"%%%") is None


def test_like_equals_the_oracle_where_it_can_express_the_case():
    """the oracle takes the pattern as a C string (no NUL inside; the rows may hold any byte)"""
    pats = S.GENERIC_PATTERNS + S.LITERAL_PATTERNS + S.PAIR_PATTERNS + [b"%" + S.LITERALS[-1] + b"%"]
    assert all(0 not in p for p in pats)
    for c in CORPORA:
        oc = oracle_column(c)
        for sel in (None, S.third_rows(c.n)):
            for pat in pats + ([S.placement_pattern(c)] if c.plants else []):
                for op in (S.OP_LIKE, S.OP_NOTLIKE):
                    got = O.select(oc, op, O.const(O.OT_VARCHAR, s=pat), sel_in=sel, n=c.n)
                    assert np.array_equal(got, S.select_reference(op, pat, c.strings, c.valid, sel)), (c.name, pat, op, sel is not None)
            for k in S.equality_constants(c):
                for op in (S.OP_EQ, S.OP_NE):
                    got = O.select(oc, op, O.const(O.OT_VARCHAR, s=k), sel_in=sel, n=c.n)
                    assert np.array_equal(got, S.select_reference(op, k, c.strings, c.valid, sel)), (c.name, k, op)


@pytest.mark.parametrize("lits", PLACEMENT_LITS, ids=lambda x: "-".join(str(len(p)) for p in x if p))
@pytest.mark.parametrize("off0", S.PLACEMENT_OFF0)
def test_placement_corpus_holds_every_class_where_the_arithmetic_says(lits, off0):
    A, B = lits
    c = S.like_placement_corpus(A, B, off0)
    U, L = c.unit, len(c.unit)
    pat = S.placement_pattern(c)
    assert c.n == S.PLACEMENT_ROWS and int(c.off[0]) == off0 and len(pat) < S.PATTERN_ROOM
    assert np.array_equal(c.off, S.like_placement_corpus(A, B, off0).off)                    # deterministic
    for cls in S.PLACEMENT_CLASSES:
        assert c.plants[cls], cls
    assert bool(c.plants["lead"]) == (off0 % 16 != 0)
    if off0:                                                                                 # the bytes before off[0] hold U, or as much of it as fits
        lead = bytes(c.data[:off0])
        assert U in lead or lead.endswith(U[:min(L - 1, off0 % 16)]) or U[-off0:] == lead
    hit = [S.like(pat, s) for s in c.strings]
    assert hit == [S.like_literals(c.lits, s) for s in c.strings] and S.literal_shape(pat) == c.lits
    for cls, plants in c.plants.items():
        for p in plants:
            r = p["row"]
            assert (hit[r] and bool(c.valid[r])) is p["match"], (cls, p)           # match: LIKE selects the row (a NULL row: never)
            assert bytes(c.data[c.off[r]:c.off[r + 1]]) == c.strings[r]
    assert all(not c.valid[p["row"]] and U in c.strings[p["row"]] for p in c.plants["i"])
    assert {0, c.n - 1} & {p["row"] for p in c.plants["h"]} == ({0, c.n - 1} if off0 % 16 == 0 else {c.n - 1})
    assert any(not p["match"] for p in c.plants["c"]) and any(not p["match"] for p in c.plants["g"]) or off0 == 5
    if L > 1:
        assert sum(not p["match"] for p in c.plants["c"]) >= 7                               # adjacent, across an empty row, across a NULL row
        assert any(not c.valid[p["row"]] for p in c.plants["c"]) and any(c.strings[p["row"]] == b"" and c.valid[p["row"]] for p in c.plants["c"])
    # the placement arithmetic, recomputed from the offsets
    for cls in "def":
        for p in c.plants[cls]:
            x, r = p["pos"], p["row"]
            assert bytes(c.data[x:x + L]) == U and c.off[r] <= x and x + L <= c.off[r + 1], (cls, p)
    assert sorted(p["pos"] % 16 for p in c.plants["d"]) == [13, 14, 15]
    for p in c.plants["e"]:
        a0 = S.group_first_offset(c, p["row"])[0] & ~15
        lo, hi = (p["pos"] - a0) // S.STRIDE, (p["pos"] + L - a0) // S.STRIDE
        assert hi == lo + 1 and ((p["pos"] + L - a0) % S.STRIDE != 0 or L == 1), p           # U lies across the multiple (one byte: ends at it)
    assert {p["row"] // S.ROWS_PER_GROUP for p in c.plants["e"]} >= {0, 1}                   # in both full workgroups
    ends = set()
    for p in c.plants["f"]:
        s1 = S.group_first_offset(c, p["row"])[1]
        assert (s1 - S.TAIL <= p["pos"] and p["pos"] + L <= s1) if L <= S.TAIL else (s1 - S.TAIL < p["pos"] + L <= s1), p
        ends.add(s1)
    assert ends == {int(c.off[S.ROWS_PER_GROUP]), int(c.off[2 * S.ROWS_PER_GROUP]), int(c.off[c.n])}
    # the workgroup boundaries
    for first, mode in zip((S.ROWS_PER_GROUP, 2 * S.ROWS_PER_GROUP), S.BOUNDARY_MODES[off0]):
        before, after = c.strings[first - 1], c.strings[first]
        if mode == "split" and L > 1:
            assert before + after[:L - len(before)] == U and not hit[first - 1] and not hit[first]
        elif mode == "whole":
            assert before.endswith(U) and after.startswith(U) and hit[first - 1] and hit[first]
        elif mode == "behind":
            assert before.endswith(U) and not hit[first] and c.off[first] % 16 == 15
    if B is not None:
        assert sum(not p["match"] for p in c.plants["j"]) == 3 + (A[-1] == B[0]) and any(p["match"] for p in c.plants["j"])


def test_stage_boundary_corpus_spans():
    for A in (b"pink", b"\xff", b"\x80\xfe\xffpi"):
        c, spans = S.stage_boundary_corpus(A)
        assert spans[:3] == [S.STAGE_BYTES - 1, S.STAGE_BYTES, S.STAGE_BYTES + 1] and spans[3] > 30_000 and spans[4] < 100
        assert int(c.off[256]) % 4 == 3
        for f in (0, 256, 512):
            assert c.strings[f].startswith(A) and c.strings[f + 255].endswith(A)
        long_row = [s for s in c.strings if len(s) == 30_000]
        assert len(long_row) == 1 and long_row[0].endswith(A) and long_row[0].count(A) == 1
        assert all(c.strings[r] == b"" for r in range(768, 1024) if len(c.strings[r]) != 30_000)


def test_patterns_cover_the_lengths_and_the_buffer():
    assert [len(a) for a in S.LITERALS] == [1, 2, 3, 4, 5, 9, 93]
    assert all(max(a) >= 0x80 and min(a) < 0x80 for a in S.LITERALS[1:]) and S.LITERALS[0] == b"\xff"
    assert sorted((len(a), len(b)) for a, b in S.PAIRS) == [(x, y) for x in (1, 3, 4, 5) for y in (1, 3, 4, 5)]
    assert all(a[-1] == b[0] for a, b in S.PAIRS[1:]) and S.PAIRS[0] == (b"\x80", b"\xff")
    assert len(S.PATTERN_TOO_LONG) == S.PATTERN_ROOM
    for p in S.GENERIC_PATTERNS:
        assert S.literal_shape(p) is None or p == b"%\\%"
    assert {0x00, 0x80, 0xFF, 0x25, 0x5F, 0x5C} <= set(S.ALPHABET)


def test_wrap_corpus_wraps_the_table_end():
    c, absent = S.strdict_wrap_corpus()
    cap = S.strdict_capacity(c.n)
    homes = {s: hip.hash_bytes(s) & (cap - 1) for s in set(c.strings)}
    slots = sorted(set(homes.values()))
    assert cap - 1 in slots and slots[0] < 4
    assert sum(h >= cap - 4 for h in homes.values()) > 4 and sum(h < 4 for h in homes.values()) >= 4
    assert all(hip.hash_bytes(s) & (cap - 1) >= cap - 4 and s not in homes for s in absent)
    live = [s for s, ok in zip(c.strings, c.valid) if ok]
    assert min(live.count(s) for s in homes) >= 3 and not c.valid.all()
    # a selection of every third row still holds more strings of the last four slots than fit there
    third = {c.strings[r] for r in S.third_rows(c.n) if c.valid[r]}
    assert sum(homes[s] >= cap - 4 for s in third) > 4
    assert [S.strdict_capacity(n) for n in (0, 1, 512, 513, 65536, 65537)] == [1024, 1024, 1024, 2048, 131072, 262144]


def test_strdict_corpora_shapes():
    cs = S.strdict_corpora()
    names = [c.name for c, _ in cs]
    assert len(cs) == 6 and [c.n for c, _ in cs[-2:]] == [65536, 65537]
    two = cs[2][0]
    assert len(set(two.strings)) == 2 and len({hip.hash_bytes(s) & 1023 for s in set(two.strings)} | {hip.hash_bytes(cs[2][1][0]) & 1023}) == 1, names
    for c, absent in cs:
        assert not set(absent) & set(c.strings)
        lk = S.lookup_column(c, absent)
        kinds = {(bool(ok), s in set(c.strings)) for s, ok in zip(lk.strings, lk.valid)}
        assert kinds == {(True, True), (True, False), (False, True), (False, False)}
    big = cs[-1][0]
    assert big.strings[-1] not in big.strings[:-1] and len(set(big.strings)) == 25


def test_interning_check_rejects_wrong_codes():
    strings, valid = [b"a", b"b", b"a", b"", b"b"], np.array([True, True, True, False, True])
    rows = np.arange(5)
    assert S.check_interning(strings, valid, rows, [0, 1, 0, -1, 1], -1) == {b"a": 0, b"b": 1}
    assert S.check_interning(strings, valid, rows, [2, 4, 2, -1, 4], -1) == {b"a": 2, b"b": 4}
    for bad in ([0, 1, 2, -1, 1], [0, 0, 0, -1, 0], [0, 1, 0, 3, 1], [0, 1, 0, -1, 3], [0, 1, 0, -2, 1]):
        with pytest.raises(AssertionError):
            S.check_interning(strings, valid, rows, bad, -1)
    assert S.lookup_reference({b"a": 2}, strings, valid, rows).tolist() == [2, -2, 2, -2, -2]


def test_substring_reference_equals_the_oracle_and_the_library():
    c, sel = S.substring_corpus()
    assert sorted(set(len(s) for s in c.strings)) == list(range(21)) and not c.valid.all() and len(set(sel)) < len(sel)
    args = S.substring_args()
    assert len(args) == 14 * 13 and (3, S.I64_MAX) in args and (0, S.I64_MIN) in args
    accepted = 0
    for o, ln in args:
        for slen in range(21):
            want = S.substring_start_end(slen, o, ln)
            assert want is None or 0 <= want[0] < want[1] <= slen
            assert hip.substring_range(slen, o, ln) == want, (slen, o, ln)                     # the host-compiled range of the library
        if ln == S.I64_MAX:                                                                    # the two-argument form
            assert all(S.substring(s, o, ln) == S.substring(s, o, 2 ** 32 - 1) for s in c.strings)
            assert all(S.substring(s, o, ln) == (s[o - 1:] if o > 0 else s[max(len(s) + o, 0):] if o < 0 else s) for s in c.strings), o
        if S.reference_accepts(o, ln) or ln == S.I64_MAX:
            accepted += 1
            for s in c.strings:
                assert O.substring(s, o, ln) == S.substring(s, o, ln), (s, o, ln)
    assert accepted == 10 * 8 + 14   # the offsets and lengths within +-2^32, and the two-argument form from every offset
