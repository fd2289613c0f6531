"""The VARCHAR (PH_STR) layer at its edges, compared exactly: LIKE / NOT LIKE / = / != through the position-parallel kernels, the staged
matcher (byte buffers that are not 16-byte aligned, and PH_LIKE_STAGED in a child process) and the per-row matcher (a selection), string
interning (ph_strdict_build / ph_strdict_lookup), ph_substring over the whole int64 argument domain, ph_table_strings and ph_hash over
strings. Inputs and references: str_edges.py (plain Python over bytes, checked without a device by test_str_edges_reference.py)."""
import collections
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":   # the PH_LIKE_STAGED child: no conftest.py has prepared the path
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "tests")]

import oracle_lib as O
import str_edges as S
from plan_amd import hip

pytestmark = pytest.mark.gpu

PLACEMENT_LITS = [(a, None) for a in S.LITERALS] + S.PAIRS
LIT_IDS = ["-".join(str(len(p)) for p in x if p) for x in PLACEMENT_LITS]
SHIFTS = (0, 4, 8)   # where the byte buffer starts inside its (256-byte aligned) allocation: 4 and 8 route to the staged matcher


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


class DevStr:
    """A Corpus on the device: offsets, validity, and the bytes at +0, +4 and +8 of three allocations (with room behind them: the staged
    copy reads whole words). col(shift) is the ph_col whose aux points at that copy."""

    def __init__(self, ctx, c, shifts=SHIFTS):
        self.ctx, self.c = ctx, c
        self.off = ctx.upload(c.off)
        v = c.packed_validity()
        self.validity = None if v is None else ctx.upload(v)
        self.bufs = {}
        for sh in shifts:
            host = np.zeros(sh + len(c.data) + 64, np.uint8)
            host[sh:sh + len(c.data)] = c.data
            self.bufs[sh] = ctx.upload(host)

    def col(self, shift=0):
        k = hip.Col()
        k.type, k.data, k.validity = hip.PH_STR, self.off, self.validity
        k.aux, k.aux_bytes = self.bufs[shift].value + shift, len(self.c.data)
        return k

    def free(self):
        self.ctx.free_many([self.off, self.validity] + list(self.bufs.values()))


def run_select(ctx, d, op, pattern, sel_dev=None, n_in=None, shift=0):
    n = d.c.n
    assert 0 not in pattern, "a pattern is a C string"
    s, cnt = hip.filter_select(ctx, d.col(shift), n, op, hip.const(hip.PH_STR, s=pattern), sel_in=sel_dev, n_in=n if sel_dev is None else n_in)
    got = ctx.download(s, np.int32, cnt).astype(np.int64) if cnt else np.empty(0, np.int64)
    ctx.free(s)
    return cnt, got


def check_patterns(ctx, c, like_patterns, eq_constants, shifts=SHIFTS):
    """every pattern x operator over all rows (each placement of the bytes) and over every third row (the per-row matcher): the count and
    the exact selection equal the reference's; returns how many rows were selected in all"""
    d = DevStr(ctx, c, shifts)
    sel = S.third_rows(c.n)
    sel_dev = ctx.upload(sel.astype(np.int32)) if len(sel) else None
    seen = 0
    for ops, pats in (((S.OP_LIKE, S.OP_NOTLIKE), like_patterns), ((S.OP_EQ, S.OP_NE), eq_constants)):
        for pat in pats:
            for op in ops:
                want = S.select_reference(op, pat, c.strings, c.valid)
                for sh in shifts:
                    cnt, got = run_select(ctx, d, op, pat, shift=sh)
                    assert cnt == len(want), (c.name, op, pat, sh, cnt, len(want))
                    assert np.array_equal(got, want), (c.name, op, pat, sh, np.setxor1d(got, want)[:8])
                if len(sel):
                    want_sel = S.select_reference(op, pat, c.strings, c.valid, sel)
                    cnt, got = run_select(ctx, d, op, pat, sel_dev, len(sel))
                    assert cnt == len(want_sel) and np.array_equal(got, want_sel), (c.name, op, pat, "selection")
                seen += len(want)
    if sel_dev is not None:
        ctx.free(sel_dev)
    d.free()
    return seen


# ------------------------------------------------------------------ LIKE / NOT LIKE / = / !=
@pytest.mark.parametrize("lits", PLACEMENT_LITS, ids=LIT_IDS)
def test_like_placement(ctx, lits):
    """the literal(s) planted at every position the kernels treat differently (str_edges.like_placement_corpus), for each start of the
    offsets: the corpus' own pattern, the unit as a whole, and = / != against rows of the corpus"""
    for off0 in S.PLACEMENT_OFF0:
        c = S.like_placement_corpus(lits[0], lits[1], off0)
        pats = [S.placement_pattern(c)]
        if lits[1] is not None and len(c.unit) + 2 < S.PATTERN_ROOM:
            pats.append(b"%" + c.unit + b"%")
        seen = check_patterns(ctx, c, pats, S.equality_constants(c)[:2])
        assert seen > c.n


GENERAL = {"random": S.random_corpus, "stage": lambda: S.stage_boundary_corpus()[0], "stage-1": lambda: S.stage_boundary_corpus(b"\xff")[0],
           "stage-5": lambda: S.stage_boundary_corpus(b"\x80\xfe\xffpi")[0]}


@pytest.mark.parametrize("name", list(GENERAL))
def test_like_patterns_over_general_corpora(ctx, name):
    """every pattern — the literal lengths 1..9 and 93, %A%B%, the generic matcher's, = / != — over a random corpus and over the rounds
    that just fit, exactly fill and just exceed the staged matcher's 24 KiB"""
    c = GENERAL[name]()
    pats = S.LITERAL_PATTERNS + S.PAIR_PATTERNS + S.GENERIC_PATTERNS + [b"%" + S.LITERALS[-1] + b"%"]
    if name.startswith("stage-"):
        pats = S.LITERAL_PATTERNS + S.PAIR_PATTERNS[:3] + [b"%_%", b"p_%_k", b"%\xff"]
    assert check_patterns(ctx, c, pats, S.equality_constants(c)) > 0


def test_like_degenerate_columns(ctx):
    for c in S.degenerate_corpora():
        check_patterns(ctx, c, S.LITERAL_PATTERNS[:6] + S.PAIR_PATTERNS[:2] + S.GENERIC_PATTERNS, S.equality_constants(c) + [b"pink\xff"])


def test_pattern_length_limit(ctx):
    """a pattern of 95 bytes is the longest the pattern buffer takes (test_like_placement runs it); one of 96 is refused, under every operator"""
    c = S.random_corpus(300)
    d = DevStr(ctx, c, (0,))
    for op in (S.OP_LIKE, S.OP_NOTLIKE, S.OP_EQ, S.OP_NE):
        with pytest.raises(hip.PlanHipError) as e:
            run_select(ctx, d, op, S.PATTERN_TOO_LONG)
        assert e.value.code == hip.PH_EUNSUPPORTED
        cnt, got = run_select(ctx, d, op, S.PATTERN_TOO_LONG[:-2] + b"%")
        assert np.array_equal(got, S.select_reference(op, S.PATTERN_TOO_LONG[:-2] + b"%", c.strings, c.valid))
    d.free()


# ------------------------------------------------------------------ the staged form, switched on for a whole process
def staged_cases():
    """(corpus, patterns) of the PH_LIKE_STAGED child: every placement corpus of three literals and two pairs, and the general corpora"""
    out = []
    for a, b in (PLACEMENT_LITS[0], PLACEMENT_LITS[2], PLACEMENT_LITS[4], PLACEMENT_LITS[6], PLACEMENT_LITS[8], PLACEMENT_LITS[22]):
        for off0 in S.PLACEMENT_OFF0:
            c = S.like_placement_corpus(a, b, off0)
            out.append((c, [S.placement_pattern(c)]))
    for name in GENERAL:
        out.append((GENERAL[name](), S.LITERAL_PATTERNS + S.PAIR_PATTERNS + [b"%_%"]))
    return out


def selection_digest(rows):
    return hashlib.sha256(np.ascontiguousarray(rows, dtype=np.int64).tobytes()).hexdigest()


def staged_child():
    ctx = hip.Ctx(0)
    for c, pats in staged_cases():
        d = DevStr(ctx, c, (0,))
        for pat in pats:
            for op in (S.OP_LIKE, S.OP_NOTLIKE):
                cnt, got = run_select(ctx, d, op, pat)
                print("LIKE", c.name.replace(" ", ""), pat.hex(), op, cnt, selection_digest(got), flush=True)
        d.free()
    ctx.close()
    print("DONE", flush=True)


def test_staged_form_in_a_child_process():
    """PH_LIKE_STAGED is read once per process: a fresh child runs the LIKE set over 16-byte aligned buffers through select_count_kernel's
    staged matcher and prints a digest of every selection, compared here with the reference's. Nothing else starts on the device in
    this test after a child that failed."""
    env = dict(os.environ, PH_LIKE_STAGED="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "staged-child"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("LIKE ")]
    assert r.stdout.rstrip().endswith("DONE")
    k = 0
    for c, pats in staged_cases():
        for pat in pats:
            for op in (S.OP_LIKE, S.OP_NOTLIKE):
                want = S.select_reference(op, pat, c.strings, c.valid)
                assert lines[k][1:5] == [c.name.replace(" ", ""), pat.hex(), str(op), str(len(want))], (lines[k], c.name, pat, op, len(want))
                assert lines[k][5] == selection_digest(want), (c.name, pat, op)
                k += 1
    assert k == len(lines)


# ------------------------------------------------------------------ interning
@pytest.fixture(scope="module")
def strdict_cases():
    return S.strdict_corpora()


@pytest.mark.parametrize("which", range(6))
def test_strdict_build_and_lookup(ctx, strdict_cases, which):
    """ph_strdict_build over all rows and over every third row: the partition check; ph_strdict_lookup of a second column that mixes
    present, absent (same home slot among them), empty and NULL rows, over all its rows and over a selection"""
    c, absent = strdict_cases[which]
    col = hip.DevColumn(ctx, hip.PH_STR, c.off, validity=c.packed_validity(), aux=c.data)
    lk = S.lookup_column(c, absent)
    lcol = hip.DevColumn(ctx, hip.PH_STR, lk.off, validity=lk.packed_validity(), aux=lk.data)
    lsel = np.arange(lk.n - 1, -1, -2, dtype=np.int64)
    lsel_dev = ctx.upload(lsel.astype(np.int32))
    for sel in (None, S.third_rows(c.n)):
        rows = np.arange(c.n) if sel is None else sel
        sel_dev = None if sel is None else ctx.upload(sel.astype(np.int32))
        d = hip.StrDict(ctx, col, sel_dev, len(rows))
        codes = ctx.download(d.codes, np.int32, len(rows))
        ids = S.check_interning(c.strings, c.valid, rows, codes, -1)
        assert set(ids) == {c.strings[int(r)] for r in rows if c.valid[int(r)]}
        for s2, rows2 in ((None, np.arange(lk.n)), (lsel_dev, lsel)):
            out = d.lookup(lcol, s2, len(rows2))
            got = ctx.download(out, np.int32, len(rows2))
            assert np.array_equal(got, S.lookup_reference(ids, lk.strings, lk.valid, rows2)), (c.name, sel is not None, s2 is not None)
            ctx.free(out)
        d.free()
        if sel_dev is not None:
            ctx.free(sel_dev)
    ctx.free(lsel_dev)
    col.free(); lcol.free()


def test_strdict_empty_dictionary_and_empty_lookup(ctx):
    """a dictionary over no rows holds nothing: every lookup is -2; a lookup column without bytes finds the empty string where the
    dictionary holds it"""
    c = S.random_corpus(200)
    col = hip.DevColumn(ctx, hip.PH_STR, c.off, validity=c.packed_validity(), aux=c.data)
    d = hip.StrDict(ctx, col, None, 0)
    out = d.lookup(col, None, c.n)
    assert np.all(ctx.download(out, np.int32, c.n) == -2)
    ctx.free(out); d.free()
    one = hip.StrDict(ctx, col, None, 1)                                # n = 1
    assert ctx.download(one.codes, np.int32, 1)[0] == (0 if c.valid[0] else -1)
    one.free()
    empty = S.Corpus([b""] * 50, np.arange(50) % 5 != 0)
    ecol = hip.DevColumn(ctx, hip.PH_STR, empty.off, validity=empty.packed_validity(), aux=empty.data)
    assert ecol.aux_bytes == 0
    for build, bcol in ((c, col), (empty, ecol)):
        d = hip.StrDict(ctx, bcol, None, build.n)
        ids = S.check_interning(build.strings, build.valid, np.arange(build.n), ctx.download(d.codes, np.int32, build.n), -1)
        out = d.lookup(ecol, None, empty.n)
        assert np.array_equal(ctx.download(out, np.int32, empty.n), S.lookup_reference(ids, empty.strings, empty.valid, np.arange(empty.n)))
        ctx.free(out); d.free()
    col.free(); ecol.free()


def test_strdict_codes_group_like_the_strings(ctx, strdict_cases):
    """count(*) by code over the wrap corpus equals a Counter over the strings (NULL rows: the NULL group)"""
    c, _ = strdict_cases[0]
    col = hip.DevColumn(ctx, hip.PH_STR, c.off, validity=c.packed_validity(), aux=c.data)
    d = hip.StrDict(ctx, col, None, c.n)
    key = hip.Col(); key.type, key.data, key.validity = hip.PH_I32, d.codes, col.validity
    ones = hip.DevColumn(ctx, hip.PH_I64, np.ones(c.n, np.int64))
    agg = hip.Agg(ctx, [hip.PH_I32], [(hip.PH_A_SUM, 0), (hip.PH_A_COUNT_STAR, 0)], 256)
    agg.sink([key], [ones, ones], None, c.n)
    r = agg.finalize(room=256)
    got = collections.Counter()
    for g in range(r["ngroups"]):
        got[None if r["key_null"][g][0] else c.strings[int(r["keys"][g][0])]] += int(r["count"][g][1])
        assert r["sum"][g][0] == int(r["count"][g][1])
    assert got == collections.Counter(s if ok else None for s, ok in zip(c.strings, c.valid))
    agg.free(); d.free(); col.free(); ones.free()


# ------------------------------------------------------------------ substring
def run_substring(ctx, col, o, ln, sel_dev, n):
    po, pb, nb = hip.substring(ctx, col, o, ln, sel_dev, n)
    off = ctx.download(po, np.int32, n + 1)
    data = ctx.download(pb, np.uint8, nb).tobytes() if nb > 0 else b""
    ctx.free(po); ctx.free(pb)
    return off, data, nb


def test_substring_over_the_int64_domain(ctx):
    """ph_substring for every (offset, length) of substring_args, over all rows and over a selection with repeated row ids: offsets,
    bytes and the total equal the unbounded evaluation of substringStartEnd; length = INT64_MAX equals 2^32 - 1 from every offset.
    (Before substr_range was made overflow-free, 30 of these 364 calls failed on the device: every offset whose start is not 0 —
    -3, -1, 3, 40, 2^32 - 1, 2^32, INT64_MAX — with the lengths INT64_MAX - 1 and INT64_MAX, and offset 2 with INT64_MAX. They returned
    negative row lengths, e.g. offsets 0, -2, -4, -6 .. and a total of -87 bytes for (-1, INT64_MAX - 1), or PH_EUNSUPPORTED for a
    byte total beyond 2^31.)"""
    c, sel = S.substring_corpus()
    col = hip.DevColumn(ctx, hip.PH_STR, c.off, validity=c.packed_validity(), aux=c.data)
    sel_dev = ctx.upload(sel.astype(np.int32))
    bad = []
    for o, ln in S.substring_args():
        for s, rows in ((None, np.arange(c.n)), (sel_dev, sel)):
            try:
                off, data, nb = run_substring(ctx, col, o, ln, s, len(rows))
            except hip.PlanHipError as e:       # no argument is refused: the result never exceeds the rows' own bytes
                bad.append((o, ln, s is not None, "error", e.code))
                continue
            want = [S.substring(c.strings[int(r)], o, ln) if c.valid[int(r)] else b"" for r in rows]
            woff = np.concatenate([[0], np.cumsum([len(w) for w in want])])
            if not (nb == woff[-1] and np.array_equal(off, woff) and data == b"".join(want)):
                bad.append((o, ln, s is not None, int(nb), off[:4].tolist()))
    assert not bad, (len(bad), bad[:12])
    for o in S.SUBSTRING_OFFSETS:
        a, b = run_substring(ctx, col, o, S.I64_MAX, None, c.n), run_substring(ctx, col, o, 2 ** 32 - 1, None, c.n)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2], o
    ctx.free(sel_dev)
    col.free()


def test_table_strings_returns_the_rows_bytes(ctx):
    """ph_table_strings (the whole string of each row: the two-argument substring from offset 1) with repeated rows, a NULL row and an
    empty row, as raw bytes"""
    c, _ = S.substring_corpus()
    t = hip.Table(ctx, [dict(typ=hip.PH_STR, arr=c.off, validity=c.packed_validity(), aux=c.data)], c.n)
    null_row = int(np.flatnonzero(~c.valid)[0])
    empty_row = next(r for r in range(c.n) if c.valid[r] and c.strings[r] == b"")
    rows = [c.n - 1, 0, null_row, 7, 7, empty_row, 7, 0, c.n - 1] + list(range(c.n))
    got = hip.table_strings_bytes(ctx, t, 0, rows)
    assert got == [c.strings[r] if c.valid[r] else b"" for r in rows]
    assert hip.table_strings_bytes(ctx, t, 0, []) == []
    t.free()


# ------------------------------------------------------------------ hash
def test_hash_of_string_columns(ctx):
    """ph_hash over a PH_STR column: every length 0..40 and 63, 64, 65 over all byte values, NULL rows, alone and combined with an INTEGER
    column (ph_hash takes no selection) — against the host's hash_bytes (pinned to the reference's HashBytes by test_abi.py) and the oracle's column hash"""
    rng = np.random.default_rng(64)
    rows = []
    for m in list(range(41)) + [63, 64, 65]:
        rows += [bytes(rng.integers(0, 256, m).astype(np.uint8)) for _ in range(4)]
        rows.append(bytes([0xFF]) * m)
        rows.append(bytes(m))
    assert set(b"".join(rows)) == set(range(256))
    c = S.Corpus(rows, rng.random(len(rows)) >= 0.1)
    ints = rng.integers(-2 ** 31, 2 ** 31 - 1, c.n).astype(np.int32)
    iv = np.packbits(rng.random(c.n) >= 0.1, bitorder="little")
    for valid in (None, c.packed_validity()):
        sc = hip.DevColumn(ctx, hip.PH_STR, c.off, validity=valid, aux=c.data)
        ic = hip.DevColumn(ctx, hip.PH_I32, ints, validity=iv)
        osc, oic = O.col(O.OT_VARCHAR, c.off, validity=valid, dictionary=c.data), O.col(O.OT_INT32, ints, validity=iv)
        for dcols, ocols in (([sc], [osc]), ([sc, ic], [osc, oic]), ([ic, sc], [oic, osc])):
            out = hip.hash_cols(ctx, dcols, c.n)
            got = ctx.download(out, np.uint64, c.n)
            ctx.free(out)
            assert np.array_equal(got, O.hash_cols(ocols, c.n)), (valid is not None, len(dcols))
            if len(dcols) == 1 and valid is None:
                assert [int(x) for x in got] == [hip.hash_bytes(s) for s in c.strings]
        sc.free(); ic.free()


if __name__ == "__main__" and sys.argv[1:] == ["staged-child"]:
    staged_child()
