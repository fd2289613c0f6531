"""ph_sort_rows at the seams of its own structure (plan_amd/csrc/ops_sort.hip): the corpora of sort_edges.py, each proven by
test_sort_edges_reference.py to reach the edge it is named for, sorted on the device and compared with sort_edges.order. Every comparison
is exact equality of int32 permutations."""
import ctypes

import numpy as np
import pytest

import sort_edges as S
from plan_amd import hip

pytestmark = pytest.mark.gpu

HIP_TYPE = {"I32": hip.PH_I32, "DATE": hip.PH_DATE, "CODE8": hip.PH_CODE8, "DEC64": hip.PH_DEC64}


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


def upload(ctx, col):
    """a DevColumn of a sort_edges NumCol / StrCol (the StrCol's own offsets and bytes, whatever their layout)"""
    valid = None if col.valid is None else np.packbits(col.valid, bitorder="little")
    if isinstance(col, S.StrCol):
        return hip.DevColumn(ctx, hip.PH_STR, col.off, validity=valid, aux=col.data)
    return hip.DevColumn(ctx, HIP_TYPE[col.type], col.values, col.scale, validity=valid)


class Uploaded:
    """the device copies of a case's columns, each distinct column uploaded once"""

    def __init__(self, ctx, cols):
        self.by_id = {}
        for c in cols:
            if id(c) not in self.by_id:
                self.by_id[id(c)] = upload(ctx, c)
        self.cols = [self.by_id[id(c)] for c in cols]

    def free(self):
        for d in self.by_id.values():
            d.free()


def device_order(ctx, dev_cols, desc, sel, n):
    m = n if sel is None else len(sel)
    sd = None if sel is None else ctx.upload(np.asarray(sel, dtype=np.int32))
    try:
        out = hip.sort_rows(ctx, dev_cols, desc, sd, m)
        got = ctx.download(out, np.int32, m).tolist()
        ctx.free(out)
    finally:
        if sd is not None:
            ctx.free(sd)
    return got


def directions(desc):
    return ",".join("DESC" if d else "ASC" for d in desc)


def assert_order(got, want, corpus, desc, selection):
    if got != want:
        at = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
        pytest.fail(f"{corpus} [{directions(desc)}; selection: {selection}]: first difference at position {at} of {len(want)}: "
                    f"device row {got[at] if at < len(got) else None}, reference row {want[at] if at < len(want) else None}")


def run_case(ctx, name, cols, desc, n, sels):
    """one case under every selection of `sels` ({kind: rows or None}); the keys are built once"""
    keys = [S.pykeys(c) for c in cols]
    up = Uploaded(ctx, cols)
    try:
        for kind, sel in sels.items():
            got = device_order(ctx, up.cols, desc, sel, n)
            assert_order(got, S.order(range(n) if sel is None else sel, keys, desc), name, desc, kind)
    finally:
        up.free()


# ------------------------------------------------------------------ numeric corpora

@pytest.mark.parametrize("kind", S.LAYOUTS)
def test_digit_layouts_at_the_tile_wave_and_chunk_seams(ctx, kind):
    """one PH_I32 key of digits 0..255 (one radix pass; none for (f)) laid out lane by lane, at every seam size, alone and with a tie-heavy
    key behind it, under every selection kind"""
    for name, cols, desc in S.digit_cases(kind):
        n = len(cols[0].values)
        run_case(ctx, name, cols, desc, n, S.selections(n))


def test_columns_that_vary_in_chosen_bytes(ctx):
    """the passes that run: one byte only (each of the 8), bytes 0 and 5, all bytes, none (a constant key as first, middle and last), the
    NULL flag alone, only row 0 differing, row 0 NULL before a constant"""
    for name, cols, desc, _ in S.byte_cases():
        run_case(ctx, name, cols, desc, S.N_BYTES, S.selections(S.N_BYTES))


def test_eight_keys(ctx):
    """the maximum of 8 keys, mixed types and directions, each key breaking ties of those before it"""
    cols, desc = S.eight_keys()
    run_case(ctx, "eight keys", cols, desc, S.N_BYTES, S.selections(S.N_BYTES))


# ------------------------------------------------------------------ VARCHAR corpora

@pytest.mark.parametrize("name", S.VARCHAR_NAMES)
def test_varchar_refinement(ctx, name):
    """every VARCHAR corpus ASC and DESC, alone and as the first of two keys under a shuffled selection"""
    col = S.varchar_corpus(name)
    n = len(col.strings)
    for label, cols, desc, sel in S.varchar_runs(col):
        run_case(ctx, name, cols, desc, n, {"none" if sel is None else "shuffled": sel})


class MisalignedStr:
    """The bytes of a StrCol uploaded behind k pad bytes: the column's aux points at base + k and aux_bytes is the corpus size. Owns the
    base pointer (k + nbytes bytes) and the offsets."""

    def __init__(self, ctx, col, k):
        self.ctx = ctx
        nbytes = len(col.data)
        self.base = ctx.upload(np.concatenate([np.full(k, 0xFF, np.uint8), col.data]))   # k + nbytes bytes
        self.off = ctx.upload(col.off)
        self.c = hip.Col()
        self.c.type, self.c.scale = hip.PH_STR, 0
        self.c.data = self.off
        self.c.validity = None
        self.c.aux = ctypes.c_void_p(self.base.value + k)
        self.c.aux_bytes = nbytes

    def free(self):
        self.ctx.free(self.base)
        self.ctx.free(self.off)


@pytest.mark.parametrize("k", [1, 3, 7])
def test_alignment_sweep_behind_a_misaligned_base(ctx, k):
    """the alignment sweep with the byte buffer's base at 1, 3 and 7 bytes past an 8-byte boundary: every word comes through the byte loads.
    The same four runs as every VARCHAR corpus: ASC and DESC, alone and as the first of two keys under a shuffled selection (the rows are
    then read through a permutation that is not the identity)"""
    for part in (0, 1):
        col, _ = S.alignment_sweep(part)
        n = len(col.strings)
        dev = MisalignedStr(ctx, col, k)
        others = {}
        try:
            assert dev.base.value % 8 == 0 and dev.c.aux % 8 == k
            for label, cols, desc, sel in S.varchar_runs(col):
                for c in cols[1:]:
                    if id(c) not in others:
                        others[id(c)] = upload(ctx, c)
                dev_cols = [dev.c] + [others[id(c)] for c in cols[1:]]
                assert cols[0] is col and (sel is None) == (len(cols) == 1)
                got = device_order(ctx, dev_cols, desc, sel, n)
                want = S.order(range(n) if sel is None else sel, [S.pykeys(c) for c in cols], desc)
                assert_order(got, want, f"alignment_sweep part {part} at base + {k}", desc, "none" if sel is None else "shuffled")
        finally:
            dev.free()
            for d in others.values():
                d.free()


# ------------------------------------------------------------------ argument edges

def test_key_count_limits(ctx):
    """9 keys and 0 keys are PH_EINVAL before any launch"""
    c = hip.DevColumn(ctx, hip.PH_I32, np.arange(10, dtype=np.int32))
    try:
        for nkeys in (9, 0):
            with pytest.raises(hip.PlanHipError) as e:
                hip.sort_rows(ctx, [c] * nkeys, [False] * nkeys, None, 10)
            assert e.value.code == hip.PH_EINVAL, nkeys
        out = hip.sort_rows(ctx, [c] * 8, [True] * 8, None, 10)       # 8 keys are the maximum
        assert ctx.download(out, np.int32, 10).tolist() == list(range(9, -1, -1))
        ctx.free(out)
    finally:
        c.free()


def test_zero_rows_leave_the_output_untouched(ctx):
    canary = np.array([0x5EED0001, -2, 0x5EED0003, 7], np.int32)
    c = hip.DevColumn(ctx, hip.PH_I32, np.arange(10, dtype=np.int32))
    s = hip.str_column(ctx, [b"a", None, b""])
    sel = ctx.upload(np.array([3, 1], np.int32))
    out = ctx.upload(canary)
    try:
        for keys in ([c], [s], [c, s]):
            for sd in (None, sel):
                desc = (hip.i32 * len(keys))(*[0] * len(keys))
                hip.check(hip.lib().ph_sort_rows(ctx.h, hip._cols(keys), desc, hip.i32(len(keys)), sd, hip.i64(0), out))
                ctx.sync()
                assert ctx.download(out, np.int32, 4).tolist() == canary.tolist()
    finally:
        for p in (sel, out):
            ctx.free(p)
        c.free()
        s.free()
