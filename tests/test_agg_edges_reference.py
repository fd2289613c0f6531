"""The constructed inputs and the plain reference of the aggregate edge tests (agg_edges.py), checked without a device: the hash twins
against the kernels' source text, the hash bits every builder claims, the values every edge table must hold, and the reference against
the oracle's GROUP BY and a double loop. A GPU test over inputs that lost their structure would still pass; this file is what fails."""
import os
import re

import numpy as np
import pytest

import agg_edges as A
import join_edges as J
import oracle_lib as O
from domain_edges import civil_days
from join_edges import I32_MAX, I32_MIN, I64_MAX, I64_MIN
from plan_amd import hip

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "plan_amd", "csrc")
CODES = O.cdict([f"code{i:03d}" for i in range(256)])


def bits(v):
    return None if v is None else np.packbits(v, bitorder="little")


# ------------------------------------------------------------------ the twins
def kh_int(ks, nm):
    h = J.mix64_int((nm + A.KH_SEED) & J.M64)
    for c, k in enumerate(ks):
        h = J.mix64_int(h ^ (0 if (nm >> c) & 1 else k & J.M64))
    return h


def lh_int(ks, nm, c1=A.LH_NULL_MUL, c2=A.LH_MUL1, c3=A.LH_MUL2, s1=A.LH_SHIFT_MID, s2=A.LH_SHIFT_END):
    m = 0xFFFFFFFF
    h = nm * c1 & m
    for c, k in enumerate(ks):
        k = 0 if (nm >> c) & 1 else k & J.M64
        h ^= k & m
        h = h * c2 & m
        h ^= ((k >> 32) + (h >> s1)) & m
        h = h * c3 & m
    return h ^ (h >> s2)


def test_hash_twins_equal_their_integer_forms_and_widen_as_the_kernels_do():
    rng = np.random.default_rng(1)
    n = 300
    a = rng.integers(I32_MIN, I32_MAX, n, endpoint=True).astype(np.int32)
    b = rng.integers(I64_MIN, I64_MAX, n, endpoint=True, dtype=np.int64)
    c = rng.integers(0, 256, n).astype(np.uint8)
    a[:3], b[:3], c[:3] = [-1, I32_MIN, 0], [I64_MIN, -1, 2 ** 32], [255, 128, 0]
    for cols in ([a], [b], [c], [a, b], [b, a], [a, a, b], [b, c, a, a]):
        for nm in (0, 1, (1 << len(cols)) - 1, rng.integers(0, 1 << len(cols), n)):
            nms = np.broadcast_to(np.asarray(nm), (n,)).tolist()
            rows = [[int(x[i]) for x in cols] for i in range(n)]
            assert A.keys_hash(cols, nm).tolist() == [kh_int(r, m) for r, m in zip(rows, nms)]
            assert A.lds_hash(cols, nm).tolist() == [lh_int(r, m) for r, m in zip(rows, nms)]
    # sign- and zero-extension: an int32 -1 is the int64 -1, a CODE8 255 is 255; bytes under a NULL do not matter
    m1_32, m1_64, c255 = np.array([-1], np.int32), np.array([-1], np.int64), np.array([255], np.uint8)
    assert A.keys_hash([m1_32]) == A.keys_hash([m1_64]) != A.keys_hash([c255]) == A.keys_hash([np.array([255], np.int64)])
    assert A.lds_hash([m1_32]) == A.lds_hash([m1_64]) != A.lds_hash([c255]) == A.lds_hash([np.array([255], np.int64)])
    assert A.keys_hash([a, b], 1).tolist() == A.keys_hash([a[::-1].copy(), b], 1).tolist()
    assert A.lds_hash([a, b], 2).tolist() == A.lds_hash([a, b[::-1].copy()], 2).tolist()
    # the mask is hashed: (NULL, 0), (0, NULL), (NULL, NULL), (0, 0) are four hash words in both hashes
    z = [np.zeros(1, np.int64), np.zeros(1, np.int64)]
    assert len({int(A.keys_hash(z, m)[0]) for m in range(4)}) == 4 and len({int(A.lds_hash(z, m)[0]) for m in range(4)}) == 4


@pytest.mark.parametrize("nk", [1, 2, 3, 4])
@pytest.mark.parametrize("nullmask", [0, "prefix"])
def test_solve_last_key_round_trips(nk, nullmask):
    rng = np.random.default_rng(nk)
    n = 5000
    types = ["i32", "code8", "i64"][: nk - 1]
    prefix = [rng.integers(I32_MIN, I32_MAX, n, endpoint=True).astype(np.int32), rng.integers(0, 256, n).astype(np.uint8),
              rng.integers(I64_MIN, I64_MAX, n, endpoint=True, dtype=np.int64)][: nk - 1]
    assert len(prefix) == len(types)
    nm = 0 if nullmask == 0 else (1 << (nk - 1)) - 1      # (one key: no prefix column to be NULL, the mask stays 0)
    wanted = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    wanted[:4] = [0, 1, 2 ** 63, 2 ** 64 - 1]
    k = A.solve_last_key(prefix, nm, wanted)
    assert k.dtype == np.int64 and np.array_equal(A.keys_hash(prefix + [k], nm), wanted)
    assert kh_int([int(p[7]) for p in prefix] + [int(k[7])], nm) == int(wanted[7])
    if nk > 1:
        with pytest.raises(AssertionError):
            A.solve_last_key(prefix, 1 << (nk - 1), wanted)


# ------------------------------------------------------------------ the twins and the layout constants against the source text
def _body(text, head, twin):
    assert head in text, f"the source no longer has `{head}` — find its successor, then update {twin} and this pin"
    at = text.index(head)
    return text[at: text.index("\n}\n", at)]


def _ints(pattern, text):
    return [int(x, 0) for x in re.findall(pattern, text)]


def _c_eval(expr, **names):
    """a C integer expression of the host code, with the given names"""
    expr = re.sub(r"\b(a->nkeys|P\.nkeys|nk)\b", "NK", expr)
    expr = re.sub(r"\b(a->naggs|P\.naggs|na)\b", "NA", expr)
    assert re.fullmatch(r"[\sNKA0-9+*()]+", expr), expr
    return eval(expr, {"__builtins__": {}}, names)


def source_pins(csrc):
    """[(what, value in the source, value in agg_edges / join_edges, the twin to update)] — every number the builders rely on, read from
    the kernels' text"""
    util = open(os.path.join(csrc, "device_util.h")).read()
    sink = open(os.path.join(csrc, "agg_sink.inc")).read()
    ops = open(os.path.join(csrc, "ops_agg.hip")).read()
    pins = []
    # mix64: multipliers and shifts, in order
    mix = _body(util, "uint64_t mix64(uint64_t x) {", "join_edges.mix64")
    steps = re.findall(r"x \^= x >> (\d+);|x \*= (0x[0-9a-fA-F]+)ULL;", mix)
    rebuilt = []
    for sh, mul in steps:
        rebuilt.append(("shift", int(sh)) if sh else ("mul", int(mul, 16)))
    pins.append(("mix64's steps", rebuilt, [("shift", 30), ("mul", J.MUL1), ("shift", 27), ("mul", J.MUL2), ("shift", 31)], "join_edges.mix64 / inv_mix64"))
    x = 0x0123456789ABCDEF

    def run(steps_, v):
        for kind, k in steps_:
            v = v ^ (v >> k) if kind == "shift" else v * k & J.M64
        return v
    pins.append(("mix64 of a test word", run(rebuilt, x), J.mix64_int(x), "join_edges.mix64"))
    # keys_hash: the seed and the fold
    kh = _body(sink, "uint64_t keys_hash(const unsigned long long *k, unsigned nullmask, int nkeys) {", "agg_edges.keys_hash")
    pins.append(("keys_hash's seed", _ints(r"uint64_t h = mix64\(\(uint64_t\)nullmask \+ (0x[0-9a-fA-F]+)ULL\);", kh), [A.KH_SEED], "agg_edges.KH_SEED / keys_hash"))
    pins.append(("keys_hash's fold", re.findall(r"if \(c < nkeys\) (h = mix64\(h \^ k\[c\]\);)", kh), ["h = mix64(h ^ k[c]);"], "agg_edges.keys_hash"))
    # lds_hash: every statement, with its constants
    lh = _body(sink, "unsigned lds_hash(const unsigned long long *k, unsigned nullmask) {", "agg_edges.lds_hash")
    stmts = [s.strip() for s in lh.split("\n")[1:] if s.strip() and not s.strip().startswith("#pragma")]
    want = [f"unsigned h = nullmask * 0x{A.LH_NULL_MUL:08X}u;", "for (int c = 0; c < NK; c++) {", "h ^= (unsigned)k[c];", f"h *= 0x{A.LH_MUL1:08X}u;",
            f"h ^= (unsigned)(k[c] >> 32) + (h >> {A.LH_SHIFT_MID});", f"h *= 0x{A.LH_MUL2:08X}u;", "}", f"return h ^ (h >> {A.LH_SHIFT_END});"]
    pins.append(("lds_hash's statements", stmts, want, "agg_edges.lds_hash and its LH_* constants"))
    # widening of the key words: all three copies of the switch
    for name, text in (("load_key", _body(sink, "unsigned long long load_key(const AggCol &c, int64_t r) {", "join_edges.as_u64")),
                       ("load_key_t", _body(sink, "unsigned long long load_key_t(int type, const void *data, int64_t r) {", "join_edges.as_u64"))):
        pins.append((f"{name}'s widening", [bool(re.search(r"case PH_I32: case PH_DATE: return \(unsigned long long\)\(long long\)\(\(const int32_t \*\)", text)),
                                            bool(re.search(r"case PH_CODE8: return \(\(const uint8_t \*\)", text))], [True, True], "join_edges.as_u64"))
    batch = _body(ops, "void bulk_keys_batch(const AggSinkParams &S, int64_t base, int64_t i1, int64_t (&ii)[BU], int64_t (&rr)[BU],", "join_edges.as_u64")
    plaink = batch[batch.index("if (PLAINK) {"): batch.index("} else {\n#pragma unroll\n        for (int u = 0; u < BU; u++) bulk_row_keys")]
    pins.append(("bulk_keys_batch's widening (PLAINK)", re.findall(r"k\[u\]\[c\] = ([^;]+);", plaink),
                 ["(unsigned long long)(long long)((const int32_t *)S.key[c].data)[rr[u]]", "((const uint8_t *)S.key[c].data)[rr[u]]",
                  "((const unsigned long long *)S.key[c].data)[rr[u]]"], "join_edges.as_u64"))
    pins.append(("bulk_keys_batch's type tests (PLAINK)", re.findall(r"(?:if|else if) \(([^)]+)\) \{\n#pragma unroll\n\s+for \(int u", plaink),
                 ["t == PH_I32 || t == PH_DATE", "t == PH_CODE8"], "join_edges.as_u64"))
    # partition bits
    pins.append(("partition of a row", len(re.findall(r"\(keys_hash\(k\[u\], nm\[u\], NK\) >> B\.shift\) & \(B\.nparts - 1\)", ops)) >= 2, True, "agg_edges.partition_of"))
    assert A.PART_FIXED[0] == A.PART_SHIFT and A.PART_FIXED[1] >= A.PART_SHIFT + A.PART_MAX_BITS - 1
    # probe windows and the closing rule
    pins.append(("probe window of the bulk builds", _ints(r"probes < (\d+) && spins < \(1 << 16\)", ops), [A.PROBE_WINDOW] * 2, "agg_edges.PROBE_WINDOW"))
    pins.append(("probe windows of the sliced / direct partial build", [list(map(int, m)) for m in re.findall(r"PROBE_MAX = DIRECT \? (\d+) : (\d+);", sink)],
                 [[A.DIRECT_PROBE_WINDOW, A.PROBE_WINDOW]], "agg_edges.PROBE_WINDOW / DIRECT_PROBE_WINDOW"))
    pins.append(("probe window of the sink's LDS table", _ints(r"probes < (\d+) && (?:__ballot|spins)", sink), [A.SINK_PROBE_WINDOW] * 2, "agg_edges.SINK_PROBE_WINDOW"))
    closing = re.findall(r">= (T - T / 4)\)", ops) + re.findall(r">= (T - T / 4)\)", sink)
    pins.append(("closing rule of the LDS tables", closing, ["T - T / 4"] * 4, "agg_edges.closes_at"))
    pins.append(("error-flag guard", _ints(r"\(guard & (\d+)\) == (?:\d+)", sink + ops) + _ints(r"\(guard & \d+\) == (\d+)", sink + ops), [A.CHUNK_GUARD] * 6, "agg_edges.CHUNK_GUARD"))
    # what orders the records a build workgroup reads: 1024 records per step (the scatter workgroups' row ranges: sizing_pins)
    pins.append(("records per build step", _ints(r"for \(int64_t t = start \+ threadIdx\.x; t < end; t \+= (\d+)\)", ops) +
                 _ints(r"for \(int64_t tb = t0; tb < t1; tb \+= (\d+) \* U\)", sink), [A.BUILD_THREADS] * 2, "agg_edges.BUILD_THREADS"))
    pins.append(("smallest table", _ints(r"next_pow2\(std::max<int64_t>\((\d+), 2 \* a->expected_groups\)\)", ops)[:1], [A.MIN_TABLE], "agg_edges.MIN_TABLE"))
    need = _body(ops, "bool agg_spec_need_cnt(const ph::AggSinkParams &P) {", "the need_cnt argument of agg_edges.spec_slots in test_gpu_agg_edges.py")
    pins.append(("agg_spec_need_cnt: an aggregate over a column with a validity bitmap", "P.agg_kind[a] != PH_A_COUNT_STAR && P.arg[P.agg_arg[a]].validity) return true;" in need, True,
                 "the need_cnt argument of agg_edges.spec_slots in test_gpu_agg_edges.py"))
    return pins


def sizing_pins():
    """the same for the sizes the host chooses (plan_amd/csrc/agg_forms.h): agg_edges' twins against the library's own rule, asked through
    ph_agg_sink_choice over a grid of (keys, aggregates)"""
    pins = []
    grid = [(nk, na) for nk in (1, 2, 3, 4) for na in (0, 1, 2, 6, 16)]
    big, small = 4_300_000, 200_000

    def ask(rows, hint, nk, na, **kw):
        return hip.agg_sink_choice(rows, hint, nkeys=nk, naggs=na, used_args=min(na, 1), **kw)
    second = [ask(big, 50_000, nk, na) for nk, na in grid]
    first = [ask(small, 100_000, nk, na) for nk, na in grid]
    pins.append(("T of the bulk forms", [[s["T"] for _, s in second], [s["T"] for _, s in first]], [[A.bulk_T(nk, na) for nk, na in grid]] * 2, "agg_edges.bulk_T"))
    pins.append(("per_entry of the bulk forms", [s["lds_build"] // s["T"] for _, s in second + first], [A.bulk_per_entry(nk, na) for nk, na in grid] * 2,
                 "agg_edges.bulk_per_entry"))
    pins.append(("partitions of the first form", [(k, s["nparts"], s["shift"]) for k, s in first],
                 [("bulk1", A.bulk1_parts(small, 100_000, A.bulk_T(nk, na)), A.PART_SHIFT) for nk, na in grid], "agg_edges.bulk1_parts / PART_SHIFT"))
    for hint in (50_000, 262_144, 262_145, 600_000):
        got, want = [], []
        for nk, na in grid:
            kind, s = ask(big, hint, nk, na)
            bins, two_level = A.bulk2_bins(hint, A.bulk_T(nk, na))
            got.append((kind, s["bins"], s["nparts"], s["shift"]))
            if bins > 1 << A.PART_MAX_BITS:       # (the first form instead)
                parts = A.bulk1_parts(big, hint, A.bulk_T(nk, na))
                want.append(("bulk1", parts, parts, A.PART_SHIFT))
            else:
                want.append(("two_level", bins, 64, A.PART_SHIFT + bins.bit_length() - 1 - 6) if two_level else ("bulk2_spec", bins, bins, A.PART_SHIFT))
        pins.append((f"bins, first level and shifts of the second form, hint {hint}", got, want, "agg_edges.bulk2_bins / PART_SHIFT"))
    most = [ask(big, (1 << A.PART_MAX_BITS) * (A.bulk_T(nk, na) // 4) + d, nk, na) for nk, na in grid for d in (0, 1)]
    pins.append(("most bins / partitions", [(k, s["bins"]) for k, s in most], [("two_level", 1 << A.PART_MAX_BITS), ("bulk1", 1 << (A.PART_MAX_BITS - 1))] * len(grid),
                 "agg_edges.PART_MAX_BITS"))
    pins.append(("scatter range of the first form", [s["rows_per_wg"] for _, s in first] + [ask((4 << 20) - 1, 100_000, 1, 2)[1]["rows_per_wg"]],
                 [A.bulk1_scatter_range(small)] * len(grid) + [A.bulk1_scatter_range((4 << 20) - 1)], "agg_edges.bulk1_scatter_range"))
    pins.append(("scatter range of the second form", [s["rows_per_wg"] for _, s in second], [A.bulk2_scatter_range(big, 256 * s["bu"]) for _, s in second],
                 "agg_edges.bulk2_scatter_range"))
    pins.append(("largest chunk of the second form", 256 * max(s["bu"] for _, s in second), A.BULK2_CHUNK_MAX, "agg_edges.BULK2_CHUNK_MAX"))
    pins.append(("second form's row threshold", [ask((4 << 20) - 1, 50_000, 1, 2)[0], ask(4 << 20, 50_000, 1, 2)[0]], ["bulk1", "bulk2_spec"],
                 "the bulk2 / two_level row counts of the GPU tests"))
    pins.append(("slots of the generic sink", [ask(5_000, 16, nk, na)[1]["slots"] for nk, na in grid], [A.sink_slots(nk, na) for nk, na in grid],
                 "agg_edges.sink_slots / sink_per_entry"))
    for hint in (16, 175, 1024, 3000, 5000, 100_000):
        for need_cnt in (False, True):       # (rows_sunk = 1: never a bulk build, whatever the hint)
            pins.append((f"slots of the specialised sink, hint {hint}, need_cnt {need_cnt}",
                         [ask(1 << 20, hint, nk, na, rows_sunk=1, need_cnt=need_cnt)[1]["slots"] for nk, na in grid],
                         [A.spec_slots(nk, na, need_cnt, hint) for nk, na in grid], "agg_edges.spec_slots / spec_per_entry"))
    return pins



def test_twins_and_layout_constants_are_those_of_the_kernel_source(monkeypatch):
    for k in ("PH_AGG_JIT", "PH_AGG_NO_BULK", "PH_AGG_BULK_V1", "PH_AGG_BULK_ONE_LEVEL"):
        monkeypatch.delenv(k, raising=False)
    wrong = [f"{what}: the source has {got!r}, the tests assume {want!r} — update {twin}" for what, got, want, twin in source_pins(CSRC) + sizing_pins() if got != want]
    assert not wrong, "\n".join(wrong)


def test_layout_functions():
    assert A.closes_at(512) == 384 and A.closes_at(4096) == 3072
    assert [A.bulk_T(nk, 6) for nk in (1, 2, 3, 4)] == [512, 512, 512, 512] and A.bulk_T(1, 2) == 2048 and A.bulk_T(1, 0) == 4096 and A.bulk_T(4, 16) == 256
    assert A.sink_slots(1, 6) == 256 and A.sink_slots(4, 6) == 256 and A.sink_slots(1, 1) == 1024 and A.sink_slots(4, 16) == 128
    assert A.spec_slots(1, 6, True, 1024) == 256 and A.spec_slots(1, 6, True, 175) == 256 and A.spec_slots(2, 1, False, 1024) == 2048
    assert A.bulk1_parts(200_000, 100_000, 512) == 1024 and A.bulk1_parts(4_300_000, 50_000, 512) == 512
    assert A.bulk2_bins(50_000, 512) == (512, False) and A.bulk2_bins(600_000, 512) == (8192, True)
    # every partition count in use is a power of two of at most 2^14 bins: bits 40..53 decide it
    assert 8192 <= 1 << (A.PART_FIXED[1] - A.PART_FIXED[0] + 1)


# ------------------------------------------------------------------ the builders' claims
LOW24 = np.uint64((1 << A.GLOBAL_SLOT_BITS) - 1)


@pytest.mark.parametrize("two_key", [False, True])
@pytest.mark.parametrize("m,victims", [(300, 40), (2000, 40)])
def test_one_global_slot_has_its_structure(m, victims, two_key):
    g = A.one_global_slot(m, victims, two_key=two_key)
    assert g.types == (["i32", "i64"] if two_key else ["i64"]) and g.cols[-1].dtype == np.int64
    h = g.hash()
    assert len(g) == m + victims and len(set(g.tuples())) == m + victims and len(np.unique(h)) == m + victims
    home = g.info["home"]
    assert ((h[:m] & LOW24) == home).all()
    assert m > A.CHUNK_GUARD + 1 and m > A.PROBE_WINDOW                # a probe walk passes the error-flag guard
    for cap in (A.MIN_TABLE, 1 << 14, 1 << 20, 1 << A.GLOBAL_SLOT_BITS):  # one home slot, and the victims strictly inside the chain, in every table
        slot = (h & np.uint64(cap - 1)).astype(np.int64)
        first = home & (cap - 1)
        assert (slot[:m] == first).all() and first + m <= cap
        assert ((slot[m:] > first) & (slot[m:] < first + m - 1)).all()
    assert len(np.unique(h[m:] & LOW24)) > victims // 2
    if two_key:
        assert {I32_MIN, -1, 0, I32_MAX} <= set(g.cols[0].tolist()) and (g.cols[0] < 0).any() and len(np.unique(g.cols[0])) > m // 2
    assert 0.3 < (g.cols[-1] < 0).mean() < 0.7                        # keys of both signs, all over the domain


@pytest.mark.parametrize("m", [100, 3 * 512, 60_000])
def test_one_partition_has_its_structure(m):
    g = A.one_partition(m)
    h = g.hash()
    assert len(g) == m and len(np.unique(g.cols[0])) == m
    p = g.info["partition"]
    for nparts in (8, 64, 512, 1024, 4096, 8192, 1 << 14):
        assert (A.partition_of(h, nparts) == (p & (nparts - 1))).all()
    for shift in (47,):                                               # first level of the two-level form at 8192 bins: bits 47..52
        assert len(np.unique((h >> np.uint64(shift)) & np.uint64(63))) == 1
    if m >= 1000:                                                      # the other bits are random: global slots and LDS slots spread
        assert len(np.unique(h & np.uint64(0xFFF))) > min(m, 4096) // 2 and len(np.unique(g.lds() & np.uint32(511))) > 400
    T = A.bulk_T(1, 6)
    assert m == 100 or m > A.closes_at(T)                              # (3 T and 60 000 overflow the table of their partition)


@pytest.mark.parametrize("m,partition", [(31, 5), (32, 5), (33, 5), (100, 5), (100, None), (A.sink_slots(1, 6) // 2 + 50, None)])
def test_one_lds_slot_has_its_structure(m, partition):
    g = A.one_lds_slot(m, partition=partition)
    assert len(g) == m and len(np.unique(g.cols[0])) == m
    low = g.lds() & np.uint32((1 << 13) - 1)
    assert (low == g.info["slot"]).all()
    for T in (128, 256, 512, 1024, 4096, 8192):                        # one slot in every LDS table
        assert len(np.unique(g.lds() & np.uint32(T - 1))) == 1
    if partition is not None:
        assert (A.partition_of(g.hash()) == partition).all()
        others = A.one_partition(2000, p=partition)
        assert (A.partition_of(others.hash()) == partition).all() and not np.isin(others.cols[0], g.cols[0]).any()
    else:
        assert len(np.unique(A.partition_of(g.hash(), 1024))) > m // 2
    assert len(np.unique(g.hash() & np.uint64(0xFFF))) > m // 2        # the global slots are spread: only the LDS slot is shared
    assert m > A.SINK_PROBE_WINDOW


@pytest.mark.parametrize("m,n", [(31, 200_000), (32, 200_000), (33, 200_000), (100, 200_000), (33, 4_300_000)])
def test_probe_window_rows_fill_the_window_before_the_table_closes(m, n):
    """the insert rule of the build tables replayed over the row order of probe_window_rows: the same-slot keys meet in the EMPTY table
    of their partition's build workgroup, min(m, 32) of them enter at the places 0 .. 31 of one chain, every further one leaves with
    32 probes made (not by the closing rule), and the table closes only later, over the ordinary keys"""
    rows = A.probe_window_rows(m, n)
    g, lead = rows.groups, rows.groups.info["lead"]
    T, W = A.bulk_T(1, 6), A.PROBE_WINDOW
    assert rows.n == n and len(g) == m + 2000 and (A.partition_of(g.hash()) == 1234).all()
    assert np.bincount(rows.src, minlength=len(g)).min() >= 50
    # the lead: one scatter workgroup's whole range in either form, at least one build step, nothing but the same-slot keys, all of them
    assert lead >= A.bulk1_scatter_range(n) and lead >= A.BUILD_THREADS and (n < (4 << 20) or lead >= A.bulk2_scatter_range(n))
    assert (rows.src[:lead] < m).all() and set(rows.src[:A.BUILD_THREADS].tolist()) == set(range(m)) and (rows.src[lead:] >= m).any()
    slot = (g.lds() & np.uint32(T - 1)).astype(np.int64)
    assert len(set(slot[:m].tolist())) == 1 and m < A.closes_at(T)
    # keys in the order of their first row; any order INSIDE the lead gives the same picture, since only same-slot keys are in it
    _, first = np.unique(rows.src, return_index=True)
    order = np.argsort(first)
    assert sorted(order[:m].tolist()) == list(range(m))
    out = A.replay_lds_inserts(g.lds()[order].astype(np.int64), T)
    assert out[: min(m, W)] == [("in", j) for j in range(min(m, W))]
    assert out[W:m] == [("window", W)] * max(0, m - W)
    assert (("in", W - 1) in out[:m]) == (m >= W)                      # the key a lookup of exactly 32 probes still finds
    rest = out[m:]
    assert sum(o[0] == "in" for o in rest) == A.closes_at(T) - min(m, W) and sum(o[0] == "closed" for o in rest) > 1000
    for seed in range(3):                                              # another order inside the lead: the same counts
        perm = np.concatenate([np.random.default_rng(seed).permutation(order[:m]), order[m:]])
        o2 = A.replay_lds_inserts(g.lds()[perm].astype(np.int64), T)
        assert [o[0] for o in o2[:m]] == ["in"] * min(m, W) + ["window"] * max(0, m - W)


def test_edge_tables_hold_every_listed_value():
    for t in ("i64", "dec64"):
        e = A.edge_table(t)
        for v in (I64_MIN, I64_MIN + 1, -2 ** 32 - 1, -2 ** 32, -2 ** 31 - 1, -2 ** 31, -1, 0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1,
                  I64_MAX - 1, I64_MAX):
            assert v in e, (t, v)
        triples = [(x, x + 2 ** 32, x << 32) for x in A.HALF_X]
        assert len(triples) >= 3
        for x, y, z in triples:
            assert x in e and y in e and z in e and (x ^ y) & 0xFFFFFFFF == 0 and x >> 32 != y >> 32 and z & 0xFFFFFFFF == 0 and z >> 32 == x
    for v in (I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX):
        assert v in A.edge_table("i32") and v in A.edge_table("date")
    assert civil_days(1, 1, 1) in A.edge_table("date") and civil_days(9999, 12, 31) in A.edge_table("date")
    assert A.edge_table("code8") == [0, 1, 127, 128, 254, 255]
    for t in ("i64", "dec64", "i32", "date", "code8"):
        e = A.edge_table(t)
        g = A.single_key(t, e)
        assert len(set(e)) == len(e) and g.cols[0].dtype == A._DT[t] and g.cols[0].astype(object).tolist() == e    # each value fits its type
        assert len(np.unique(g.hash())) == len(e)


@pytest.mark.parametrize("types", A.TUPLE_TYPES, ids=["-".join(t) for t in A.TUPLE_TYPES])
def test_tuple_edges_hold_every_listed_pattern(types):
    g = A.tuple_edges(types)
    nk = len(types)
    tuples = g.tuples()
    have = set(tuples)
    for c, t in enumerate(types):
        assert g.cols[c].dtype == A._DT[t]
    # pairs that differ in exactly one column, for every position; for 8-byte columns a pair that differs in the high half only
    for c in range(nk):
        pairs = [(t, u) for t, u, cc in g.info["one_col"] if cc == c]
        assert len(pairs) >= 5
        for t, u in pairs:
            assert t in have and u in have and [i for i in range(nk) if t[i] != u[i]] == [c]
        if types[c] == "i64":
            assert any((t[c] ^ u[c]) & 0xFFFFFFFF == 0 for t, u in pairs)
    # transposed tuples
    assert len(g.info["transposed"]) >= nk * (nk - 1) // 2
    for t, u in g.info["transposed"]:
        d = [i for i in range(nk) if t[i] != u[i]]
        assert t in have and u in have and len(d) == 2 and (t[d[0]], t[d[1]]) == (u[d[1]], u[d[0]])
    assert any(-1 in t for t, _ in g.info["transposed"]) or "code8" in types
    # all NULL patterns over the same values, 0 among them, every NULL pattern in rows of different payload
    zero = tuple([0] * nk)
    assert zero in g.info["null_base"] and zero in have
    for base in g.info["null_base"]:
        for mask in range(1 << nk):
            want = tuple(None if (mask >> c) & 1 else base[c] for c in range(nk))
            at = [i for i, t in enumerate(tuples) if t == want]
            assert len(at) >= (3 if mask else 1), (want,)
            for c in range(nk):
                if (mask >> c) & 1:
                    under = {int(g.cols[c][i]) for i in at}
                    assert len(under) >= 2 and A._lowest(types[c]) in under and A._minus_one(types[c]) in under, (want, c, under)
    assert len({int(m) for m in g.nullmask().tolist()}) == 1 << nk
    # with validity on fewer columns the bytes under the former NULLs are values: more groups, never fewer
    assert len(set(g.keep_validity([0]).tuples())) > len(have) and len(set(g.keep_validity([]).tuples())) > len(have)


def test_rows_of_spreads_every_group():
    g = A.tuple_edges(("i64", "code8", "i32", "date"))
    for rows in (A.rows_of(g, 5000, dup=3), A.tiled(g, 20_011, dup=3)):
        assert rows.n in (5000, 20_011) and np.bincount(rows.src, minlength=len(g)).min() >= 3
        assert (np.diff(rows.src) != 1).mean() > 0.9                  # shuffled
        for c in range(4):
            v = rows.valid[c]
            assert np.array_equal(rows.cols[c][v], g.cols[c][rows.src][v]) and rows.cols[c].dtype == g.cols[c].dtype
            null = np.flatnonzero(~v)
            by_src = {}
            for i in null.tolist():
                by_src.setdefault(int(rows.src[i]), set()).add(int(rows.cols[c][i]))
            assert all(len(s) >= 2 for s in by_src.values())           # the bytes under a NULL differ between the rows of one group
        assert (~rows.arg_valid).any() and set(rows.kind.tolist()) == set(range(len(A.VALUES)))
        ref = A.group_reference(rows.cols, rows.valid, rows.kind, rows.arg_valid)
        t = g.tuples()
        assert ref[t[0]][3] == ref[t[0]][4] == I64_MIN and ref[t[1]][3] == ref[t[1]][4] == I64_MAX and ref[t[3]][2] == 0 and ref[t[3]][5] >= 3
        assert ref[t[2]][3] == I64_MIN and ref[t[2]][4] == I64_MAX


# ------------------------------------------------------------------ the reference
def oracle_type(t, col):
    """the oracle's DATE hashes (year, month, day): days outside the calendar go in as INT32, DEC64 as its unscaled INT64 — the same equality"""
    if t == "date":
        return O.OT_DATE if A.DATE_LO <= int(col.min()) and int(col.max()) <= A.DATE_HI else O.OT_INT32
    return {"i64": O.OT_INT64, "dec64": O.OT_INT64, "i32": O.OT_INT32, "code8": O.OT_CODE8}[t]


def oracle_groups(rows, valid, sel):
    """{key tuple: (first row, sum of kind, count of non-NULL arguments, rows)} by the oracle's GROUP BY; its argument is the INT32 index
    into VALUES (the oracle's integer sums take INT32)"""
    keys = [O.col(oracle_type(t, c), c, validity=bits(v), dictionary=CODES if t == "code8" else None) for t, c, v in zip(rows.types, rows.cols, valid)]
    kind32 = rows.kind.astype(np.int32)
    args = [O.col(O.OT_INT32, kind32, validity=bits(rows.arg_valid)), O.col(O.OT_INT32, kind32)]
    m = rows.n if sel is None else len(sel)
    ng, first, gk, gn, vals = O.groupby(keys, args, [(O.OA_SUM, 0), (O.OA_COUNT, 0), (O.OA_COUNT, 1)], None if sel is None else sel.astype(np.int64), m, rows.n + 8)
    out = {}
    for g in range(ng):
        key = tuple(None if gn[g][c] else int(gk[g][c]) for c in range(len(keys)))
        s, c, r = vals[3 * g], vals[3 * g + 1], vals[3 * g + 2]
        out[key] = (int(first[g]), None if s.kind == O.OV_NULL else s.h.value(), 0 if c.kind == O.OV_NULL else c.h.value(), r.h.value())
    assert len(out) == ng
    return out


def built_rows():
    """(name, Rows) of every builder at a few thousand rows"""
    out = [(f"edge_table({t})", A.rows_of(A.single_key(t, A.edge_table(t)), 3000, seed=5)) for t in ("i64", "dec64", "i32", "date", "code8")]
    out += [("tuple_edges(" + ",".join(ts) + ")", A.rows_of(A.tuple_edges(ts), 4000, seed=6)) for ts in A.TUPLE_TYPES]
    out += [("one_global_slot", A.rows_of(A.one_global_slot(300, 40), 3000)), ("one_global_slot/2", A.rows_of(A.one_global_slot(300, 40, two_key=True), 3000)),
            ("one_partition", A.rows_of(A.one_partition(1536), 5000)), ("one_lds_slot", A.rows_of(A.one_lds_slot(100), 3000)),
            ("one_lds_slot/p", A.rows_of(A.one_lds_slot(33, partition=9).concat(A.one_partition(500, p=9)), 3000))]
    return out


def test_group_reference_agrees_with_the_oracle_on_every_builder():
    for name, rows in built_rows():
        rng = np.random.default_rng(len(name))
        sel = np.flatnonzero(rng.random(rows.n) < 0.6)
        modes = [rows.valid, [None] * len(rows.types)] + ([[rows.valid[0]] + [None] * (len(rows.types) - 1)] if len(rows.types) > 1 else [])
        for valid in modes:
            for s in (None, sel):
                want = oracle_groups(rows, valid, s)
                got = A.group_reference(rows.cols, valid, rows.kind, rows.arg_valid, sel=s)
                assert set(got) == set(want), name
                for key, (first, _, cnt, _, _, nrows) in got.items():
                    assert (first, cnt, nrows) == (want[key][0], want[key][2], want[key][3]), (name, key)
                src_rows = np.arange(rows.n) if s is None else s
                ks = {}
                for key, r in zip(A.Groups(rows.types, rows.cols, valid).tuples(), range(rows.n)):
                    ks.setdefault(key, []).append(r)
                live = set(src_rows.tolist())
                for key, w in want.items():                            # the oracle's own sum, of the indices into VALUES
                    mine = [r for r in ks[key] if r in live and rows.arg_valid[r]]
                    assert w[1] == (sum(int(rows.kind[r]) for r in mine) if mine else None), (name, key)
                    assert got[key][1] == sum(A.VALUES[int(rows.kind[r])] for r in mine)
        # the promise of copies (src) gives the same groups, and row_base moves the first rows only
        a = A.group_reference(rows.cols, rows.valid, rows.kind, rows.arg_valid, sel=sel, row_base=1000)
        b = A.group_reference(rows.cols, rows.valid, rows.kind, rows.arg_valid, sel=sel, src=rows.src)
        assert a == {k: (v[0] + 1000,) + v[1:] for k, v in b.items()}
    with pytest.raises(AssertionError):                                # a promise that does not hold is noticed
        r = A.rows_of(A.tuple_edges(("i32", "i64")), 3000)
        A.group_reference(r.cols, [None, None], r.kind, r.arg_valid, src=r.src)


def test_group_reference_against_a_double_loop():
    for ts in A.TUPLE_TYPES + [("i64",), ("code8",)]:
        g = A.tuple_edges(ts) if len(ts) > 1 else A.single_key(ts[0], A.edge_table(ts[0]) * 3)
        rng = np.random.default_rng(len(ts))
        pick = rng.choice(len(g), min(len(g), 60), replace=False)
        sub = A.Groups(g.types, [c[pick] for c in g.cols], [v[pick] for v in g.valid])
        rows = A.rows_of(sub, 200, dup=1)
        sel = np.flatnonzero(rng.random(200) < 0.7)
        for valid in (rows.valid, [None] * len(ts)):
            for s in (None, sel):
                want = A.loop_reference(rows.cols, valid, rows.kind, rows.arg_valid, s, 17)
                assert A.group_reference(rows.cols, valid, rows.kind, rows.arg_valid, s, 17) == want
                assert sum(v[5] for v in want.values()) == (200 if s is None else len(s)) and len(want) > 5
    # by hand: NULL groups whatever lies under it, the mask tells (NULL, 0) from (0, NULL) from (0, 0)
    k0, k1 = np.array([0, 7, 0, -5, 0, 0], np.int32), np.array([0, 0, 9, 0, I64_MIN, 0], np.int64)
    v0, v1 = np.array([1, 0, 1, 0, 1, 0], bool), np.array([1, 1, 0, 1, 0, 0], bool)
    kind, ok = np.array([3, 4, 4, 7, 0, 6]), np.array([1, 1, 1, 1, 0, 1], bool)
    assert A.group_reference([k0, k1], [v0, v1], kind, ok) == {
        (0, 0): (0, 0, 1, 0, 0, 1), (None, 0): (1, 1 + 12_345, 2, 1, 12_345, 2), (0, None): (2, 1, 1, 1, 1, 2), (None, None): (5, I64_MAX, 1, I64_MAX, I64_MAX, 1)}
