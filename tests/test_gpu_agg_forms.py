"""Which form ph_agg_sink takes, as ph_agg_sink_kind reports it: the cases of test_agg_forms_reference.py — one on each side of every
threshold of the choice, every switch that turns a form off — run on the device at those sizes (the thresholds are row counts, so
these are the smallest inputs that reach the forms), for one BIGINT key with SUM + COUNT(*). Each case sinks, checks the kind and
compares the groups in first-seen order, their first rows, 128-bit sums and counts with numpy, exactly. The rows are prefixes of one
array of 4 Mi rows over 65 536 distinct keys, so the answer of a row count is computed once.

A hint below the number of groups is not a wrong result but a bulk build that hands over: at 4 Mi rows a hint of 2 868 sizes the
second form's 16 partitions for 2 868 groups, their LDS tables (16 x 2048 entries) cannot take 65 536, the attempt is void and the
first form sinks the rows ("bulk1" — against "spec" for a hint of 2 867, where no bulk build is tried). The same threshold over 2 048
distinct keys, which fit, stays "bulk2_spec"."""
import numpy as np
import pytest

from plan_amd import hip

pytestmark = pytest.mark.gpu

MI = 1 << 20
SWITCHES = ("PH_AGG_JIT", "PH_AGG_NO_BULK", "PH_AGG_BULK_V1", "PH_AGG_BULK_ONE_LEVEL")
AGGS = [(hip.PH_A_SUM, 0), (hip.PH_A_COUNT_STAR, -1)]
ROW_BASE = 1000

CASES = [
    # id, rows, hint, environment, distinct keys, kind
    ("rows_below_bulk", 65_535, 32_768, {}, 65_536, "generic"),
    ("rows_at_bulk", 65_536, 32_768, {}, 65_536, "bulk1"),
    ("hint_below_bulk_min", 65_536, 32_767, {}, 65_536, "generic"),
    ("rows_below_second", 4 * MI - 1, 65_536, {}, 65_536, "bulk1"),
    ("rows_at_second", 4 * MI, 65_536, {}, 65_536, "bulk2_spec"),
    ("hint_below_lowered_bulk_min", 4 * MI, 2_867, {}, 65_536, "spec"),
    ("hint_at_lowered_bulk_min_outgrown", 4 * MI, 2_868, {}, 65_536, "bulk1"),
    ("hint_at_lowered_bulk_min", 4 * MI, 2_868, {}, 2_048, "bulk2_spec"),
    ("hint_one_level", 4 * MI, 262_144, {}, 65_536, "bulk2_spec"),
    ("hint_two_level", 4 * MI, 262_145, {}, 65_536, "two_level"),
    ("hint_8192_bins", 4 * MI, 4_194_304, {}, 65_536, "two_level"),
    ("hint_above_8192_bins", 4 * MI, 4_194_305, {}, 65_536, "bulk1"),          # (about 1 GB of table: the one case of its size)
    ("rows_below_spec", MI - 1, 1024, {}, 65_536, "generic"),
    ("rows_at_spec", MI, 1024, {}, 65_536, "spec"),
    ("jit_off_incremental", MI, 1024, {"PH_AGG_JIT": "0"}, 65_536, "generic"),
    ("jit_off_second_form", 4 * MI, 65_536, {"PH_AGG_JIT": "0"}, 65_536, "bulk2"),
    ("one_level_only", 4 * MI, 262_145, {"PH_AGG_BULK_ONE_LEVEL": "1"}, 65_536, "bulk1"),
    ("no_bulk", 4 * MI, 65_536, {"PH_AGG_NO_BULK": "1"}, 65_536, "spec"),
    ("first_form_only", 4 * MI, 65_536, {"PH_AGG_BULK_V1": "1"}, 65_536, "bulk1"),
]


class Rows:
    """4 Mi rows over 65 536 distinct keys (a prefix has the groups it has), their values, and per (row count, distinct keys) the numpy
    answer: keys in first-seen order, first rows, sums, counts"""

    def __init__(self):
        rng = np.random.default_rng(20250)
        self.key = rng.integers(0, 65_536, 4 * MI).astype(np.int64) * 1_000_003 - (1 << 40)
        self.val = rng.integers(-10**6, 10**6, 4 * MI).astype(np.int64)
        self.answers = {}

    def keys(self, n, distinct):
        k = self.key[:n]
        return k if distinct == 65_536 else ((k + (1 << 40)) // 1_000_003 % distinct) * 1_000_003 - (1 << 40)

    def answer(self, n, distinct):
        if (n, distinct) not in self.answers:
            k, v = self.keys(n, distinct), self.val[:n]
            order = np.argsort(k, kind="stable")
            starts = np.flatnonzero(np.r_[True, k[order][1:] != k[order][:-1]])
            first = order[starts]                                   # (stable: the first row of every run is the group's first)
            seen = np.argsort(first)
            sums = np.add.reduceat(v[order], starts)                # exact: |sum| < 4 Mi x 10^6 < 2^63
            counts = np.diff(np.r_[starts, n])
            self.answers[(n, distinct)] = (k[first][seen], first[seen], sums[seen], counts[seen])
        return self.answers[(n, distinct)]


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def rows():
    return Rows()


def sink_and_check(ctx, rows, n, hint, distinct, kind=None):
    """one sink of the first n rows into a table created for `hint` groups: the kind it reports (when the library says), the groups exactly"""
    keys, first, sums, counts = rows.answer(n, distinct)
    dk, dv = hip.DevColumn(ctx, hip.PH_I64, rows.keys(n, distinct)), hip.DevColumn(ctx, hip.PH_I64, rows.val[:n])
    agg = hip.Agg(ctx, [hip.PH_I64], AGGS, hint)
    try:
        assert kind is None or agg.sink_kind == ""
        agg.sink([dk], [dv], None, n, row_base=ROW_BASE)
        assert kind is None or agg.sink_kind == kind, (agg.sink_kind, kind)
        r = agg.finalize(python_ints=False)
        assert r["ngroups"] == len(keys)
        assert np.array_equal(r["keys"][:, 0], keys) and np.array_equal(r["first_row"], first + ROW_BASE)
        assert np.array_equal(r["sum_lo"][:, 0].astype(np.int64), sums)
        assert np.array_equal(r["sum_hi"][:, 0], np.where(sums < 0, -1, 0))
        assert np.array_equal(r["count"][:, 1], counts)
    finally:
        agg.free(); dk.free(); dv.free()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_sink_form(ctx, monkeypatch, rows, case):
    name, n, hint, env, distinct, kind = case
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    # what the rule chooses is what ran, except where the rows outgrow the hint
    assert hip.agg_sink_choice(n, hint, nkeys=1, naggs=2, used_args=1)[0] == ("bulk2_spec" if name.endswith("outgrown") else kind)
    sink_and_check(ctx, rows, n, hint, distinct, kind)


def test_second_sink_and_sorted_sink_report_their_own_kind(ctx, monkeypatch, rows):
    """the kind is that of the MOST RECENT rows: an incremental sink into a bulk-built table, and the streaming aggregate"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    n = 65_536
    dk, dv = hip.DevColumn(ctx, hip.PH_I64, rows.keys(n, 65_536)), hip.DevColumn(ctx, hip.PH_I64, rows.val[:n])
    agg = hip.Agg(ctx, [hip.PH_I64], AGGS, 32_768)
    agg.sink([dk], [dv], None, n)
    assert agg.sink_kind == "bulk1"
    agg.sink([dk], [dv], None, 0, row_base=n)            # no rows: nothing sank them
    assert agg.sink_kind == "bulk1"
    agg.sink([dk], [dv], None, n, row_base=n)
    assert agg.sink_kind == "generic"
    keys, first, sums, counts = rows.answer(n, 65_536)
    r = agg.finalize(python_ints=False)
    assert np.array_equal(r["keys"][:, 0], keys) and np.array_equal(r["first_row"], first)
    assert np.array_equal(r["sum_lo"][:, 0].astype(np.int64), 2 * sums) and np.array_equal(r["count"][:, 1], 2 * counts)
    agg.free(); dk.free(); dv.free()
    ks = np.sort(rows.keys(n, 65_536))
    dk, dv = hip.DevColumn(ctx, hip.PH_I64, ks), hip.DevColumn(ctx, hip.PH_I64, rows.val[:n])
    agg = hip.Agg(ctx, [hip.PH_I64], AGGS, 32_768)
    assert agg.sink_sorted([dk], [dv], n)
    assert agg.sink_kind == "sorted"
    assert agg.group_count() == len(keys)
    agg.free(); dk.free(); dv.free()
