"""The sink form ph_agg_sink chooses (plan_amd/csrc/agg_forms.h, DESIGN.md "sink forms") through ph_agg_sink_choice, without a
device: one case on each side of every threshold of the rule for one BIGINT key with SUM + COUNT(*), every switch that turns a form
off, and the scatter shapes the sizing can yield. The sizes behind the thresholds, for that shape:
  * an entry of a bulk build's LDS table is 4 + 8 keys + 8 + 20 aggregates = 60 bytes, so the largest power-of-two table within
    120 KiB has T = 2048 entries (2048 x 60 = 122 880 = 120 KiB exactly) and a bin is meant to hold T / 4 = 512 groups;
  * an entry of the specialised incremental kernel's table is 12 + 8 keys + 8 aggregates = 36 bytes (no aggregate counts its own
    inputs), so the largest table within 144 KiB has 4096 entries (4096 x 36 = 147 456 = 144 KiB exactly)."""
import pytest

from plan_amd import hip

MI = 1 << 20
SWITCHES = ("PH_AGG_JIT", "PH_AGG_NO_BULK", "PH_AGG_BULK_V1", "PH_AGG_BULK_ONE_LEVEL")


def choice(monkeypatch, rows, hint, env=None, **shape):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    shape = {"nkeys": 1, "naggs": 2, "used_args": 1, **shape}
    return hip.agg_sink_choice(rows, hint, **shape)


THRESHOLDS = [
    # id, rows, hint, kind
    # a bulk build is tried from 65 536 rows
    ("rows_below_bulk", 65_535, 32_768, "generic"),
    ("rows_at_bulk", 65_536, 32_768, "bulk1"),
    # ... for a hint of at least bulk_min = 32 768
    ("hint_below_bulk_min", 65_536, 32_767, "generic"),
    ("hint_at_bulk_min", 65_536, 32_768, "bulk1"),
    # the second form from 4 Mi rows
    ("rows_below_second", 4 * MI - 1, 65_536, "bulk1"),
    ("rows_at_second", 4 * MI, 65_536, "bulk2_spec"),
    # from 4 Mi rows bulk_min drops to 70 % of the largest 144 KiB table of the incremental kernel, plus one:
    # 4096 entries x 7 / 10 = 2867 (integer division), + 1 = 2868
    ("hint_below_lowered_bulk_min", 4 * MI, 2_867, "spec"),
    ("hint_at_lowered_bulk_min", 4 * MI, 2_868, "bulk2_spec"),
    # bins = the power of two (from 16) that reaches ceil(hint / 512): 512 bins hold 512 x 512 = 262 144 groups, one more takes 1024
    # bins, and more than 512 bins are built on two levels
    ("hint_one_level", 4 * MI, 262_144, "bulk2_spec"),
    ("hint_two_level", 4 * MI, 262_145, "two_level"),
    # 8192 bins hold 8192 x 512 = 4 194 304 groups; one more would take 16 384 bins: back to the first form
    ("hint_8192_bins", 4 * MI, 4_194_304, "two_level"),
    ("hint_above_8192_bins", 4 * MI, 4_194_305, "bulk1"),
    # the incremental kernel's specialised body from 2^20 rows
    ("rows_below_spec", MI - 1, 1024, "generic"),
    ("rows_at_spec", MI, 1024, "spec"),
    # the second form's row ids are 32 bits wide
    ("rows_below_2^31", (1 << 31) - 1, 65_536, "bulk2_spec"),
    ("rows_at_2^31", 1 << 31, 65_536, "bulk1"),
]


@pytest.mark.parametrize("rows,hint,kind", [pytest.param(*c[1:], id=c[0]) for c in THRESHOLDS])
def test_thresholds(monkeypatch, rows, hint, kind):
    assert choice(monkeypatch, rows, hint)[0] == kind


SWITCHED = [
    # id, rows, hint, environment, kind with it (the kind without it is the threshold case above)
    ("jit_off_incremental", MI, 1024, {"PH_AGG_JIT": "0"}, "generic"),
    ("jit_off_second_form", 4 * MI, 65_536, {"PH_AGG_JIT": "0"}, "bulk2"),
    ("jit_on", 4 * MI, 65_536, {"PH_AGG_JIT": "1"}, "bulk2_spec"),
    ("no_bulk_small", 65_536, 32_768, {"PH_AGG_NO_BULK": "1"}, "generic"),
    ("no_bulk_big", 4 * MI, 65_536, {"PH_AGG_NO_BULK": "1"}, "spec"),
    ("first_form_only", 4 * MI, 65_536, {"PH_AGG_BULK_V1": "1"}, "bulk1"),
    ("one_level_only_above_512_bins", 4 * MI, 262_145, {"PH_AGG_BULK_ONE_LEVEL": "1"}, "bulk1"),
    ("one_level_only_at_512_bins", 4 * MI, 262_144, {"PH_AGG_BULK_ONE_LEVEL": "1"}, "bulk2_spec"),
]


@pytest.mark.parametrize("rows,hint,env,kind", [pytest.param(*c[1:], id=c[0]) for c in SWITCHED])
def test_switches(monkeypatch, rows, hint, env, kind):
    assert choice(monkeypatch, rows, hint, env)[0] == kind


def test_only_a_first_sink_is_a_bulk_build(monkeypatch):
    assert choice(monkeypatch, 4 * MI, 65_536, rows_sunk=1)[0] == "spec"
    assert choice(monkeypatch, 65_536, 65_536, rows_sunk=1)[0] == "generic"


def test_more_arguments_than_the_partition_records_carry(monkeypatch):
    """the bulk builds carry up to four argument columns (BK_MAX_ARGS)"""
    assert choice(monkeypatch, 4 * MI, 65_536, naggs=5, used_args=4)[0] == "bulk2_spec"
    assert choice(monkeypatch, 4 * MI, 65_536, naggs=5, used_args=5)[0] == "spec"
    assert choice(monkeypatch, 65_536, 65_536, naggs=5, used_args=5)[0] == "generic"


def test_sizes_of_the_named_shape(monkeypatch):
    """the sizes the module docstring derives, and the sizing of one second-form case worked out by hand: 65 536 groups / 512 = 128
    partitions, 4 slices each (512 workgroups in all), row = 8 x (1 key + 1 argument) + 8 = 24 bytes, tables 3 x 128 x 4 = 1536 bytes,
    16 chunks of 256 rows: 1536 + 4096 x 24 = 99 840 bytes of LDS; 4 Mi rows / 512 = 8192 rows a workgroup = two chunks of 4096"""
    kind, s = choice(monkeypatch, 4 * MI, 65_536)
    assert kind == "bulk2_spec"
    assert (s["T"], s["nparts"], s["bins"], s["shift"], s["slices"]) == (2048, 128, 128, 40, 4)
    assert (s["tpb"], s["bu"], s["lds_scatter"], s["lds_build"], s["rows_per_wg"]) == (1024, 16, 99_840, 122_880, 8192)
    kind, s = choice(monkeypatch, 4 * MI, 262_145)          # 1024 bins = 2^10: 64 partitions by the top 6 bits first
    assert kind == "two_level" and (s["nparts"], s["bins"], s["shift"], s["slices"]) == (64, 1024, 44, 1)
    kind, s = choice(monkeypatch, 4 * MI - 1, 65_536)       # first form: at least 512 partitions from 4 Mi rows, 8 below
    assert kind == "bulk1" and (s["T"], s["nparts"]) == (2048, 128)
    assert choice(monkeypatch, 4 * MI, 4_194_305)[1]["nparts"] == 4096
    kind, s = choice(monkeypatch, 4 * MI, 2_867)            # the table that 2867 groups fill to 70 %: 4096 entries, past 64 KiB: 1024 threads
    assert kind == "spec" and (s["slots"], s["threads"]) == (4096, 1024)
    kind, s = choice(monkeypatch, MI, 175)                  # 32 KiB / 36 bytes: 512 entries (358 groups at 70 %), 512 threads
    assert kind == "spec" and (s["slots"], s["threads"]) == (512, 512)
    kind, s = choice(monkeypatch, MI - 1, 175)              # generic: 32 KiB / (12 + 8 + 2 x 12 = 44 bytes): 512 entries, 256 threads
    assert kind == "generic" and (s["slots"], s["threads"]) == (512, 256)


def test_scatter_shapes_the_sizing_yields(monkeypatch):
    """over every key count, used-argument count (the bulk builds carry up to four), with and without NULLs, 0..16 aggregates and every
    bin count of the second form (16 .. 8192, through the hint): the staged scatter runs 1024 threads with 16 or 4 chunks of 256 rows —
    the two instances bulk2_scatter_kernel has — and never passes the 124 KiB its workgroup may use"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    seen = set()
    for nkeys in range(1, 5):
        for naggs in range(0, 17):
            T = hip.agg_sink_choice(4 * MI, 1 << 22, nkeys=nkeys, naggs=naggs, used_args=0)[1]["T"]
            for used in range(0, min(naggs, 4) + 1):
                for nulls in (False, True):
                    for log_bins in range(4, 14):
                        hint = (1 << log_bins) * (T // 4)
                        kind, s = hip.agg_sink_choice(4 * MI, hint, nkeys=nkeys, naggs=naggs, used_args=used, any_nulls=nulls, need_cnt=nulls)
                        if kind in ("generic", "spec"):          # (a hint below the lowered bulk_min)
                            continue
                        assert kind == ("two_level" if log_bins > 9 else "bulk2_spec") and s["bins"] == 1 << log_bins, (nkeys, naggs, used, nulls, log_bins)
                        assert s["lds_scatter"] <= 124 * 1024
                        seen.add((s["tpb"], s["bu"]))
    assert seen == {(1024, 16), (1024, 4)}
