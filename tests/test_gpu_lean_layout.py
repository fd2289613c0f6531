"""GPU tests of the row layout of the lean narrow lowcard_chain scan (ph_scan_plan_variant == "narrow32_lean"): a lane owns
four groups of four consecutive rows of a 4096-row tile, 256 rows apart (row = tile + 1024 wave + 256 group + 4 lane + k), so that every
load instruction of a wave reads consecutive bytes. What can go wrong is which row a code belongs to: sums per slot, counts, first row ids
and the row-range mask at the edges of a group, of a wave's 1024 rows and of a tile, and the loads of a last tile that reaches past the
columns' padding. Every case is checked against exact Python / numpy integers (the helpers of test_gpu_narrow_scan.py), asserts the
variant, and is compared bit for bit with the same case under PH_SCAN_LEAN=0 in a child process (the kernel from before the lean
instance, a lane's 16 rows consecutive; the switch is read once per process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from plan_amd import hip  # noqa: E402
from test_gpu_lean_scan import D0, TILE, ranges  # noqa: E402
from test_gpu_narrow_scan import I32_MAX, I32_MIN, lc_plan, lc_result, lc_table, lc_want  # noqa: E402

pytestmark = pytest.mark.gpu

N = 5 * TILE + 7
GROUP, WAVE = 256, 1024   # rows between a lane's groups, rows of a wave
PASSING = (D0, D0 + 100)  # dates of passing rows are D0 + i % 7; FAIL_DATE lies outside
FAIL_DATE = D0 + 500


def run_lowcard(ctx, c, intervals, row_ranges, grids):
    """[variant, [[grid, lo, hi, b, e, groups]...]]: every (interval, grid, range) of one table, each checked against numpy"""
    t = lc_table(ctx, c)
    out, variant = [], None
    for lo, hi in intervals:
        pl = lc_plan(ctx, t, lo, hi, c["ptype"])
        assert pl.kind == "lowcard_chain"
        variant = pl.variant
        for grid in grids:   # PH_SCAN_GRID is read at every run
            if grid is None:
                os.environ.pop("PH_SCAN_GRID", None)
            else:
                os.environ["PH_SCAN_GRID"] = grid
            for b, e_ in row_ranges:
                pl.run(b, e_)
                got = lc_result(pl.fetch())
                want = lc_want(c, lo, hi, b, e_)
                assert [g[1:] for g in got] == [(w[1], w[2], w[3]) for w in want], (grid, lo, hi, b, e_)
                assert [g[0] for g in got] == [w[0] for w in want], (grid, lo, hi, b, e_)
                out.append([grid, lo, hi, b, e_, got])
        os.environ.pop("PH_SCAN_GRID", None)
        pl.free()
    t.free()
    return [variant, out]


def base_columns(n, seed, q=(3, 258), e=(90_000, 10_000_000), d=(2, 257), t=(0, 8)):
    """Q1's code widths (p 2, q 1, e 4, d 1, t 1); every row in slot (0, 0); every column's min in row 0 and max in row 1"""
    rng = np.random.default_rng(seed)
    i = np.arange(n)

    def col(lo, hi):
        v = rng.integers(lo, hi, n, endpoint=True, dtype=np.int64)
        v[0], v[1] = lo, hi
        return v

    p = D0 + i % 7
    p[0], p[1] = D0, D0 + 600   # two-byte codes; the row of the maximum fails PASSING
    c = dict(p=p.astype(np.int32), q=col(*q).astype(np.int32), e=col(*e), d=col(*d), t=col(*t), k0=np.zeros(n, np.uint8),
             k1=np.zeros(n, np.uint8), ptype=hip.PH_DATE)
    assert int(np.abs(c["e"]).max()) * max(abs(100 - int(c["d"].min())), abs(100 - int(c["d"].max()))) <= I32_MAX   # the 32-bit form
    return c


# ---------------------------------------------------------------- every row in its own place: six slots, both signs
LONE_SLOT, LONE_ROW = (2, 1), 5000   # a slot used by a single row
LAST_SLOT = (2, 0)                   # a slot used only in the last, partial tile


def six_slot_columns(n=N, seed=12):
    c = base_columns(n, seed, q=(-300, -45), e=(-5_000_000, 5_000_000), d=(-55, 200), t=(-200, 55))
    rng = np.random.default_rng(seed + 1)
    c["k0"], c["k1"] = rng.integers(0, 2, n).astype(np.uint8), rng.integers(0, 2, n).astype(np.uint8)
    if n > LONE_ROW:
        c["k0"][LONE_ROW], c["k1"][LONE_ROW] = LONE_SLOT
    c["k0"][[n - 3, n - 1]], c["k1"][[n - 3, n - 1]] = LAST_SLOT
    return c


def edge_ranges():
    """row ranges that begin or end one row before, at and after a lane's group of 4, a group stride of 256, a wave's 1024 rows and a tile;
    a row_begin that is no multiple of 16 moves every tile (tiles start at row_begin rounded down to 16)"""
    cuts = [4, GROUP, WAVE, 3 * WAVE + 3 * GROUP, TILE, TILE + WAVE + GROUP]
    out = []
    for c in cuts:
        out += [(0, c - 1), (0, c), (0, c + 1), (c - 1, N), (c, N), (c + 1, N), (c - 1, c + 1)]
    return out + [(17, 17 + GROUP), (GROUP - 3, WAVE + 5), (WAVE + 250, WAVE + 2 * GROUP + 2), (TILE - 1, TILE + GROUP + 1)]


def run_six_slots(ctx):
    return run_lowcard(ctx, six_slot_columns(), [(I32_MIN, I32_MAX), PASSING], ranges(N) + edge_ranges(), ("2", None))


# ---------------------------------------------------------------- first row id
THIRD_TILE = (1, 0), 2 * TILE + WAVE + GROUP + 37 * 4 + 2    # a slot whose first row lies in the third tile (the third of its lane at PH_SCAN_GRID=1)
AFTER_FAIL = (1, 1), 100, 102                               # a slot whose first row fails the predicate; the next one, in the same group of 4, passes
NEXT_GROUP = (0, 1), 2 * WAVE + 9 * 4 + 1                   # a failing row; the same lane's next group (+ 256) and the next wave (+ 1024) pass
BELOW_BEGIN = (2, 0), 1200 * 4 + 1, 1200 * 4 + 3            # a slot with two rows in one group of 4: row_begin between them
FAIL_TILES = (2, 1), 160 + 2, 3 * TILE + 160 + 2            # the failing row and the passing one at the same place of a lane, three tiles apart


def first_row_columns():
    c = base_columns(N, 14)

    def put(slot, rows):
        c["k0"][rows], c["k1"][rows] = slot

    put(THIRD_TILE[0], [THIRD_TILE[1], THIRD_TILE[1] + 7, 3 * TILE + 5, 4 * TILE + WAVE + GROUP + 37 * 4 + 2])
    put(AFTER_FAIL[0], [AFTER_FAIL[1], AFTER_FAIL[2], 2 * TILE + 1])
    put(NEXT_GROUP[0], [NEXT_GROUP[1], NEXT_GROUP[1] + WAVE, NEXT_GROUP[1] + GROUP])
    put(BELOW_BEGIN[0], [BELOW_BEGIN[1], BELOW_BEGIN[2], 4 * TILE + 1])
    put(FAIL_TILES[0], [FAIL_TILES[1], FAIL_TILES[2], FAIL_TILES[2] + TILE])
    c["p"][[AFTER_FAIL[1], NEXT_GROUP[1], FAIL_TILES[1]]] = FAIL_DATE
    return c


def first_row_ranges():
    b = BELOW_BEGIN
    return [(0, N), (1, N - 1), (b[1], N), (b[1] + 1, N), (b[1] + 2, b[2] + 1), (b[2], N), (b[2] + 1, N), (AFTER_FAIL[1] + 1, N), (2 * TILE, N)]


def run_first_rows(ctx):
    return run_lowcard(ctx, first_row_columns(), [PASSING, (I32_MIN, I32_MAX)], first_row_ranges(), ("1", "2", None))


# ---------------------------------------------------------------- a last tile that reaches past the columns' padding
PAD = 8192   # columns are padded to a multiple of 8192 rows


def run_pad_edge(ctx):
    """a table of exactly 8192 rows: with row_begin = 16 the second tile is rows [4112, 8208), past the padded columns; one of 8192 + 5 rows"""
    out = {}
    for n in (PAD, PAD + 5):
        c = six_slot_columns(n, 20 + n % 7)
        out[str(n)] = run_lowcard(ctx, c, [(I32_MIN, I32_MAX)], [(0, n), (4, n), (16, n), (16, n - 1), (TILE - 1, n), (n - 5, n), (n - 1, n)], ("1", "2", None))
    return out


# ---------------------------------------------------------------- fixtures
def run_all(ctx):
    return {"six_slots": run_six_slots(ctx), "first_rows": run_first_rows(ctx), "pad_edge": run_pad_edge(ctx)}


@pytest.fixture(scope="module")
def ctx():
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lean(ctx):
    return json.loads(json.dumps(run_all(ctx)))


@pytest.fixture(scope="module")
def parent():
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"layout_child_{os.getpid()}.json")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, PH_SCAN_LEAN="0"), check=True, timeout=600)
    with open(out) as f:
        res = json.load(f)
    os.remove(out)
    return res


def test_rows_at_group_wave_and_tile_edges(lean, parent):
    """six slots, values of both signs, row ranges cut around every stride of the layout: sums, counts and first row ids"""
    assert lean["six_slots"][0] == "narrow32_lean" and parent["six_slots"][0] == "narrow32"
    assert lean["six_slots"][1] == parent["six_slots"][1]
    whole = [r for r in lean["six_slots"][1] if r[1] == I32_MIN and r[3:5] == [0, N]]
    assert whole and all(len(r[5]) == 6 for r in whole)
    assert all([g for g in r[5] if tuple(g[1]) == LONE_SLOT][0][3] == 1 for r in whole)
    assert all([g for g in r[5] if tuple(g[1]) == LAST_SLOT][0][0] == N - 3 for r in whole)
    assert all(g[2][0] < 0 for r in whole for g in r[5])   # Σq is negative in every slot


def test_first_row_ids(lean, parent):
    """the first row id of a slot is its first passing row inside the range: not a row that fails the predicate, not a row below row_begin
    in the same group of 4, not a later row that the lane meets in an earlier group; a first row in a lane's third tile is found"""
    assert lean["first_rows"][0] == "narrow32_lean" and parent["first_rows"][0] == "narrow32"
    assert lean["first_rows"][1] == parent["first_rows"][1]

    def first(grid, lo, b, e_, slot):
        (r,) = [r for r in lean["first_rows"][1] if r[0] == grid and r[1] == lo and r[3:5] == [b, e_]]
        return [g[0] for g in r[5] if tuple(g[1]) == slot]

    for grid in ("1", "2", None):
        assert first(grid, PASSING[0], 0, N, THIRD_TILE[0]) == [THIRD_TILE[1]]
        assert first(grid, PASSING[0], 0, N, AFTER_FAIL[0]) == [AFTER_FAIL[2]]
        assert first(grid, I32_MIN, 0, N, AFTER_FAIL[0]) == [AFTER_FAIL[1]]
        assert first(grid, PASSING[0], 0, N, NEXT_GROUP[0]) == [NEXT_GROUP[1] + GROUP]
        assert first(grid, I32_MIN, 0, N, NEXT_GROUP[0]) == [NEXT_GROUP[1]]
        assert first(grid, PASSING[0], 0, N, FAIL_TILES[0]) == [FAIL_TILES[2]]
        assert first(grid, I32_MIN, 0, N, FAIL_TILES[0]) == [FAIL_TILES[1]]
        assert first(grid, PASSING[0], BELOW_BEGIN[1], N, BELOW_BEGIN[0]) == [BELOW_BEGIN[1]]
        assert first(grid, PASSING[0], BELOW_BEGIN[1] + 1, N, BELOW_BEGIN[0]) == [BELOW_BEGIN[2]]
        assert first(grid, PASSING[0], BELOW_BEGIN[2] + 1, N, BELOW_BEGIN[0]) == [4 * TILE + 1]


def test_last_tile_past_the_padding(lean, parent):
    for n in (str(PAD), str(PAD + 5)):
        assert lean["pad_edge"][n][0] == "narrow32_lean" and parent["pad_edge"][n][0] == "narrow32"
        assert lean["pad_edge"][n][1] == parent["pad_edge"][n][1]
        assert any(r[3] == 16 and len(r[5]) >= 5 for r in lean["pad_edge"][n][1])


if __name__ == "__main__":   # the parent fixture's child: every case under another environment
    _ctx = hip.Ctx(0)
    _res = run_all(_ctx)
    _ctx.close()
    with open(sys.argv[1], "w") as _f:
        json.dump(_res, _f)
