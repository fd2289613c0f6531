"""ORDER BY over VARCHAR keys on the device: ph_sort_rows with PH_STR keys.

The order restated from the reference: RadixScatterStringVector writes a NULL byte and an 11-byte
zero-padded prefix (inverted for DESC) into the key (sort_radix.go:728-805, sort_layout.go:55-66), and
rows whose prefixes tie are re-sorted by the whole string with bytes.Compare, times -1 for DESC
(sort_radix.go:180-230, CompareVal :898-933, common/string.go:37-41). That is bytewise lexicographic
order with unsigned bytes (a proper prefix first), NULLs first in both directions, DESC the exact
reverse. oracle_sort_rows has no VARCHAR case, so the order is restated here: a stable sort per key,
last key first, NULLs moved in front."""
import os
import subprocess
from decimal import ROUND_HALF_EVEN, Decimal

import numpy as np
import pytest

from plan_amd import tpchgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTER = os.path.join(ROOT, "plan_amd", "host_tester")

ALPHABET = np.array([0x00, 0x01, 0x41, 0x42, 0x7F, 0x80, 0xFE, 0xFF], dtype=np.uint8)
LENGTHS = (0, 1, 7, 8, 9, 10, 11, 12, 15, 16, 17, 24, 63, 64, 65, 80)


def py_order(rows, keys, desc):
    """rows (input order) sorted by keys: each key a list over row ids of None (NULL) or a comparable value"""
    order = list(rows)
    for vals, d in reversed(list(zip(keys, desc))):
        nulls = [r for r in order if vals[r] is None]
        rest = sorted((r for r in order if vals[r] is not None), key=lambda r: vals[r], reverse=d)
        order = nulls + rest
    return order


def gen_strings(n, rng):
    """strings over a small alphabet with 0x00, 0xFF and bytes >= 0x80: cut from a few 80-byte bases (so they are prefixes of one
    another and share their first 8, 11, 16 or 64 bytes), some with one byte changed right after such a shared prefix; empty
    strings and NULLs"""
    bases = [bytes(rng.choice(ALPHABET, 80)) for _ in range(4)]
    base = rng.integers(0, len(bases), n)
    cut = rng.choice(np.array(LENGTHS), n)
    rnd = rng.random(n) < 0.3
    cut[rnd] = rng.integers(0, 81, int(rnd.sum()))
    mutate = rng.random(n) < 0.4
    mpos = rng.choice(np.array([8, 9, 11, 12, 16, 17, 64, 65, 3]), n)
    mbyte = rng.choice(ALPHABET, n)
    null = rng.random(n) < 0.05
    out = []
    for i in range(n):
        if null[i]:
            out.append(None)
            continue
        s = bases[base[i]][:cut[i]]
        if mutate[i] and mpos[i] < len(s):
            s = s[:mpos[i]] + bytes([mbyte[i]]) + s[mpos[i] + 1:]
        out.append(s)
    return out


def cents(x):
    return int((Decimal(int(x)) / Decimal(10000)).quantize(Decimal("0.01"), rounding=ROUND_HALF_EVEN) * 100)


def run_sort(ctx, hip, cols, desc, sel, m):
    sd = None if sel is None else ctx.upload(np.asarray(sel, dtype=np.int32))
    out = hip.sort_rows(ctx, cols, desc, sd, m)
    got = ctx.download(out, np.int32, m).tolist() if m else []
    ctx.free(out)
    if sd is not None:
        ctx.free(sd)
    return got


@pytest.mark.gpu
def test_sort_rows_varchar_keys_match_bytes_compare():
    """PH_STR keys alone, twice, and first / in the middle / last among INTEGER, DECIMAL(scale 4), DATE and dictionary-code keys;
    ASC and DESC; with and without a selection; 1 row to 2 M rows"""
    from plan_amd import hip
    ctx = hip.Ctx(0)
    for n, seed in ((1, 1), (255, 2), (5000, 3), (300_000, 4), (2_000_000, 5)):
        rng = np.random.default_rng(seed)
        s1, s2 = gen_strings(n, rng), gen_strings(n, rng)
        i32 = rng.integers(-3, 4, n).astype(np.int32)
        dec = rng.integers(-20000, 20000, n).astype(np.int64)
        dec[rng.integers(0, n, n // 10)] = 1234550
        date = rng.integers(8000, 8006, n).astype(np.int32)
        code = rng.integers(0, 5, n).astype(np.uint8)
        vi = rng.random(n) > 0.05
        dev = {"s1": hip.str_column(ctx, s1), "s2": hip.str_column(ctx, s2),
               "i32": hip.DevColumn(ctx, hip.PH_I32, i32, validity=np.packbits(vi, bitorder="little")),
               "dec": hip.DevColumn(ctx, hip.PH_DEC64, dec, 4), "date": hip.DevColumn(ctx, hip.PH_DATE, date),
               "code": hip.DevColumn(ctx, hip.PH_CODE8, code)}
        py = {"s1": s1, "s2": s2, "i32": [int(v) if ok else None for v, ok in zip(i32.tolist(), vi.tolist())],
              "dec": [cents(v) for v in dec], "date": date.tolist(), "code": code.tolist()}
        cases = [(["s1"], [False]), (["s1"], [True]), (["s1", "s2"], [True, False]), (["s2", "s1"], [False, True]),
                 (["s1", "i32", "code"], [True, False, True]), (["dec", "s1", "date"], [True, False, False]),
                 (["code", "date", "i32", "s2"], [False, True, True, True])]
        if n >= 2_000_000:
            cases = cases[:3]
        sels = (None, np.sort(rng.choice(n, max(1, n // 2), replace=False)))
        for names, desc in cases:
            for sel in sels:
                rows = range(n) if sel is None else sel.tolist()
                got = run_sort(ctx, hip, [dev[k] for k in names], desc, sel, len(rows))
                want = py_order(rows, [py[k] for k in names], desc)
                assert got == want, (n, names, desc, sel is not None)
        for c in dev.values():
            c.free()
    ctx.close()


@pytest.mark.gpu
def test_sort_rows_varchar_edge_columns():
    """an all-equal column, one with only NULLs and empty strings, 'Customer#%09d' names (a long constant prefix) and strings equal in
    their first 8 / 11 / 16 / 64 bytes that differ in the next byte; the type checks"""
    from plan_amd import hip
    ctx = hip.Ctx(0)
    rng = np.random.default_rng(9)
    n = 70_000
    cols = [[b"same value"] * n,
            [None if i % 3 == 0 else b"" for i in range(n)],
            [b"Customer#%09d" % v for v in rng.integers(0, 150_000, n).tolist()],
            [b"\xff" * p + bytes([b]) + b"tail" * t for p, b, t in zip(rng.choice([8, 11, 16, 64], n).tolist(),
                                                                      rng.choice(ALPHABET, n).tolist(), rng.integers(0, 3, n).tolist())],
            [bytes([0x80 + (i % 3)]) + b"\x00" * (i % 5) for i in range(n)]]
    for vals in cols:
        col = hip.str_column(ctx, vals)
        for desc in (False, True):
            assert run_sort(ctx, hip, [col], [desc], None, n) == py_order(range(n), [vals], [desc])
        col.free()
    for t, arr in ((hip.PH_I64, np.arange(10, dtype=np.int64)), (hip.PH_F32, np.ones(10, np.float32)), (hip.PH_F64, np.ones(10))):
        c = hip.DevColumn(ctx, t, arr)
        with pytest.raises(hip.PlanHipError) as e:   # no RadixScatter case in the reference
            hip.sort_rows(ctx, [c], [False], None, 10)
        assert e.value.code == hip.PH_EUNSUPPORTED
        c.free()
    big = hip.str_column(ctx, [b"a"] * 10)
    big.aux_bytes = 2**31                              # int32 offsets: refused before any launch
    with pytest.raises(hip.PlanHipError) as e:
        hip.sort_rows(ctx, [big], [False], None, 10)
    assert e.value.code == hip.PH_EINVAL and "2^31" in str(e.value)
    big.free()
    ctx.close()


@pytest.mark.gpu
def test_sort_rows_o_comment_desc_orderkey_sf1():
    """SF1 orders (1.5 M rows) by o_comment DESC, o_orderkey"""
    from plan_amd import hip
    O = tpchgen.orders((1, 1), columns=["o_orderkey", "o_comment"])
    off, data, key = O["o_comment_off"], O["o_comment_bytes"], O["o_orderkey"]
    n = len(key)
    ctx = hip.Ctx(0)
    com = hip.DevColumn(ctx, hip.PH_STR, off, aux=data)
    k = hip.DevColumn(ctx, hip.PH_I32, key.astype(np.int32))   # SF1 order keys < 6 000 000
    got = run_sort(ctx, hip, [com, k], [True, False], None, n)
    b = data.tobytes()
    text = [b[off[i]:off[i + 1]] for i in range(n)]
    assert got == py_order(range(n), [text, key.tolist()], [True, False])
    com.free()
    k.free()
    ctx.close()


def run_tester(*args, env=None):
    e = dict(os.environ, **(env or {}))
    return subprocess.run([TESTER, *args], check=True, capture_output=True, timeout=900, env=e).stdout


@pytest.mark.gpu
def test_order_text_through_the_operator_interface():
    """host_tester order_text (c_comment DESC, c_address, c_custkey over SF1's 150 000 customers): the device PH_STR sort, the host-rank
    route (PH_ORDER_HOST_RANKS=1) and the host form (PH_ORDER_HOST_ROWS above the row count) print the same bytes, in the restated order"""
    default = run_tester("order_text", "1", "1")
    ranks = run_tester("order_text", "1", "1", env={"PH_ORDER_HOST_RANKS": "1"})
    host = run_tester("order_text", "1", "1", env={"PH_ORDER_HOST_ROWS": "1000000"})
    assert default == ranks == host
    C = tpchgen.customer((1, 1), text=True)
    n = len(C["c_custkey"])

    def strings(name):
        off, b = C[name + "_off"], C[name + "_bytes"].tobytes()
        return [b[off[i]:off[i + 1]] for i in range(n)]
    com, addr, key = strings("c_comment"), strings("c_address"), C["c_custkey"].tolist()
    order = py_order(range(n), [com, addr, key], [True, False, False])
    want = b"#\t\t\n" + b"".join(b"%s\t%s\t%d\n" % (com[r], addr[r], key[r]) for r in order)
    assert default == want
