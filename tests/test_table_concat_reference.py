"""The host twins of ph_table_concat's rules, without a GPU: ph_validity_concat_host (the same __host__ __device__ function the validity
kernel runs per 32-bit word) against numpy's unpackbits / packbits over the concatenated bit arrays, and ph_dict_merge_host (the
dictionary rule) against sorted(set(...)) over bytes."""
import numpy as np
import pytest

from plan_amd import hip

ALIGN_ROWS = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 0, 2047]


def make_parts(rng, rows, null_some):
    """per part a bitmap of (rows + 7) // 8 bytes whose unused tail bits are GARBAGE (ones), or None; and the rows' bits"""
    bitmaps, bits = [], []
    for k, n in enumerate(rows):
        b = rng.integers(0, 2, n).astype(np.uint8)
        if null_some and rng.integers(0, 3) == 0:
            bitmaps.append(None)
            bits.append(np.ones(n, np.uint8))
            continue
        tail = np.ones((-n) % 8, np.uint8)                      # what lies behind a part's last row must not leak into the result
        packed = np.packbits(np.concatenate([b, tail]), bitorder="little")
        bitmaps.append(packed if n else np.zeros(1, np.uint8))
        bits.append(b)
    return bitmaps, bits


def expect(bits, out_bytes):
    allbits = np.concatenate(bits) if bits else np.zeros(0, np.uint8)
    packed = np.packbits(allbits, bitorder="little")
    return np.concatenate([packed, np.zeros(out_bytes - len(packed), np.uint8)])


def check(rows, seed, null_some=False, extra=0):
    rng = np.random.default_rng(seed)
    bitmaps, bits = make_parts(rng, rows, null_some)
    out_bytes = (sum(rows) + 7) // 8 + extra
    got = hip.validity_concat_host(bitmaps, rows, out_bytes)
    want = expect(bits, out_bytes)
    assert got.tobytes() == want.tobytes(), (rows, seed)
    # the round trip through unpackbits: every row's bit, and nothing at or beyond the total
    un = np.unpackbits(got, bitorder="little")
    assert np.array_equal(un[:sum(rows)], np.concatenate(bits) if sum(rows) else un[:0]) and not un[sum(rows):].any()


def test_validity_every_alignment():
    check(ALIGN_ROWS, 1)
    check(ALIGN_ROWS, 2, null_some=True)
    check(ALIGN_ROWS[::-1], 3, null_some=True, extra=9)       # the tail of the last byte and the bytes behind it are 0


def test_validity_all_zero_rows():
    for n in (1, 2, 5):
        got = hip.validity_concat_host([None] * n, [0] * n, 4)
        assert got.tobytes() == b"\0" * 4
    assert len(hip.validity_concat_host([None, None], [0, 0])) == 0


def test_validity_forty_parts_of_one_row_and_one_part_alone():
    check([1] * 40, 4)
    check([1] * 40, 5, null_some=True)
    for n in (1, 8, 31, 32, 33, 2047):
        check([n], 6 + n)
    got = hip.validity_concat_host([None], [13], 3)
    assert got.tobytes() == bytes([0xff, 0x1f, 0])


def test_validity_random_splits():
    rng = np.random.default_rng(99)
    for k in range(300):
        nparts = int(rng.integers(1, 12))
        hi = int(rng.choice([3, 10, 40, 70, 300]))
        rows = [int(r) for r in rng.integers(0, hi, nparts)]
        check(rows, 1000 + k, null_some=True, extra=int(rng.integers(0, 6)))


def test_validity_buffer_too_small_is_ecapacity():
    with pytest.raises(hip.PlanHipError) as e:
        hip.validity_concat_host([None, None], [8, 1], 1)
    assert e.value.code == hip.PH_ECAPACITY and "need 2 bytes" in str(e.value)
    assert hip.validity_concat_host([None, None], [8, 1], 2).tobytes() == bytes([0xff, 0x01])


# ---------------------------------------------------------------- dictionaries

def check_merge(dicts):
    merged, remap, identical = hip.dict_merge_host(dicts)
    same = all(d == dicts[0] for d in dicts)
    assert identical == same
    if same:
        assert merged == list(dicts[0])
    else:
        assert merged == sorted(set(e for d in dicts for e in d))       # bytes sort as unsigned bytes
    if len(merged) <= 256:
        for p, d in enumerate(dicts):
            for c, e in enumerate(d):
                assert merged[remap[p][c]] == e, (p, c)
            assert not remap[p][len(d):].any()
    else:
        assert not remap.any()
    return merged, remap, identical


def test_dict_identical_unsorted_is_kept():
    d = [b"zeta", b"alpha", b"mid", b""]
    merged, remap, identical = check_merge([d, list(d), list(d)])
    assert identical and merged == d
    for p in range(3):
        assert list(remap[p][:4]) == [0, 1, 2, 3]
    assert check_merge([d])[2]                                           # one part alone is identical to itself


def test_dict_disjoint_and_overlapping():
    merged, remap, identical = check_merge([[b"b", b"d"], [b"a", b"c"]])
    assert not identical and merged == [b"a", b"b", b"c", b"d"] and list(remap[0][:2]) == [1, 3] and list(remap[1][:2]) == [0, 2]
    check_merge([[b"b", b"d", b"x"], [b"d", b"a", b"b"], [b"x"]])
    # the same entries in ANOTHER order are not identical: the result is the sorted union
    merged, _r, identical = check_merge([[b"b", b"a"], [b"a", b"b"]])
    assert not identical and merged == [b"a", b"b"]


def test_dict_union_of_256_and_257():
    names = [b"k%03d" % i for i in range(257)]
    merged, remap, _i = check_merge([names[:200], names[100:256]])
    assert len(merged) == 256 and remap[1][155] == 255
    merged, remap, identical = check_merge([names[:200], names[100:257]])
    assert len(merged) == 257 and not identical


def test_dict_unsigned_order_prefixes_and_empty_string():
    d0 = [b"ab", b"a", b"abc", b"\xc3\xa9", b"z"]
    d1 = [b"", b"\x80", b"\x7f", b"a\xff", b"ab"]
    merged, _r, _i = check_merge([d0, d1])
    assert merged == [b"", b"a", b"ab", b"abc", b"a\xff", b"z", b"\x7f", b"\x80", b"\xc3\xa9"]
    assert merged.index(b"\x7f") < merged.index(b"\x80")                 # a signed comparison would put 0x80 first


def test_dict_duplicate_inside_one_part_and_empty_dictionary():
    merged, remap, identical = check_merge([[b"x", b"a", b"x"], [b"a"]])
    assert merged == [b"a", b"x"] and list(remap[0][:3]) == [1, 0, 1] and not identical
    merged, remap, identical = check_merge([[], [b"q", b"p"]])
    assert merged == [b"p", b"q"] and not identical and not remap[0].any()
    merged, _r, identical = check_merge([[], []])
    assert merged == [] and identical


def test_dict_merged_buffer_too_small_is_ecapacity():
    with pytest.raises(hip.PlanHipError) as e:
        hip.dict_merge_host([[b"abc"], [b"de"]], cap=6)
    assert e.value.code == hip.PH_ECAPACITY
    assert hip.dict_merge_host([[b"abc"], [b"de"]], cap=7)[0] == [b"abc", b"de"]
