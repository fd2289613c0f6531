"""The layout rule of the packed scan groups (plan_amd/csrc/pack_layout.h) through ph_pack_scan_layout /
ph_pack_scan_bits: no device. Fields go first fit, largest first, into the two dwords of a 64-bit word; none straddles them."""
import ctypes

import pytest

from plan_amd import hip

i32 = ctypes.c_int32


def layout(widths):
    """the shifts of the fields, or None when the rule refuses them"""
    n = len(widths)
    shifts = (i32 * n)()
    rc = hip.lib().ph_pack_scan_layout(i32(n), (i32 * n)(*widths), shifts)
    if rc == hip.PH_EUNSUPPORTED:
        return None
    assert rc == hip.PH_OK, hip.last_error()
    return list(shifts)


def bits(span):
    hip.lib().ph_pack_scan_bits.restype = i32
    return int(hip.lib().ph_pack_scan_bits(ctypes.c_uint64(span)))


def check_placement(widths, shifts):
    """every field inside one dword, no two fields share a bit"""
    used = 0
    for w, s in zip(widths, shifts):
        assert 0 <= s and s + w <= 64
        assert s // 32 == (s + w - 1) // 32, (w, s)   # no straddle
        mask = ((1 << w) - 1) << s
        assert used & mask == 0, (w, s)
        used |= mask
    assert bin(used).count("1") == sum(widths)


# lineitem's Q1 columns (p, q, e, d, t as value ranges, then the six slots of returnflag x linestatus)
LINEITEM_RANGES = [(8036, 10561), (1, 50), (90100, 10494950), (0, 10), (0, 8)]


def test_lineitem_widths_give_53_bits_in_two_dwords():
    widths = [bits(hi - lo) for lo, hi in LINEITEM_RANGES] + [bits(3 * 2 - 1)]
    assert widths == [12, 6, 24, 4, 4, 3] and sum(widths) == 53
    shifts = layout(widths)
    assert shifts is not None
    check_placement(widths, shifts)
    # first fit, largest first: e, q in the low dword; p, d, t, the slot in the high one
    assert shifts == [32, 24, 0, 44, 48, 52]


def test_exactly_64_bits_fit():
    for widths in ([32, 32], [16, 16, 16, 16], [20, 12, 20, 12], [31, 1, 30, 2], [8] * 8):
        assert sum(widths) == 64
        shifts = layout(widths)
        assert shifts is not None, widths
        check_placement(widths, shifts)


def test_65_bits_are_refused():
    for widths in ([32, 32, 1], [24, 12, 6, 4, 4, 3, 12], [13] * 5, [16, 16, 16, 16, 1]):
        assert sum(widths) == 65
        assert layout(widths) is None, widths


def test_at_most_64_bits_that_cannot_be_placed_without_a_straddle_are_refused():
    for widths in ([22, 22, 20], [17, 17, 17], [30, 30, 3], [20, 20, 20]):
        assert sum(widths) <= 64
        assert layout(widths) is None, widths


def test_a_field_wider_than_a_dword_is_refused():
    assert layout([33]) is None
    assert layout([40, 8]) is None


def test_every_field_has_at_least_one_bit():
    assert bits(0) == 1          # a constant column still gets a field
    assert bits(1) == 1 and bits(2) == 2 and bits(3) == 2 and bits(4) == 3
    assert bits(255) == 8 and bits(256) == 9 and bits(2 ** 32 - 1) == 32 and bits(2 ** 32) == 33 and bits(2 ** 64 - 1) == 64
    assert layout([0, 4]) is None   # a field without bits is not a field
    widths = [bits(0)] * 6
    shifts = layout(widths)
    assert shifts == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("widths", [[24, 12, 6, 4, 4, 3], [16, 8, 32, 8, 8, 4], [9, 1, 17, 5, 2, 1], [16, 8, 20, 8, 8, 4]])
def test_ties_and_order_are_stable(widths):
    """equal widths are placed in the order given; the rule is a pure function of the widths"""
    a, b = layout(widths), layout(widths)
    assert a == b
    if a is not None:
        check_placement(widths, a)
