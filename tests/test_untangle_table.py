"""CPU: the conjugate symmetry of the 16 kHz plan's untangle table (SpxPlanDev::tw2, tw2[k] = (cos, -sin)(2 pi k / 480),
k = 0 .. 239), entry by entry and bit for bit.

Bins p and 240 - p of the packed real transform are untangled from the same two points Z[p], Z[240 - p]; their factors are
mirror images, tw2[240 - p] = (-wx, +wy) of tw2[p] = (wx, wy), in exact arithmetic.  A kernel that untangles the two bins in one
lane may load ONE factor per pair and negate instead of loading two only if the TABLE says so exactly -- which this test decides,
for p = 1 .. 119 (bins 0 and 120 pair with themselves).  It holds because both entries are the correctly rounded values of
exact negatives (tests/test_lane_consts.py checks the rounding); a table from another source need not have the property, so a
failure here lists the entries where it fails.  spx_debug_lane_consts is host code and needs no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 240


@pytest.fixture(scope="module")
def tw2():
    import speedy_amd
    speedy_amd.build()
    L = C.CDLL(os.path.join(ROOT, "speedy_amd", "lib", "libspeedy_hip.so"))
    L.spx_debug_lane_consts.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_float)]
    L.spx_debug_lane_consts.restype = C.c_int
    out = np.zeros(15 * 64 * 16, np.uint8)
    tw, t2, win = np.zeros(2 * W), np.zeros(2 * W), np.zeros(W, np.float32)
    assert L.spx_debug_lane_consts(16000, out.ctypes.data, tw.ctypes.data_as(C.POINTER(C.c_double)),
                                   t2.ctypes.data_as(C.POINTER(C.c_double)), win.ctypes.data_as(C.POINTER(C.c_float))) == out.size
    return t2.reshape(W, 2)


def bits(v):
    return np.float64(v).view(np.uint64)


def test_factor_of_bin_240_minus_p_is_the_mirror_image_bit_for_bit(tw2):
    bad = []
    for p in range(1, W // 2):
        wx, wy = tw2[p]
        mx, my = tw2[W - p]
        if bits(mx) != bits(-wx) or bits(my) != bits(wy):
            bad.append((p, float(wx).hex(), float(wy).hex(), float(mx).hex(), float(my).hex()))
    assert not bad, "tw2[240 - p] != (-wx, +wy) of tw2[p] at %d entries: %r" % (len(bad), bad[:8])


def test_the_self_paired_entries(tw2):
    """Bin 0's factor is (1, -0) and bin 120's (0, -1) exactly: what the two bins that pair with themselves multiply by."""
    assert tw2[0][0] == 1.0 and tw2[0][1] == 0.0
    assert tw2[W // 2][0] == 0.0 and tw2[W // 2][1] == -1.0


def test_no_entry_is_zero_signed_away_by_the_negation(tw2):
    """-wx of a zero would be -0.0, which is not the bits of +0.0: no paired entry (p = 1 .. 119 and its mirror) is a zero."""
    for p in range(1, W):
        if p != W // 2:
            assert tw2[p][0] != 0.0 and tw2[p][1] != 0.0, p
