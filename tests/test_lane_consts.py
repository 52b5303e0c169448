"""CPU: the lane-major constant table of a 16 kHz plan (SpxPlanDev::lane_consts, speedy_amd/csrc/spx_plan.hip).

spx_analysis_kernel<16, 240> no longer holds a lane's twiddles, untangle factors and window values in registers across its tile:
it loads entry [c][lane] of this table right before the stage that uses it.  The table must therefore hold, bit for bit, the
values the kernel used to index out of the plan's tables itself (the <8, 240> instantiation still does):

    c = 0..2    tw[bb j],            j = 1..3, bb = lane if lane < 60 else 0          (stage 1)
    c = 3..5    tw[4 (bb >> 2) j]                                                      (stage 2)
    c = 6..9    tw[16 p3], tw[32 p3] for b3 = lane, lane + 64; p3 = b3 >> 4 if b3 < 80 else 0   (stage 3)
    c = 10..13  tw2[k],              k = lane + 64 u if below 240 else 0              (untangle)
    c = 14      window[2 bb], [2 bb + 1], [2 bb + 120], [2 bb + 121], each times 2^-15 as a float

with tw[t] = (cos, -sin)(2 pi t / 240), tw2[k] = (cos, -sin)(2 pi k / 480) and the Hamming window of speedy.c:256-258.  The
expected values come from the 60-digit evaluation of tools/twiddle_tables.py, not from the library; spx_debug_lane_consts is host
code and needs no GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import twiddle_tables as tt  # noqa: E402

ENTRIES, W = 15, 240


@pytest.fixture(scope="module")
def tables():
    import speedy_amd
    speedy_amd.build()
    L = C.CDLL(os.path.join(ROOT, "speedy_amd", "lib", "libspeedy_hip.so"))
    L.spx_debug_lane_consts.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_float)]
    L.spx_debug_lane_consts.restype = C.c_int
    out = np.zeros(ENTRIES * 64 * 16, np.uint8)
    tw, tw2, win = np.zeros(2 * W), np.zeros(2 * W), np.zeros(W, np.float32)
    n = L.spx_debug_lane_consts(16000, out.ctypes.data, tw.ctypes.data_as(C.POINTER(C.c_double)),
                                tw2.ctypes.data_as(C.POINTER(C.c_double)), win.ctypes.data_as(C.POINTER(C.c_float)))
    assert n == out.size
    return L, out, tw.reshape(W, 2), tw2.reshape(W, 2), win


def _expected_tables():
    tw = np.array([(c, 0.0 - s) for c, s in (tt.entry(t, W) for t in range(W))])
    tw2 = np.array([(c, 0.0 - s) for c, s in (tt.entry(t, 2 * W) for t in range(W))])
    win = np.array([np.float32(0.54 - 0.46 * tt.entry(t, W - 1)[0]) for t in range(W)], np.float32)
    return tw, tw2, win


def test_source_tables_are_the_correctly_rounded_ones(tables):
    _, _, tw, tw2, win = tables
    etw, etw2, ewin = _expected_tables()
    assert np.array_equal(tw.view(np.uint64), etw.view(np.uint64))
    assert np.array_equal(tw2.view(np.uint64), etw2.view(np.uint64))
    assert np.array_equal(win.view(np.uint32), ewin.view(np.uint32))


def test_lane_major_table_is_what_the_kernel_indexed(tables):
    _, out, _, _, _ = tables
    tw, tw2, win = _expected_tables()
    d = out.view(np.float64).reshape(ENTRIES, 64, 2)
    f = out.view(np.float32).reshape(ENTRIES, 64, 4)
    scale = np.float32(2.0 ** -15)
    for lane in range(64):
        bb = lane if lane < 60 else 0
        want = []
        for j in (1, 2, 3):
            want.append(tw[bb * j])
        for j in (1, 2, 3):
            want.append(tw[4 * (bb >> 2) * j])
        for u in (0, 1):
            b3 = lane + 64 * u
            p3 = (b3 >> 4) if b3 < 80 else 0
            want += [tw[16 * p3], tw[32 * p3]]
        for u in range(4):
            k = lane + 64 * u
            want.append(tw2[k if k < W else 0])
        got = d[:14, lane]
        assert np.array_equal(got.view(np.uint64), np.array(want).view(np.uint64)), lane
        wn = np.array([win[2 * bb] * scale, win[2 * bb + 1] * scale, win[2 * bb + 120] * scale, win[2 * bb + 121] * scale], np.float32)
        assert wn.dtype == np.float32 and np.array_equal(f[14, lane].view(np.uint32), wn.view(np.uint32)), lane
        # the scale is a power of two: nothing is rounded (no window value is anywhere near subnormal)
        assert np.array_equal(f[14, lane].astype(np.float64) * 32768.0, np.array([win[2 * bb], win[2 * bb + 1], win[2 * bb + 120], win[2 * bb + 121]], np.float64))


def test_rates_without_the_table(tables):
    L = tables[0]
    out = np.zeros(ENTRIES * 64 * 16, np.uint8)
    tw, tw2, win = np.zeros(2 * W), np.zeros(2 * W), np.zeros(W, np.float32)
    args = (tw.ctypes.data_as(C.POINTER(C.c_double)), tw2.ctypes.data_as(C.POINTER(C.c_double)), win.ctypes.data_as(C.POINTER(C.c_float)))
    for rate in (8000, 22050, 44100):
        assert L.spx_debug_lane_consts(rate, out.ctypes.data, *args) == 0
    assert not out.any()
    assert L.spx_debug_lane_consts(16000, None, *args) == -1
