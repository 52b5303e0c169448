"""speedy_amd/csrc/spx_frame_math.h -- the one text of the frame-rate feature chain that the tension kernels, the unit-level API
and the analysis kernel compile -- built for the host (plain g++ -ffp-contract=off, speedy_amd/lib/libspx_mode_table.so) and held
to the CPU oracle bit for bit, teacher-forced: every stage is fed the oracle's own float32 taps of the stage before and must
return the oracle's float32 bits (compared as uint32).  No GPU: a cast, a constant or a rounding point that slips in the header
fails here before any kernel runs.

Stages per feature row k (tests/features_ref.py has the time base): f1 (energy low-pass, row 0 from the header's start value through
the F - 1 frames before it), f2 = local(f0[k + F], f1[k]), f3, f4, f5, f7, f8 (row 0 from the header's start value), f9, f10, f11,
the tension tap; then the speed taps from the tension taps for every branch of the speed law.  The F rows whose energy f0[k + F]
no feature row shows are left out of f2, nothing else is: the counts are asserted."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import features_ref as fr  # noqa: E402
import spectrum_ref as sr  # noqa: E402
from feature_inputs import clicks_in_silence, jumping_tone, speech, square_wave  # noqa: E402
from test_oracle_feature_definition import oracle_taps  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32P = C.POINTER(C.c_float)
STAGES = ["f1", "f2", "f3", "f4", "f5", "f7", "f8", "f9", "f10", "f11", "tension"]


@pytest.fixture(scope="module")
def fm():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "modetable"])
    L = C.CDLL(os.path.join(ROOT, "speedy_amd", "lib", "libspx_mode_table.so"))
    L.spx_frame_math_lowpass.argtypes = [C.c_int, C.c_float, C.c_float, F32P, F32P, F32P]
    for name in ("local_energy", "weighted", "relative", "tension"):
        getattr(L, "spx_frame_math_" + name).argtypes = [C.c_int, F32P, F32P, F32P]
    for name in ("compress", "clamp"):
        getattr(L, "spx_frame_math_" + name).argtypes = [C.c_int, F32P, F32P]
    L.spx_frame_math_tapered_max.argtypes = [C.c_int, F32P, F32P]
    L.spx_frame_math_tapered_max.restype = C.c_float
    L.spx_frame_math_hysteresis.argtypes = [C.c_float, C.c_float]
    L.spx_frame_math_hysteresis.restype = C.c_float
    L.spx_frame_math_low.argtypes = [C.c_int, F32P, C.c_int, C.c_int, F32P]
    L.spx_frame_math_low_threshold.restype = C.c_float
    L.spx_frame_math_start_values.argtypes = [F32P]
    L.spx_frame_math_speed.argtypes = [C.c_int, F32P, C.c_float, C.c_float, C.c_float, F32P, F32P]
    return L


def _p(a):
    return a.ctypes.data_as(F32P)


def stage(fn, *arrays):
    """out[i] = the header's stage on row i of the float32 arrays."""
    arrays = [np.ascontiguousarray(a, np.float32) for a in arrays]
    out = np.zeros(arrays[0].size, np.float32)
    fn(out.size, *[_p(a) for a in arrays], _p(out))
    return out


def same_bits(what, got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, "%s: %d of %d rows differ, first row %d: got %r, oracle %r" % (
        what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])
    return got.size


INPUTS = {"speech": speech, "clicks": clicks_in_silence, "square": square_wave, "jumping": jumping_tone}
# (input, rate, matlab): the rates at which tests/test_oracle_feature_definition.py asserts that each input reaches its branch
CASES = [("speech", 16000, False), ("speech", 16000, True), ("clicks", 16000, False), ("square", 16000, False),
         ("jumping", 16000, False), ("jumping", 22050, False)]
_TAPS = {}


def taps_of(orc, name, rate, matlab, **kw):
    key = (name, rate, matlab, tuple(sorted(kw.items())))
    if key not in _TAPS:
        _TAPS[key] = oracle_taps(orc, INPUTS[name](rate), rate, matlab=matlab, **kw)
    return _TAPS[key]


def check_chain(L, taps, rate, matlab):
    """Every stage of every row through the header; returns (values compared, rows, reach counts)."""
    f = taps["features"]
    K = f.shape[0]
    W = sr.window_size(rate)
    F, P = fr.hysteresis_shape(matlab)
    T = taps["spectrogram"].shape[0]
    assert K == T + 1 - F and K > F + P
    alpha = np.float32(math.exp(-1.0 / np.float32(100.0)))   # the plan's two filter weights (speedy.c:67,74)
    oma = np.float32(np.float32(1) - alpha)
    start = np.zeros(2, np.float32)
    L.spx_frame_math_start_values(_p(start))
    n = dict.fromkeys(STAGES, 0)

    # the energy of time t (speedy.c:633-640: float squares added in turn): f0 of row t where a row shows it, the same sum over
    # the spectrogram tap's row t - 1 behind the last row -- the same bits wherever both exist
    sq = taps["spectrogram"][:, 1:W] * taps["spectrogram"][:, 1:W]
    e_spec = np.concatenate([[np.float32(0)], np.cumsum(sq, axis=1, dtype=np.float32)[:, -1]]).astype(np.float32)   # index = time
    same_bits("f0 against the spectrogram tap", e_spec[:K], f[:, 0])

    # f1: the low-pass runs from the header's start value over times 1 .. F - 1, which no row shows, then row by row
    state, c_early = start[:1].copy(), {}
    for t in range(1, F):
        state = stage(lambda m, *a: L.spx_frame_math_lowpass(m, oma, alpha, *a), e_spec[t:t + 1], state)
        c_early[t] = stage(L.spx_frame_math_compress, stage(L.spx_frame_math_local_energy, e_spec[t:t + 1], state))[0]
    prev1 = np.concatenate([state, f[:-1, 1]])
    n["f1"] = same_bits("f1", stage(lambda m, *a: L.spx_frame_math_lowpass(m, oma, alpha, *a), e_spec[F:F + K], prev1), f[:, 1])
    # f2 from the f0 of F rows later: the last F rows have none
    n["f2"] = same_bits("f2", stage(L.spx_frame_math_local_energy, f[F:, 0], f[:K - F, 1]), f[:K - F, 2])
    n["f3"] = same_bits("f3", stage(L.spx_frame_math_compress, f[:, 2]), f[:, 3])

    # f4: tapered maxima over the compressed energies of times k .. k + F and k .. k - P (zero before time 1)
    def c(t):
        return f[t - F, 3] if t >= F else c_early.get(t, np.float32(0))

    tf = (np.arange(F, -1, -1, dtype=np.float32) / np.float32(F)).astype(np.float32)   # speedy.c:597,604
    tp = (np.arange(P, -1, -1, dtype=np.float32) / np.float32(P)).astype(np.float32)
    f4 = np.zeros(K, np.float32)
    for k in range(K):
        fut = np.array([c(k + i) for i in range(F + 1)], np.float32)
        past = np.array([c(k - i) for i in range(P + 1)], np.float32)
        f4[k] = L.spx_frame_math_hysteresis(L.spx_frame_math_tapered_max(P + 1, _p(past), _p(tp)),
                                            L.spx_frame_math_tapered_max(F + 1, _p(fut), _p(tf)))
    n["f4"] = same_bits("f4", f4, f[:, 4])

    # f5 from f0, k and the first row; f14 is the header's threshold
    low = np.zeros(K, np.float32)
    L.spx_frame_math_low(K, _p(np.ascontiguousarray(f[:, 0])), 0, 0, _p(low))
    n["f5"] = same_bits("f5", low, f[:, 5])
    same_bits("f14", np.full(K, L.spx_frame_math_low_threshold(), np.float32), f[:, 14])
    lowb = f[:, 5] != 0
    zero = np.zeros(K, np.float32)

    n["f7"] = same_bits("f7", np.where(lowb, zero, stage(L.spx_frame_math_weighted, f[:, 6], f[:, 4])), f[:, 7])
    prev8 = np.concatenate([start[1:], f[:-1, 8]])
    n["f8"] = same_bits("f8", stage(lambda m, *a: L.spx_frame_math_lowpass(m, oma, alpha, *a), f[:, 7], prev8), f[:, 8])
    n["f9"] = same_bits("f9", np.where(lowb, zero, stage(L.spx_frame_math_relative, f[:, 7], f[:, 8])), f[:, 9])
    n["f10"] = same_bits("f10", np.where(lowb, zero, stage(L.spx_frame_math_clamp, f[:, 9])), f[:, 10])
    f11 = stage(L.spx_frame_math_tension, f[:, 4], f[:, 10])
    n["f11"] = same_bits("f11", f11, f[:, 11])
    n["tension"] = same_bits("tension tap", f11, taps["tension"])

    assert n["f2"] == K - F and all(n[s] == K for s in STAGES if s != "f2"), n
    reach = dict(low=int(lowb.sum()), after_low=int((lowb[:-1] & ~lowb[1:]).sum()), f2_limited=int((f[:, 2] > 2.0).sum()),
                 clamped=int((f[:, 9] > np.float32(fr.CLAMP)).sum()))
    return sum(n.values()), K, F, reach


@pytest.mark.parametrize("name,rate,matlab", CASES)
def test_every_stage_of_every_row_returns_the_oracles_bits(orc, fm, name, rate, matlab):
    total, K, F, reach = check_chain(fm, taps_of(orc, name, rate, matlab), rate, matlab)
    print("\n%s %d Hz matlab=%s: %d rows, %d values compared, %r" % (name, rate, matlab, K, total, reach))
    assert total == K * len(STAGES) - F
    if name == "clicks":       # long low runs, non-low frames right after a low one
        assert reach["low"] >= 10 and reach["after_low"] >= 3, reach
    if name == "square":       # the energy jumps far above its low-pass: min(f2, 2)
        assert reach["f2_limited"] >= 5, reach
    if name == "jumping":      # f9 beyond 4 * mean: the clamp
        assert reach["clamped"] >= 5, reach


@pytest.mark.parametrize("fb", [0.0, 0.1])
@pytest.mark.parametrize("nl", [1.0, 0.5])
@pytest.mark.parametrize("R", [2.0, 0.8])
def test_the_speed_sequence_from_the_tension_taps(orc, fm, R, nl, fb):
    """Both branches on R > 1, with and without feedback, with nl = 1 (blended speed = requested speed exactly) and nl = 0.5: the
    whole sequence with the carried duration sums, bit for bit."""
    taps = taps_of(orc, "speech", 16000, False, R=R, nl=nl, fb=fb)
    ten = np.ascontiguousarray(taps["tension"], np.float32)
    K = ten.size
    same_bits("tension is the same for every speed", ten, taps_of(orc, "speech", 16000, False)["tension"])
    durations = np.zeros(2, np.float32)
    out = np.zeros(K, np.float32)
    half = K // 2   # in two calls: the duration sums are carried from one to the next
    fm.spx_frame_math_speed(half, _p(ten), R, nl, fb, _p(durations), _p(out))
    fm.spx_frame_math_speed(K - half, _p(ten[half:]), R, nl, fb, _p(durations), _p(out[half:]))
    assert same_bits("speed R=%g nl=%g fb=%g" % (R, nl, fb), out, taps["speed"]) == K >= 150
    assert np.unique(out).size > 10                          # the law moved the speed
    assert durations[0] > 0 and durations[1] > 0
