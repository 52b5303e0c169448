"""Inputs shared by tests/test_dtw_definition.py and tests/test_gpu_dtw.py: the reference's own DTW test pair -- tapestry.wav at 3x,
linear and nonlinear, through the oracle, measured with ComputeSpectrogram (sonic_test.cc:211-240) exactly as
sonic_props.check_speech_dtw sets it up -- and its answers by the definition (tests/dtw_ref.py), computed once per process."""
import functools

import numpy as np

import dtw_ref
from util import read_wav

SPEED, HALF_WIDTH = 3.0, 10


def local_costs(a, b):
    """dtw_ref.local_cost for every cell at once: the same float32 operations in the same order of k -- one subtraction, one
    multiplication, one addition, each over the whole matrix and each rounded to float32 -- so the Python loop runs over k alone
    (the scalar form costs a second per 4 000 cells at dim = 240).  tests/test_dtw_definition.py holds it to the scalar form bit for
    bit."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    s = np.zeros((a.shape[0], b.shape[0]), np.float32)
    for k in range(a.shape[1]):
        t = a[:, k][:, None] - b[:, k][None, :]
        s = s + t * t
    return np.sqrt(s)


def answer(a, b, half_width=HALF_WIDTH):
    """dtw_ref.dtw with the local costs from local_costs."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    if a.ndim == 1:
        a, b = a[:, None], b[:, None]
    return dtw_ref.dtw(a, b, half_width, d_matrix=local_costs(a, b))


@functools.lru_cache(maxsize=None)
def tapestry_rows():
    """dict(original, linear, nonlinear): ComputeSpectrogram rows, float32 [rows][N / 2], the upper half of each row zero."""
    from oracle import pyorc
    from test_oracle_sonic_properties import _spectrogram
    pyorc.build()
    x, rate, ch = read_wav("tapestry.wav")
    spec = _spectrogram(pyorc)
    out = {"original": spec(x, rate)}
    for name, nonlinear in (("linear", 0.0), ("nonlinear", 1.0)):
        y = pyorc.compress_sound(x, rate, ch, SPEED, nonlinear, 0.0, True, chunk=1024, taps=False)["out"]
        out[name] = spec(y, rate)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tapestry_answer(name):
    """dtw_ref.dtw of (original, `name`).  The rows' upper halves are zeros on both sides: they add +0 to every sum, so the
    definition runs over the lower halves and gives the full rows' result."""
    rows = tapestry_rows()
    half = rows["original"].shape[1] // 2
    assert not rows["original"][:, half:].any() and not rows[name][:, half:].any()
    return dtw_ref.dtw(rows["original"][:, :half], rows[name][:, :half], HALF_WIDTH)


def reference_thresholds(name, r):
    """TestSpeechSample's own limits (sonic_test.cc:669-721)."""
    assert float(r["cost"]) < 13000000
    assert abs(float(r["slope"]) - 1.0 / SPEED) <= (0.02 if name == "linear" else 0.1), r["slope"]
    assert abs(float(r["local_mean"]) - float(r["slope"])) <= 0.02
    assert float(r["local_std"]) < 0.2
    assert not np.isnan(np.asarray(dtw_ref.local_slopes([tuple(p) for p in r["path"]], HALF_WIDTH), np.float32)).any()
