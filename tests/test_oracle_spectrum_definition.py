"""The oracle's analysis transform against the float64 definition (tests/spectrum_ref.py) at EVERY window size the library
accepts: W = (int)(1.5 rate / 100) for rates 1 000 .. 127 999 Hz, so W = 15 .. 1919.  The bit-equality tests tie the HIP
kernels to the oracle; these tie the oracle to numpy's float64 FFT, bin by bin, so that a mistake both share (a radix or a
Rader size no other test reaches) cannot pass."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrum_ref as sr  # noqa: E402

W_ALL = range(sr.window_size(1000), sr.window_size(127999) + 1)
RADER = [W for W in W_ALL if sr.rader_window(W)]


def _first_of_each_largest_prime():
    seen, out = set(), []
    for W in W_ALL:
        p = sr.largest_prime_factor(W)
        if p not in seen:
            seen.add(p)
            out.append(W)
    return out


FIRST_BY_PRIME = _first_of_each_largest_prime()


def test_window_range_and_rader_sizes():
    assert (W_ALL.start, W_ALL.stop - 1) == (15, 1919)
    assert len(RADER) == 80 and {67, 71, 97, 241, 421, 661, 1153, 1873} <= set(RADER)


@pytest.mark.parametrize("block", range(8))
def test_oracle_spectrum_at_every_window_size(orc, block):
    """orc_spectrum_magnitudes (the packed W-point transform + untangle) for W = 15 .. 1919, all 2W bins of six frames each,
    within one float32 ulp of the bin plus the float64 noise floor (spectrum_ref.NOISE64).  In eight blocks of W."""
    L = orc.lib()
    worst = (0.0, None)
    for W in list(W_ALL)[block::8]:
        mags = np.zeros(2 * W, np.float32)
        for name, v in sr.definition_frames(W, W).items():
            L.orc_spectrum_magnitudes(W, orc.fptr(v), orc.fptr(mags))
            err, k = sr.spectrum_error(mags, v)
            assert err <= 1.0, "W=%d frame=%s bin=%d: %.3g bounds off" % (W, name, k, err)
            worst = max(worst, (err, (W, name, k)))
    print("worst error / bound: %.3f at W, frame, bin = %s" % worst)


@pytest.mark.parametrize("n", sorted(set(RADER) | set(FIRST_BY_PRIME)))
def test_oracle_dft_against_naive_and_numpy(orc, n):
    """orc_dft_forward (the W-point complex transform the spectrum is built on) against the O(n^2) definition and numpy
    at every Rader size and at the first W of every distinct largest prime factor (every odd-prime stage the plans use)."""
    L = orc.lib()
    rng = np.random.default_rng(n)
    x = rng.standard_normal(2 * n)
    a = np.zeros(2 * n)
    b = np.zeros(2 * n)
    L.orc_dft_forward(n, orc.dptr(x), orc.dptr(a))
    L.orc_dft_naive(n, orc.dptr(x), orc.dptr(b))
    ref = np.fft.fft(x[0::2] + 1j * x[1::2])
    tol = 2e-14 * max(1, math.log2(n + 1)) * (np.abs(ref).max() + 1.0)
    got = a[0::2] + 1j * a[1::2]
    assert np.abs(got - ref).max() < tol, n
    assert np.abs(b[0::2] + 1j * b[1::2] - ref).max() < 2e-14 * n * (np.abs(ref).max() + 1.0), n   # naive: n-term sums
    assert np.abs(a - b).max() < tol, n


def _oracle_callback_rows(orc, x, rate, ch, chunks=None):
    L = orc.lib()
    rows = []
    h = L.orc_sonicCreateStream(rate, ch, 0)
    nb = L.orc_sonicSpectrogramSize(h)
    cb = orc.FEATURES_FN(lambda s, t, p: rows.append(np.ctypeslib.as_array(p, shape=(nb,)).copy()))
    L.orc_sonicSpectrogramCallback(h, cb)
    L.orc_sonicSetSpeed(h, 2.0)
    L.orc_sonicEnableNonlinearSpeedup(h, 1.0)
    x = np.ascontiguousarray(x, np.int16)
    pos = 0
    for c in (chunks or [x.size // ch]):
        L.orc_sonicWriteShortToStream(h, orc.sptr(x[pos * ch:]), c)
        pos += c
    L.orc_sonicDestroyStream(h)
    return np.array(rows).reshape(-1, nb)


@pytest.mark.parametrize("rate,ch", [(16000, 1), (11025, 3), (6467, 2), (44100, 1)])
def test_framing_matches_the_oracles_callback(orc, rate, ch):
    """spectrum_ref.analysis_frames (written from soniclib.c / speedy.c) against the oracle's spectrogram callback: the same
    number of frames, and every bin within the definition's bound.  A framing mistake in the test shows up here, not as a
    kernel bug.  Channel sums are negative and odd, so that C's truncation and numpy's flooring differ."""
    from speedy_amd.synth import speech_like
    n = int(0.37 * rate) + 11
    mono = speech_like(n, rate, seed=rate).astype(np.int64)
    rng = np.random.default_rng(rate)
    x = np.repeat(mono[:, None], ch, axis=1)
    if ch > 1:
        x[:, 0] = np.clip(mono - rng.integers(0, 3, n), -32768, 32767)   # sums of every residue modulo ch
    x = x.astype(np.int16).ravel()
    frames = sr.analysis_frames(x, ch, rate)
    rng2 = np.random.default_rng(1)
    cuts = []
    left = n
    while left > 0:
        c = int(min(left, rng2.integers(1, 700)))
        cuts.append(c)
        left -= c
    for chunks in (None, cuts):
        rows = _oracle_callback_rows(orc, x, rate, ch, chunks)
        assert rows.shape == (frames.shape[0], 2 * frames.shape[1]), (rows.shape, frames.shape)
        for j in range(rows.shape[0]):
            err, k = sr.spectrum_error(rows[j], frames[j])
            assert err <= 1.0, (rate, ch, j, k, err)


def test_mono_mix_truncates_toward_zero():
    x = np.array([-3, 0, -1, -1, 5, 0, -32768, -32767, -32768, 32767, 32767, 32767], np.int16)
    assert sr.mono_mix(x, 2).tolist() == [-1, -1, 2, -32767, 0, 32767]
    assert sr.mono_mix(np.array([-3, 0, -1, -1, 5, 0], np.int16), 3).tolist() == [-1, 1]
    assert sr.mono_mix(np.array([-5, 0, 0], np.int16), 3).tolist() == [-1]   # floor would give -2
