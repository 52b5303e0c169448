"""The directed inputs of the pitch-decision tests (tests/test_oracle_pitch_decision.py on the CPU, tests/test_gpu_pitch_decision.py
on the device): quiet hum in a nearly silent recording -- rectangular waves of a few LSB with a non-integer period just below the
longest lag, and a low-level tone in a few LSB of noise.  On these the AMDF sums are small integers, so that different lags
reach the same key floor(d 2^16 / p) with different ratios d / p, and minDiff and maxDiff are small enough to sit on the edges of
the previous-period rule.  The parameters are fixed; tests/pitch_ref.py's census (asserted by the CPU test) says what each reaches.
"""
import numpy as np


def rect(rate, a, per, duty, centred, seconds):
    """x[t] = a where frac(t / per) < duty, else 0; minus a // 2 if centred."""
    t = np.arange(int(rate * seconds), dtype=np.float64)
    x = np.where(np.mod(t / per, 1.0) < duty, a, 0)
    return (x - (a // 2 if centred else 0)).astype(np.int16)


def hum(rate, level, freq, noise, seed, seconds, density=1.0):
    """round(level sin(2 pi freq t / rate)) plus uniform integer noise of +- noise LSB on a share `density` of the samples."""
    t = np.arange(int(rate * seconds), dtype=np.float64)
    rng = np.random.default_rng(seed)
    e = rng.integers(-noise, noise + 1, size=t.size) * (rng.random(t.size) < density)
    return (np.round(level * np.sin(2 * np.pi * freq * t / rate)) + e).astype(np.int16)


def sprinkle(x, seed, density, amp):
    """x with +- amp LSB added to a share `density` of its samples."""
    rng = np.random.default_rng(seed)
    return (x + rng.integers(-amp, amp + 1, size=x.size) * (rng.random(x.size) < density)).astype(np.int16)


def duplicated_stereo(x):
    return np.stack([x, x], axis=1).reshape(-1).astype(np.int16)


def one_sided_stereo(x):
    """(2 a, 0): the channel mean, and every decimated sum divided by 2 skip, is the mono signal's exactly."""
    return np.stack([2 * x.astype(np.int32), np.zeros(x.size, np.int32)], axis=1).reshape(-1).astype(np.int16)


# rect: (a, period, duty, centred, seconds); hum: (level, freq, noise, seed, seconds, density); sprinkled: (seed, density, amp)
_RECT = [
    ("rect11k", 11025, (1, 160.37, 0.4, True, 0.8)),          # 72 coarse lags; every lag product below 2^16
    ("rect22k", 22050, (1, 325.51, 0.685, True, 0.8)),
    ("rect44k", 44100, (5, 673.49, 0.414, True, 0.6)),
    ("rect48k", 48000, (1, 643.309, 0.337, False, 0.6)),
    ("rect64k", 63999, (1, 573.833, 0.159, False, 0.5)),     # key ties of unequal ratio on both sides of lag index 64 (a fold boundary)
    ("rect96k", 96000, (3, 1372.416, 0.341, True, 0.5)),
]
_SPRINKLED = [
    ("rect44k_n", 44100, (13, 639.613, 0.165, True, 0.5), (171, 0.5, 2)),   # the general selector's 1 + 2^-16 window, minimum side
    ("rect96k_n", 96000, (22, 1451.082, 0.325, True, 0.4), (199, 0.5, 1)),  # ... maximum side
]
_HUM = [
    ("hum16k", 16000, (32, 70.0, 4, 12, 0.8, 1.0)),     # 2 minDiff = 3 prevMinDiff
    ("hum22k", 22050, (17, 100.3, 3, 2, 0.8, 1.0)),     # maxDiff = 3 minDiff with the previous period taken
    ("hiss22k", 22050, (2, 150.0, 2, 46, 0.8, 0.53)),   # minDiff between 0 and 1
]
_CACHE = None


def directed():
    """[(name, rate, channels, int16 interleaved samples)] -- built once per process, never modified."""
    global _CACHE
    if _CACHE is None:
        out = [(name, rate, 1, rect(rate, *p)) for name, rate, p in _RECT]
        out += [(name, rate, 1, sprinkle(rect(rate, *p), *q)) for name, rate, p, q in _SPRINKLED]
        out += [(name, rate, 1, hum(rate, *p)) for name, rate, p in _HUM]
        by = {name: x for name, _, _, x in out}
        out.append(("rect22k_dup", 22050, 2, duplicated_stereo(by["rect22k"])))
        out.append(("rect48k_left", 48000, 2, one_sided_stereo(by["rect48k"])))
        for item in out:
            item[3].setflags(write=False)
        _CACHE = out
    return _CACHE
