"""A float64 definition of the analysis spectrum, written from the reference's text (speedy.c, soniclib.c) and not from
oracle/: the second, independent check the spectrum tests hold the oracle and the HIP kernels to.

frame_spectrum     |DFT_2W| of a windowed float32 frame, in float64, with a per-bin bound
hamming            speedy.c:256-258 with a 50-digit cosine
analysis_frames    the windowed frames the streaming shim hands to Speedy (soniclib.c:246-310,391-452; speedy.c:416-425,553-565)
normalized_bound   speedy.c:628-647 and the bound its float32 sequential sum earns
"""
import functools
import math

import mpmath
import numpy as np

FRAME_RATE_HZ = 100.0   # speedy.c:90 kFrameRateHz


def window_size(rate):
    return int(1.5 * rate / FRAME_RATE_HZ)      # speedy.c:213


def frame_step(rate):
    return int(rate / FRAME_RATE_HZ)            # speedy.c:335-338


def rader_window(W):
    """The plan's rule (DESIGN.md "DFT spec"): Rader's algorithm for a prime W > 64 whose W - 1 is 13-smooth."""
    if W <= 64 or any(W % q == 0 for q in range(2, int(W ** 0.5) + 1)):
        return False
    m = W - 1
    for q in (2, 3, 5, 7, 11, 13):
        while m % q == 0:
            m //= q
    return m == 1


def largest_prime_factor(n):
    p, best = 2, 1
    while p * p <= n:
        while n % p == 0:
            best, n = p, n // p
        p += 1
    return max(best, n) if n > 1 else best


# The float64 reference and the float32 result it is compared with differ by (a) the rounding of the float32 result,
# at most half an ulp of the bin for a correctly rounded magnitude, and (b) the error of the two float64 transforms (the one
# under test and numpy's), each about eps64 * log2(2W) * sum|v| for a frame v: eps64 = 1.1e-16, log2(2 * 1919) < 12, so
# both together stay below 3e-15 * sum|v|.  1e-13 * sum|v| is thirty times that and still a hundred times below
# float32 resolution of the largest bin (which is at most sum|v|): a wrong twiddle, permutation, index or sign moves bins by
# 1e-3 of sum|v| or more and fails by orders of magnitude.  Not loosened per case.
NOISE64 = 1e-13


def frame_spectrum(v32):
    """v32: a windowed float32 frame of W samples.  Returns (|fft(v, 2W)| in float64, per-bin bound): one float32 ulp of
    the bin plus the float64 noise floor NOISE64 * sum|v|."""
    v = np.asarray(v32, np.float32).astype(np.float64)
    ref = np.abs(np.fft.fft(v, 2 * v.size))
    bound = np.spacing(ref.astype(np.float32)).astype(np.float64) + NOISE64 * np.abs(v).sum()
    return ref, bound


def spectrum_error(got32, v32):
    """max over bins of |got - ref| / bound (<= 1 passes) and the bin where it is largest."""
    ref, bound = frame_spectrum(v32)
    r = np.abs(np.asarray(got32, np.float32).astype(np.float64) - ref) / bound
    k = int(np.argmax(r))
    return float(r[k]), k


def definition_frames(W, seed):
    """The frame set of the sweeps: random normal, impulses at 0 and W-1, DC, alternating +-1, and random values whose
    magnitudes span 1e-6 .. 1e4 (small bins are then checked against their own ulp)."""
    rng = np.random.default_rng(seed)
    frames = {"normal": rng.standard_normal(W)}
    for name, at in (("impulse0", 0), ("impulseW-1", W - 1)):
        v = np.zeros(W)
        v[at] = 1.0
        frames[name] = v
    frames["dc"] = np.ones(W)
    frames["alternating"] = np.where(np.arange(W) % 2 == 0, 1.0, -1.0)
    frames["scaled"] = rng.standard_normal(W) * np.exp(rng.uniform(math.log(1e-6), math.log(1e4), W))
    return {k: v.astype(np.float32) for k, v in frames.items()}


@functools.lru_cache(maxsize=None)
def hamming(W):
    """speedy.c:256-258, 0.54 - 0.46 cos(2 pi i / (W - 1)) in double stored as float, with the cosine evaluated at 50
    digits and rounded to double (the library's tables are machine-independent the same way)."""
    with mpmath.workdps(50):
        half = [float(mpmath.cospi(mpmath.mpf(2 * i) / (W - 1))) for i in range(W // 2 + 1)]
    c = np.array([half[min(i, W - 1 - i)] for i in range(W)], np.float64)
    w = (0.54 - 0.46 * c).astype(np.float32)
    w.flags.writeable = False
    return w


def mono_mix(x16, channels):
    """soniclib.c:262-287: the integer sum over channels divided by the channel count with C's truncation toward zero
    (numpy's // floors, which differs for negative sums that are not multiples of the count)."""
    s = np.asarray(x16, np.int16).reshape(-1, channels).astype(np.int64).sum(axis=1)
    q = np.abs(s) // channels
    return np.where(s < 0, -q, q).astype(np.int16)


def n_frames(n_mono, rate):
    """Frames the shim sends for n_mono samples: frame j (samples j*B .. j*B+W-1) goes out when the sample at j*B + W has
    been written (soniclib.c:433-437: writeBufferFrameIndex >= speedyBufferFrameIndex + W/B and location == W%B + 1)."""
    W, B = window_size(rate), frame_step(rate)
    return max(0, (n_mono - W - 1) // B + 1)


def analysis_frames(x16, channels, rate):
    """The windowed float32 frames Speedy transforms for an int16 interleaved stream, shape (frames, W)."""
    W, B = window_size(rate), frame_step(rate)
    mono = mono_mix(x16, channels)
    T = n_frames(mono.size, rate)
    win = hamming(W)
    out = np.zeros((T, W), np.float32)
    state = np.float32(0.0)                      # speedy.c:217 preemph_state
    for j in range(T):
        v = (mono[j * B:j * B + W] / 32768.0).astype(np.float32)        # speedy.c:558-559, double quotient stored as float
        prev = np.concatenate([[state], v[:-1]]).astype(np.float32)
        e = (1.0 * v.astype(np.float64) - 0.97 * prev.astype(np.float64)).astype(np.float32)   # speedy.c:420-424
        state = v[-1]                            # the last raw sample of THIS window carries into the next one
        out[j] = e * win                         # speedy.c:462, float times float
    return out


def normalized_bound(spec32, W):
    """speedy.c:628-647 over the first W bins of a float32 spectrogram row: spec / (sqrt(sum_{i=1}^{W-1} spec_i^2) + eps),
    in float64, and a per-bin bound.  The reference sums the squares in float32, one after another: relative error at most
    (W - 1) * 2^-24 from the additions plus one rounding per square, so (W/2 + 4) * 2^-24 bounds the relative error of
    the square root; the quotient and its float32 store add a few more roundings, covered by the + 4."""
    s = np.asarray(spec32, np.float32)[:W].astype(np.float64)
    energy = float((s[1:W] ** 2).sum())
    ref = s / (np.sqrt(energy) + 2.2204e-16)
    return ref, (W / 2 + 4) * 2.0 ** -24 * np.abs(ref)
