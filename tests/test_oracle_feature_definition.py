"""Every stage of every frame of the oracle's feature chain (rows a6 - a9 of DESIGN.md section 1: the fifteen feature values,
the tension, the speed) against the float64 definition of tests/features_ref.py, teacher-forced: each stage is fed the oracle's
own float32 taps of the stage before, so every gate is decided exactly and every bound is a count of roundings.  The
bit-equality tests tie the HIP kernels to the oracle; these tie the oracle to the reference's text, so that a constant, a loop
bound, a taper weight, a comparison or a time offset that both share cannot pass.

Worst error / bound per stage on this oracle (all inputs of this file; 1.0 is the bound): f0 0.15, f1 0.59, f2 0.98, f3 0.98,
f4 0.79, f6 0.03, f7 0.97, f8 0.57, f9 0.50, f11 0.15, speed 0.22 without and 0.46 with feedback; f5, f10, f12 - f14, the tension
tap and every value of a low frame exact.  profiles/feature_definition.txt holds the table per rate."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import features_ref as fr  # noqa: E402
import spectrum_ref as sr  # noqa: E402
from feature_inputs import clicks_in_silence, jumping_tone, speech, square_wave, white_noise  # noqa: E402
from util import matlab_fixture, read_wav  # noqa: E402

N_STAGES = len(fr.STAGES)
WORST = fr.Worst()


@pytest.fixture(scope="module", autouse=True)
def worst_table():
    """Prints (with -s) the worst error / bound per stage and rate over everything this module checked on the oracle."""
    yield
    print("\n\nCPU oracle, worst error / bound per stage and sample rate\n" + WORST.text())


def oracle_taps(orc, x, rate, ch=1, R=2.0, nl=1.0, fb=0.0, matlab=False, chunks=None):
    """spectrogram / features / tension / speed callbacks of one orc_sonic* stream (written, read, destroyed)."""
    L = orc.lib()
    h = L.orc_sonicCreateStream(rate, ch, int(matlab))
    nb = L.orc_sonicSpectrogramSize(h)
    spec, feat, ten, spd = [], [], [], []
    cbs = [orc.FEATURES_FN(lambda s, t, p: spec.append(np.ctypeslib.as_array(p, shape=(nb,)).copy())),
           orc.FEATURES_FN(lambda s, t, p: feat.append((t, np.ctypeslib.as_array(p, shape=(15,)).copy()))),
           orc.TENSION_FN(lambda s, t, v: ten.append(v)), orc.TENSION_FN(lambda s, t, v: spd.append(v))]
    L.orc_sonicSpectrogramCallback(h, cbs[0])
    L.orc_sonicFeaturesCallback(h, cbs[1])
    L.orc_sonicTensionCallback(h, cbs[2])
    L.orc_sonicSpeedCallback(h, cbs[3])
    L.orc_sonicSetSpeed(h, R)
    L.orc_sonicEnableNonlinearSpeedup(h, nl)
    L.orc_sonicSetDurationFeedbackStrength(h, fb)
    x = np.ascontiguousarray(x, np.int16)
    buf = np.zeros(1 << 16, np.int16)
    pos = 0
    for c in (chunks or [x.size // ch]):
        assert L.orc_sonicWriteShortToStream(h, orc.sptr(x[pos * ch:]), c) == 1
        pos += c
        while L.orc_sonicReadShortFromStream(h, orc.sptr(buf), buf.size // ch) > 0:
            pass
    L.orc_sonicDestroyStream(h)
    assert [t for t, _ in feat] == list(range(len(feat)))
    return dict(spectrogram=np.array(spec, np.float32).reshape(-1, nb),
                features=np.array([v for _, v in feat], np.float32).reshape(-1, 15),
                tension=np.array(ten, np.float32), speed=np.array(spd, np.float32))


def checked(taps, rate, R=2.0, nl=1.0, fb=0.0, matlab=False, what="", t0=1):
    """check(), the table printed, every stage asserted, the count asserted: frames x stages, nothing left out."""
    tb = fr.check(taps, rate, R, nl, fb, matlab, t0=t0)
    K = taps["features"].shape[0]
    print("\n%s: %d frames (%d low, %d right after a low one, clamp in %d, f2 > 2 in %d, most kept bins %d)" % (
        what, K, tb.low_frames, tb.after_low, tb.clamped, tb.f2_limited, tb.max_kept))
    print("  " + "  ".join("%s %.3g" % (s, tb[s]["ratio"]) for s in fr.STAGES))
    bad = tb.failures()
    assert not bad, "; ".join(tb.describe(s, what) for s in bad)
    if not what.startswith("float32 port"):
        WORST.add(rate, tb)
    assert K > 0 and tb.checked() == K * N_STAGES and all(tb[s]["n"] == K for s in fr.STAGES), (K, tb.checked())
    return tb


RATES = [6467, 8000, 11025, 16000, 22050, 44100, 48000]


@pytest.mark.parametrize("matlab", [False, True])
@pytest.mark.parametrize("rate", RATES)
def test_speech_at_every_rate_and_both_hysteresis_shapes(orc, rate, matlab):
    x = speech(rate)
    checked(oracle_taps(orc, x, rate, matlab=matlab), rate, matlab=matlab, what="speech %d Hz matlab=%s" % (rate, matlab))


def test_three_channels_and_random_write_chunking(orc):
    rate, ch = 16000, 3
    x = speech(rate, ch=ch)
    rng = np.random.default_rng(2)
    cuts, left = [], x.size // ch
    while left > 0:
        cuts.append(int(min(left, rng.integers(1, 900))))
        left -= cuts[-1]
    whole = oracle_taps(orc, x, rate, ch=ch, fb=0.1)
    cut = oracle_taps(orc, x, rate, ch=ch, fb=0.1, chunks=cuts)
    checked(whole, rate, fb=0.1, what="3 channels, one write")
    checked(cut, rate, fb=0.1, what="3 channels, %d writes" % len(cuts))
    for k in whole:
        assert whole[k].tobytes() == cut[k].tobytes(), k


@pytest.mark.parametrize("name", ["tapestry.wav", "tapestry22050.wav", "negative_speed.wav"])
def test_golden_wavs(orc, name):
    data, rate, ch = read_wav(name)
    checked(oracle_taps(orc, data, rate, ch=ch, fb=0.1), rate, fb=0.1, what=name)
    checked(oracle_taps(orc, data, rate, ch=ch, matlab=True), rate, matlab=True, what=name + " matlab")


def test_clicks_in_digital_silence(orc):
    rate = 16000
    tb = checked(oracle_taps(orc, clicks_in_silence(rate), rate), rate, what="clicks in silence")
    assert tb.low_frames >= 10 and tb.after_low >= 3, (tb.low_frames, tb.after_low)


def test_very_quiet_stream_is_low_throughout(orc):
    rate = 16000
    taps = oracle_taps(orc, speech(rate) // 300, rate)
    tb = checked(taps, rate, what="speech // 300")
    assert tb.low_frames == taps["features"].shape[0] >= 100


def test_full_scale_square_wave_reaches_the_sqrt2_limit(orc):
    rate = 16000
    taps = oracle_taps(orc, square_wave(rate), rate)
    tb = checked(taps, rate, what="square wave")
    assert tb.f2_limited >= 5, tb.f2_limited
    assert np.float32(math.sqrt(2.0)) in taps["features"][:, 3]


def test_white_noise_keeps_nearly_every_bin(orc):
    rate = 16000
    tb = checked(oracle_taps(orc, white_noise(rate), rate), rate, what="white noise")
    assert tb.max_kept >= 200, tb.max_kept


@pytest.mark.parametrize("rate", [16000, 22050])
def test_jumping_tone_drives_f9_into_the_clamp(orc, rate):
    tb = checked(oracle_taps(orc, jumping_tone(rate), rate), rate, what="jumping tone %d Hz" % rate)
    assert tb.clamped >= 5, tb.clamped


@pytest.mark.parametrize("fb", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("nl", [1.0, 0.5, 1e-5])
@pytest.mark.parametrize("R", [3.5, 1.5, 0.6, 1.0])
def test_speed_for_every_branch_of_the_speed_law(orc, R, nl, fb):
    rate = 11025
    x = speech(rate, seconds=3.0, seed=9)
    tb = checked(oracle_taps(orc, x, rate, R=R, nl=nl, fb=fb), rate, R=R, nl=nl, fb=fb, what="R=%g nl=%g fb=%g" % (R, nl, fb))
    assert tb["speed"]["n"] >= 280


# ---- the definition pinned from outside: the reference's own data, no oracle ----------------------------------------

def _definition_spectra(x, rate):
    frames = fr.unit_level_frames(x, rate)
    W = frames.shape[1]
    return np.array([sr.frame_spectrum(v)[0][:W] for v in frames])


def test_definition_passes_the_references_tension_kat():
    """speedy_test.cc:457-530 on run(): 99 frames in, 91 out, min -0.6, max 0.14273257 +- 1e-6, last -0.31351471 +- 1e-5."""
    from test_oracle_kat import _decaying_sine
    S = _definition_spectra(_decaying_sine(), 22050)
    out = fr.run(S, 2.0, 1.0, 0.0, True, t0=0)
    t = out["tension"]
    assert S.shape[0] == 99 and t.size == 91
    assert abs(t.min() - (-0.6)) < 1e-5
    assert abs(t.max() - 0.14273257553577423) < 1e-6
    assert abs(t[-1] - (-0.31351470947265625)) < 1e-5


def test_definition_passes_the_references_matlab_fixture():
    """speedy_test.cc:859-1057 on run() over the definition's own float64 spectra of tapestry22050.wav: the reference's best
    delays and SNR thresholds per feature (the list of tests/test_oracle_matlab_fixture.py), without the oracle.  The frames are
    those of the reference test's own loop (features_ref.unit_level_frames: step 220.5, first frame at time 0), windowed and
    transformed by spectrum_ref; the shim's framing (step 220, first frame at time 1) misses every delay by one frame and the
    thresholds with it, as it would with the reference's own code."""
    from test_oracle_matlab_fixture import _xcorr
    exp_feat = matlab_fixture()["features"]
    data, rate, ch = read_wav("tapestry22050.wav")
    x = (data.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    S = _definition_spectra(x, rate)
    feat = fr.run(S, 2.0, 1.0, 0.0, True, t0=0)["features"]
    assert S.shape[0] == 314 and feat.shape[0] == 306
    feature_list = [("Spectrogram energy", 0, 2e5), ("Energy Lowpass", 8, 7e5), ("Energy Local", 8, 4e4),
                    ("Energy Compressed", 8, 9e5), ("Energy Hysteresis", 0, 320), ("Low Energy Frame", 0, 1e8),
                    ("Local Spectral Difference", 0, 19), ("Emphasis Weighted Local Difference", 0, 29),
                    ("Emphasis Weighted Lowpass Filter", -1, 2300), ("Relative Spectral Difference", 0, 28),
                    ("Speech Changes", 0, 7), ("Audio Tension", 0, 8)]
    for k, (name, best_delay, thr) in enumerate(feature_list):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = _xcorr(list(feat[:, k]), list(exp_feat[:, k]), 10)
        r = [(-1 if (v != v) else v) for v in r]
        best = int(np.argmax(r))
        assert best - 10 == best_delay, (name, best - 10, r[best])
        assert r[best] > thr, (name, r[best])


# ---- teeth: a plain float32 port with the slips a kernel or the oracle could really make ----------------------------

def impl32(spec, R, nl, fb, matlab, slip=""):
    """The chain in float32 with C's evaluation order (speedy.c, soniclib.c), for spectra of times 1 .. T.  Unslipped it must
    pass check(); `slip` names one deliberate mistake."""
    f32, f64 = np.float32, np.float64
    S = np.asarray(spec, f32)
    T, W = S.shape[0], S.shape[1] // 2
    F, P = fr.hysteresis_shape(matlab)
    K = max(0, T + 1 - F)
    alpha = f32(math.exp(-1.0 / (99.0 if slip == "f1 alpha" else 100.0)))
    alpha8 = f32(math.exp(-1.0 / 100.0))
    eps = f32(2.2204e-16)

    def lp(a, state, x):
        return f32(f32((f32(1) - a) * f32(x)) + f32(a * state))

    def energy(row):
        sq = row[1:W] * row[1:W]
        if slip == "f0 drops a bin":
            sq = np.delete(sq, W // 2)
        return np.cumsum(sq, dtype=f32)[-1]

    def at(t):
        return S[t - 1] if 1 <= t <= T else np.zeros(2 * W, f32)

    st = f32(2.14204)
    f1, f2, f3 = {}, {}, {}
    for t in range(1, T + 1):
        e = energy(S[t - 1])
        st = lp(alpha, st, e)
        f1[t], f2[t] = st, f32(e / st)
        f3[t] = f32(math.sqrt(f64(min(f2[t], f32(2)))))
    feat = np.zeros((K, 15), f32)
    speed = np.zeros(K, f32)
    f8 = f32(123.837)
    cur = des = f32(0)
    Rf, nlf, fbf = f32(R), f32(nl), f32(fb)
    for k in range(K):
        r = feat[k]
        tt = k + F + (1 if slip == "f1 - f3 one row late" and k + F + 1 <= T else 0)
        r[1], r[2], r[3], r[12], r[13] = f1[tt], f2[tt], f3[tt], k + F, k
        halves = []
        for n, sign in ((F, 1), (P, -1)):
            best = f32(0)
            for i in range(n + 1):
                w = f32(f32(n - i) / f32(n + 1 if slip == "f4 taper" else n))
                v = f32(f3.get(k + sign * i, f32(0)) * w)
                best = max(best, v)
            halves.append(best)
        r[4] = f32(f64(f32(halves[0] + halves[1])) / 2.0)
        row, last = at(k), at(k - 1)
        r[0] = energy(row)
        r[14] = f32(0.04 * f64(f32(1.41421)))
        low = (r[0] < r[14] if slip == "f5 <" else r[0] <= r[14]) or k == 0
        r[5] = low
        if low:
            f8 = lp(alpha8, f8, 0)
        else:
            thr = f32(f64(row[1:W].max()) / 100.0)
            keep = np.zeros(2 * W, bool)
            keep[1:W] = ((row[1:W] >= thr) & (last[1:W] >= thr)) if slip == "bin gate >=" else ((row[1:W] > thr) & (last[1:W] > thr))
            n1 = row * f32(1.0 / (math.sqrt(f64(r[0])) + f64(eps)))
            n0 = last * f32(1.0 / (math.sqrt(f64(energy(last))) + f64(eps)))
            terms = np.abs(np.log(((n1[keep] + eps) / (n0[keep] + eps)).astype(f64)))
            acc = f32(0)
            for v in terms:
                acc = f32(f64(acc) + v)
            r[6] = acc
            r[7] = f32(r[6] * r[4])
            f8 = lp(alpha8, f8, r[7])
            r[9] = f32(f64(r[7]) / (f64(f8) + (0.011 if slip == "f9 mean" else 0.01) * f64(f32(123.979))))
            r[10] = min(r[9], f32(4) * f32(0.971975))
        r[8] = f8
        r[11] = f32(f32(f32(0.5) * f32(r[4] - f32(0.7))) + f32(f32(0.25) * f32(r[10] - f32(1))))
        if Rf > 1.0:
            s = f32(max(1.0, f64(f32(Rf + f32(f32(f32(1) - Rf) * r[11])))))
        else:
            s = f32(max(0.01, min(1.0, f64(f32(Rf - f32(f32(f32(1) - Rf) * r[11]))))))
        if fbf > 0:
            s = f32(f64(s) + max(0.01, f64(f32(fbf * f32(cur - des)))))
        fd = f32(1.0 / 100.0)
        cur, des = f32(cur + f32(fd / s)), f32(des + f32(fd / Rf))
        speed[k] = f32(f32(s * nlf) + f32(Rf * f32(f32(1) - nlf)))
    taps = dict(spectrogram=S, features=feat, tension=feat[:, 11].copy(), speed=speed)
    if slip == "spectrogram one row late":
        taps["spectrogram"] = np.concatenate([S[:1], S[:-1]])
    return taps


@pytest.fixture(scope="module")
def real_spectra(orc):
    rate = 16000
    return rate, oracle_taps(orc, speech(rate), rate)["spectrogram"]


def tie_spectra(W, rows=60):
    """Spectra made of quarters: the peak of each row is 25, 50 or 75, so max / 100 is exact and many bins EQUAL the threshold."""
    rng = np.random.default_rng(5)
    S = np.zeros((rows, 2 * W), np.float32)
    S[:, 1:W] = rng.integers(1, 13, (rows, W - 1)) * 0.25
    S[np.arange(rows), rng.integers(1, W, rows)] = 25.0 * rng.integers(1, 4, rows)
    return S


def threshold_energy_spectra(W, rows=48):
    """Noise rows, and from row 20 on two-bin rows whose float32 energy EQUALS the low-energy threshold 0.04 * 1.41421f."""
    target = np.float32(0.04 * float(np.float32(1.41421)))
    a = np.float32(math.sqrt(float(target) / 2))
    pair = None
    for i in range(-4000, 4000):
        p = np.nextafter(a, np.float32(1), dtype=np.float32) if i == 0 else np.float32(a + np.float32(i) * np.spacing(a))
        for j in range(-40, 40):
            q = np.float32(a + np.float32(j) * np.spacing(a))
            if np.float32(np.float32(p * p) + np.float32(q * q)) == target:
                pair = (p, q)
                break
        if pair:
            break
    assert pair, "no float pair reaches the threshold energy"
    S = tie_spectra(W, rows)
    S[20:] = 0
    S[20:, 3], S[20:, 7] = pair
    return S


def test_the_unslipped_float32_port_passes(real_spectra):
    rate, S = real_spectra
    for matlab, fb, R, nl in ((False, 0.0, 2.0, 1.0), (True, 0.1, 0.6, 0.5)):
        checked(impl32(S, R, nl, fb, matlab), rate, R=R, nl=nl, fb=fb, matlab=matlab, what="float32 port")
    W = sr.window_size(rate)
    tb = checked(impl32(tie_spectra(W), 2.0, 1.0, 0.0, False), rate, what="float32 port, threshold ties")
    assert tb.max_kept >= 100
    tb = checked(impl32(threshold_energy_spectra(W), 2.0, 1.0, 0.0, False), rate, what="float32 port, energy == threshold")
    assert tb.low_frames >= 10


# (the slip, the spectra it shows on, the stage that must fail, the least factor over its bound), each floor derived for W = 240:
#   f4 taper       every weight moves by 1 / (F + 1) of itself, f4 by 1 / 13 of itself against 2 u: 6.4e5, floor 5e5
#   f1 alpha       f1 moves by (alpha' - alpha) (f1[k-1] - e) = 1.005e-4 |f1[k-1] - e| against 3 u f1; in a frame with f2 > 2
#                  (asserted below) e > 2 f1 and f1[k-1] < f1, so |f1[k-1] - e| > f1: 1.005e-4 / 3 u = 562, floor 500
#   bin gate >=    each kept tie adds its whole |log| term.  A row of quarters 1 .. 12 has (W - 1) / 12 = 20 bins equal to
#                  the threshold on average, at least half with a previous bin >= it, mean |log| of a ratio of two such
#                  values 0.7: >= 7 against g (W + 10) u + (g + 1) u f6 = 5e-3 (g = 200, f6 = 160): 1.4e3, floor 1e3
#   f5 <           an exact stage: any difference is infinitely many bounds
#   f9 mean        the denominator f8 + 1.24 moves by 0.124; f8 <= 123.837 at the start, so f9 moves by >= 0.124 / 125.2 =
#                  9.9e-4 of itself against 2 u: 8.3e3, floor 8e3
#   rows one late  the value is its neighbour's: speech energies differ by tens of per cent from frame to frame against
#                  (W + 2) u = 1.4e-5 (f0) and 3 u with a weight of 1 - alpha = 1e-2 (f1: 1e-3 / 1.8e-7): floors 1e4 and 5e3
#   f0 drops a bin the mean share of a bin is 1 / (W - 1) of the energy against (W + 2) u: 290 in a frame where the dropped
#                  bin holds the mean share or more, floor 250
SLIPS = [("f4 taper", "real", "f4", 5e5), ("f1 alpha", "real", "f1", 500.0), ("bin gate >=", "ties", "f6", 1e3),
         ("f5 <", "threshold", "f5", math.inf), ("f9 mean", "real", "f9", 8e3), ("f1 - f3 one row late", "real", "f1", 5e3),
         ("spectrogram one row late", "real", "f0", 1e4), ("f0 drops a bin", "real", "f0", 250.0)]


@pytest.mark.parametrize("slip,spectra,stage,factor", SLIPS)
def test_a_real_slip_fails_at_its_stage(real_spectra, slip, spectra, stage, factor):
    rate, S = real_spectra
    W = sr.window_size(rate)
    S = {"real": S, "ties": tie_spectra(W), "threshold": threshold_energy_spectra(W)}[spectra]
    tb = fr.check(impl32(S, 2.0, 1.0, 0.0, False, slip), rate, 2.0, 1.0, 0.0, False)
    bad = tb.failures()
    print("\n%-26s fails %s" % (slip, ", ".join("%s x %.3g (frame %d)" % (s, e["ratio"], e["frame"]) for s, e in bad.items())))
    assert stage in bad and bad[stage]["ratio"] >= factor, (slip, stage, tb[stage])
    if slip == "f1 alpha":
        assert tb.f2_limited >= 1              # the frame the floor was derived for exists
    if slip == "f5 <":
        assert bad["f5"]["frame"] >= 21          # the first row whose energy equals the threshold is time 21
