"""The HIP feature chain (spx_analysis.hip phases 2 - 4, spx_tension.hip, the speed kernel: rows a6 - a9 of DESIGN.md section 1)
against the float64 definition of tests/features_ref.py, not against the oracle: every stage of every frame of the batch taps,
of the streaming callbacks and of the unit-level speedy* surface, teacher-forced with the kernels' own float32 taps.  The
bit-equality tests elsewhere say "some frame differs from the oracle"; these say WHICH stage of WHICH frame moved, by how many
bounds, and where the frame sits in its 16-frame tile and in the tension kernel's 512-frame chunk -- and they catch a mistake the
oracle shares."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import features_ref as fr  # noqa: E402
import spectrum_ref as sr  # noqa: E402
import feature_inputs as cpu  # noqa: E402
from util import read_wav  # noqa: E402

pytestmark = pytest.mark.gpu

N_STAGES = len(fr.STAGES)
WORST = fr.Worst()
T_START = time.time()


@pytest.fixture(scope="module", autouse=True)
def worst_table():
    """Prints (with -s) the worst error / bound per stage and rate over everything this module checked on the GPU."""
    yield
    print("\n\nHIP kernels, worst error / bound per stage and sample rate (%.1f s for the module)\n%s"
          % (time.time() - T_START, WORST.text()))


def checked(taps, rate, R, nl, fb, matlab, what, t0=1):
    tb = fr.check(taps, rate, R, nl, fb, matlab, t0=t0)
    K = taps["features"].shape[0]
    bad = tb.failures()
    assert not bad, "; ".join(tb.describe(s, what) for s in bad)
    assert tb.checked() == K * N_STAGES and all(tb[s]["n"] == K for s in fr.STAGES), (what, K, tb.checked())
    WORST.add(rate, tb)
    return tb


def samples_for_rows(rate, K, matlab=False):
    """The shortest mono stream with K feature rows: T = K + F - 1 analysis frames (spectrum_ref.n_frames)."""
    F, _ = fr.hysteresis_shape(matlab)
    return (K + F - 2) * sr.frame_step(rate) + sr.window_size(rate) + 1


def run_batch(streams, rate, matlab, what, concurrent=None):
    """streams: [(name, int16 interleaved, channels, R, nl, fb)] in ONE call; every stream's taps checked.  {name: table}.
    concurrent: None = whatever mode the engine picks; True / False = the concurrent three-kernel mode / the kernels in
    sequence, and the call must report that it ran in that mode (a fall-back fails instead of testing less)."""
    from speedy_amd import lib
    from speedy_amd.batch import compress_batch
    L = lib()
    if concurrent is not None:
        L.spx_set_concurrent(int(concurrent))
    try:
        _, b = compress_batch([s[1] for s in streams], rate, [s[2] for s in streams], [s[3] for s in streams],
                              [s[4] for s in streams], [s[5] for s in streams], matlab, taps=True, spectrogram_taps=True)
        mode = L.spx_debug_last_call_concurrent()
    finally:
        L.spx_set_concurrent(1)
    if concurrent is not None:
        assert mode == int(concurrent), "%s: asked for concurrent=%s, the call reports mode %d" % (what, concurrent, mode)
    out = {}
    for i, (name, x, ch, R, nl, fb) in enumerate(streams):
        taps = b.tap_arrays(i)
        assert taps["features"].shape[0] == max(0, sr.n_frames(x.size // ch, rate) + 1 - fr.hysteresis_shape(matlab)[0])
        out[name] = checked(taps, rate, R, nl, fb, matlab, "%s, %d Hz, stream %d (%s, %d channels)" % (what, rate, i, name, ch))
    return out


# the compiled-in windows, one plan-driven rate (11 025) and one Rader rate (6 467, W = 97)
RATES = [8000, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 11025, 6467]


@pytest.mark.parametrize("rate", RATES)
def test_batch_taps_of_every_input_kind(rate):
    """Speech (mono, 3 channels, 4 channels; speed-up, slow-down, interpolated, with feedback) and the branch inputs in one call
    per rate.  Each branch input asserts that it reached its branch on the GPU too."""
    from speedy_amd.synth import speech_like
    W = sr.window_size(rate)
    streams = [("speech", cpu.speech(rate), 1, 2.0, 1.0, 0.0),
               ("speech x3", cpu.speech(rate, seed=4, ch=3), 3, 0.6, 0.5, 0.1),
               ("speech x4", speech_like(int(0.9 * rate), rate, seed=5, channels=4), 4, 3.5, 1e-5, 0.5),
               ("clicks", cpu.clicks_in_silence(rate), 1, 1.5, 1.0, 0.1),
               ("quiet", cpu.speech(rate) // 300, 1, 2.0, 1.0, 0.0),
               ("square", cpu.square_wave(rate), 1, 1.0, 1.0, 0.5),
               ("noise", cpu.white_noise(rate), 1, 2.0, 0.5, 0.0),
               ("jumps", cpu.jumping_tone(rate), 1, 3.5, 1.0, 0.0)]
    tb = run_batch(streams, rate, False, "batch")
    assert tb["clicks"].low_frames >= 10 and tb["clicks"].after_low >= 3, (tb["clicks"].low_frames, tb["clicks"].after_low)
    assert tb["quiet"].low_frames == tb["quiet"]["f0"]["n"] >= 100
    assert tb["square"].f2_limited >= 5
    assert tb["noise"].max_kept >= 0.8 * (W - 1), (tb["noise"].max_kept, W)
    assert tb["jumps"].clamped >= 5, tb["jumps"].clamped


def test_batch_taps_with_the_matlab_hysteresis_shape():
    data, rate, ch = read_wav("tapestry22050.wav")
    streams = [("tapestry22050.wav", data, ch, 2.0, 1.0, 0.1), ("speech", cpu.speech(rate), 1, 0.6, 1.0, 0.0),
               ("clicks", cpu.clicks_in_silence(rate), 1, 2.0, 1.0, 0.0)]
    run_batch(streams, rate, True, "matlab shape")


@pytest.mark.parametrize("matlab", [False, True])
@pytest.mark.parametrize("name", ["tapestry.wav", "negative_speed.wav"])
def test_batch_taps_of_the_golden_wavs(name, matlab):
    data, rate, ch = read_wav(name)
    run_batch([(name, data, ch, 2.0, 1.0, 0.0 if matlab else 0.1)], rate, matlab, "golden, matlab=%s" % matlab)


# feature rows on both sides of a 16-frame tile / hand-off chunk, of the tension kernel's 512-frame LDS chunk and of several
EDGE_ROWS = [15, 16, 17, 31, 33, 511, 512, 513, 1023, 1024, 1025, 1100, 1111, 1537]


@pytest.mark.parametrize("concurrent", [False, True])
@pytest.mark.parametrize("rate", [8000, 16000])
def test_long_streams_across_tile_and_chunk_edges(rate, concurrent):
    """Streams of 15 .. 1 537 feature rows in one call, once in each launch mode -- the two kinds of edge in the tension
    kernel exclude each other.  With the kernels in sequence (concurrent=False) the tension kernel sees every frame of a stream
    at once and walks them in LDS chunks of 512: the recurrences (f1, f8, the two duration sums) are carried across frames 512,
    1 024 and 1 536.  In the concurrent mode it takes 16 new frames per pass as the analysis tiles are published: the state
    record carries the recurrences, the hysteresis window and the previous spectrum reach across every hand-off, and no
    512-frame edge is met.  Each run asserts the mode it ran in.  A failure names the frame, frame mod 16 and frame mod 512."""
    from speedy_amd.synth import speech_like
    rows = EDGE_ROWS if rate == 8000 else [17, 513, 1025, 1100]
    streams = []
    for i, K in enumerate(rows):
        n = samples_for_rows(rate, K)
        x = speech_like(n, rate, seed=20 + i)
        if i % 3 == 1:
            x[n // 3:n // 2] = 0                                  # a low run in mid-stream
        streams.append(("%d rows" % K, x, 1, [2.0, 0.6, 3.5][i % 3], 1.0, [0.0, 0.1, 0.5][i % 3]))
    tb = run_batch(streams, rate, False, "long streams, concurrent=%s" % concurrent, concurrent=concurrent)
    for K in rows:
        assert tb["%d rows" % K]["f0"]["n"] == K
    assert max(rows) >= 1100


def _stream_taps(rate, ch, x, R, nl, fb, matlab, coalesce, seed):
    from speedy_amd.sonic2 import SonicStream
    spec, feat, ten, spd = [], [], [], []
    s = SonicStream(rate, ch, match_matlab=matlab, coalesce=coalesce)
    try:
        s.set_speed(R)
        s.enable_nonlinear(nl)
        s.set_feedback(fb)
        s.on_spectrogram(lambda t, v: spec.append(v))
        s.on_features(lambda t, v: feat.append((t, v)))
        s.on_tension(lambda t, v: ten.append(v))
        s.on_speed(lambda t, v: spd.append(v))
        rng = np.random.default_rng(seed)
        pos, n = 0, x.size // ch
        while pos < n:
            c = int(rng.integers(1, 2500))
            assert s.write_short(x[pos * ch:(pos + c) * ch]) == 1
            s.read_short(8192)
            pos += c
        s.flush()
        while s.read_short(8192).size:
            pass
    finally:
        s.close()
    assert [t for t, _ in feat] == list(range(len(feat)))
    nb = 2 * sr.window_size(rate)
    return dict(spectrogram=np.array(spec, np.float32).reshape(-1, nb),
                features=np.array([v for _, v in feat], np.float32).reshape(-1, 15),
                tension=np.array(ten, np.float32), speed=np.array(spd, np.float32))


@pytest.mark.parametrize("coalesce", [False, True])
@pytest.mark.parametrize("rate,ch,matlab", [(16000, 1, False), (11025, 2, True)])
def test_streaming_callbacks_with_random_writes(rate, ch, matlab, coalesce):
    """The sonic2 callbacks with writes of random sizes: the state record (filter states, hysteresis history, skip count,
    duration sums, the previous spectrum) is carried from call to call.  Eager and pooled handles."""
    from speedy_amd.synth import speech_like
    mono = np.concatenate([cpu.clicks_in_silence(rate, 1.0), speech_like(int(1.7 * rate), rate, seed=8)])
    x = np.repeat(mono[:, None], ch, axis=1).ravel()
    R, nl, fb = (0.6, 1.0, 0.1) if matlab else (2.0, 0.5, 0.5)
    taps = _stream_taps(rate, ch, x, R, nl, fb, matlab, coalesce, seed=rate)
    tb = checked(taps, rate, R, nl, fb, matlab, "streaming, %d Hz, coalesce=%s" % (rate, coalesce))
    assert tb["f0"]["n"] == sr.n_frames(mono.size, rate) + 1 - fr.hysteresis_shape(matlab)[0] >= 250
    assert tb.low_frames >= 10 and tb.after_low >= 3


def test_unit_level_surface():
    """The speedy* functions (the one-lane hook kernels) driven as speedy_test.cc:911-935 drives them: the first frame is
    time 0, so the definition runs with t0 = 0."""
    from speedy_amd.speedy import Speedy
    from speedy_amd.synth import speech_like
    rate, R, fb = 22050, 2.0, 0.1
    x = (speech_like(int(1.5 * rate), rate, seed=6).astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    s = Speedy(rate, match_matlab=True)
    try:
        W = s.frame_size
        step = np.float32(rate / np.float32(100))
        spec, feat, ten, spd = [], [], [], []
        for t in range(int((x.size - W) / step + 1)):
            start = int(np.floor(float(np.float32(t) * step) + 0.5))
            s.add_data(x[start:start + W], t)
            spec.append(s.spectrogram())
            ok, v = s.compute_tension(len(ten))
            if ok:
                ten.append(v)
                feat.append(s.features())
                spd.append(s.speed_from_tension(v, R, fb))
    finally:
        s.close()
    taps = dict(spectrogram=np.array(spec, np.float32), features=np.array(feat, np.float32),
                tension=np.array(ten, np.float32), speed=np.array(spd, np.float32))
    tb = checked(taps, rate, R, 1.0, fb, True, "unit level", t0=0)
    assert tb["f0"]["n"] == len(spec) - 8 >= 100
