"""GPU: spx_analysis_kernel<16, 240> untangles the packed transform in conjugate pairs -- one lane takes bins p and 240 - p from
the two points Z[p], Z[240 - p] they share (p = lane and lane + 64 up to 120; bins 0 and 120 pair with themselves), with one
untangle factor per pair (tests/test_untangle_table.py: the other is its mirror image bit for bit).  Which lane computes a bin,
where it stores it (at once, or for a wave's last slot -- rows 13 .. 16 -- from registers behind a barrier) and which factor it
multiplies by all changed; no value may.

Every spectrogram row against the CPU oracle's, bit for bit, at 16 kHz for streams of 1, 2, 15, 16, 17, 33 and 100 frames -- a
tile with empty slots, a full tile, the halo slot taken from the previous tile -- and for a stream resumed in the middle of a tile
(the streaming API).  Inputs: silence, a full-scale square wave, an impulse at sample 0 and at sample 239, noise.  Each batch once
as mono int16 streams (the kernel reads its samples from global memory) and once with a stereo stream in the launch (the staged
span in LDS).  Bins 0, 1, 119, 120, 121 and 239 are asserted by name before the whole row: they are lane 0's two passes' ends,
the self-paired bins and their neighbours, and a failure says which pairing broke.  Tension, speed and the fifteen features of
every tension frame (they carry each frame record's energy and spectral difference) and the int16 audio likewise."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RATE, W, B = 16000, 240, 160
FRAMES = (1, 2, 15, 16, 17, 33, 100)
KINDS = ("silence", "square", "impulse0", "impulse239", "noise")
NAMED_BINS = (0, 1, 119, 120, 121, 239)

_REF = {}


def signal(kind, frames):
    """int16, exactly `frames` analysis frames ((n - W - 1) / B + 1) and a few samples behind the last window."""
    n = W + 1 + (frames - 1) * B + 37
    x = np.zeros(n, np.int16)
    if kind == "square":
        x[:] = np.where((np.arange(n) // 23) % 2 == 0, 32767, -32767)
    elif kind == "impulse0":
        x[0] = 32767
    elif kind == "impulse239":
        x[239] = 32767
    elif kind == "noise":
        x[:] = np.random.default_rng([frames, 11]).integers(-32768, 32768, n).astype(np.int16)
    return x


def oracle_spectrogram(orc, x, ch):
    L = orc.lib()
    rows = []
    h = L.orc_sonicCreateStream(RATE, ch, 0)
    nb = L.orc_sonicSpectrogramSize(h)
    cb = orc.FEATURES_FN(lambda s, t, p: rows.append(np.ctypeslib.as_array(p, shape=(nb,)).copy()))
    L.orc_sonicSpectrogramCallback(h, cb)
    L.orc_sonicSetSpeed(h, 3.5)
    L.orc_sonicEnableNonlinearSpeedup(h, 1.0)
    L.orc_sonicWriteShortToStream(h, orc.sptr(x), x.size // ch)
    L.orc_sonicDestroyStream(h)
    return np.array(rows, np.float32).reshape(len(rows), nb)


def reference(orc, key, x, ch):
    """The oracle's taps, audio and spectrogram rows of one stream: computed once, shared by the two launches that use it."""
    if key not in _REF:
        ref = orc.compress_sound(x, RATE, ch, 3.5, 1.0, 0.0, False, chunk=1000)
        ref["spectrogram"] = oracle_spectrogram(orc, x, ch)
        _REF[key] = ref
    return _REF[key]


def assert_rows(got, ref, what):
    assert got.shape == ref.shape and ref.shape[1] == 2 * W, (what, got.shape, ref.shape)
    g, r = got.view(np.uint32), ref.view(np.uint32)
    for k in NAMED_BINS:
        bad = np.nonzero(g[:, k] != r[:, k])[0]
        assert bad.size == 0, "%s: bin %d differs from the oracle in rows %s" % (what, k, bad[:8])
        if k > 0:
            bad = np.nonzero(g[:, 2 * W - k] != r[:, 2 * W - k])[0]
            assert bad.size == 0, "%s: bin %d's mirror %d differs from the oracle in rows %s" % (what, k, 2 * W - k, bad[:8])
    bad = np.nonzero(g[:, W] != r[:, W])[0]
    assert bad.size == 0, "%s: bin 240 (stored with bin 0) differs from the oracle in rows %s" % (what, bad[:8])
    rows, cols = np.nonzero(g != r)
    assert rows.size == 0, "%s: %d values differ from the oracle, first (row, bin) %s" % (what, rows.size, list(zip(rows[:6], cols[:6])))


def check_launch(orc, streams, ch):
    """streams: [(key, int16 samples)]; ch: channels per stream.  One plain call with every tap."""
    from speedy_amd.batch import Batch, Plan
    plan = Plan(RATE, False)
    xs = [x for _, x in streams]
    b = Batch(plan, [x.size // c for x, c in zip(xs, ch)], ch, 3.5, 1.0, 0.0, taps=True, spectrogram_taps=True)
    b.upload(xs)
    b.run()
    outs = b.results()
    for i, (key, x) in enumerate(streams):
        ref = reference(orc, key, x, ch[i])
        taps = b.tap_arrays(i)
        assert_rows(taps["spectrogram"], ref["spectrogram"], "%s (stream %d, %d channel(s))" % (key, i, ch[i]))
        for name in ("tension", "speed", "features"):
            assert taps[name].shape == ref[name].shape, (key, name, taps[name].shape, ref[name].shape)
            assert taps[name].tobytes() == ref[name].tobytes(), (key, name)
        assert np.array_equal(outs[i], ref["out"]), (key, "audio")
    plan.close()


def mono_streams():
    return [("%s, %d frames" % (kind, f), signal(kind, f)) for f in FRAMES for kind in KINDS]


def test_mono_launch_reads_global_memory(orc):
    streams = mono_streams()
    assert sorted({(x.size - W - 1) // B + 1 for _, x in streams}) == list(FRAMES)
    check_launch(orc, streams, [1] * len(streams))


def test_launch_with_a_stereo_stream_takes_the_staged_span(orc):
    streams = mono_streams()
    l, r = signal("noise", 33), signal("square", 33)
    streams.insert(len(streams) // 2, ("stereo noise | square, 33 frames", np.stack([l, r], axis=1).ravel()))
    ch = [2 if key.startswith("stereo") else 1 for key, _ in streams]
    check_launch(orc, streams, ch)


def test_stream_resumed_in_the_middle_of_a_tile(orc):
    """The streaming API, one launch sequence per write: the second job begins at frame 10 and the third at frame 25, so a tile's
    halo slot is a frame whose samples lie in front of the job's first frame."""
    from speedy_amd.sonic2 import SonicStream
    x = signal("noise", 100)
    ref = reference(orc, "noise, 100 frames", x, 1)
    rows = []
    s = SonicStream(RATE, 1, False, coalesce=False)
    s.set_speed(3.5)
    s.enable_nonlinear(1.0)
    s.set_feedback(0.0)
    s.on_spectrogram(lambda t, f: rows.append(f))
    outs, pos = [], 0
    for n in (W + 1 + 9 * B + 19, 15 * B, x.size):      # 10 frames, 25 frames, the rest
        seg = x[pos:pos + n]
        assert s.write_short(seg) == 1
        pos += seg.size
        outs.append(s.read_short(100000))
    s.flush()
    while True:
        got = s.read_short(100000)
        if got.size == 0:
            break
        outs.append(got)
    s.close()
    assert pos == x.size
    spec = ref["spectrogram"]
    assert len(rows) >= spec.shape[0] == 100
    assert_rows(np.array(rows[:spec.shape[0]], np.float32), spec, "resumed stream")
    assert np.array_equal(np.concatenate(outs), ref["out"])
