"""GPU: spx_analysis_kernel<16, 240> (16 kHz, sixteen-frame tiles) as built for three workgroups per CU beside two lean walk
workgroups: its constants loaded from the plan's lane-major table at their use, mono samples read from global memory (no staged
span), the last four magnitude rows held in registers and stored over wave 0's transform buffer behind a barrier.

Results: bit-equality with the CPU oracle -- tension, speed and the fifteen features of every tension frame (they carry each frame
record's energy and spectral difference), every spectrogram row, the int16 audio -- at the smallest shapes where the changed code
can go wrong.  Resources: what the engine's mode decision is fed for the headline shape fits three analysis workgroups and two
lean walk workgroups in a SIMD's registers and a CU's LDS."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RATE, W, B = 16000, 240, 160


def _stream(frames, extra, seed):
    """int16 noise with a speech-like envelope: exactly `frames` analysis frames (spx_plan_frames: (n - W - 1) / B + 1) and
    `extra` < B samples behind the last window."""
    n = W + 1 + (frames - 1) * B + extra
    rng = np.random.default_rng([frames, extra, seed])
    env = 0.15 + 0.85 * np.abs(np.sin(np.arange(n) * (2 * np.pi / 1900.0) + seed))
    return (rng.normal(0.0, 6000.0, n) * env).clip(-32000, 32000).astype(np.int16)


def _oracle_spectrogram(orc, x, ch):
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


def _check_batch(orc, xs, ch):
    from speedy_amd.batch import Batch, Plan
    plan = Plan(RATE, False)
    b = Batch(plan, [x.size // ch for x in xs], ch, 3.5, 1.0, 0.0, taps=True, spectrogram_taps=True)
    assert any(o % 2 for o in b.in_offs) or ch == 2, b.in_offs     # odd offsets into the packed buffer
    assert b.d_in.numel() == b.total_in + 64                       # the last stream ends where the documented padding begins
    b.upload(xs)
    b.run()
    outs = b.results()
    plain = Batch(plan, [x.size // ch for x in xs], ch, 3.5, 1.0, 0.0)          # without taps: the launch a caller makes
    plain.upload(xs)
    plain.run()
    outs_plain = plain.results()
    for i, x in enumerate(xs):
        ref = orc.compress_sound(x, RATE, ch, 3.5, 1.0, 0.0, False, chunk=1000)
        taps = b.tap_arrays(i)
        for key in ("tension", "speed", "features"):
            assert taps[key].shape == ref[key].shape, (i, key, taps[key].shape, ref[key].shape)
            assert np.array_equal(taps[key], ref[key]), (i, key)
        spec = _oracle_spectrogram(orc, x, ch)
        assert taps["spectrogram"].shape == spec.shape, (i, taps["spectrogram"].shape, spec.shape)
        assert np.array_equal(taps["spectrogram"], spec), (i, np.nonzero((taps["spectrogram"] != spec).any(axis=1))[0][:8])
        assert np.array_equal(outs[i], ref["out"]), i
        assert np.array_equal(outs_plain[i], ref["out"]), i


# 1: the halo row is all zero and fifteen slots have no frame; 15 / 16 / 17: a tile's ragged tail, a full tile, one frame in a
# second tile whose halo is the previous tile's last frame; 32 / 33 likewise with tension frames that reach across the tile border
FRAMES = (1, 15, 16, 17, 32, 33)


@pytest.mark.parametrize("order", ["up", "down"])
def test_mono_streams_at_the_tile_borders(orc, order):
    """Odd lengths: every second stream starts at an odd in_off, and (order down) the one-frame stream is the packed buffer's last."""
    cases = [(f, e) for f, e in zip(FRAMES, (0, 158, 2, 76, 0, 38))]
    if order == "down":
        cases = cases[::-1]
    xs = [_stream(f, e, 7) for f, e in cases]
    assert all(x.size % 2 == 1 for x in xs)
    _check_batch(orc, xs, 1)


def test_stereo_batch_takes_the_staged_path(orc):
    """A launch with a multi-channel stream keeps the staged span (the mono mix is made in LDS): unchanged results."""
    xs = []
    for f, e in ((16, 5), (17, 0), (33, 121)):
        l, r = _stream(f, e, 1), _stream(f, e, 2)
        xs.append(np.stack([l, r], axis=1).ravel())
    _check_batch(orc, xs, 2)


def test_stream_resumed_in_the_middle_of_a_tile(orc):
    """The streaming API, one launch sequence per write: the second job begins at frame 10 and the third at frame 25 -- its first
    tile's halo slot is a frame whose samples lie in front of frame_begin.  Every tension frame's tension, speed and features
    (the frame records' energy and spectral difference are among them), every spectrogram row and the audio."""
    from speedy_amd.sonic2 import SonicStream
    x = _stream(60, 33, 3)
    full = orc.compress_sound(x, RATE, 1, 3.5, 1.0, 0.0, False, chunk=1000)
    ref = full["out"]
    taps = dict(tension=[], speed=[], features=[], spec=[])
    s = SonicStream(RATE, 1, False, coalesce=False)
    s.set_speed(3.5)
    s.enable_nonlinear(1.0)
    s.set_feedback(0.0)
    s.on_tension(lambda t, v: taps["tension"].append(v))
    s.on_speed(lambda t, v: taps["speed"].append(v))
    s.on_features(lambda t, f: taps["features"].append(f))
    s.on_spectrogram(lambda t, f: taps["spec"].append(f))
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
    n = len(full["tension"])
    assert n >= 45 and len(taps["tension"]) >= n and len(taps["speed"]) >= n and len(taps["features"]) >= n
    assert np.array_equal(np.float32(taps["tension"][:n]), full["tension"])
    assert np.array_equal(np.float32(taps["speed"][:n]), full["speed"])
    assert np.array_equal(np.array(taps["features"][:n], np.float32), full["features"])
    spec = _oracle_spectrogram(orc, x, 1)
    assert len(taps["spec"]) >= 60 and np.array_equal(np.array(taps["spec"][:spec.shape[0]], np.float32), spec)
    assert np.array_equal(np.concatenate(outs), ref)


def test_three_analysis_workgroups_fit_beside_two_lean_walk_workgroups():
    """The headline shape (256 mono streams, every job a speed-up): analysis <= 88 registers without scratch, and 2 x lean walk +
    3 x analysis within a SIMD's 512 registers and a CU's LDS -- with the LDS rounded up to the allocation granule (1280 bytes
    on a CU with 160 KiB; 512 bytes checked as well)."""
    from speedy_amd._lib import lib
    L = lib()
    res = (C.c_longlong * 22)()
    assert L.spx_debug_mode_resources(RATE, 1, 256, 1, res) == 0
    f = ["cu_count", "lds_per_cu", "walk_lds", "walk_waves", "walk_vgprs", "walk_fast", "walk_nwc", "lean_lds", "lean_waves", "lean_vgprs",
         "lean_fast", "lean_nwc", "lean_valid", "tension_lds", "tension_vgprs", "tile_default", "tile_big", "tile_small", "an_lds_default",
         "an_lds_small", "an_vgprs_default", "an_vgprs_small"]
    r = dict(zip(f, (int(v) for v in res)))
    info = (C.c_int * 4)()
    assert L.spx_debug_analysis_info(RATE, info) == 0
    assert r["tile_default"] == 16 and r["lean_valid"] == 1 and r["lean_nwc"] == 0 and r["lean_waves"] == 4, r
    assert 0 < r["an_vgprs_default"] <= 88 and info[0] == r["an_vgprs_default"] and info[1] == 0, (r, list(info))
    assert info[2] == r["an_lds_default"], (r, list(info))        # the mono launch's LDS is what the mode decision is fed
    assert 2 * r["lean_vgprs"] + 3 * r["an_vgprs_default"] <= 512, r
    assert 2 * r["lean_lds"] + 3 * r["an_lds_default"] <= r["lds_per_cu"], r
    for granule in (512, 1280):
        up = lambda v: -(-v // granule) * granule   # noqa: E731
        assert 2 * up(r["lean_lds"]) + 3 * up(r["an_lds_default"]) <= r["lds_per_cu"], (granule, r)
    # a launch with a stereo stream keeps the staged span: more LDS than the mono launch, less than two of it
    assert L.spx_debug_mode_resources(RATE, 2, 256, 1, res) == 0
    assert r["an_lds_default"] < int(res[18]) < 2 * r["an_lds_default"], (r, int(res[18]))
