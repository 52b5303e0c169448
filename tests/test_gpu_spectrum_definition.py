"""The HIP analysis kernels against the float64 spectrum definition (tests/spectrum_ref.py), not against the oracle: every
window size the library accepts through the plan-driven kernel, and the int16 path through every analysis instantiation
the batch taps reach.  The bit-equality tests elsewhere tie the kernels to the oracle; these catch a mistake both share."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrum_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

RATE_LO, RATE_HI = 1000, 127999


def _window_rate_ends():
    """{W: (lowest rate, highest rate)} over the accepted rates."""
    ends = {}
    for rate in range(RATE_LO, RATE_HI + 1):
        W = sr.window_size(rate)
        lo, _ = ends.get(W, (rate, rate))
        ends[W] = (lo, rate)
    return ends


def _plan_class(L, rate):
    """(analysis tile frames, transforming waves, Rader?, instantiation of the int16 path) of the plan of `rate`."""
    from speedy_amd.batch import Plan
    res = (C.c_longlong * 22)()
    assert L.spx_debug_mode_resources(rate, 1, 1, 0, res) == 0, rate
    info = (C.c_int * 4)()
    assert L.spx_debug_analysis_info(rate, info) == 0, rate
    plan = Plan(rate, False)
    try:
        inst = L.spx_batch_kernel_names(plan.h, 1, 1, 0).decode().split(";")[0]
    finally:
        plan.close()
    return int(res[15]), int(info[3]), sr.rader_window(sr.window_size(rate)), inst


@pytest.fixture(scope="module")
def plan_classes():
    """{rate: class} for the lowest and the highest rate of every window size: 3 810 plans."""
    from speedy_amd import lib
    L = lib()
    t0 = time.time()
    out = {}
    for W, (lo, hi) in sorted(_window_rate_ends().items()):
        for rate in (lo, hi):
            out[rate] = _plan_class(L, rate)
    print("\nplan classes of %d plans: %.1f s" % (len(out), time.time() - t0))
    return out


def test_plan_driven_kernel_at_every_window_size(plan_classes):
    """speedySpectrogram (spx_launch_analysis_frames: the plan-driven kernel with the plan's tile and transforming waves) on
    the frame set of the CPU sweep, at the lowest and the highest rate of every W = 15 .. 1919, against |DFT_2W| in float64
    -- every bin within one float32 ulp plus the float64 noise floor.  Every W creates a plan; every class met (tile,
    waves, Rader or not, instantiation) is met at both ends of a window's rate range."""
    from speedy_amd.speedy import Speedy
    ends = _window_rate_ends()
    assert sorted(ends) == list(range(15, 1920))
    t0 = time.time()
    worst = (0.0, None)
    for W, (lo, hi) in sorted(ends.items()):
        win = sr.hamming(W)
        frames = sr.definition_frames(W, W)
        refs = {name: (v * win, sr.frame_spectrum(v * win)) for name, v in frames.items()}
        for rate in (lo, hi):
            s = Speedy(rate, match_matlab=False)
            try:
                assert (s.frame_size, s.fft_size) == (W, 2 * W), rate
                for name, v in frames.items():
                    got = s.spectrogram(v).astype(np.float64)
                    ref, bound = refs[name][1]
                    r = np.abs(got - ref) / bound
                    k = int(np.argmax(r))
                    assert r[k] <= 1.0, "rate=%d W=%d class=%s frame=%s bin=%d: %.3g bounds off (got %r, want %r)" % (
                        rate, W, plan_classes[rate], name, k, r[k], got[k], ref[k])
                    worst = max(worst, (float(r[k]), (rate, W, name, k)))
            finally:
                s.close()
    dt = time.time() - t0
    table = {}
    for W, (lo, hi) in sorted(ends.items()):
        for end, rate in (("lo", lo), ("hi", hi)):
            e = table.setdefault(plan_classes[rate], {"lo": [], "hi": []})
            e[end].append(rate)
    print("\nspectrum sweep: %d plans x %d frames in %.1f s; worst error / bound %.3f at (rate, W, frame, bin) = %s"
          % (2 * len(ends), 6, dt, worst[0], worst[1]))
    print("%-6s %-5s %-6s %-28s %-16s %s" % ("tile", "waves", "rader", "instantiation", "rates", "windows (lo / hi ends)"))
    for cls, e in sorted(table.items()):
        rates = e["lo"] + e["hi"]
        print("%-6d %-5d %-6s %-28s %6d..%-8d %d / %d" % (cls[0], cls[1], cls[2], cls[3], min(rates), max(rates),
                                                        len(e["lo"]), len(e["hi"])))
    for cls, e in table.items():
        assert e["lo"] and e["hi"], ("class met at one end of the window ranges only", cls, e)
    assert {c[:3] for c in table} >= {(16, 4, False), (16, 4, True), (8, 4, False), (4, 1, False)}


def _tile_boundaries(plan_classes):
    """One rate on each side of every change of (tile, transforming waves) along the rate axis."""
    rates = sorted(plan_classes)
    out = []
    for a, b in zip(rates, rates[1:]):
        if plan_classes[a][:2] != plan_classes[b][:2]:
            out += [a, b]
    return out


# The int16 path: (rate, instantiation the case claims to cover).  Tile-class boundaries are added from the plan sweep.
INT16_RATES = [(8000, "spx_analysis_kernel<16, 120>"), (11025, "spx_analysis_kernel<16, 0>"),
               (12000, "spx_analysis_kernel<16, 180>"), (16000, "spx_analysis_kernel<16, 240>"),
               (22050, "spx_analysis_kernel<16, 330>"), (24000, "spx_analysis_kernel<16, 360>"),
               (32000, "spx_analysis_kernel<16, 480>"), (44100, "spx_analysis_kernel<8, 661>"),
               (48000, "spx_analysis_kernel<8, 720>"), (6467, "spx_analysis_kernel<16, 0>"),   # W = 97: plan-driven Rader
               (127999, "spx_analysis_kernel<4, 0>")]


def _widest_channel_count(L, rate, n_streams):
    """64 channels where the walk kernel's LDS window holds them (the TSM stage's limit, not the analysis'), else the most
    that fit (spx_batch_run refuses a batch whose walk window exceeds one CU's 160 KiB)."""
    res = (C.c_longlong * 22)()
    for ch in (64, 48, 32, 24, 16, 8, 4):
        assert L.spx_debug_mode_resources(rate, ch, n_streams, 1, res) == 0, rate
        if res[2] <= 160 * 1024:
            return ch
    raise AssertionError("no multi-channel batch fits at %d Hz" % rate)


def _int16_streams(rate, tf, seed, wide):
    """(interleaved int16 stream, channels) of every input kind, of different lengths; `wide` channels for the widest."""
    from speedy_amd.synth import speech_like
    W, B = sr.window_size(rate), sr.frame_step(rate)
    rng = np.random.default_rng(seed)
    tile_len = tf * B                                        # samples between the first frames of two tiles
    n = 2 * tile_len + W + 3 * B + 7                         # a partial last tile
    out = [(speech_like(int(0.55 * rate) + 13, rate, seed=seed), 1)]
    runs = np.repeat(np.where(np.arange(40) % 2 == 0, -32768, 32767), rng.integers(1, 3 * W, 40))[:n]
    out.append((runs.astype(np.int16), 1))
    quiet = np.zeros(n + 5, np.int16)
    quiet[n // 2:] = rng.integers(-1, 2, n + 5 - n // 2)       # digital silence, then a 1-LSB signal
    out.append((quiet, 1))
    imp = np.zeros(n + B, np.int16)
    imp[tile_len] = 32767                                    # the first sample of tile 1's first frame
    imp[tile_len + (tf - 1) * B + W - 1] = -32768            # the last sample of tile 1's last frame
    imp[0] = -32768
    out.append((imp, 1))
    for ch in (2, 3, wide):
        m = rng.integers(-3000, 2000, (n + 3 * ch, 1))
        x = m + rng.integers(-ch, 1, (m.shape[0], ch))       # channel sums mostly negative, every residue modulo ch
        out.append((np.clip(x, -32768, 32767).astype(np.int16).ravel(), ch))
    sp = speech_like(n - 9, rate, seed=seed + 1).astype(np.int32)
    out.append((np.stack([sp, -sp], axis=1).clip(-32767, 32767).astype(np.int16).ravel(), 2))   # a pair that cancels
    out.append((speech_like(W - 5, rate, seed=seed + 2), 1))                                     # shorter than a window
    return out


def _check_stream_taps(taps, x, ch, rate, what):
    W = sr.window_size(rate)
    frames = sr.analysis_frames(x, ch, rate)
    spec = taps["spectrogram"]
    assert spec.shape == (frames.shape[0], 2 * W), (what, spec.shape, frames.shape)
    for j in range(frames.shape[0]):
        err, k = sr.spectrum_error(spec[j], frames[j])
        assert err <= 1.0, "%s: frame %d bin %d, %.3g bounds off" % (what, j, k, err)
    # the normalised spectrogram of tension frame k is that of the spectrogram stamped with time k: the shim stamps
    # analysis frame j with time j + W/B (soniclib.c:298-299, the write index when the frame goes out)
    lag = W // sr.frame_step(rate)
    norm = taps["normalized"]
    for k in range(norm.shape[0]):
        if k < lag:
            assert not norm[k].any(), (what, k)
            continue
        ref, bound = sr.normalized_bound(spec[k - lag], W)
        assert np.all(np.abs(norm[k].astype(np.float64) - ref) <= bound), "%s: normalized row %d" % (what, k)


@pytest.fixture(scope="module")
def int16_cases(plan_classes):
    cases = [(r, inst, "named") for r, inst in INT16_RATES]
    for r in _tile_boundaries(plan_classes):
        cases.append((r, plan_classes[r][3], "tile boundary %s" % (plan_classes[r][:2],)))
    return cases


def test_int16_taps_through_every_analysis_instantiation(plan_classes, int16_cases):
    """compress_batch(..., spectrogram_taps=True): the compiled-in windows, the 16 / 8 / 4-frame tiles, the tile halo frame,
    the pre-emphasis carry into each tile, the mono mix -- every bin of every frame of every stream against spectrum_ref's
    framing and |DFT_2W|, the normalised tap against the float32 normalisation bound.  Several streams of different
    lengths in one batch (per-stream tap offsets).  Each case asserts the instantiation it claims to cover."""
    from speedy_amd import lib
    from speedy_amd.batch import Plan, compress_batch
    L = lib()
    seen = set()
    print()
    for rate, inst, why in int16_cases:
        tf = int(inst.split("<")[1].split(",")[0])
        streams = _int16_streams(rate, tf, seed=rate % 1009, wide=_widest_channel_count(L, rate, 9))
        chans = [c for _, c in streams]
        plan = Plan(rate, False)
        try:
            got = L.spx_batch_kernel_names(plan.h, len(streams), max(chans), 0).decode().split(";")[0]
        finally:
            plan.close()
        assert got == inst, (rate, why, got, inst)
        seen.add(got)
        _, b = compress_batch([x for x, _ in streams], rate, chans, 2.0, 1.0, 0.0, False, taps=True, spectrogram_taps=True)
        for i, (x, ch) in enumerate(streams):
            _check_stream_taps(b.tap_arrays(i), x, ch, rate, "rate %d (%s), stream %d, %d channels" % (rate, why, i, ch))
        print("int16 taps: %6d Hz  %-28s %-30s channels %s" % (rate, got, why, sorted(set(chans))))
    names = {inst for _, inst in INT16_RATES} | {plan_classes[r][3] for r in _tile_boundaries(plan_classes)}
    assert seen == names


@pytest.mark.parametrize("rate", [16000, 6467])
def test_streaming_spectrogram_callback_with_random_chunks(rate):
    """The sonic2 spectrogram callback with writes of random sizes (the pre-emphasis carry and the framing across writes),
    at 16 kHz (a compiled-in window) and at 6.467 kHz (W = 97, plan-driven Rader)."""
    from speedy_amd.sonic2 import SonicStream
    from speedy_amd.synth import speech_like
    x = speech_like(int(1.3 * rate) + 3, rate, seed=5)
    rows = []
    s = SonicStream(rate, 1)
    try:
        s.set_speed(2.0)
        s.enable_nonlinear(1.0)
        s.on_spectrogram(lambda t, v: rows.append(v))
        rng = np.random.default_rng(rate)
        pos = 0
        while pos < x.size:
            c = int(rng.integers(1, 900))
            assert s.write_short(x[pos:pos + c]) == 1
            s.read_short(4096)
            pos += c
        s.flush()
        while s.read_short(4096).size:
            pass
    finally:
        s.close()
    frames = sr.analysis_frames(x, 1, rate)
    assert len(rows) == frames.shape[0], (len(rows), frames.shape)
    for j, row in enumerate(rows):
        err, k = sr.spectrum_error(row, frames[j])
        assert err <= 1.0, (rate, j, k, err)
