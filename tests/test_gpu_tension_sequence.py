"""spx_tension_seq_kernel (speedy_amd/csrc/spx_tension_seq.hip: the tension pass of every launch without tile flags -- one pass
over LDS rings, the three recurrences on three waves) against spx_tension_kernel, bit for bit, and against the oracle.

The new kernel walks its slots in blocks of 64 through rings of 512 (SPX_TSQ_BLK, SPX_TSQ_RING); slot = frame + 1 in a batch job.
The frame counts below sit on both sides of a block, of the ring's wrap and of the hysteresis reach (F future, Pp past frames).
spx_set_tension_form(1) makes every launch take the old kernel: the same library runs both sides of each comparison."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import features_ref as fr  # noqa: E402

pytestmark = pytest.mark.gpu

BLK, RING = 64, 512
SPEEDS, NLS, FBS = [3.5, 1.5, 0.8], [1.0, 0.5], [0.0, 0.1]


def n_samples(frames, rate=16000):
    """The shortest stream of `frames` analysis frames: (n - 1) steps and one window + 1; 0 frames: too short for one."""
    B, W = rate // 100, int(1.5 * rate / 100)
    return (frames - 1) * B + W + 1 if frames > 0 else W // 2


def frame_counts(matlab):
    F, Pp = fr.hysteresis_shape(matlab)
    return [0, 1, F - 1, F, F + 1, F + Pp + 1, 63, 64, 65, 127, 128, 129,
            RING - BLK, RING - 1, RING, RING + 1, RING + BLK, 2 * RING + F + Pp + 3]


def edge_batch(matlab):
    """[(int16 samples, channels, speed, nonlinear, feedback)]: every frame count, speeds on both sides of 1, interpolated and
    linear streams, both feedback settings, one all-zero stream."""
    from speedy_amd.synth import speech_like
    jobs = []
    for i, n in enumerate(frame_counts(matlab)):
        jobs.append((speech_like(n_samples(n), 16000, seed=300 + i), 1, SPEEDS[(i + 1) % 3], NLS[(i // 3) % 2], FBS[i % 2]))
    jobs.append((speech_like(n_samples(200), 16000, seed=340), 1, 3.5, 0.0, 0.0))            # linear: the kernel returns at once
    jobs.append((speech_like(n_samples(90), 16000, seed=341), 1, 0.8, 0.0, 0.1))
    jobs.append((np.zeros(n_samples(300), np.int16), 1, 3.5, 1.0, 0.0))                        # the gate closed on every frame
    jobs.append((np.zeros(n_samples(70), np.int16), 1, 0.8, 1.0, 0.1))
    return jobs


def stereo_batch():
    from speedy_amd.synth import speech_like
    rate = 22050
    return [(speech_like(n_samples(150, rate), rate, seed=350, channels=2), 2, 3.5, 1.0, 0.0),
            (speech_like(n_samples(65, rate), rate, seed=351), 1, 0.8, 0.5, 0.1),
            (speech_like(n_samples(RING + 1, rate), rate, seed=352, channels=2), 2, 1.5, 1.0, 0.1)]


def run(jobs, rate, matlab, form, concurrent=0, chunks=None, spec=False):
    """One plain call under spx_set_tension_form(form): (outputs, taps per stream, step counts, the form that ran)."""
    from speedy_amd import lib
    from speedy_amd.batch import compress_batch
    L = lib()
    try:
        L.spx_set_concurrent(concurrent)
        L.spx_set_tension_form(form)
        if chunks is not None:
            L.spx_set_pipeline_chunks(chunks)
        outs, b = compress_batch([j[0] for j in jobs], rate, [j[1] for j in jobs], [j[2] for j in jobs], [j[3] for j in jobs],
                                 [j[4] for j in jobs], matlab, taps=True, spectrogram_taps=spec)
        ran = L.spx_debug_last_tension_form()
        steps = b.step_counts()
        taps = [b.tap_arrays(i) for i in range(len(jobs))]
    finally:
        L.spx_set_tension_form(0)
        L.spx_set_concurrent(1)
        if chunks is not None:
            L.spx_set_pipeline_chunks(1)
    return outs, taps, steps, ran


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same_run(new, old, what):
    (o0, t0, s0, r0), (o1, t1, s1, r1) = new, old
    assert (r0, r1) == (1, 0), (what, r0, r1)     # spx_tension_seq_kernel, spx_tension_kernel
    assert np.array_equal(s0, s1), what
    for i in range(len(o0)):
        assert same_bits(o0[i], o1[i]), (what, "audio / n_out", i)
        for k in ("features", "tension", "speed"):
            assert same_bits(t0[i][k], t1[i][k]), (what, k, i, np.nonzero(t0[i][k].ravel().view(np.uint32) !=
                                                                             t1[i][k].ravel().view(np.uint32))[0][:8])


_RUNS = {}


def edge_runs(matlab):
    if matlab not in _RUNS:
        jobs = edge_batch(matlab)
        _RUNS[matlab] = (jobs, run(jobs, 16000, matlab, 0, spec=True), run(jobs, 16000, matlab, 1, spec=True))
    return _RUNS[matlab]


@pytest.mark.parametrize("matlab", [False, True])
def test_both_kernels_bit_for_bit(matlab):
    jobs, new, old = edge_runs(matlab)
    from speedy_amd.batch import Plan
    plan = Plan(16000, matlab)
    F = plan.F
    for (x, ch, _, nl, _), n, t in zip(jobs, frame_counts(matlab), new[1]):
        assert plan.frames(x.size // ch) == n and t["features"].shape[0] == max(0, n - F + 1), n
    plan.close()
    assert_same_run(new, old, "edge batch, matlab=%s" % matlab)


def test_stereo_22050_bit_for_bit():
    jobs = stereo_batch()
    assert_same_run(run(jobs, 22050, False, 0), run(jobs, 22050, False, 1), "22.05 kHz, stereo and mono")


def check_oracle(jobs, rate, matlab, result, what):
    from oracle import pyorc
    pyorc.build()
    outs, taps, _, _ = result
    for i, (x, ch, R, nl, fb) in enumerate(jobs):
        ref = pyorc.compress_sound(x, rate, ch, R, nl, fb, matlab, taps=nl != 0)
        assert np.array_equal(outs[i], ref["out"]), (what, "audio", i)
        if nl == 0:
            continue
        K = taps[i]["features"].shape[0]
        assert ref["speed"].size == K, (what, i, K, ref["speed"].size)
        for k in ("speed", "tension", "features"):
            assert same_bits(taps[i][k], ref[k]), (what, k, i)
        if K:
            tb = fr.check(taps[i], rate, R, nl, fb, matlab)
            assert not tb.failures(), "; ".join(tb.describe(s, "%s, stream %d" % (what, i)) for s in tb.failures())


@pytest.mark.parametrize("matlab", [False, True])
def test_new_kernel_against_the_oracle_and_the_definition(matlab):
    jobs, new, _ = edge_runs(matlab)
    assert new[3] == 1
    check_oracle(jobs, 16000, matlab, new, "edge batch, matlab=%s" % matlab)


def test_stereo_22050_against_the_oracle():
    jobs = stereo_batch()
    new = run(jobs, 22050, False, 0, spec=True)
    assert new[3] == 1
    check_oracle(jobs, 22050, False, new, "22.05 kHz")


@pytest.mark.parametrize("chunks", [2, 3])
def test_resumed_jobs_of_time_chunks(chunks):
    """300 streams of 2 s in 2 and 3 time chunks: every chunk after the first is a job with frame_begin > 0, which loads the
    compressed energies of the F + Pp frames before it and carries the three recurrences in the state record."""
    from speedy_amd.synth import speech_like
    base = [speech_like(32000 + 160 * i, 16000, seed=400 + i) for i in range(10)]
    jobs = [(base[i % 10][: 32000 - 160 * (i // 10)], 1, SPEEDS[i % 3], NLS[i % 2], FBS[(i // 2) % 2]) for i in range(300)]
    new = run(jobs, 16000, False, 0, chunks=chunks)
    old = run(jobs, 16000, False, 1, chunks=chunks)
    assert_same_run(new, old, "%d time chunks" % chunks)


def plain_form1(plan, lens, ch, speeds, nl, fb, xs):
    """The plain call with the old kernel: the reference of every pipelined path."""
    from speedy_amd.batch import Batch
    L = plan.L if hasattr(plan, "L") else plan[0].L
    try:
        L.spx_set_tension_form(1)
        b = Batch(plan, lens, ch, speeds, nl, fb)
        b.upload(xs)
        b.run()
        outs = b.results()
        assert L.spx_debug_last_tension_form() == 0
    finally:
        L.spx_set_tension_form(0)
    return outs


def test_pipeline_of_depth_3_with_three_job_tables():
    import torch
    from speedy_amd.batch import Pipeline, Plan
    from speedy_amd.synth import speech_like
    rate, n, lane = 16000, 256, 17600
    plan = Plan(rate, False)
    rng = np.random.default_rng(7)
    base = [speech_like(lane, rate, seed=500 + i) for i in range(12)]
    tables = [([lane] * n, [3.5] * n, 1.0, 0.0),
              ([int(v) for v in rng.integers(3200, lane + 1, n)], [SPEEDS[int(v)] for v in rng.integers(0, 2, n)], 1.0, 0.1),
              ([0 if i % 5 == 2 else int(v) for i, v in enumerate(rng.integers(3200, lane + 1, n))], [1.5] * n, 0.5, 0.0)]
    pipe = Pipeline(plan, [lane] * n, 1, 3.5, 1.0, 0.0, depth=3, device_out=True)
    xs = [[base[(i + k) % 12][: tab[0][i]] for i in range(n)] for k, tab in enumerate(tables)]
    want = [plain_form1(plan, tab[0], 1, tab[1], tab[2], tab[3], xs[k]) for k, tab in enumerate(tables)]
    dev = []
    for k, tab in enumerate(tables):
        d = torch.zeros(pipe.total_in + 64, dtype=torch.int16, device="cuda")
        d[: pipe.total_in] = torch.from_numpy(pipe.pack(xs[k], tab[0])).cuda()
        dev.append(d)
    torch.cuda.synchronize()
    tickets, forms = [], []
    for k, tab in enumerate(tables):
        tickets.append(pipe.submit_jobs(dev[k], tab[0], speed=tab[1], nonlinear=tab[2], feedback=tab[3]))
        forms.append(plan.L.spx_debug_last_tension_form())
    assert forms == [1, 1, 1], forms
    for k in range(3):
        outs = pipe.results(tickets[k])
        for i in range(n):
            assert same_bits(outs[i], want[k][i]), (k, i)
    pipe.close()
    plan.close()


def test_two_ahead_calls_on_two_workspaces():
    from speedy_amd.batch import Batch, Plan
    from speedy_amd.synth import speech_like
    rate, n = 16000, 256
    plan = Plan(rate, False)
    base = [speech_like(20000, rate, seed=520 + i) for i in range(9)]
    sets = []
    for k in range(2):
        lens = [20000 - 160 * ((i + 3 * k) % 17) for i in range(n)]
        xs = [base[(i + k) % 9][: lens[i]] for i in range(n)]
        speeds, fb = [SPEEDS[(i + k) % 2] for i in range(n)], FBS[k]
        sets.append((lens, xs, speeds, fb, plain_form1(plan, lens, 1, speeds, 1.0, fb, xs)))
    bs = []
    for lens, xs, speeds, fb, _ in sets:
        b = Batch(plan, lens, 1, speeds, 1.0, fb)
        b.upload(xs)
        bs.append(b)
    forms = []
    for b in bs:
        b.run_ahead()
        forms.append(plan.L.spx_debug_last_tension_form())
    assert forms == [1, 1], forms
    for b, s in zip(bs, sets):
        for i, o in enumerate(b.results()):
            assert same_bits(o, s[4][i]), i
    plan.close()


def test_mixed_rate_call():
    from speedy_amd import lib
    from speedy_amd.batch import MixedBatch, Plan
    from speedy_amd.synth import speech_like
    plans = [Plan(16000, False), Plan(22050, False)]
    n = 24
    pidx = [i % 2 for i in range(n)]
    rates = [16000, 22050]
    lens = [n_samples(60 + 37 * i, rates[pidx[i]]) for i in range(n)]
    xs = [speech_like(lens[i], rates[pidx[i]], seed=540 + i) for i in range(n)]
    speeds, nls, fbs = [SPEEDS[i % 3] for i in range(n)], [NLS[(i // 2) % 2] for i in range(n)], [FBS[(i // 4) % 2] for i in range(n)]
    L = lib()
    res = []
    for form in (0, 1):
        try:
            L.spx_set_tension_form(form)
            mb = MixedBatch(plans, pidx, lens, 1, speeds, nls, fbs, taps=True)
            mb.upload(xs)
            mb.run()
            res.append((mb.results(), [mb.tap_arrays(i) for i in range(n)], mb.step_counts(), L.spx_debug_last_call_concurrent()))
        finally:
            L.spx_set_tension_form(0)
    for i in range(n):
        assert same_bits(res[0][0][i], res[1][0][i]), i
        for k in ("features", "tension", "speed"):
            assert same_bits(res[0][1][i][k], res[1][1][i][k]), (k, i)
    assert np.array_equal(res[0][2], res[1][2])
    for p in plans:
        p.close()


def test_streaming_and_unit_level_calls_keep_the_old_kernel():
    """Neither goes through the batch engine's run_impl: spx_debug_last_tension_form() stays what a batch call left it."""
    from speedy_amd import lib
    from speedy_amd.sonic2 import SonicStream
    from speedy_amd.speedy import Speedy
    from speedy_amd.synth import speech_like
    L = lib()
    x = speech_like(16000, 16000, seed=560)
    for form in (0, 1):
        _, _, _, ran = run([(x, 1, 3.5, 1.0, 0.0)], 16000, False, form)
        assert ran == 1 - form
        s = SonicStream(16000, 1)
        s.set_speed(3.5)
        s.enable_nonlinear(1.0)
        s.write_short(x)
        s.flush()
        assert s.read_short(16000).size > 0
        s.close()
        assert L.spx_debug_last_tension_form() == ran
        u = Speedy(16000, False)
        xf = (x / 32768.0).astype(np.float32)
        for t in range(20):
            u.add_data(xf[t * u.frame_step: t * u.frame_step + u.frame_size], t)
        ok, _ = u.compute_tension(0)
        assert ok
        u.close()
        assert L.spx_debug_last_tension_form() == ran
