"""spx_batch_run_rate on the MI355X: a playback rate per stream (sonicSetRate before the first write) in ONE batch call.

Every comparison is bit-exact -- bytes and counts, no tolerance.  The expected output of a job is the oracle STREAM
(tests/test_batch_rate_abi.py oracle_rate_stream: create, set speed / rate / nonlinear / feedback, writes of 1000 frames each
followed by reads until 0, flush, reads until 0); that file also shows that this output does not depend on the chunking.

The rate kernel divides by the new sample rate with the plain integer division: there is no reciprocal whose equality with the
division would have to be checked exhaustively."""
import ctypes as C
import os
import subprocess
import sys
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_batch_rate_abi import oracle_rate_stream  # noqa: E402
from util import read_wav  # noqa: E402

pytestmark = pytest.mark.gpu

SPEEDS = [(3.5, 1.0), (2.0, 0.0), (1.5, 0.6), (1.0, 0.0), (0.7, 0.0), (0.5, 1.0)]
RATES = [0.5, 0.8, 1.25, 2.0]
CANARY = 0x5a5a   # an int16 pattern no kernel writes on purpose


def _bc(v, n):
    return np.broadcast_to(np.asarray(v, np.float32), (n,))


def _oracles(orc, streams, rate_hz, ch, speed, nl, rate, mm=False, feedback=0.0):
    """The oracle stream of every job (the oracle is plain C behind ctypes: threads run it side by side)."""
    n = len(streams)
    ch, speed, nl, rate, feedback = (np.broadcast_to(np.asarray(ch, np.int32), (n,)), _bc(speed, n), _bc(nl, n), _bc(rate, n),
                                     _bc(feedback, n))
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(lambda i: oracle_rate_stream(orc, streams[i], rate_hz, int(ch[i]), float(speed[i]), float(nl[i]),
                                                        float(rate[i]), mm, float(feedback[i])), range(n)))


def _counts(b):
    import torch
    torch.cuda.synchronize(b.device)
    return b.d_nout.cpu().numpy().copy()


def _outputs(b, nout=None):
    """Per-stream outputs without moving the whole (capacity-sized) buffer to the host."""
    nout = _counts(b) if nout is None else nout
    assert (nout >= 0).all(), "capacity exceeded / lost producer: %s" % nout
    res = []
    for i in range(b.n):
        k = int(nout[i]) * int(b.channels[i])
        assert int(nout[i]) <= b.out_caps[i]
        res.append(b.d_out[b.out_offs[i]:b.out_offs[i] + k].cpu().numpy().copy())
    return res


def _assert_equal(got, want, what=""):
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.size == w.size, "%s stream %d: %d values, the oracle has %d" % (what, i, g.size, w.size)
        assert np.array_equal(g, w), "%s stream %d differs from the oracle (first at %d of %d)" % (
            what, i, int(np.nonzero(g != w)[0][0]), g.size)


_BASE = {}


def _base(rate_hz, ch):
    """One long speech-like signal per (sample rate, channels); the streams of a batch are slices of it."""
    from speedy_amd.synth import speech_like
    key = (rate_hz, ch)
    if key not in _BASE:
        n = 7 * rate_hz
        _BASE[key] = np.stack([speech_like(n, rate_hz, seed=500 + 17 * ch + c) for c in range(ch)], axis=1).reshape(-1)
    return _BASE[key]


def _ragged(rate_hz, ch, W, B, shift):
    """Ten ragged streams: 0, 1, 2 frames, one frame short of an analysis window, exactly one window, a few frames more, and
    longer ones up to more than 5 s."""
    lengths = [0, 1, 2, W, W + 1, 3 * B + 5, 1000 + shift, rate_hz // 3 + 7 * shift, rate_hz + 11, 5 * rate_hz + 37 + shift]
    x = _base(rate_hz, ch)
    streams, pos = [], shift * 13
    for n in lengths:
        streams.append(x[pos * ch:(pos + n) * ch].copy())
        pos += n // 5 + 3
    return lengths, streams


@pytest.mark.parametrize("ch", [1, 2, 3])
@pytest.mark.parametrize("rate_hz", [8000, 16000, 22050, 44100])
def test_single_shape_batches_match_the_oracle_stream(orc, rate_hz, ch):
    """Sample rate x channels x (speed, nonlinear) x rate, ten ragged streams each; both hysteresis modes on a subset, feedback
    0 and 0.1 by turns.  Counts stay inside spx_plan_out_capacity_rate (Batch sizes its buffers with it)."""
    from speedy_amd.batch import Batch, Plan
    plans = {False: Plan(rate_hz, False), True: Plan(rate_hz, True)}
    try:
        k = 0
        for (speed, nl) in SPEEDS:
            for rate in RATES:
                k += 1
                mm = nl != 0.0 and rate == 1.25
                fb = 0.1 if (k % 2 == 0 and nl != 0.0) else 0.0
                plan = plans[mm]
                lengths, streams = _ragged(rate_hz, ch, plan.W, plan.B, k)
                b = Batch(plan, lengths, ch, speed, nl, fb, rate=rate)
                b.upload(streams)
                b.run()
                got = _outputs(b)
                want = _oracles(orc, streams, rate_hz, ch, speed, nl, rate, mm, fb)
                assert want[-1].size // ch > lengths[-1] / (2.0 * max(speed, 1.0) * rate), "the oracle produced next to nothing"
                _assert_equal(got, want, "%d Hz x %d, speed %g nl %g rate %g mm %d fb %g:" % (rate_hz, ch, speed, nl, rate, mm, fb))
                del b
    finally:
        for p in plans.values():
            p.close()


@pytest.mark.parametrize("ch", [16, 20])
def test_many_channels(orc, ch):
    """The batched kernel carries no per-channel record: the 16 channels of the streaming API's rate stage are no limit here."""
    from speedy_amd.batch import Batch, Plan
    from speedy_amd.synth import speech_like
    plan = Plan(16000, False)
    try:
        lengths = [4000, 1, 9000]
        streams = [speech_like(n, 16000, seed=70 + i, channels=ch) for i, n in enumerate(lengths)]
        b = Batch(plan, lengths, ch, 2.0, 1.0, 0.0, rate=[0.8, 1.25, 2.0])
        b.upload(streams)
        b.run()
        _assert_equal(_outputs(b), _oracles(orc, streams, 16000, ch, 2.0, 1.0, [0.8, 1.25, 2.0]), "%d channels:" % ch)
    finally:
        plan.close()


def test_a_rate_per_stream_300_streams(orc):
    """One call, more streams than CUs, a different rate / speed / nonlinear factor per stream and rate 1 among them: every stream
    is its own oracle stream, and the rate-1 streams are byte for byte what spx_batch_run gives the same jobs."""
    from speedy_amd.batch import Batch, Plan
    n = 300
    plan = Plan(16000, False)
    try:
        x = _base(16000, 1)
        rng = np.random.default_rng(7)
        lengths = [int(v) for v in rng.integers(4000, 28000, n)]
        lengths[5], lengths[17] = 0, 2
        streams = [x[(37 * i) % 60000:(37 * i) % 60000 + lengths[i]].copy() for i in range(n)]
        rates = np.asarray([[1.0, 0.5, 0.8, 1.25, 2.0, 1.1, 3.0][i % 7] for i in range(n)], np.float32)
        sp = np.asarray([SPEEDS[i % 6][0] for i in range(n)], np.float32)
        nl = np.asarray([SPEEDS[i % 6][1] for i in range(n)], np.float32)
        b = Batch(plan, lengths, 1, sp, nl, 0.0, rate=rates)
        b.upload(streams)
        b.run()
        got = _outputs(b)
        _assert_equal(got, _oracles(orc, streams, 16000, 1, sp, nl, rates), "300 streams:")
        p = Batch(plan, lengths, 1, sp, nl, 0.0)
        p.upload(streams)
        p.run()
        plain = _outputs(p)
        ones = [i for i in range(n) if rates[i] == 1.0]
        assert len(ones) >= 40
        for i in ones:
            assert np.array_equal(got[i], plain[i]), "rate-1 stream %d differs from spx_batch_run" % i
    finally:
        plan.close()


def _tap_bytes(b):
    import torch
    torch.cuda.synchronize(b.device)
    return [t.cpu().numpy().tobytes() for t in (b.t_tension, b.t_speed, b.t_features, b.t_spec, b.t_norm)]


def _job_set():
    lengths = [16000, 0, 33333, 241, 52000, 8000]
    x = _base(16000, 1)
    return lengths, [x[1000 * i:1000 * i + n].copy() for i, n in enumerate(lengths)]


def test_no_rates_and_all_ones_are_spx_batch_run():
    """rates = NULL and a table of ones: output buffer, counts and taps byte-equal to spx_batch_run's."""
    import torch
    from speedy_amd.batch import Batch, Plan
    plan = Plan(16000, False)
    try:
        lengths, streams = _job_set()
        sp, nl = [3.5, 2.0, 0.7, 3.5, 1.5, 0.5], [1.0, 0.0, 0.0, 1.0, 0.6, 1.0]
        p = Batch(plan, lengths, 1, sp, nl, 0.0, taps=True, spectrogram_taps=True)
        p.upload(streams)
        p.run()
        want = (_counts(p), p.d_out.cpu().numpy().copy(), _tap_bytes(p))
        o = Batch(plan, lengths, 1, sp, nl, 0.0, taps=True, spectrogram_taps=True, rate=1.0)
        o.upload(streams)
        o.run()
        assert np.array_equal(_counts(o), want[0]) and np.array_equal(o.d_out.cpu().numpy(), want[1]) and _tap_bytes(o) == want[2]
        # NULL: through the C entry point itself, on a plain batch's buffers
        z = Batch(plan, lengths, 1, sp, nl, 0.0, taps=True, spectrogram_taps=True)
        z.upload(streams)
        L = plan.L
        assert L.spx_batch_workspace_bytes_rate(plan.h, z.jobs, None, z.n) == L.spx_batch_workspace_bytes(plan.h, z.jobs, z.n)
        rc = L.spx_batch_run_rate(plan.h, z.jobs, None, z.n, z.d_in.data_ptr(), z.d_out.data_ptr(), z.d_nout.data_ptr(),
                                  z.d_ws.data_ptr(), z.d_ws.numel(), C.byref(z.taps), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, L.spx_last_error()
        assert np.array_equal(_counts(z), want[0]) and np.array_equal(z.d_out.cpu().numpy(), want[1]) and _tap_bytes(z) == want[2]
        for n_in, s, f in ((16000, 3.5, 1.0), (5000, 0.5, 1.0), (0, 0.7, 0.0)):
            assert L.spx_plan_out_capacity_rate(plan.h, n_in, s, f, 1.0) == L.spx_plan_out_capacity_for(plan.h, n_in, s, f)
    finally:
        plan.close()


def test_taps_of_a_rate_call_are_those_of_spx_batch_run():
    """The rate stage lies behind everything the taps observe."""
    from speedy_amd.batch import Batch, Plan
    plan = Plan(16000, False)
    try:
        lengths, streams = _job_set()
        sp, nl = [3.5, 2.0, 0.7, 3.5, 1.5, 0.5], [1.0, 0.0, 0.0, 1.0, 0.6, 1.0]
        p = Batch(plan, lengths, 1, sp, nl, 0.1, taps=True, spectrogram_taps=True)
        p.upload(streams)
        p.run()
        r = Batch(plan, lengths, 1, sp, nl, 0.1, taps=True, spectrogram_taps=True, rate=[1.25, 0.5, 2.0, 1.0, 0.8, 1.25])
        r.upload(streams)
        r.run()
        assert (_counts(r) >= 0).all()
        assert _tap_bytes(r) == _tap_bytes(p)
        assert any(np.frombuffer(t, np.uint8).any() for t in _tap_bytes(p))
    finally:
        plan.close()


def test_out_cap_too_small_is_reported_and_respected(orc):
    """out_cap cut below the produced count: n_out is negative and a canary behind out_off + out_cap * channels is untouched;
    the neighbours with room are unharmed."""
    import torch
    from speedy_amd.batch import Batch, Plan
    plan = Plan(16000, False)
    try:
        ch = 2
        lengths = [20000, 30000, 12000, 30000]
        x = _base(16000, ch)
        streams = [x[2000 * i * ch:(2000 * i + n) * ch].copy() for i, n in enumerate(lengths)]
        rates = [1.25, 0.5, 2.0, 0.8]
        want = _oracles(orc, streams, 16000, ch, 2.0, 1.0, rates)
        full = [w.size // ch for w in want]
        b = Batch(plan, lengths, ch, 2.0, 1.0, 0.0, rate=rates)
        b.upload(streams)
        cut = {1: full[1] - 1, 3: full[3] // 2 + 3}
        for i, cap in cut.items():
            assert 0 < cap < full[i]
            b.jobs[i].out_cap = cap
        b.d_out.fill_(CANARY)
        b.run()
        nout = _counts(b)
        out = b.d_out.cpu().numpy()
        for i in range(b.n):
            lo = b.out_offs[i]
            hi = b.out_offs[i + 1] if i + 1 < b.n else out.size
            if i in cut:
                assert nout[i] < 0, "stream %d: n_out %d with out_cap %d of %d" % (i, nout[i], cut[i], full[i])
                assert (out[lo + cut[i] * ch:hi] == CANARY).all(), "stream %d wrote past out_off + out_cap * channels" % i
                assert np.array_equal(out[lo:lo + cut[i] * ch], want[i][:cut[i] * ch])
            else:
                assert nout[i] == full[i] and np.array_equal(out[lo:lo + full[i] * ch], want[i])
                assert (out[lo + full[i] * ch:hi] == CANARY).all()
        torch.cuda.synchronize()
    finally:
        plan.close()


def test_bad_rates_are_refused_before_anything_is_launched():
    """Rate 0, -1, NaN, +inf and a rate so large that (int)(sample rate / rate) < 1: -1 and a message, buffers untouched."""
    import torch
    from speedy_amd.batch import Batch, Plan
    plan = Plan(16000, False)
    try:
        lengths, streams = _job_set()
        b = Batch(plan, lengths, 1, 3.5, 1.0, 0.0, rate=1.25)
        b.upload(streams)
        L = plan.L
        for bad in (0.0, -1.0, float("nan"), float("inf"), 1.0e6):
            b.d_out.fill_(CANARY)
            b.d_nout.fill_(-77)
            b.rates = np.ascontiguousarray(np.full(b.n, 1.25, np.float32))
            b.rates[3] = bad
            with pytest.raises(RuntimeError) as e:
                b.run()
            assert "rate" in str(e.value), str(e.value)
            rc = L.spx_batch_run_rate(plan.h, b.jobs, b._rates_ptr(), b.n, b.d_in.data_ptr(), b.d_out.data_ptr(), b.d_nout.data_ptr(),
                                      b.d_ws.data_ptr(), b.d_ws.numel(), None, torch.cuda.current_stream().cuda_stream)
            assert rc == -1 and L.spx_last_error()
            torch.cuda.synchronize()
            assert bool((b.d_out == CANARY).all()) and bool((b.d_nout == -77).all()), "rate %r: a refused call wrote its buffers" % bad
            assert L.spx_batch_workspace_bytes_rate(plan.h, b.jobs, b._rates_ptr(), b.n) == 0
            assert L.spx_plan_out_capacity_rate(plan.h, 16000, 3.5, 1.0, bad) == -1
        # ... and a good rate on a job whose SPEED is refused: the message names the speed (nobody sizes a buffer from it first)
        b.rates = np.ascontiguousarray(np.full(b.n, 1.25, np.float32))
        b.jobs[3].speed = float("nan")
        b.d_out.fill_(CANARY)
        b.d_nout.fill_(-77)
        rc = L.spx_batch_run_rate(plan.h, b.jobs, b._rates_ptr(), b.n, b.d_in.data_ptr(), b.d_out.data_ptr(), b.d_nout.data_ptr(),
                                  b.d_ws.data_ptr(), b.d_ws.numel(), None, torch.cuda.current_stream().cuda_stream)
        assert rc == -1 and "speed" in L.spx_last_error().decode(), L.spx_last_error()
        torch.cuda.synchronize()
        assert bool((b.d_out == CANARY).all()) and bool((b.d_nout == -77).all()), "speed NaN: a refused call wrote its buffers"
        assert L.spx_batch_workspace_bytes_rate(plan.h, b.jobs, b._rates_ptr(), b.n) == 0
        assert "speed" in L.spx_last_error().decode()
        assert L.spx_plan_out_capacity_rate(plan.h, 16000, float("nan"), 0.0, 1.25) == -1
    finally:
        plan.close()


def test_the_same_buffers_call_after_call(orc):
    """Five calls on one workspace / out / n_out, two rate tables by turns: each call's result is its own oracle's."""
    from speedy_amd.batch import Batch, Plan
    plan = Plan(22050, False)
    try:
        ch = 1
        lengths = [22050, 3, 40000, 15000, 0, 30011, 9000, 26000]
        x = _base(22050, ch)
        streams = [x[500 * i:500 * i + n].copy() for i, n in enumerate(lengths)]
        sp = [3.5, 2.0, 1.5, 0.7, 1.0, 3.5, 2.0, 1.5]
        nl = [1.0, 0.0, 0.6, 0.0, 0.0, 1.0, 1.0, 0.0]
        tables = [np.asarray([1.25, 0.8, 1.0, 2.0, 0.5, 1.0, 0.8, 1.25], np.float32),
                  np.asarray([0.5, 1.0, 2.0, 1.0, 1.25, 0.8, 1.0, 0.5], np.float32)]
        want = [_oracles(orc, streams, 22050, ch, sp, nl, t) for t in tables]
        # buffers sized for both tables: the smaller rate of the two has the larger capacity, and a stream whose rate is 1 in one
        # table only still needs its share of the workspace (a rate just below 1 asks for both)
        lo = np.minimum(tables[0], tables[1])
        b = Batch(plan, lengths, ch, sp, nl, 0.0, rate=np.where(lo == 1.0, np.float32(0.999), lo))
        b.upload(streams)
        for call in range(5):
            b.rates = np.ascontiguousarray(tables[call % 2])
            b.run()
            _assert_equal(_outputs(b), want[call % 2], "call %d:" % call)
    finally:
        plan.close()


def test_bench_shape_with_rate_1_25(orc):
    """BASELINE configs[3]'s shape -- 256 streams x 10 s, 16 kHz mono, 3.5x nonlinear, the bench's own inputs -- at rate 1.25: count
    and CRC-32 of every stream against the oracle stream."""
    from speedy_amd.batch import Batch, Plan
    sys.path.insert(0, ROOT)
    import bench
    n = 10 * bench.RATE
    streams = bench.make_streams(bench.STREAMS_PER_GPU, n, 0)
    assert len(streams) == 256 and bench.RATE == 16000
    plan = Plan(bench.RATE, False)
    try:
        b = Batch(plan, [n] * len(streams), 1, 3.5, 1.0, 0.0, rate=1.25)
        b.upload(streams)
        b.run()
        got = _outputs(b)
        want = _oracles(orc, streams, bench.RATE, 1, 3.5, 1.0, 1.25)
        bad = [i for i in range(len(streams))
               if got[i].size != want[i].size or zlib.crc32(got[i].tobytes()) != zlib.crc32(want[i].tobytes())]
        assert not bad, "streams %s differ from the oracle stream" % bad[:8]
        assert min(w.size for w in want) > 20000
        # spx_batch_pack_outputs and spx_batch_read_steps work on the result unchanged
        packed, offsets = b.pack_outputs()
        offs = offsets.cpu().numpy()
        pk = packed.cpu().numpy()
        for i in (0, 100, 255):
            assert np.array_equal(pk[offs[i]:offs[i + 1]], want[i])
        assert (b.step_counts() > 100).all()
    finally:
        plan.close()


def test_c_example_prints_the_oracles_counts_and_crcs(orc, tmp_path):
    """tools/batch_rate_example.c (plain C99 over include/speedy_hip.h): one call, one stream per playback rate."""
    exe = os.path.join(ROOT, "speedy_amd", "lib", "batch_rate_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "rateexample"])
    x, rate_hz, ch = read_wav("tapestry.wav")
    x = x[: 3 * rate_hz * ch]
    raw = str(tmp_path / "in.raw")
    x.astype("<i2").tofile(raw)
    rates = [1.0, 1.25, 0.5, 2.0]
    r = subprocess.run([exe, raw, str(rate_hz), str(ch), "3.5", "1.0"] + [str(v) for v in rates], capture_output=True, text=True,
                       timeout=180)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("stream ")]
    assert len(lines) == len(rates), r.stdout
    for i, v in enumerate(rates):
        ref = oracle_rate_stream(orc, x, rate_hz, ch, 3.5, 1.0, v)
        assert int(lines[i][1]) == i and int(lines[i][5]) == ref.size // ch, (lines[i], ref.size // ch)
        assert int(lines[i][7], 16) == zlib.crc32(ref.astype("<i2").tobytes()), lines[i]
