"""spx_batch_run_float on the MI355X: batch jobs on FLOAT samples in device memory, converted on the GPU.

Every comparison is bit-exact -- int16 bytes, counts, and the float output as uint32 patterns; no tolerance.  The expected output of
a job is the oracle FLOAT stream (tests/test_batch_float_abi.py oracle_float_stream); that file also shows that it is the oracle
short stream on the numpy definition of the input conversion (float_to_short_def), divided by 32767."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_batch_float_abi import float_to_short_def, oracle_float_stream  # noqa: E402
from util import read_wav  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY16 = 0x5a5a            # an int16 pattern no kernel writes on purpose
CANARY32 = 0x7fc05a5a        # a float pattern (a NaN) no conversion produces
LENGTHS = [0, 1, 7, 8, 9, 2047, 2048, 2049, 4103]
SLOT = 4296                  # values per placement slot: the longest vector + both offsets' room, a multiple of 8


def _hs():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _specials():
    """+-0, +-1, +-0.99999994, the neighbours of k / 32768 and k / 32767 around k = 0, 1, 32767, 32768 (the value and one ulp to
    either side: the products straddle the integer), +-1.5, +-65536, +-6.6e4, +-1e10, +-inf, NaN, denormals, 4096 randoms."""
    f = np.float32
    v = [0.0, -0.0, 1.0, -1.0, 0.99999994, -0.99999994, 1.5, -1.5, 65536.0, -65536.0, 6.6e4, -6.6e4, 1e10, -1e10,
         np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38, 1.17549435e-38]
    for scale in (32768.0, 32767.0):
        for k in (0, 1, 32767, 32768):
            for h in (-0.5, 0.0, 0.5):
                c = f((k + h) / scale)
                for w in (np.nextafter(c, f(-np.inf)), c, np.nextafter(c, f(np.inf))):
                    v += [float(w), -float(w)]
    rng = np.random.default_rng(2024)
    x = np.concatenate([np.asarray(v, f), rng.uniform(-1.0, 1.0, 4096).astype(f)])
    assert max(LENGTHS) <= x.size <= SLOT - 32 and x.size - 4096 < 2047   # every special value lies inside the lengths from 2047 up
    return x


def test_float_to_short_matches_the_definition_at_every_length_and_offset():
    """spx_float_to_short, both scales, on the special values: every length x destination offset 0..7 values x source offset 0..3
    values into larger buffers; the destination buffer as a whole -- canaries around every result included -- is what the
    definition gives."""
    import torch
    from speedy_amd._lib import lib
    L = lib()
    x = _specials()
    cases = [(n, d, s) for n in LENGTHS + [x.size] for d in range(8) for s in range(4)]   # (... and the whole vector)
    srcs = []
    for s in range(4):   # (a torch allocation is at least 256-byte aligned: the vector at offset s is 4 s bytes off a 16-byte boundary)
        t = torch.zeros(x.size + 8, dtype=torch.float32, device="cuda")
        t[s:s + x.size] = torch.from_numpy(x)
        srcs.append(t)
    for nl in (1, 0):
        want = np.full(len(cases) * SLOT, CANARY16, np.int16)
        dst = torch.full((len(cases) * SLOT,), CANARY16, dtype=torch.int16, device="cuda")
        assert dst.data_ptr() % 16 == 0
        q = float_to_short_def(x, bool(nl))
        for k, (n, d, s) in enumerate(cases):
            at = k * SLOT + 16 + d
            want[at:at + n] = q[:n]
            rc = L.spx_float_to_short(srcs[s].data_ptr() + 4 * s, dst.data_ptr() + 2 * at, n, nl, _hs())
            assert rc == 0, L.spx_last_error()
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "scale %s: first difference in case %s at value %d: %d, the definition has %d" % (
            "32768.0" if nl else "32767.0f", cases[bad[0] // SLOT], bad[0] % SLOT - 16, got[bad[0]], want[bad[0]])
    # full scale on the nonlinear scale wraps, as the streaming API's host loop does
    assert float_to_short_def(np.float32([1.0]), True)[0] == -32768


def test_short_to_float_is_the_ieee_quotient_for_every_int16():
    """spx_short_to_float: all 65 536 int16 values in one call, and a shuffled vector of them at every length x destination offset
    0..7 values x source offset 0..7 values (a 16-byte group of int16 has 8 positions), canaries included."""
    import torch
    from speedy_amd._lib import lib
    L = lib()
    allv = np.arange(-32768, 32768, dtype=np.int16)
    d_all = torch.from_numpy(allv).cuda()
    o_all = torch.zeros(65536, dtype=torch.float32, device="cuda")
    assert L.spx_short_to_float(d_all.data_ptr(), o_all.data_ptr(), 65536, _hs()) == 0, L.spx_last_error()
    torch.cuda.synchronize()
    want_all = allv.astype(np.float32) / np.float32(32767)
    assert np.array_equal(o_all.cpu().numpy().view(np.uint32), want_all.view(np.uint32))
    v = np.random.default_rng(5).permutation(allv)[:max(LENGTHS)]
    v[:6] = [-32768, 32767, -32767, 0, 1, -1]
    q = v.astype(np.float32) / np.float32(32767)
    cases = [(n, d, s) for n in LENGTHS for d in range(8) for s in range(8)]
    srcs = []
    for s in range(8):
        t = torch.zeros(v.size + 16, dtype=torch.int16, device="cuda")
        t[s:s + v.size] = torch.from_numpy(v)
        srcs.append(t)
    want = np.full(len(cases) * SLOT, CANARY32, np.uint32)
    dst = torch.from_numpy(want.view(np.float32).copy()).cuda()
    assert dst.data_ptr() % 32 == 0
    for k, (n, d, s) in enumerate(cases):
        at = k * SLOT + 16 + d
        want[at:at + n] = q[:n].view(np.uint32)
        rc = L.spx_short_to_float(srcs[s].data_ptr() + 2 * s, dst.data_ptr() + 4 * at, n, _hs())
        assert rc == 0, L.spx_last_error()
    torch.cuda.synchronize()
    got = dst.cpu().numpy().view(np.uint32)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "first difference in case %s at value %d" % (cases[bad[0] // SLOT], bad[0] % SLOT - 16)


# ---- the whole call ----
SPEEDS = [(3.5, 1.0), (2.0, 0.0), (1.5, 0.6), (0.7, 0.0), (0.5, 1.0)]
RATES = [None, 0.8, 1.25]
_BASE = {}


def _bc(v, n, dt=np.float32):
    return np.broadcast_to(np.asarray(v, dt), (n,))


def _base(rate_hz, ch):
    """One speech-like signal per (sample rate, channels) as floats: scaled by 1 / 32768 and by 0.97, so that no value is a
    short's exact image; the streams of a batch are slices of it."""
    from speedy_amd.synth import speech_like
    key = (rate_hz, ch)
    if key not in _BASE:
        n = 4 * rate_hz
        s = np.stack([speech_like(n, rate_hz, seed=900 + 17 * ch + c) for c in range(ch)], axis=1).reshape(-1)
        _BASE[key] = (s.astype(np.float32) / np.float32(32768.0) * np.float32(0.97)).astype(np.float32)
    return _BASE[key]


def _ragged(rate_hz, ch, W, B, k):
    lengths = [0, 1, 2, W, W + 1, 3 * B + 5, 1000 + k, rate_hz // 3, rate_hz + 11, 2 * rate_hz + 37]
    x = _base(rate_hz, ch)
    streams, pos = [], 13 * k
    for n in lengths:
        streams.append(x[pos * ch:(pos + n) * ch].copy())
        pos += n // 5 + 3
    return lengths, streams


def _oracles(orc, streams, rate_hz, ch, speed, nl, rate, mm=False, feedback=0.0):
    """The oracle float stream of every job (plain C behind ctypes: threads run it side by side).  rate: None, one, or per job."""
    n = len(streams)
    ch, speed, nl, feedback = _bc(ch, n, np.int32), _bc(speed, n), _bc(nl, n), _bc(feedback, n)
    rates = [None] * n if rate is None else [float(r) for r in _bc(rate, n)]
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(lambda i: oracle_float_stream(orc, streams[i], rate_hz, int(ch[i]), float(speed[i]), float(nl[i]),
                                                         rates[i], mm, float(feedback[i])), range(n)))


def _counts(b):
    import torch
    torch.cuda.synchronize(b.device)
    return b.d_nout.cpu().numpy().copy()


def _outputs(b, nout=None):
    nout = _counts(b) if nout is None else nout
    assert (nout >= 0).all(), "capacity exceeded / lost producer: %s" % nout
    res = []
    for i in range(b.n):
        assert int(nout[i]) <= b.out_caps[i]
        k = int(nout[i]) * int(b.channels[i])
        res.append(b.d_out[b.out_offs[i]:b.out_offs[i] + k].cpu().numpy().copy())
    return res


def _assert_equal(got, want, what=""):
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float32 and w.dtype == np.float32
        assert g.size == w.size, "%s stream %d: %d values, the oracle has %d" % (what, i, g.size, w.size)
        gu, wu = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(gu, wu), "%s stream %d differs from the oracle float stream (first at %d of %d)" % (
            what, i, int(np.nonzero(gu != wu)[0][0]), g.size)


@pytest.mark.parametrize("ch", [1, 2, 3])
@pytest.mark.parametrize("rate_hz", [16000, 22050])
def test_ragged_batches_match_the_oracle_float_stream(orc, rate_hz, ch):
    """Sample rate x channels x (speed, nonlinear) x rate, ten ragged streams each: both input scales, with and without the rate
    stage, feedback 0 and 0.1 by turns."""
    from speedy_amd.batch import FloatBatch, Plan
    plan = Plan(rate_hz, False)
    try:
        k = 0
        for (speed, nl) in SPEEDS:
            for rate in RATES:
                k += 1
                fb = 0.1 if (k % 2 == 0 and nl != 0.0) else 0.0
                lengths, streams = _ragged(rate_hz, ch, plan.W, plan.B, k)
                b = FloatBatch(plan, lengths, ch, speed, nl, fb, rate=rate)
                b.upload(streams)
                b.run()
                got = _outputs(b)
                want = _oracles(orc, streams, rate_hz, ch, speed, nl, rate, False, fb)
                assert want[-1].size // ch > lengths[-1] / (2.0 * max(speed, 1.0) * (rate or 1.0)), "the oracle produced next to nothing"
                _assert_equal(got, want, "%d Hz x %d, speed %g nl %g rate %s fb %g:" % (rate_hz, ch, speed, nl, rate, fb))
                del b
    finally:
        plan.close()


def _mixed_set(ch=2):
    """Eight jobs that mix linear and nonlinear jobs and rates 1 and != 1: both input scales occur in one launch."""
    lengths = [16000, 0, 9001, 241, 20000, 8000, 3, 12345]
    x = _base(16000, ch)
    streams = [x[700 * i * ch:(700 * i + n) * ch].copy() for i, n in enumerate(lengths)]
    sp = [3.5, 2.0, 0.7, 3.5, 1.5, 0.5, 2.0, 2.0]
    nl = [1.0, 0.0, 0.0, 1.0, 0.6, 1.0, 0.0, 0.0]
    rates = [1.25, 1.0, 0.8, 1.0, 1.0, 2.0, 1.25, 1.0]
    return lengths, streams, sp, nl, rates


def test_one_batch_mixes_scales_and_rates(orc):
    from speedy_amd.batch import FloatBatch, Plan, compress_batch_float
    plan = Plan(16000, False)
    try:
        lengths, streams, sp, nl, rates = _mixed_set()
        assert len({(a != 0.0, r != 1.0) for a, r in zip(nl, rates)}) == 4
        b = FloatBatch(plan, lengths, 2, sp, nl, 0.0, rate=rates)
        b.upload(streams)
        b.run()
        want = _oracles(orc, streams, 16000, 2, sp, nl, rates)
        _assert_equal(_outputs(b), want, "mixed batch:")
        # set_input: a packed float32 CUDA tensor that is exactly as long as the jobs' values
        import torch
        b2 = FloatBatch(plan, lengths, 2, sp, nl, 0.0, rate=rates)
        packed = torch.from_numpy(np.concatenate(streams)).cuda()
        assert packed.numel() == b2.total_in
        b2.set_input(packed)
        b2.run()
        _assert_equal(b2.results(), want, "set_input:")
        # the one-call convenience
        outs, _ = compress_batch_float(streams, 16000, 2, sp, nl, 0.0, rate=rates)
        _assert_equal(outs, want, "compress_batch_float:")
    finally:
        plan.close()


def _tap_bytes(b):
    import torch
    torch.cuda.synchronize(b.device)
    return [t.cpu().numpy().tobytes() for t in (b.t_tension, b.t_speed, b.t_features, b.t_spec, b.t_norm)]


@pytest.mark.parametrize("with_rates", [False, True])
def test_the_call_is_the_three_steps_run_by_the_caller(with_rates):
    """spx_batch_run_float = spx_short_to_float o spx_batch_run_rate o spx_float_to_short on the same tables: the caller converts
    every job's samples at the job's scale, runs the int16 call, converts what it produced -- same values, same counts, same
    taps; and spx_batch_read_steps works on the float call's workspace."""
    import torch
    from speedy_amd.batch import Batch, FloatBatch, Plan
    plan = Plan(16000, False)
    try:
        lengths, streams, sp, nl, rates = _mixed_set()
        rate = rates if with_rates else None
        fb = FloatBatch(plan, lengths, 2, sp, nl, 0.1, taps=True, spectrogram_taps=True, rate=rate)
        fb.upload(streams)
        fb.run()
        ib = Batch(plan, lengths, 2, sp, nl, 0.1, taps=True, spectrogram_taps=True, rate=rate)
        assert ib.in_offs == fb.in_offs and ib.out_offs == fb.out_offs and ib.out_caps == fb.out_caps
        L = plan.L
        for i in range(ib.n):
            k = int(lengths[i]) * 2
            rc = L.spx_float_to_short(fb.d_in.data_ptr() + 4 * fb.in_offs[i], ib.d_in.data_ptr() + 2 * ib.in_offs[i], k,
                                      1 if nl[i] != 0.0 else 0, _hs())
            assert rc == 0, L.spx_last_error()
        ib.run()
        nout = _counts(ib)
        assert (nout >= 0).all() and np.array_equal(_counts(fb), nout)
        mine = torch.full_like(fb.d_out, float("nan"))
        for i in range(ib.n):
            rc = L.spx_short_to_float(ib.d_out.data_ptr() + 2 * ib.out_offs[i], mine.data_ptr() + 4 * ib.out_offs[i],
                                      int(nout[i]) * 2, _hs())
            assert rc == 0, L.spx_last_error()
        torch.cuda.synchronize()
        for i in range(ib.n):
            lo, k = ib.out_offs[i], int(nout[i]) * 2
            assert np.array_equal(fb.d_out[lo:lo + k].cpu().numpy().view(np.uint32), mine[lo:lo + k].cpu().numpy().view(np.uint32)), i
        assert sum(int(v) for v in nout) > 10000
        assert _tap_bytes(fb) == _tap_bytes(ib)
        assert any(np.frombuffer(t, np.uint8).any() for t in _tap_bytes(fb))
        assert np.array_equal(fb.step_counts(), ib.step_counts()) and fb.step_counts().max() > 50
    finally:
        plan.close()


def _placed(plan, shift, lengths, ch, sp, nl, rates):
    """A FloatBatch whose in_off and out_off are all `shift` values further on, in buffers that much larger."""
    import torch
    from speedy_amd.batch import FloatBatch
    b = FloatBatch(plan, lengths, ch, sp, nl, 0.0, rate=rates)
    for i in range(b.n):
        b.jobs[i].in_off += shift
        b.jobs[i].out_off += shift
    b.in_offs = [v + shift for v in b.in_offs]
    b.out_offs = [v + shift for v in b.out_offs]
    b.d_in = torch.zeros(b.total_in + shift, dtype=torch.float32, device=b.device)
    b.d_out = torch.zeros(b.total_out + shift + 8, dtype=torch.float32, device=b.device)
    wsb = plan.L.spx_batch_workspace_bytes_float(plan.h, b.jobs, b._rates_ptr(), b.n)
    assert wsb > 0
    b.d_ws = torch.zeros(wsb, dtype=torch.uint8, device=b.device)
    return b


def test_placement_and_capacity(orc):
    """in_off and out_off shifted by 1, 2, 3 and 5 values: the output buffer, pre-filled with 0x7fc05a5a, holds the oracle's
    stream in [out_off, out_off + n_out * C) and the pattern everywhere else.  Then out_cap cut to half of what two streams
    need: n_out < 0, exactly out_cap frames written, equal to the prefix of the full result, nothing behind them."""
    import torch
    from speedy_amd.batch import Plan
    plan = Plan(16000, False)
    try:
        ch = 2
        lengths, streams, sp, nl, rates = _mixed_set(ch)
        want = _oracles(orc, streams, 16000, ch, sp, nl, rates)
        full = [w.size // ch for w in want]
        for shift in (1, 2, 3, 5):
            b = _placed(plan, shift, lengths, ch, sp, nl, rates)
            b.upload(streams)
            b.d_out = torch.from_numpy(np.full(b.d_out.numel(), CANARY32, np.uint32).view(np.float32).copy()).cuda()
            b.run()
            nout = _counts(b)
            assert list(nout) == full, "shift %d: counts %s, the oracle has %s" % (shift, list(nout), full)
            expect = np.full(b.d_out.numel(), CANARY32, np.uint32)
            for i in range(b.n):
                expect[b.out_offs[i]:b.out_offs[i] + want[i].size] = want[i].view(np.uint32)
            got = b.d_out.cpu().numpy().view(np.uint32)
            bad = np.nonzero(got != expect)[0]
            assert bad.size == 0, "shift %d: first difference at value %d" % (shift, bad[0])
        # half the capacity: one job with a rate stage (0), one without (4)
        b = _placed(plan, 3, lengths, ch, sp, nl, rates)
        b.upload(streams)
        cut = {0: full[0] // 2, 4: full[4] // 2}
        for i, cap in cut.items():
            assert 0 < cap < full[i]
            b.jobs[i].out_cap = cap
        b.d_out = torch.from_numpy(np.full(b.d_out.numel(), CANARY32, np.uint32).view(np.float32).copy()).cuda()
        b.run()
        nout = _counts(b)
        expect = np.full(b.d_out.numel(), CANARY32, np.uint32)
        for i in range(b.n):
            k = cut.get(i, full[i]) * ch
            assert (nout[i] < 0) if i in cut else (nout[i] == full[i]), "stream %d: n_out %d" % (i, nout[i])
            expect[b.out_offs[i]:b.out_offs[i] + k] = want[i][:k].view(np.uint32)
        got = b.d_out.cpu().numpy().view(np.uint32)
        bad = np.nonzero(got != expect)[0]
        assert bad.size == 0, "half capacity: first difference at value %d" % bad[0]
    finally:
        plan.close()


def test_refusals_launch_nothing():
    """A misaligned out, a workspace one byte short, a rate of 0 (and what else the int16 call refuses: a speed of 0, a nonlinear
    factor of 2, a null input): -1 with a message; n_out and out keep their canaries."""
    import torch
    from speedy_amd.batch import FloatBatch, Plan
    plan = Plan(16000, False)
    try:
        lengths, streams, sp, nl, rates = _mixed_set()
        b = FloatBatch(plan, lengths, 2, sp, nl, 0.0, rate=rates)
        b.upload(streams)
        L = plan.L
        good_rates = b.rates.copy()

        def call(out_ptr=None, ws_bytes=None, in_ptr=None):
            return L.spx_batch_run_float(plan.h, b.jobs, b._rates_ptr(), b.n, b.d_in.data_ptr() if in_ptr is None else in_ptr,
                                         b.d_out.data_ptr() if out_ptr is None else out_ptr, b.d_nout.data_ptr(), b.d_ws.data_ptr(),
                                         b.d_ws.numel() if ws_bytes is None else ws_bytes, None, _hs())

        def refused(what, **kw):
            b.d_out = torch.from_numpy(np.full(b.d_out.numel(), CANARY32, np.uint32).view(np.float32).copy()).cuda()
            b.d_nout.fill_(-77)
            rc = call(**kw)
            msg = L.spx_last_error()
            assert rc == -1 and msg, "%s: rc %d, message %r" % (what, rc, msg)
            torch.cuda.synchronize()
            assert bool((b.d_nout == -77).all()), what + ": a refused call wrote n_out"
            assert (b.d_out.cpu().numpy().view(np.uint32) == CANARY32).all(), what + ": a refused call wrote out"
            return msg.decode()

        refused("misaligned out", out_ptr=b.d_out.data_ptr() + 2)
        assert "workspace" in refused("workspace one byte short", ws_bytes=b.d_ws.numel() - 1)
        b.rates = good_rates.copy()
        b.rates[2] = 0.0
        assert "rate" in refused("rate 0")
        assert L.spx_batch_workspace_bytes_float(plan.h, b.jobs, b._rates_ptr(), b.n) == 0
        with pytest.raises(RuntimeError):
            b.run()
        b.rates = good_rates.copy()
        b.jobs[1].speed = 0.0
        assert "speed" in refused("speed 0")
        b.jobs[1].speed = 2.0
        b.jobs[3].nonlinear = 2.0
        assert "nonlinear" in refused("nonlinear 2")
        b.jobs[3].nonlinear = 1.0
        refused("misaligned in", in_ptr=b.d_in.data_ptr() + 1)
        # ... and the same object still runs
        b.d_nout.fill_(0)
        b.run()
        assert (_counts(b) >= 0).all() and _counts(b).sum() > 10000
    finally:
        plan.close()


def test_c_example_writes_the_oracles_float_stream(orc, tmp_path):
    """tools/batch_float_example.c (plain C99 over include/speedy_hip.h) on tests/golden/tapestry.wav."""
    exe = os.path.join(ROOT, "speedy_amd", "lib", "batch_float_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "floatexample"])
    w, rate_hz, ch = read_wav("tapestry.wav")
    x = w.astype(np.float32) / np.float32(32768.0)   # the program's own scaling
    for k, (speed, nl, rate) in enumerate([(3.5, 1.0, 1.0), (2.0, 0.0, 1.25)]):
        out = str(tmp_path / ("out%d.f32" % k))
        r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "tapestry.wav"), out, str(speed), str(nl), str(rate)],
                           capture_output=True, text=True, timeout=180)
        assert r.returncode == 0, r.stderr
        want = oracle_float_stream(orc, x, rate_hz, ch, speed, nl, rate)
        f = r.stdout.split()
        assert f[0] == "rate" and int(f[1]) == rate_hz and int(f[3]) == ch and int(f[5]) == w.size // ch, r.stdout
        assert int(f[7]) == want.size // ch > 1000, (r.stdout, want.size // ch)
        got = np.fromfile(out, "<f4")
        assert got.size == want.size and np.array_equal(got.view(np.uint32), want.view(np.uint32))
