"""The pipeline object on FLOAT samples (SPX_PIPELINE_FLOAT: spx_pipeline_submit_float / _submit_jobs_float / _wait_float /
_host_input_float) on the MI355X: both conversions on the GPU, in the pipeline's own order.

The expected output of every lane is the oracle FLOAT stream (tests/test_batch_float_abi.py oracle_float_stream); every comparison
is bit for bit, the float output as uint32 patterns, no tolerance."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_batch_float_abi import float_to_short_def, oracle_float_stream  # noqa: E402
from test_gpu_batch_float import _assert_equal, _base, _oracles, _outputs, _ragged  # noqa: E402
from util import read_wav  # noqa: E402

pytestmark = pytest.mark.gpu

# (speed, nonlinear) per lane, taking turns: linear and nonlinear lanes in every table, so both input scales occur in one
# conversion launch; the slow-down lanes are linear (a nonlinear slow-down lane's capacity assumes the 0.01 clamp: 100 x the input)
LANE_MODES = [(3.5, 1.0), (2.0, 0.0), (1.5, 0.6), (0.7, 0.0)]
_WANT = {}


def _modes(n):
    return [LANE_MODES[i % 4][0] for i in range(n)], [LANE_MODES[i % 4][1] for i in range(n)]


def _batch(orc, plan, rate, ch, k):
    """Submit k of the ragged test: _ragged's ten lengths rotated by k, with the oracle float stream of every lane -- and
    FloatBatch's output on the same jobs, which must be the same bits.  Computed once per (rate, ch, k)."""
    from speedy_amd.batch import FloatBatch
    key = (rate, ch, k)
    if key not in _WANT:
        lengths, streams = _ragged(rate, ch, plan.W, plan.B, k)
        r = k % len(lengths)
        lengths, streams = lengths[r:] + lengths[:r], streams[r:] + streams[:r]
        sp, nl = _modes(len(lengths))
        want = _oracles(orc, streams, rate, ch, sp, nl, None)
        b = FloatBatch(plan, lengths, ch, sp, nl, 0.0)
        b.upload(streams)
        b.run()
        _assert_equal(_outputs(b), want, "FloatBatch, %d Hz x %d, submit %d:" % (rate, ch, k))
        assert sum(w.size for w in want) // ch > 1000
        _WANT[key] = (lengths, streams, want)
    return _WANT[key]


def _host_outs(pipe, t, lens):
    """One wait on a float pipeline: the per-lane outputs (copies), with what the packed layout promises checked on the way."""
    out, offsets, counts = pipe.wait(t)
    assert out.dtype == np.float32
    assert all(int(o) % 32 == 0 for o in offsets), t
    assert (counts >= 0).all(), (t, counts)
    res = []
    for i in range(pipe.n):
        c = int(pipe.channels[i])
        if lens[i] == 0:
            assert int(counts[i]) == 0 and int(offsets[i + 1]) == int(offsets[i]), (t, i)   # an empty lane takes no room at all
        assert int(offsets[i + 1]) - int(offsets[i]) == (int(counts[i]) * c + 31) // 32 * 32, (t, i)
        res.append(out[int(offsets[i]):int(offsets[i]) + int(counts[i]) * c].copy())
    return res


def _lane_pipeline(plan, rate, ch, depth, n=10, **kw):
    """Ten lanes created at 2 * rate + 37 frames, each with the (speed, nonlinear) it keeps for every batch."""
    from speedy_amd.batch import Pipeline
    sp, nl = _modes(n)
    return Pipeline(plan, [2 * rate + 37] * n, ch, sp, nl, 0.0, depth=depth, float_samples=True, **kw)


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("ch", [1, 2, 3])
@pytest.mark.parametrize("rate", [16000, 22050])
def test_ragged_tables_host_to_host(orc, rate, ch, depth):
    """Six submits of ragged tables (lengths 0, 1, 2, W, W + 1 ... rotated per submit), from a pinned tensor, a pageable array and
    the pipeline's own pinned staging by turns, waited for depth - 1 submits late."""
    import torch
    from speedy_amd.batch import Plan
    plan = Plan(rate, False)
    try:
        pipe = _lane_pipeline(plan, rate, ch, depth)
        assert pipe.depth == depth and pipe.L.spx_pipeline_input_values(pipe.h) == 10 * (2 * rate + 37) * ch
        batches = [_batch(orc, plan, rate, ch, k) for k in range(6)]
        tickets, lag = [], depth - 1

        def check(k):
            lens, _, want = batches[k]
            _assert_equal(_host_outs(pipe, tickets[k], lens), want, "%d Hz x %d depth %d, submit %d:" % (rate, ch, depth, k))

        for k, (lens, streams, _) in enumerate(batches):
            packed = pipe.pack(streams, lens)
            assert packed.dtype == np.float32
            if k % 3 == 0:
                x = torch.from_numpy(packed).pin_memory()
            elif k % 3 == 1:
                x = packed
            else:
                x = pipe.host_input()
                assert x.dtype == np.float32 and x.size == pipe.total_in
                x[:] = packed
            assert pipe.fits(lens)
            tickets.append(pipe.submit_jobs(x, lens))
            assert tickets[k] == k
            if k >= lag:
                check(k - lag)
        for k in range(6 - lag, 6):
            check(k)
        pipe.close()
    finally:
        plan.close()


def test_unaligned_lanes(orc):
    """in_offs shifted by 1, 2, 3 and 5 values: the float source is off its 16-byte boundary and the int16 staging off its own;
    lengths 7, 8, 9, 2047, 2048 and 2049 cross the edges of a conversion thread's group and of a conversion block."""
    from speedy_amd.batch import Plan
    rate, ch = 16000, 1
    plan = Plan(rate, False)
    try:
        pipe = _lane_pipeline(plan, rate, ch, 2)
        sp, nl = _modes(10)
        lens = [0, 7, 8, 9, 2047, 2048, 2049, plan.W + 1, rate // 3, rate + 11]
        x = _base(rate, ch)
        tickets, wants = [], []
        for k, shift in enumerate((1, 2, 3, 5)):
            streams = [x[(977 * k + 131 * i) * ch:(977 * k + 131 * i + n) * ch].copy() for i, n in enumerate(lens)]
            offs = [o + shift for o in pipe.in_offs]
            host = np.full(pipe.total_in, np.nan, np.float32)   # (what no lane reads must not matter)
            for o, s in zip(offs, streams):
                host[o:o + s.size] = s
            wants.append(_oracles(orc, streams, rate, ch, sp, nl, None))
            tickets.append(pipe.submit_jobs(host, lens, in_offs=offs))
            if k >= 1:
                _assert_equal(_host_outs(pipe, tickets[k - 1], lens), wants[k - 1], "shift of submit %d:" % (k - 1))
        _assert_equal(_host_outs(pipe, tickets[3], lens), wants[3], "shift 5:")
        pipe.close()
    finally:
        plan.close()


def test_device_in_device_out(orc):
    """SPX_PIPELINE_FLOAT | SPX_PIPELINE_DEVICE_OUT with a CUDA float32 tensor of EXACTLY the batch's extent (lanes packed densely,
    no padding behind the last value): values and counts from the static capacity layout."""
    import torch
    from speedy_amd.batch import Plan
    rate, ch = 16000, 2
    plan = Plan(rate, False)
    try:
        pipe = _lane_pipeline(plan, rate, ch, 3, device_out=True)
        sp, nl = _modes(10)
        caps = [(plan.out_capacity(2 * rate + 37, sp[i], nl[i]) * ch + 31) // 32 * 32 for i in range(10)]
        static = [int(v) for v in np.concatenate(([0], np.cumsum(caps)))]
        tickets, batches = [], []
        for k in range(3):
            lens, streams, want = _batch(orc, plan, rate, ch, k)
            offs = [int(v) for v in np.concatenate(([0], np.cumsum([n * ch for n in lens])[:-1]))]
            d = torch.from_numpy(np.concatenate(streams)).cuda()
            assert d.dtype == torch.float32 and d.numel() == offs[-1] + lens[-1] * ch == sum(lens) * ch
            torch.cuda.synchronize()
            tickets.append(pipe.submit_jobs(d, lens, in_offs=offs))
            batches.append(want)
        for k in range(3):
            ptr, offsets, cnt_ptr = pipe.wait(tickets[k])
            assert ptr and cnt_ptr and [int(v) for v in offsets] == static, k
            cnt = np.zeros(10, np.int64)
            pipe.L.spx_copy_to_host(cnt.ctypes.data, cnt_ptr, 80, None)
            pipe.L.spx_stream_synchronize(None)
            assert [int(v) for v in cnt] == [w.size // ch for w in batches[k]], k
            _assert_equal(pipe.results(tickets[k]), batches[k], "device out, submit %d:" % k)
        pipe.close()
    finally:
        plan.close()


def test_input_consumed_frees_either_kind_of_float_input(orc):
    """input_consumed(t) on a float pipeline returns once the conversion has read the input -- device or host: the whole input is
    then overwritten with NaN and the next batch submitted from another buffer; batch t is still the oracle's."""
    import torch
    from speedy_amd.batch import Plan
    rate, ch = 16000, 1
    plan = Plan(rate, False)
    try:
        pipe = _lane_pipeline(plan, rate, ch, 3)
        (la, sa, wa), (lb, sb, wb) = _batch(orc, plan, rate, ch, 0), _batch(orc, plan, rate, ch, 1)
        pa, pb = pipe.pack(sa, la), pipe.pack(sb, lb)
        for kind in ("device", "host"):
            a = torch.from_numpy(pa.copy())
            a = a.cuda() if kind == "device" else a.pin_memory()
            b = torch.from_numpy(pb.copy()).cuda() if kind == "device" else pb.copy()
            torch.cuda.synchronize()
            t = pipe.submit_jobs(a, la)
            pipe.input_consumed(t)
            a.fill_(float("nan"))
            torch.cuda.synchronize()
            t2 = pipe.submit_jobs(b, lb)
            assert t2 == t + 1
            _assert_equal(_host_outs(pipe, t, la), wa, kind + " input, the batch whose input was overwritten:")
            _assert_equal(_host_outs(pipe, t2, lb), wb, kind + " input, the batch behind it:")
        pipe.close()
    finally:
        plan.close()


def _crc(outs):
    return [zlib.crc32(np.ascontiguousarray(o).tobytes()) for o in outs]


def test_pipelined_order_is_kept(orc):
    """256 mono lanes at 16 kHz, depth 3, four submits with fresh content: every lane's CRC is FloatBatch's, lanes 0 / 128 / 255 are
    the oracle's, and from the second submit on the batch call reports the pipelined order (spx_debug_last_call_concurrent() == 2):
    the float path does not cost the overlap."""
    import torch
    from speedy_amd.batch import FloatBatch, Pipeline, Plan
    rate, n = 16000, 256
    lane = rate // 3
    plan = Plan(rate, False)
    try:
        x = _base(rate, 1)
        fb = FloatBatch(plan, [lane] * n, 1, 3.5, 1.0, 0.0)
        want, packed = [], []
        pipe = Pipeline(plan, [lane] * n, 1, 3.5, 1.0, 0.0, depth=3, float_samples=True)
        for k in range(4):
            streams = [x[(211 * i + 5003 * k) % (x.size - lane):][:lane].copy() for i in range(n)]
            fb.upload(streams)
            fb.run()
            outs = _outputs(fb)
            for i in (0, 128, 255):
                ref = oracle_float_stream(orc, streams[i], rate, 1, 3.5, 1.0)
                assert ref.size > 1000 and np.array_equal(outs[i].view(np.uint32), ref.view(np.uint32)), (k, i)
            want.append(_crc(outs))
            packed.append(torch.from_numpy(pipe.pack(streams)).pin_memory())
        assert len({tuple(w) for w in want}) == 4
        tickets, modes = [], []
        for k in range(4):
            tickets.append(pipe.submit(packed[k]))
            modes.append(plan.L.spx_debug_last_call_concurrent())
            if k >= 2:
                assert _crc(_host_outs(pipe, tickets[k - 2], [lane] * n)) == want[k - 2], k - 2
        for k in (2, 3):
            assert _crc(_host_outs(pipe, tickets[k], [lane] * n)) == want[k], k
        print("launch order per submit:", modes)
        assert modes[1:] == [2, 2, 2], modes
        pipe.close()
    finally:
        plan.close()


def test_mixed_sample_rates(orc):
    """spx_pipeline_create_mixed with the flag: plans of 16 kHz and 22.05 kHz, six lanes, two batches."""
    from speedy_amd.batch import Pipeline, Plan
    rates = [16000, 22050]
    plans = [Plan(r, False) for r in rates]
    try:
        n = 6
        pidx = [i % 2 for i in range(n)]
        chs = [1, 1, 2, 2, 1, 2]
        sp, nl = _modes(n)
        lanes = [rates[pidx[i]] + 11 for i in range(n)]
        pipe = Pipeline(plans, lanes, chs, sp, nl, 0.0, depth=2, plan_index=pidx, float_samples=True)
        tabs = [lanes, [0, 2049, rates[0] // 3, 7, lanes[4] - 1, rates[1] // 2]]
        tickets, wants = [], []
        for k, lens in enumerate(tabs):
            streams = [_base(rates[pidx[i]], chs[i])[(401 * k + 97 * i) * chs[i]:(401 * k + 97 * i + lens[i]) * chs[i]].copy() for i in range(n)]
            wants.append([oracle_float_stream(orc, streams[i], rates[pidx[i]], chs[i], sp[i], nl[i]) for i in range(n)])
            tickets.append(pipe.submit_jobs(pipe.pack(streams, lens), lens))
        for k, lens in enumerate(tabs):
            _assert_equal(_host_outs(pipe, tickets[k], lens), wants[k], "mixed rates, batch %d:" % k)
        assert sum(w.size for w in wants[1]) > 1000
        pipe.close()
    finally:
        for p in plans:
            p.close()


def test_refusals_use_up_no_ticket(orc):
    """The int16 calls on a float pipeline, the _float calls on an int16 pipeline, a float host pointer at + 2 bytes and a table
    with speed 0 in lane 3: -1 (NULL) with a message, the next good submit gets the next ticket and delivers the oracle's output."""
    from speedy_amd.batch import Pipeline, Plan
    rate, ch = 16000, 1
    plan = Plan(rate, False)
    L = plan.L
    try:
        fpipe = _lane_pipeline(plan, rate, ch, 2)
        sp, nl = _modes(10)
        ipipe = Pipeline(plan, [2 * rate + 37] * 10, ch, sp, nl, 0.0, depth=2)
        lens, streams, want = _batch(orc, plan, rate, ch, 2)
        packed = fpipe.pack(streams, lens)
        # (the int16 pipeline's input: the defined conversion of the same floats, so that its output x 1 / 32767 is the same oracle's)
        packed16 = ipipe.pack([float_to_short_def(s, nl[i] != 0.0) for i, s in enumerate(streams)], lens)
        spare = np.zeros(packed.size + 1, np.float32)
        jobs = fpipe.table(lens)
        o, f, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        expect = 0

        def refused(rc, needle):
            msg = L.spx_last_error()
            assert rc in (-1, None) and msg and needle in msg.decode(), (rc, msg)

        def good(pipe, n_refusals):
            nonlocal expect
            t = pipe.submit_jobs(packed if pipe is fpipe else packed16, lens)
            assert t == expect, (t, expect, n_refusals)
            return t

        # ---- the int16 calls on a float pipeline ----
        live = good(fpipe, 0)
        refused(L.spx_pipeline_submit(fpipe.h, packed.ctypes.data, 0), "SPX_PIPELINE_FLOAT")
        refused(L.spx_pipeline_submit_jobs(fpipe.h, jobs, packed.ctypes.data, 0), "SPX_PIPELINE_FLOAT")
        refused(L.spx_pipeline_wait(fpipe.h, live, C.byref(o), C.byref(f), C.byref(c)), "SPX_PIPELINE_FLOAT")
        refused(L.spx_pipeline_host_input(fpipe.h), "SPX_PIPELINE_FLOAT")
        # ---- a float host pointer that is not 4-byte aligned; a table the engine's rules refuse ----
        refused(L.spx_pipeline_submit_float(fpipe.h, spare.ctypes.data + 2, 0), "aligned")
        refused(L.spx_pipeline_submit_jobs_float(fpipe.h, jobs, spare.ctypes.data + 2, 0), "aligned")
        bad = fpipe.table(lens)
        bad[3].speed = 0.0
        refused(L.spx_pipeline_submit_jobs_float(fpipe.h, bad, packed.ctypes.data, 0), "lane 3")
        assert L.spx_pipeline_jobs_fit(fpipe.h, bad) == -1 and b"lane 3" in L.spx_last_error()
        expect = 1
        nxt = good(fpipe, 7)
        _assert_equal(_host_outs(fpipe, live, lens), want, "the batch in flight during the refusals:")
        _assert_equal(_host_outs(fpipe, nxt, lens), want, "the submit behind the refusals:")
        # ---- the _float calls on an int16 pipeline ----
        expect = 0
        live = good(ipipe, 0)
        refused(L.spx_pipeline_submit_float(ipipe.h, packed.ctypes.data, 0), "SPX_PIPELINE_FLOAT")
        refused(L.spx_pipeline_submit_jobs_float(ipipe.h, ipipe.table(lens), packed.ctypes.data, 0), "SPX_PIPELINE_FLOAT")
        refused(L.spx_pipeline_wait_float(ipipe.h, live, C.byref(o), C.byref(f), C.byref(c)), "SPX_PIPELINE_FLOAT")
        refused(L.spx_pipeline_host_input_float(ipipe.h), "SPX_PIPELINE_FLOAT")
        expect = 1
        nxt = good(ipipe, 4)
        for t in (live, nxt):
            outs = ipipe.results(t)
            assert all(v.dtype == np.int16 for v in outs)
            _assert_equal([v.astype(np.float32) / np.float32(32767) for v in outs], want, "the int16 pipeline, ticket %d:" % t)
        fpipe.close()
        ipipe.close()
    finally:
        plan.close()


def test_c_example_writes_the_oracles_float_stream(orc, tmp_path):
    """tools/pipeline_float_example.c (plain C99 over include/speedy_hip.h) on tests/golden/tapestry.wav."""
    exe = os.path.join(ROOT, "speedy_amd", "lib", "pipeline_float_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "pipefloatexample"])
    w, rate_hz, ch = read_wav("tapestry.wav")
    x = w.astype(np.float32) / np.float32(32768.0)   # the program's own scaling
    for k, (speed, nl) in enumerate([(3.5, 1.0), (2.0, 0.0)]):
        out = str(tmp_path / ("out%d.f32" % k))
        r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "tapestry.wav"), out, str(speed), str(nl)],
                           capture_output=True, text=True, timeout=180)
        assert r.returncode == 0, r.stderr
        want = oracle_float_stream(orc, x, rate_hz, ch, speed, nl)
        f = r.stdout.split()
        assert f[0] == "rate" and int(f[1]) == rate_hz and int(f[3]) == ch and int(f[5]) == w.size // ch, r.stdout
        assert int(f[7]) == want.size // ch > 1000, (r.stdout, want.size // ch)
        got = np.fromfile(out, "<f4")
        assert got.size == want.size and np.array_equal(got.view(np.uint32), want.view(np.uint32))
