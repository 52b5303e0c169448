"""The RATE pipeline on the MI355X (spx_pipeline_create_rate, spx_pipeline_jobs_fit_rate, spx_pipeline_submit_jobs_rate / _rate_float):
a playback rate per lane and per batch (sonicSetRate before the first write) through the pipeline object.

The expected output of every lane is the oracle STREAM with that rate (tests/test_batch_rate_abi.py oracle_rate_stream); every
comparison is bit for bit -- bytes and counts, the float output as uint32 patterns -- with no tolerance.

Shapes: ten lanes of 0, 1, 2, W, W + 1, 3 B + 5, 1000, 5333, sample rate + 11 and 24000 frames (W the plan's window, B its step),
signals sliced from speedy_amd.synth.speech_like; every pipeline is created with this (the longest) table and, per lane, the
smallest rate the lane sees in the test."""
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
from test_batch_float_abi import float_to_short_def  # noqa: E402
from test_batch_rate_abi import oracle_rate_stream  # noqa: E402
from util import read_wav  # noqa: E402

pytestmark = pytest.mark.gpu

RATE_SET = [1.0, 0.5, 0.8, 1.25, 2.0, 3.0]
SPEEDS = [(3.5, 1.0), (2.0, 0.0), (1.5, 0.6), (1.0, 0.0), (0.7, 0.0), (0.5, 1.0)]
N = 10
_BASE, _ORACLE = {}, {}


def _lens(plan, hz):
    return [0, 1, 2, plan.W, plan.W + 1, 3 * plan.B + 5, 1000, 5333, hz + 11, 24000]


def _modes():
    """(speed, nonlinear, feedback) per lane, fixed for the lane's life: all six speed classes, feedback 0 and 0.1 by turns."""
    sp = [SPEEDS[i % 6][0] for i in range(N)]
    nl = [SPEEDS[i % 6][1] for i in range(N)]
    fb = [0.1 if (i % 2 == 0 and nl[i] != 0.0) else 0.0 for i in range(N)]
    return sp, nl, fb


def _rates(k):
    """The rate table of ticket k: every value of RATE_SET in every table, a rate of 1 among the others, no two tables alike."""
    return [RATE_SET[(i + k) % 6] for i in range(N)]


def _min_rates(ks):
    return [min(_rates(k)[i] for k in ks) for i in range(N)]


def _streams(hz, ch, lens, k):
    from speedy_amd.synth import speech_like
    key = (hz, ch)
    if key not in _BASE:
        _BASE[key] = np.stack([speech_like(3 * hz, hz, seed=900 + 13 * ch + c) for c in range(ch)], axis=1).reshape(-1)
    x = _BASE[key]
    return [x[(500 * i + 101 * k) * ch:(500 * i + 101 * k + n) * ch].copy() for i, n in enumerate(lens)]


def _want(orc, hz, ch, lens, k, rates):
    """The oracle stream of every lane of signal set k at these rates; computed once per (lane, signal, rate) and never changed."""
    sp, nl, fb = _modes()
    streams = _streams(hz, ch, lens, k)
    todo = [i for i in range(N) if (hz, ch, i, k, float(rates[i])) not in _ORACLE]
    with ThreadPoolExecutor(8) as ex:
        got = list(ex.map(lambda i: oracle_rate_stream(orc, streams[i], hz, ch, sp[i], nl[i], float(rates[i]), False, fb[i]), todo))
    for i, g in zip(todo, got):
        g.setflags(write=False)
        _ORACLE[(hz, ch, i, k, float(rates[i]))] = g
    return [_ORACLE[(hz, ch, i, k, float(rates[i]))] for i in range(N)]


def _pipeline(plan, hz, ch, depth, rate, **kw):
    from speedy_amd.batch import Pipeline
    sp, nl, fb = _modes()
    return Pipeline(plan, _lens(plan, hz), ch, sp, nl, fb, depth=depth, rate=rate, **kw)


def _host_outs(pipe, t, lens):
    """One wait: the per-lane outputs (copies), with what the packed layout promises checked on the way."""
    out, offsets, counts = pipe.wait(t)
    assert all(int(o) % 32 == 0 for o in offsets), (t, offsets)
    assert (counts >= 0).all(), (t, counts)
    res = []
    for i in range(pipe.n):
        c = int(pipe.channels[i])
        if lens[i] == 0:
            assert int(counts[i]) == 0 and int(offsets[i + 1]) == int(offsets[i]), (t, i)   # an empty lane takes no room
        assert int(offsets[i + 1]) - int(offsets[i]) == (int(counts[i]) * c + 31) // 32 * 32, (t, i)
        res.append(out[int(offsets[i]):int(offsets[i]) + int(counts[i]) * c].copy())
    assert int(offsets[pipe.n]) == sum((int(counts[i]) * int(pipe.channels[i]) + 31) // 32 * 32 for i in range(pipe.n))   # the extent
    return res


def _assert_equal(got, want, what=""):
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.size == w.size, "%s lane %d: %d values, expected %d" % (what, i, g.size, w.size)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), "%s lane %d differs (first at %d of %d)" % (what, i, int(np.nonzero(g != w)[0][0]), g.size)


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("hz", [16000, 22050])
def test_per_batch_rate_tables_match_the_oracle(orc, hz, ch, depth):
    """Six tickets, six rate tables (a rate of 1 inside each), fresh samples per ticket, from a pageable array and the pipeline's pinned
    staging by turns.  Depth 2: tickets waited for in submit order, one submit late; depth 3: three in flight, waited for in reverse."""
    from speedy_amd.batch import Plan
    plan = Plan(hz, False)
    try:
        lens = _lens(plan, hz)
        pipe = _pipeline(plan, hz, ch, depth, _min_rates(range(6)))
        assert pipe.depth == depth
        wants = [_want(orc, hz, ch, lens, k, _rates(k)) for k in range(6)]
        assert all(sum(w.size for w in ws) // ch > 5000 for ws in wants)   # (the oracle did produce)
        tickets = []

        def submit(k):
            packed = pipe.pack(_streams(hz, ch, lens, k))
            if k % 2:
                x = pipe.host_input()
                x[:] = packed
            else:
                x = packed
            assert pipe.fits(lens, rate=_rates(k))
            tickets.append(pipe.submit_jobs(x, lens, rate=_rates(k)))
            assert tickets[k] == k

        def check(k):
            _assert_equal(_host_outs(pipe, tickets[k], lens), wants[k], "%d Hz x %d depth %d ticket %d:" % (hz, ch, depth, k))

        if depth == 2:
            for k in range(6):
                submit(k)
                if k >= 1:
                    check(k - 1)
            check(5)
        else:
            for g in (0, 3):
                for k in range(g, g + 3):
                    submit(k)
                for k in reversed(range(g, g + 3)):
                    check(k)
        pipe.close()
    finally:
        plan.close()


def test_the_pipeline_equals_the_batch_call():
    """The same tables through Batch(..., rate=...) -- spx_batch_run_rate on the caller's buffers: identical counts and bytes."""
    import torch
    from speedy_amd.batch import Batch, Plan
    hz, ch = 16000, 2
    plan = Plan(hz, False)
    try:
        lens = _lens(plan, hz)
        sp, nl, fb = _modes()
        pipe = _pipeline(plan, hz, ch, 3, _min_rates(range(6)))
        for g in (0, 3):
            tickets = [pipe.submit_jobs(pipe.pack(_streams(hz, ch, lens, k)), lens, rate=_rates(k)) for k in range(g, g + 3)]
            got = []
            for t in tickets:   # (the pipeline's three batches first: the batch calls below then run on an idle plan)
                counts = pipe.wait(t)[2].copy()
                got.append((counts, _host_outs(pipe, t, lens)))
            for k, (counts, outs) in zip(range(g, g + 3), got):
                b = Batch(plan, lens, ch, sp, nl, fb, rate=_rates(k))
                b.upload(_streams(hz, ch, lens, k))
                b.run()
                torch.cuda.synchronize()
                nout = b.d_nout.cpu().numpy()
                assert (nout >= 0).all()
                batch = [b.d_out[b.out_offs[i]:b.out_offs[i] + int(nout[i]) * ch].cpu().numpy() for i in range(N)]
                assert [int(v) for v in counts] == [int(v) for v in nout], k
                _assert_equal(outs, batch, "ticket %d against Batch:" % k)
                assert sum(o.size for o in outs) // ch > 5000
        pipe.close()
    finally:
        plan.close()


def test_all_ones_batches_are_ordinary_batches(orc):
    """A rate pipeline created at rate 1 and an ordinary Pipeline from the same table: submit, submit_jobs and submit_jobs with rates
    of one give the ordinary pipeline's outputs, offsets and counts -- and spx_pipeline_submit_jobs_rate with rates == NULL too."""
    from speedy_amd.batch import Pipeline, Plan
    hz, ch = 16000, 1
    plan = Plan(hz, False)
    try:
        lens = _lens(plan, hz)
        sp, nl, fb = _modes()
        rpipe = _pipeline(plan, hz, ch, 2, 1.0)
        opipe = Pipeline(plan, lens, ch, sp, nl, fb, depth=2)
        want = _want(orc, hz, ch, lens, 0, [1.0] * N)
        packed = opipe.pack(_streams(hz, ch, lens, 0))
        ref = [v.copy() for v in opipe.wait(opipe.submit(packed))]
        _assert_equal(_host_outs(opipe, 0, lens), want, "the ordinary pipeline:")
        null_rates = lambda: rpipe._ticket(rpipe.L.spx_pipeline_submit_jobs_rate(rpipe.h, rpipe.table(lens), None, packed.ctypes.data, 0),  # noqa: E731
                                           packed, "spx_pipeline_submit_jobs_rate")
        for what, t in (("submit", lambda: rpipe.submit(packed)), ("submit_jobs", lambda: rpipe.submit_jobs(packed, lens)),
                        ("submit_jobs, ones", lambda: rpipe.submit_jobs(packed, lens, rate=1.0)), ("rates NULL", null_rates)):
            ticket = t()
            _, offsets, counts = rpipe.wait(ticket)
            assert np.array_equal(offsets, ref[1]) and np.array_equal(counts, ref[2]), what
            _assert_equal(_host_outs(rpipe, ticket, lens), want, what + ":")
        assert rpipe.fits(lens) and rpipe.fits(lens, rate=1.0)
        rpipe.close()
        opipe.close()
    finally:
        plan.close()


@pytest.mark.parametrize("depth", [2, 3, 4])
def test_all_ones_and_mixed_tables_alternate(orc, depth):
    """Eight tickets, all-ones (the overlapped order) and mixed-rate tables (kernels in sequence on the run stream) by turns, `depth`
    in flight: each ticket is its own oracle streams."""
    from speedy_amd.batch import Plan
    hz, ch = 16000, 1
    plan = Plan(hz, False)
    try:
        lens = _lens(plan, hz)
        pipe = _pipeline(plan, hz, ch, depth, _min_rates(range(6)))
        tables = [[1.0] * N if k % 2 == 0 else _rates(k % 6) for k in range(8)]
        wants = [_want(orc, hz, ch, lens, k % 6, tables[k]) for k in range(8)]
        tickets = []
        for k in range(8):
            x = pipe.pack(_streams(hz, ch, lens, k % 6))
            tickets.append(pipe.submit_jobs(x, lens, rate=tables[k]) if k % 4 != 0 else pipe.submit_jobs(x, lens))
            assert tickets[k] == k
            if k >= depth - 1:
                j = k - (depth - 1)
                _assert_equal(_host_outs(pipe, tickets[j], lens), wants[j], "depth %d ticket %d:" % (depth, j))
        for j in range(8 - (depth - 1), 8):
            _assert_equal(_host_outs(pipe, tickets[j], lens), wants[j], "depth %d ticket %d:" % (depth, j))
        pipe.close()
    finally:
        plan.close()


def test_full_width_batches_of_both_kinds_alternate(orc):
    """256 mono lanes at 16 kHz -- a walk workgroup per CU, so the kernels of neighbouring tickets really do run side by side -- depth
    3, six tickets with fresh content, batches of ones (the overlapped order on the library's streams) and batches at rate 1.25 (in
    sequence on the run stream) by turns: every lane's count and CRC are those of the batch call on the same table, lanes 0 / 128 /
    255 are the oracle's, a rate batch reports the sequential launch order and a batch of ones behind it the pipelined one."""
    from speedy_amd.batch import Batch, Pipeline, Plan
    from speedy_amd.synth import speech_like
    hz, n = 16000, 256
    lane = hz // 3
    plan = Plan(hz, False)
    try:
        x = speech_like(4 * hz, hz, seed=77)
        tables = [1.0 if k % 2 == 0 else 1.25 for k in range(6)]
        want, packed = [], []
        pipe = Pipeline(plan, [lane] * n, 1, 3.5, 1.0, 0.0, depth=3, rate=1.0)   # (rate 1 has the larger capacity of the two)
        for k, r in enumerate(tables):
            streams = [x[(211 * i + 5003 * k) % (x.size - lane):][:lane].copy() for i in range(n)]
            b = Batch(plan, [lane] * n, 1, 3.5, 1.0, 0.0, rate=r)
            b.upload(streams)
            b.run()
            outs = b.results()
            for i in (0, 128, 255):
                ref = oracle_rate_stream(orc, streams[i], hz, 1, 3.5, 1.0, r)
                assert ref.size > 1000 and np.array_equal(outs[i], ref), (k, i)
            want.append([(o.size, zlib.crc32(o.tobytes())) for o in outs])
            packed.append(pipe.pack(streams))
            del b
        assert len({tuple(w) for w in want}) == 6
        tickets, modes = [], []

        def check(k):
            got = [(o.size, zlib.crc32(o.tobytes())) for o in _host_outs(pipe, tickets[k], [lane] * n)]
            assert got == want[k], "ticket %d: lanes %s differ from the batch call" % (k, [i for i in range(n) if got[i] != want[k][i]][:8])

        for k, r in enumerate(tables):
            tickets.append(pipe.submit_jobs(packed[k], [lane] * n, rate=r))
            modes.append(plan.L.spx_debug_last_call_concurrent())
            if k >= 2:
                check(k - 2)
        for k in (4, 5):
            check(k)
        print("launch order per submit:", modes)
        assert [modes[k] for k in (1, 3, 5)] == [0, 0, 0] and [modes[k] for k in (2, 4)] == [2, 2], modes
        pipe.close()
    finally:
        plan.close()


def _static_layout(plan, lens, ch, rates):
    sp, nl, _ = _modes()
    caps = [plan.out_capacity(lens[i], sp[i], nl[i], rate=rates[i]) for i in range(N)]
    return caps, [int(v) for v in np.concatenate(([0], np.cumsum([(c * ch + 31) // 32 * 32 for c in caps])))]


def test_device_out(orc):
    """SPX_PIPELINE_DEVICE_OUT: the offsets are the static layout of the creation capacities in FINAL frames, the counts are in device
    memory, the bytes are the oracle's -- for rate batches and for a batch of ones (detached) between them."""
    from speedy_amd.batch import Plan
    hz, ch = 16000, 2
    plan = Plan(hz, False)
    try:
        lens = _lens(plan, hz)
        tables = [_rates(1), [1.0] * N, _rates(2)]
        sized = [min(t[i] for t in tables) for i in range(N)]   # (the batch of ones counts: rate 1 needs more room than rate 1.25)
        pipe = _pipeline(plan, hz, ch, 3, sized, device_out=True)
        _, static = _static_layout(plan, lens, ch, sized)
        tickets = [pipe.submit_jobs(pipe.pack(_streams(hz, ch, lens, k)), lens, rate=tables[k]) for k in range(3)]
        for k in range(3):
            want = _want(orc, hz, ch, lens, k, tables[k])
            ptr, offsets, cnt_ptr = pipe.wait(tickets[k])
            assert ptr and cnt_ptr and [int(v) for v in offsets] == static, k
            cnt = np.zeros(N, np.int64)
            pipe.L.spx_copy_to_host(cnt.ctypes.data, cnt_ptr, 8 * N, None)
            pipe.L.spx_stream_synchronize(None)
            assert [int(v) for v in cnt] == [w.size // ch for w in want], k
            _assert_equal(pipe.results(tickets[k]), want, "device out, ticket %d:" % k)
        pipe.close()
    finally:
        plan.close()


def test_float_samples(orc):
    """SPX_PIPELINE_FLOAT on a rate pipeline, host and device input, host and device output: every value is the int16 rate pipeline's
    (fed the defined conversion of the same floats) / 32767.0f, and FloatBatch's with the same rates.  A device input is a tensor of
    exactly the batch's extent, and input_consumed lets the caller overwrite an input of either kind while its batch still runs."""
    import torch
    from speedy_amd.batch import FloatBatch, Plan
    hz, ch = 16000, 2
    plan = Plan(hz, False)
    try:
        lens = _lens(plan, hz)
        sp, nl, fb = _modes()
        sized = [min(1.0, v) for v in _min_rates((3, 4))]   # (batches of ones run between the rate batches)
        ipipe = _pipeline(plan, hz, ch, 2, sized)
        hpipe = _pipeline(plan, hz, ch, 2, sized, float_samples=True)
        dpipe = _pipeline(plan, hz, ch, 2, sized, float_samples=True, device_out=True)
        dense = [int(v) for v in np.concatenate(([0], np.cumsum([n * ch for n in lens])[:-1]))]
        for k in (3, 4):
            rates = _rates(k)
            fl = [s.astype(np.float32) / np.float32(32768.0) for s in _streams(hz, ch, lens, k)]
            t16 = ipipe.submit_jobs(ipipe.pack([float_to_short_def(s, nl[i] != 0.0) for i, s in enumerate(fl)]), lens, rate=rates)
            want = [o.astype(np.float32) / np.float32(32767.0) for o in _host_outs(ipipe, t16, lens)]
            assert sum(w.size for w in want) // ch > 5000
            b = FloatBatch(plan, lens, ch, sp, nl, fb, rate=rates)
            b.upload(fl)
            b.run()
            _assert_equal(b.results(), want, "FloatBatch, table %d:" % k)
            spare = hpipe.pack(_streams(hz, ch, lens, 0)).astype(np.float32) / np.float32(32768.0)
            for pipe in (hpipe, dpipe):
                for kind in ("host", "device"):
                    if kind == "host":
                        x = torch.from_numpy(pipe.pack(fl)).pin_memory()
                        t = pipe.submit_jobs(x, lens, rate=rates)
                    else:
                        x = torch.from_numpy(np.concatenate(fl)).cuda()   # exactly the batch's extent: no padding behind the last value
                        assert x.numel() == sum(lens) * ch
                        torch.cuda.synchronize()
                        t = pipe.submit_jobs(x, lens, in_offs=dense, rate=rates)
                    pipe.input_consumed(t)
                    x.fill_(float("nan"))
                    torch.cuda.synchronize()
                    t2 = pipe.submit_jobs(spare, lens)   # (a batch of ones behind it, from another buffer)
                    assert t2 == t + 1
                    got = pipe.results(t) if pipe is dpipe else _host_outs(pipe, t, lens)
                    assert all(g.dtype == np.float32 for g in got)
                    _assert_equal(got, want, "float, %s input, %s output, table %d:" % (kind, "device" if pipe is dpipe else "host", k))
        for p in (ipipe, hpipe, dpipe):
            p.close()
    finally:
        plan.close()


def test_refusals_use_up_no_ticket(orc):
    """A rate of 0, -1, NaN, +inf or 1e6 in lane 3 at creation, at fit and at submit; a rate whose capacity in final frames exceeds
    the lane's; the _rate calls on an ordinary pipeline: -1 (NULL) with the lane and the limit in the message, no ticket used up, the
    batch in flight across the refusals untouched.  And a lane created at rate 1 takes rate 2."""
    from speedy_amd._lib import StreamJob
    from speedy_amd.batch import Pipeline, Plan
    hz, ch = 16000, 1
    plan = Plan(hz, False)
    L = plan.L
    try:
        lens = _lens(plan, hz)
        sp, nl, fb = _modes()
        fptr = lambda v: np.ascontiguousarray(v, np.float32).ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731

        def refused(rc, *needles):
            msg = (L.spx_last_error() or b"").decode()
            assert rc in (-1, None) and all(n in msg for n in needles), (rc, msg, needles)

        # ---- creation ----
        jobs = (StreamJob * N)()
        off = 0
        for i in range(N):
            jobs[i].in_off, jobs[i].n_in, jobs[i].channels = off, lens[i], ch
            jobs[i].speed, jobs[i].nonlinear, jobs[i].feedback = sp[i], nl[i], fb[i]
            off += lens[i] * ch
        for bad in (0.0, -1.0, float("nan"), float("inf"), 1.0e6):
            r = [1.25] * N
            r[3] = bad
            refused(L.spx_pipeline_create_rate(plan.h, jobs, fptr(r), N, 2, 0), "spx_pipeline: lane 3:", "rate")
        jobs[3].speed = 0.0
        refused(L.spx_pipeline_create_rate(plan.h, jobs, fptr([1.25] * N), N, 2, 0), "spx_pipeline: lane 3:", "speed")
        # ---- fit and submit: lanes created at rate 1 ----
        pipe = _pipeline(plan, hz, ch, 2, 1.0)
        packed = pipe.pack(_streams(hz, ch, lens, 0))
        live_rates = [2.0] * N   # a lane created at rate 1 accepts rate 2
        assert pipe.fits(lens, rate=live_rates)
        live = pipe.submit_jobs(packed, lens, rate=live_rates)
        assert live == 0
        table = pipe.table(lens)
        for bad in (0.0, -1.0, float("nan"), float("inf"), 1.0e6):
            r = [1.25] * N
            r[3] = bad
            refused(L.spx_pipeline_jobs_fit_rate(pipe.h, table, fptr(r)), "lane 3", "rate")
            refused(L.spx_pipeline_submit_jobs_rate(pipe.h, table, fptr(r), packed.ctypes.data, 0), "lane 3", "rate")
            assert not pipe.fits(lens, rate=r)
        # a rate whose capacity in final frames exceeds the lane's, by the function's own values
        cap1 = plan.out_capacity(lens[8], sp[8], nl[8], rate=1.0)
        cap_half = plan.out_capacity(lens[8], sp[8], nl[8], rate=0.5)
        assert cap_half > cap1
        r = [1.0] * N
        r[8] = 0.5
        refused(L.spx_pipeline_jobs_fit_rate(pipe.h, table, fptr(r)), "lane 8", str(cap_half), str(cap1), "spx_plan_out_capacity_rate")
        refused(L.spx_pipeline_submit_jobs_rate(pipe.h, table, fptr(r), packed.ctypes.data, 0), "lane 8", str(cap_half), str(cap1))
        with pytest.raises(RuntimeError, match="lane 8"):
            pipe.submit_jobs(packed, lens, rate=r)
        nxt_rates = [[1.25, 1.0, 2.0, 3.0][i % 4] for i in range(N)]
        assert pipe.fits(lens, rate=nxt_rates)
        nxt = pipe.submit_jobs(packed, lens, rate=nxt_rates)
        assert nxt == 1   # behind all the refusals: the next ticket, none skipped
        _assert_equal(_host_outs(pipe, live, lens), _want(orc, hz, ch, lens, 0, live_rates), "the batch in flight across the refusals:")
        _assert_equal(_host_outs(pipe, nxt, lens), _want(orc, hz, ch, lens, 0, nxt_rates), "the submit behind them:")
        # ---- the _rate calls on an ordinary pipeline ----
        opipe = Pipeline(plan, lens, ch, sp, nl, fb, depth=2)
        live = opipe.submit(packed)
        ones = fptr([1.0] * N)
        refused(L.spx_pipeline_jobs_fit_rate(opipe.h, table, ones), "spx_pipeline_create_rate")
        refused(L.spx_pipeline_submit_jobs_rate(opipe.h, table, ones, packed.ctypes.data, 0), "spx_pipeline_create_rate")
        refused(L.spx_pipeline_submit_jobs_rate_float(opipe.h, table, ones, packed.ctypes.data, 0), "spx_pipeline_create_rate")
        refused(L.spx_pipeline_submit_jobs_rate(opipe.h, table, None, packed.ctypes.data, 0), "spx_pipeline_create_rate")
        assert opipe.submit(packed) == live + 1
        want = _want(orc, hz, ch, lens, 0, [1.0] * N)
        _assert_equal(_host_outs(opipe, live, lens), want, "the ordinary pipeline, in flight across the refusals:")
        _assert_equal(_host_outs(opipe, live + 1, lens), want, "the ordinary pipeline, behind them:")
        # the int16 / float wrong-kind rule stays: the int16 _rate call on a float rate pipeline names the flag
        fpipe = _pipeline(plan, hz, ch, 2, 1.0, float_samples=True)
        refused(L.spx_pipeline_submit_jobs_rate(fpipe.h, table, ones, packed.ctypes.data, 0), "SPX_PIPELINE_FLOAT")
        refused(L.spx_pipeline_submit_jobs_rate_float(pipe.h, table, ones, packed.ctypes.data, 0), "SPX_PIPELINE_FLOAT")
        for p in (pipe, opipe, fpipe):
            p.close()
    finally:
        plan.close()


def test_c_example_prints_the_oracles_counts_and_crcs(orc, tmp_path):
    """tools/pipeline_rate_example.c (plain C99 over include/speedy_hip.h): two batches of one lane per rate, the second with the
    rate list reversed, on the first 3 s of tests/golden/tapestry.wav."""
    exe = os.path.join(ROOT, "speedy_amd", "lib", "pipeline_rate_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "piperateexample"])
    x, hz, ch = read_wav("tapestry.wav")
    x = x[: 3 * hz * ch]
    raw = str(tmp_path / "in.raw")
    x.astype("<i2").tofile(raw)
    rates = [1.0, 1.25, 0.5, 2.0]
    r = subprocess.run([exe, raw, str(hz), str(ch), "3.5", "1.0"] + [str(v) for v in rates], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("batch ")]
    assert len(lines) == 2 * len(rates), r.stdout
    ref = {v: oracle_rate_stream(orc, x, hz, ch, 3.5, 1.0, v) for v in rates}
    for b, table in enumerate((rates, rates[::-1])):
        for i, v in enumerate(table):
            f = lines[b * len(rates) + i]
            assert (int(f[1]), int(f[3]), float(f[5])) == (b, i, v), f
            assert int(f[7]) == ref[v].size // ch > 1000, (f, ref[v].size // ch)
            assert int(f[9], 16) == zlib.crc32(ref[v].astype("<i2").tobytes()), f
