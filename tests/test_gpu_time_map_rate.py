"""spx_batch_run_rate_map and spx_batch_run_float_map on the MI355X: the time map of a call with playback rates, in final frames.

Every comparison is exact.  A job's expected rows are the oracle stream's with sonicSetRate set, observed at every hand-off
(tests/time_map_rate_ref.py; tests/test_time_map_rate_abi.py shows that they are F of the rows at rate 1 and do not depend on the
chunking); out and n_out are compared with spx_batch_run_rate's (spx_batch_run_float's) on the same table, byte for byte; the
lookups with time_map_ref.ExactMap on the same rows."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_map_rate_ref as tr  # noqa: E402
import time_map_ref as tm  # noqa: E402

pytestmark = pytest.mark.gpu

MAP_CANARY = -12345
RATE_HZ = 16000
# (n_in, speed, nonlinear, feedback, rate): 16 kHz mono.  The last job has 301 rows: more than one block has threads.
JOBS = [(4000, 3.5, 1.0, 0.0, 1.3), (8000, 0.5, 1.0, 0.1, 2.0), (3200, 2.0, 0.5, 0.1, 0.75), (159, 3.0, 1.0, 0.0, 2.0),
        (160, 3.0, 1.0, 0.0, 0.5), (4000, 2.0, 0.0, 0.0, 1.3), (0, 3.5, 1.0, 0.0, 2.0), (4000, 3.5, 1.0, 0.0, 1.0),
        (48000, 0.8, 1.0, 0.1, 3.0)]
ONE = 7   # the job with rate 1
RATES = [j[4] for j in JOBS]

_REF = {}


def _streams():
    if "streams" not in _REF:
        _REF["streams"] = [tm.signal(RATE_HZ, 1, j[0], seed=900 + 31 * i) for i, j in enumerate(JOBS)]
    return _REF["streams"]


def _want(orc, mm=False):
    """The oracle's rows of every job of the table at its rate, computed once per hysteresis mode."""
    if ("rows", mm) not in _REF:
        _REF[("rows", mm)] = [tr.oracle_rate_map(orc, x, RATE_HZ, 1, s, nl, fb, r, 1000, mm)
                              for x, (_n, s, nl, fb, r) in zip(_streams(), JOBS)]
    return _REF[("rows", mm)]


def _batch(plan, cls=None, jobs=JOBS, ch=1, **kw):
    from speedy_amd.batch import Batch
    return (cls or Batch)(plan, [j[0] for j in jobs], ch, [j[1] for j in jobs], [j[2] for j in jobs], [j[3] for j in jobs], **kw)


def _snapshot(b):
    import torch
    torch.cuda.synchronize(b.device)
    return b.d_nout.cpu().numpy().copy(), b.d_out.cpu().numpy().copy()


def _all_rows(b):
    import torch
    torch.cuda.synchronize(b.device)
    return b.d_map.cpu().numpy().copy()


def _run_with_map(plan, streams, **kw):
    b = _batch(plan, time_map=True, **kw)
    b.upload(streams)
    b.d_map.fill_(MAP_CANARY)
    b.run()
    return b


def _check_rows(b, want, nout):
    rows = _all_rows(b)
    assert b.map_offs[-1] == rows.size == sum(w.size for w in want)
    assert not (rows == MAP_CANARY).any(), "cells left unwritten: %s" % np.nonzero(rows == MAP_CANARY)[0][:8]
    for i, w in enumerate(want):
        got = rows[b.map_offs[i]:b.map_offs[i + 1]]
        assert np.array_equal(got, w), "job %d: rows %s, the oracle has %s" % (i, got, w)
        assert got[-1] == nout[i], "job %d: the last row is not n_out" % i
    return rows


@pytest.mark.parametrize("mm", [False, True], ids=["plain", "matlab"])
def test_one_mixed_call(orc, mm):
    """Nine jobs, eight of them with a rate other than 1: out and n_out are spx_batch_run_rate's, every cell of the canary-filled
    map is written, every stream's rows are the oracle's, the last row is n_out, the rate-1 job's rows are spx_batch_run_map's."""
    from speedy_amd.batch import Plan
    streams, want = _streams(), _want(orc, mm)
    plan = Plan(RATE_HZ, mm)
    try:
        p = _batch(plan, rate=RATES)
        p.upload(streams)
        p.run()
        nout, out = _snapshot(p)
        assert (nout >= 0).all()
        b = _run_with_map(plan, streams, rate=RATES)
        nout_m, out_m = _snapshot(b)
        assert np.array_equal(nout_m, nout), "n_out differs from spx_batch_run_rate's: %s against %s" % (nout_m, nout)
        assert np.array_equal(out_m, out), "out differs from spx_batch_run_rate's"
        for i, (n, _s, nl, _fb, _r) in enumerate(JOBS):
            assert plan.L.spx_plan_map_rows(plan.h, n, nl) == want[i].size
        _check_rows(b, want, nout)
        m = _run_with_map(plan, streams)   # spx_batch_run_map
        assert np.array_equal(b.time_map(ONE), m.time_map(ONE))
    finally:
        plan.close()


def test_halving_and_channels(orc):
    """22.05 kHz stereo at 1.3 -- (16961, 22050) is halved to (8480, 11025) and drops a bit -- and at 0.5, halved twice."""
    from speedy_amd.batch import Plan
    jobs = [(11025, 1.5, 1.0, 0.0, 1.3), (11025, 1.5, 1.0, 0.0, 0.5)]
    assert tr.rate_pair(22050, 1.3) == (8480, 11025)
    rates = [j[4] for j in jobs]
    streams = [tm.signal(22050, 2, j[0], seed=900 + 31 * i) for i, j in enumerate(jobs)]
    want = [tr.oracle_rate_map(orc, x, 22050, 2, s, nl, fb, r, 1000) for x, (_n, s, nl, fb, r) in zip(streams, jobs)]
    plan = Plan(22050, False)
    try:
        p = _batch(plan, jobs=jobs, ch=2, rate=rates)
        p.upload(streams)
        p.run()
        nout, out = _snapshot(p)
        b = _run_with_map(plan, streams, jobs=jobs, ch=2, rate=rates)
        nout_m, out_m = _snapshot(b)
        assert (nout >= 0).all() and np.array_equal(nout_m, nout) and np.array_equal(out_m, out)
        _check_rows(b, want, nout)
    finally:
        plan.close()


def test_all_ones_is_spx_batch_run_map():
    """rates == NULL, and every rate 1: rows, out and n_out are spx_batch_run_map's, byte for byte."""
    import torch
    from speedy_amd.batch import Plan
    streams = _streams()
    plan = Plan(RATE_HZ, False)
    try:
        m = _run_with_map(plan, streams)   # spx_batch_run_map
        nout, out = _snapshot(m)
        rows = _all_rows(m)
        assert (nout >= 0).all() and not (rows == MAP_CANARY).any()
        ones = _run_with_map(plan, streams, rate=1.0)
        assert np.array_equal(_all_rows(ones), rows)
        assert all(np.array_equal(a, b) for a, b in zip(_snapshot(ones), (nout, out)))
        # rates == NULL: the C call on a map batch's own buffers (the workspace is spx_batch_workspace_bytes then)
        b = _batch(plan, time_map=True)
        b.upload(streams)
        b.d_map.fill_(MAP_CANARY)
        rc = plan.L.spx_batch_run_rate_map(plan.h, b.jobs, None, b.n, b.d_in.data_ptr(), b.d_out.data_ptr(), b.d_nout.data_ptr(),
                                           b.d_map.data_ptr(), b.d_ws.data_ptr(), b.d_ws.numel(), None,
                                           torch.cuda.current_stream().cuda_stream)
        assert rc == 0, plan.L.spx_last_error().decode()
        assert np.array_equal(_all_rows(b), rows)
        assert all(np.array_equal(a, c) for a, c in zip(_snapshot(b), (nout, out)))
    finally:
        plan.close()


@pytest.mark.parametrize("chunks", [2, 3])
def test_forced_time_chunks(orc, chunks):
    """The table under spx_set_pipeline_chunks(2) and (3): the call runs in that many chunks on the general kernel, and the rows
    conversion -- once, behind the rate kernel of the whole call -- leaves the rows and bytes of the unchunked call."""
    from speedy_amd.batch import Plan
    streams, want = _streams(), _want(orc)
    plan = Plan(RATE_HZ, False)
    try:
        u = _run_with_map(plan, streams, rate=RATES)
        nout, out = _snapshot(u)
        rows = _check_rows(u, want, nout)
        plan.L.spx_set_pipeline_chunks(chunks)
        b = _run_with_map(plan, streams, rate=RATES)
        nout_c, out_c = _snapshot(b)
        ran, form = plan.L.spx_debug_last_call_chunks(), plan.L.spx_debug_last_walk_form()
        assert ran == chunks and form == 0, (ran, form)
        assert np.array_equal(nout_c, nout) and np.array_equal(out_c, out)
        assert np.array_equal(_all_rows(b), rows)
    finally:
        plan.L.spx_set_pipeline_chunks(1)
        plan.close()


def test_float_samples(orc):
    """FloatBatch(time_map=True): the rows are Batch(rate=, time_map=True)'s on the int16 values the defined conversion gives, and
    the oracle float stream's; out is spx_batch_run_float's as bit patterns."""
    from speedy_amd.batch import FloatBatch, Plan
    from test_batch_float_abi import float_to_short_def
    xs = [(x.astype(np.float32) / np.float32(32768.0) * np.float32(0.97)).astype(np.float32) for x in _streams()]
    assert all(np.abs(x).max() < 1.0 for x in xs if x.size)
    plan = Plan(RATE_HZ, False)
    try:
        p = _batch(plan, FloatBatch, rate=RATES)
        p.upload(xs)
        p.run()
        nout, out = _snapshot(p)
        assert (nout >= 0).all()
        f = _run_with_map(plan, xs, cls=FloatBatch, rate=RATES)
        nout_f, out_f = _snapshot(f)
        assert np.array_equal(nout_f, nout) and np.array_equal(out_f.view(np.uint32), out.view(np.uint32))
        rows = _all_rows(f)
        assert not (rows == MAP_CANARY).any()
        b = _run_with_map(plan, [float_to_short_def(x, j[2]) for x, j in zip(xs, JOBS)], rate=RATES)
        assert np.array_equal(_all_rows(b), rows), "the float call's rows are not the int16 call's on the converted samples"
        want = [tr.oracle_rate_map_float(orc, x, RATE_HZ, 1, s, nl, fb, r, 1000) for x, (_n, s, nl, fb, r) in zip(xs, JOBS)]
        _check_rows(f, want, nout)
    finally:
        plan.close()


def test_lookups_on_a_rate_map(orc):
    """spx_map_lookup, forward and inverse, on the table's rate map: nodes, +-1 around them, flat runs, out of range, against ExactMap
    on the same rows -- the output side in final frames -- and forward(inverse(u)) <= u."""
    from speedy_amd.batch import Plan
    from test_gpu_time_map import _queries
    streams, want = _streams(), _want(orc)
    plan = Plan(RATE_HZ, False)
    try:
        b = _run_with_map(plan, streams, rate=RATES)
        qs = [_queries(want[i], plan.B, j[0], j[2]) for i, j in enumerate(JOBS)]
        fw = b.lookup_all([q[0] for q in qs])
        iv = b.lookup_all([q[1] for q in qs], inverse=True)
        us = [np.arange(0, int(w[-1]) + 1, dtype=np.int64) for w in want]
        back = b.lookup_all(b.lookup_all(us, inverse=True))
        for i, j in enumerate(JOBS):
            assert np.array_equal(b.time_map(i), want[i])
            exact = tm.ExactMap(want[i], plan.B, j[0], j[2])
            assert fw[i].tolist() == [exact.forward(t) for t in qs[i][0]], "forward, job %d" % i
            assert iv[i].tolist() == [exact.inverse(u) for u in qs[i][1]], "inverse, job %d" % i
            assert (back[i] <= us[i]).all(), "forward(inverse(u)) > u, job %d" % i
        assert np.array_equal(b.lookup(0, qs[0][0]), fw[0])
    finally:
        plan.close()


def test_refusals_launch_nothing_and_a_good_call_works_right_after(orc):
    """A NULL map, a rate of 0, a rate so large that (int)(sample rate / rate) < 1, a speed of 0, a float `in` that is not 4-byte
    aligned: -1 with a message, n_out and the canary map untouched; the same buffers then serve a good call."""
    import torch
    from speedy_amd.batch import FloatBatch, Plan
    streams, want = _streams(), _want(orc)
    plan = Plan(RATE_HZ, False)
    try:
        L = plan.L
        hs = torch.cuda.current_stream().cuda_stream
        b = _batch(plan, rate=RATES, time_map=True)
        b.upload(streams)
        f = _batch(plan, FloatBatch, rate=RATES, time_map=True)
        f.upload([x.astype(np.float32) / np.float32(32768.0) for x in streams])

        def call(x, fn, rates=None, null_map=False, in_ptr=None):
            x.d_nout.fill_(-77)
            x.d_map.fill_(MAP_CANARY)
            r = np.asarray(RATES if rates is None else rates, np.float32)
            rc = fn(plan.h, x.jobs, r.ctypes.data_as(C.POINTER(C.c_float)), x.n, in_ptr or x.d_in.data_ptr(), x.d_out.data_ptr(),
                    x.d_nout.data_ptr(), None if null_map else x.d_map.data_ptr(), x.d_ws.data_ptr(), x.d_ws.numel(), None, hs)
            msg = L.spx_last_error().decode() if rc != 0 else ""
            torch.cuda.synchronize()
            return rc, msg, bool((x.d_nout == -77).all()) and bool((x.d_map == MAP_CANARY).all())

        for x, fn in ((b, L.spx_batch_run_rate_map), (f, L.spx_batch_run_float_map)):
            rc, msg, untouched = call(x, fn, null_map=True)
            assert rc == -1 and "map" in msg and untouched, (rc, msg, untouched)
            rc, msg, untouched = call(x, fn, rates=RATES[:-1] + [0.0])
            assert rc == -1 and "rate" in msg and untouched, (rc, msg, untouched)
            rc, msg, untouched = call(x, fn, rates=RATES[:-1] + [1e9])
            assert rc == -1 and "rate too large" in msg and untouched, (rc, msg, untouched)
            good = x.jobs[x.n - 1].speed
            x.jobs[x.n - 1].speed = 0.0
            rc, msg, untouched = call(x, fn)
            x.jobs[x.n - 1].speed = good
            assert rc == -1 and "speed" in msg and untouched, (rc, msg, untouched)
        rc, msg, untouched = call(f, L.spx_batch_run_float_map, in_ptr=f.d_in.data_ptr() + 2)
        assert rc == -1 and "aligned" in msg and untouched, (rc, msg, untouched)
        rc, msg, untouched = call(b, L.spx_batch_run_rate_map)
        assert rc == 0 and not untouched, msg
        _check_rows(b, want, b.d_nout.cpu().numpy())
        rc, msg, untouched = call(f, L.spx_batch_run_float_map)
        assert rc == 0 and not untouched and not (_all_rows(f) == MAP_CANARY).any(), msg
        assert np.array_equal(_all_rows(f)[f.map_offs[1] - 1:f.map_offs[1]], f.d_nout.cpu().numpy()[:1])
    finally:
        plan.close()


def test_c_example_prints_the_oracles_rows_and_the_exact_answers(orc, tmp_path):
    """tools/batch_rate_map_example.c (plain C99 over include/speedy_hip.h): one clip at rate 1.25, two caption times both ways."""
    exe = os.path.join(ROOT, "speedy_amd", "lib", "batch_rate_map_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "ratemapexample"])
    n, speed, nl, rate, captions = 8000, 3.5, 1.0, 1.25, (2000, 6500)
    x = tm.signal(RATE_HZ, 1, n, seed=77)
    raw = str(tmp_path / "in.raw")
    x.astype("<i2").tofile(raw)
    r = subprocess.run([exe, raw, str(RATE_HZ), "1", str(speed), str(nl), str(rate)] + [str(t) for t in captions],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = tr.oracle_rate_map(orc, x, RATE_HZ, 1, speed, nl, 0.0, rate, 1000)
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert [int(ln[1]) for ln in lines if ln[0] == "frames"] == [int(want[-1])], r.stdout
    assert [(int(ln[1]), int(ln[2])) for ln in lines if ln[0] == "row"] == list(enumerate(want.tolist())), r.stdout
    exact = tm.ExactMap(want, RATE_HZ // 100, n, nl)
    caps = [ln for ln in lines if ln[0] == "caption"]
    assert len(caps) == 2, r.stdout
    for i, t in enumerate(captions):
        u = exact.forward(t)
        assert [int(caps[i][k]) for k in (1, 3, 5, 7)] == [i, t, u, exact.inverse(u)], caps[i]
        assert 0 < u < want[-1]
