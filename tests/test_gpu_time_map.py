"""spx_batch_run_map and spx_map_lookup on the MI355X.

Every comparison is exact.  A job's expected rows are the oracle stream's, observed through its hand-off callback
(tests/time_map_ref.py; tests/test_time_map_abi.py shows they do not depend on the chunking); out, n_out and the speed tap are
compared with spx_batch_run's on the same table, byte for byte; the lookups with the numpy statement of the definition."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_map_ref as tm  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 0x5a5a
# (sample rate, channels, [(n_in, speed, nonlinear, feedback)])
TABLE8 = (16000, 1, [(4000, 3.5, 1.0, 0.0), (3200, 2.0, 0.5, 0.0), (700, 3.5, 1.0, 0.2), (160, 3.5, 1.0, 0.0), (159, 3.5, 1.0, 0.0),
                     (0, 3.5, 1.0, 0.0), (8000, 0.5, 1.0, 0.0), (4000, 2.0, 0.0, 0.0)])
CASES = {
    "table8": TABLE8,
    "22k-stereo": (22050, 2, [(11025, 1.5, 1.0, 0.0)]),
    "11k-mono": (11025, 1, [(5512, 3.0, 1.0, 0.0)]),
    "16k-stereo": (16000, 2, [(4000, 3.5, 1.0, 0.0)]),   # the walk window with the raw plane
}

_REF = {}


def _case(orc, name, mm):
    """(streams, oracle rows per job) of a case, computed once per hysteresis mode."""
    key = (name, mm)
    if key not in _REF:
        rate_hz, ch, jobs = CASES[name]
        streams = [tm.signal(rate_hz, ch, n, seed=900 + 31 * i) for i, (n, _s, _nl, _fb) in enumerate(jobs)]
        rows = [tm.oracle_map(orc, x, rate_hz, ch, s, nl, mm, fb, chunk=1000)[0] for x, (_n, s, nl, fb) in zip(streams, jobs)]
        _REF[key] = (streams, rows)
    return _REF[key]


def _batch(plan, name, **kw):
    from speedy_amd.batch import Batch
    rate_hz, ch, jobs = CASES[name]
    return Batch(plan, [j[0] for j in jobs], ch, [j[1] for j in jobs], [j[2] for j in jobs], [j[3] for j in jobs], taps=True, **kw)


def _snapshot(b):
    import torch
    torch.cuda.synchronize(b.device)
    return b.d_nout.cpu().numpy().copy(), b.d_out.cpu().numpy().copy(), b.t_speed.cpu().numpy().tobytes()


@pytest.mark.parametrize("mm", [False, True], ids=["plain", "matlab"])
@pytest.mark.parametrize("name", list(CASES))
def test_map_equals_the_oracles_and_the_rest_is_spx_batch_run(orc, name, mm):
    from speedy_amd.batch import Plan
    rate_hz, ch, jobs = CASES[name]
    streams, want = _case(orc, name, mm)
    plan = Plan(rate_hz, mm)
    try:
        p = _batch(plan, name)
        p.upload(streams)
        p.run()
        nout, out, speed = _snapshot(p)
        assert (nout >= 0).all()
        b = _batch(plan, name, time_map=True)
        b.upload(streams)
        b.d_map.fill_(-12345)
        b.run()
        nout_m, out_m, speed_m = _snapshot(b)
        assert np.array_equal(nout_m, nout), "n_out differs from spx_batch_run's: %s against %s" % (nout_m, nout)
        assert np.array_equal(out_m, out), "out differs from spx_batch_run's"
        assert speed_m == speed and np.frombuffer(speed, np.uint8).any(), "the speed tap differs from spx_batch_run's"
        assert b.map_offs[-1] == sum(w.size for w in want) == b.d_map.numel()
        for i, (n, _s, nl, _fb) in enumerate(jobs):
            assert plan.L.spx_plan_map_rows(plan.h, n, nl) == want[i].size == tm.map_rows(plan.B, n, nl)
            got = b.time_map(i)
            assert np.array_equal(got, want[i]), "job %d: rows %s, the oracle has %s" % (i, got, want[i])
            assert got[-1] == nout[i]
    finally:
        plan.close()


def _queries(M, B, n, nl):
    """Every node, every position of a short stream (a spread of a long one's), both ends out of range."""
    X, Y = tm.nodes(M, B, n, nl)
    edge = np.asarray([-5, -1, n + 1, n + 1000, Y[-1] + 1, Y[-1] + 77], np.int64)
    t = np.arange(0, n + 1, dtype=np.int64) if n <= 4000 else np.arange(0, n + 1, 7, dtype=np.int64)
    u = np.arange(0, Y[-1] + 1, dtype=np.int64)
    return np.concatenate([X, X - 1, X + 1, t, edge]), np.concatenate([Y, Y - 1, Y + 1, u, edge])


def test_lookup_matches_the_numpy_definition(orc):
    """spx_map_lookup, forward and inverse, over the eight-job table: nodes, every u of every stream, out-of-range queries, and
    one stream with no query at all."""
    from speedy_amd.batch import Plan
    rate_hz, ch, jobs = TABLE8
    streams, want = _case(orc, "table8", False)
    plan = Plan(rate_hz, False)
    try:
        b = _batch(plan, "table8", time_map=True)
        b.upload(streams)
        b.run()
        qs = [_queries(want[i], plan.B, n, nl) for i, (n, _s, nl, _fb) in enumerate(jobs)]
        empty = np.zeros(0, np.int64)
        skip = 2   # this stream asks nothing
        fw = b.lookup_all([empty if i == skip else q[0] for i, q in enumerate(qs)])
        iv = b.lookup_all([empty if i == skip else q[1] for i, q in enumerate(qs)], inverse=True)
        assert fw[skip].size == 0 and iv[skip].size == 0
        for i, (n, _s, nl, _fb) in enumerate(jobs):
            if i == skip:
                continue
            assert np.array_equal(b.time_map(i), want[i])
            assert np.array_equal(fw[i], tm.forward(want[i], plan.B, n, nl, qs[i][0])), "forward, job %d" % i
            assert np.array_equal(iv[i], tm.inverse(want[i], plan.B, n, nl, qs[i][1])), "inverse, job %d" % i
        # one stream alone through Batch.lookup
        n, _s, nl, _fb = jobs[skip]
        assert np.array_equal(b.lookup(skip, qs[skip][0]), tm.forward(want[skip], plan.B, n, nl, qs[skip][0]))
        assert np.array_equal(b.lookup(skip, qs[skip][1], inverse=True), tm.inverse(want[skip], plan.B, n, nl, qs[skip][1]))
    finally:
        plan.close()


def test_refusals_launch_nothing_and_a_good_call_works_right_after(orc):
    """A null map, a bad speed in the LAST job, a workspace that is too small: -1 with a message, out / n_out / map untouched;
    the same buffers then serve a good call."""
    import torch
    from speedy_amd.batch import Plan
    rate_hz, ch, jobs = TABLE8
    streams, want = _case(orc, "table8", False)
    plan = Plan(rate_hz, False)
    try:
        L = plan.L
        b = _batch(plan, "table8", time_map=True)
        b.upload(streams)
        hs = torch.cuda.current_stream().cuda_stream

        def call(ws_bytes=None, null_map=False):
            b.d_out.fill_(CANARY)
            b.d_nout.fill_(-77)
            b.d_map.fill_(-78)
            rc = L.spx_batch_run_map(plan.h, b.jobs, b.n, b.d_in.data_ptr(), b.d_out.data_ptr(), b.d_nout.data_ptr(),
                                     None if null_map else b.d_map.data_ptr(), b.d_ws.data_ptr(),
                                     b.d_ws.numel() if ws_bytes is None else ws_bytes, C.byref(b.taps), hs)
            msg = L.spx_last_error().decode() if rc != 0 else ""
            torch.cuda.synchronize()
            untouched = bool((b.d_out == CANARY).all()) and bool((b.d_nout == -77).all()) and bool((b.d_map == -78).all())
            return rc, msg, untouched

        rc, msg, untouched = call(null_map=True)
        assert rc == -1 and "map" in msg and untouched, (rc, msg, untouched)
        good = b.jobs[b.n - 1].speed
        b.jobs[b.n - 1].speed = float("nan")
        rc, msg, untouched = call()
        assert rc == -1 and "speed" in msg and untouched, (rc, msg, untouched)
        rc_plain = L.spx_batch_run(plan.h, b.jobs, b.n, b.d_in.data_ptr(), b.d_out.data_ptr(), b.d_nout.data_ptr(), b.d_ws.data_ptr(),
                                   b.d_ws.numel(), None, hs)
        assert rc_plain == -1 and L.spx_last_error().decode() == msg, "the message is spx_batch_run's"
        b.jobs[b.n - 1].speed = good
        need = L.spx_batch_workspace_bytes(plan.h, b.jobs, b.n)
        rc, msg, untouched = call(ws_bytes=need - 1)
        assert rc == -1 and "workspace" in msg and untouched, (rc, msg, untouched)
        rc, msg, untouched = call(ws_bytes=need)   # exactly spx_batch_workspace_bytes is enough
        assert rc == 0 and not untouched, msg
        for i in range(b.n):
            assert np.array_equal(b.time_map(i), want[i]), "job %d after the refusals" % i
        assert np.array_equal(b.d_nout.cpu().numpy(), [w[-1] for w in want])
    finally:
        plan.close()
