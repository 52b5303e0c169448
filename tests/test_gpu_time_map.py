"""spx_batch_run_map and spx_map_lookup on the MI355X.

Every comparison is exact.  A job's expected rows are the oracle stream's, observed through its hand-off callback
(tests/time_map_ref.py; tests/test_time_map_abi.py shows they do not depend on the chunking); out, n_out and the speed tap are
compared with spx_batch_run's on the same table, byte for byte; the lookups with the numpy statement of the definition.
Map calls in time chunks -- forced, and by the engine's own rule above two streams per CU -- assert the chunk count they ran in.
(The rows against their own definition: tests/test_gpu_tsm_definition.py; the lookups on planted maps: tests/test_gpu_map_lookup.py.)"""
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


# ------------------------------------------------------------------ map calls in time chunks ------------------------------------------------------------------
# A call of more than two streams per CU runs in two time chunks by itself (speedy_amd/csrc/spx_mode.h), spx_set_pipeline_chunks
# forces any count: every chunk but the first runs the map kernel on a RESUMED job (events from `handed` on, the last row under
# the flush alone), and every chunk's job records carry the stream's map_row.

SPEEDS, NONLINEARS, FEEDBACKS = (3.5, 1.5, 0.8), (1.0, 0.5), (0.0, 0.1)
MAP_CANARY = -12345


def _knobs(i):
    """Every (speed, nonlinear, feedback) combination, twelve of them, by index."""
    return SPEEDS[i % 3], NONLINEARS[(i // 3) % 2], FEEDBACKS[(i // 6) % 2]


def _chunk_streams(lengths):
    """[(signal, speed, nonlinear, feedback)] -- one distinct stream per length."""
    return [(tm.signal(16000, 1, n, seed=4100 + 17 * i),) + _knobs(i) for i, n in enumerate(lengths)]


def _want_rows(orc, s):
    """The oracle's rows of a distinct stream, once per (signal, speed, nonlinear, feedback)."""
    x, speed, nl, fb = s
    key = ("chunks", x.size, x.tobytes()[:64], speed, nl, fb)
    if key not in _REF:
        _REF[key] = tm.oracle_map(orc, x, 16000, 1, speed, nl, False, fb, chunk=1000)[0]
    return _REF[key]


def _map_call_against_the_plain_call(orc, plan, streams, before_map_call=None):
    """spx_batch_run, then spx_batch_run_map on the same table (before_map_call() in between): out and n_out byte-equal, every
    stream's rows the oracle's, every cell of the canary-filled map written and none outside the streams' ranges to write.
    Returns (the plain call's chunk count, the map call's, the map call's walk form)."""
    from speedy_amd.batch import Batch
    L = plan.L
    args = ([s[0].size for s in streams], 1, [s[1] for s in streams], [s[2] for s in streams], [s[3] for s in streams])
    p = Batch(plan, *args)
    p.upload([s[0] for s in streams])
    p.run()
    nout, out = _counts_and_output(p)
    plain_chunks = L.spx_debug_last_call_chunks()
    if before_map_call:
        before_map_call()
    b = Batch(plan, *args, time_map=True)
    b.upload([s[0] for s in streams])
    b.d_map.fill_(MAP_CANARY)
    b.run()
    nout_m, out_m = _counts_and_output(b)
    chunks, form = L.spx_debug_last_call_chunks(), L.spx_debug_last_walk_form()
    assert (nout >= 0).all() and np.array_equal(nout_m, nout), "n_out differs from spx_batch_run's"
    assert np.array_equal(out_m, out), "out differs from spx_batch_run's"
    rows = b.d_map.cpu().numpy()
    want = [_want_rows(orc, s) for s in streams]
    assert b.map_offs[-1] == rows.size == sum(w.size for w in want)        # no cell outside the streams' ranges exists
    assert not (rows == MAP_CANARY).any(), "cells left unwritten: %s" % np.nonzero(rows == MAP_CANARY)[0][:8]
    bad = [(i, streams[i][0].size) for i in range(len(streams)) if not np.array_equal(rows[b.map_offs[i]:b.map_offs[i + 1]], want[i])]
    assert bad == [], "streams whose rows are not the oracle's (index, frames): %s" % bad[:8]
    assert all(rows[b.map_offs[i + 1] - 1] == nout[i] for i in range(len(streams)))
    return plain_chunks, chunks, form


def _counts_and_output(b):
    import torch
    torch.cuda.synchronize(b.device)
    return b.d_nout.cpu().numpy().copy(), b.d_out.cpu().numpy().copy()


@pytest.mark.parametrize("chunks", [2, 3])
def test_a_map_call_in_forced_time_chunks(orc, chunks):
    """24 streams of different lengths (1.0 to 2.0 s, one of 0 frames, one shorter than a ring buffer), every combination of
    speed 3.5 / 1.5 / 0.8, nonlinear 1.0 / 0.5 and feedback 0 / 0.1, under spx_set_pipeline_chunks(2) and (3)."""
    from speedy_amd.batch import Plan
    lengths = [16000 + 677 * i for i in range(22)] + [0, 100]
    assert len(set(lengths)) == 24 and max(lengths) <= 32000 and {_knobs(i) for i in range(24)} == {(s, n, f) for s in SPEEDS for n in NONLINEARS for f in FEEDBACKS}
    streams = _chunk_streams(lengths)
    plan = Plan(16000, False)
    assert plan.B == 160
    try:
        plain, ran, form = _map_call_against_the_plain_call(orc, plan, streams, lambda: plan.L.spx_set_pipeline_chunks(chunks))
        print("forced chunks: the plain call ran in", plain, "the map call in", ran, "walk form", form)
        assert ran == chunks and form == 0, (ran, form)
    finally:
        plan.L.spx_set_pipeline_chunks(1)
        plan.close()


def _chunk_rule(n, cus, **kw):
    """The time chunks spx_mode.h gives a map call of n streams on a device of `cus` CUs (tests/mode_table.py, the library as
    build() left it): a map call's kernels run in sequence (run_impl), and with the concurrent mode off the chunk rule reads none of
    a shape's resource numbers but the CU count -- the 16 kHz mono shape's stand in."""
    import mode_table
    return mode_table.load(build=False)("16000,1,2048,1", n=n, force_total_streams=n, cu_count=cus, concurrent_enabled=0, **kw)["nch"]


def throughput_rule_case():
    """The body of the test below; runs in a process of its own (see there).  Raises on any difference."""
    import torch
    from oracle import pyorc
    from speedy_amd.batch import Plan
    pyorc.build()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * cus + 8
    assert _chunk_rule(n, cus) == 2 and _chunk_rule(2 * cus, cus) == 1 and _chunk_rule(n, cus, chunks_set=1, chunks=1) == 1
    distinct = _chunk_streams([8000 + 650 * k for k in range(12)])
    assert max(s[0].size for s in distinct) <= 16000
    streams = [distinct[(i * 5 + i // 12) % 12] for i in range(n)]
    assert len({id(s) for s in streams}) == 12
    plan = Plan(16000, False)
    try:
        plain, ran, form = _map_call_against_the_plain_call(pyorc, plan, streams)
        print("throughput rule:", n, "streams on", cus, "CUs: the plain call ran in", plain, "chunks, the map call in", ran, "walk form", form)
        assert ran == 2 and form == 0, (plain, ran, form)
    finally:
        plan.close()


def test_a_map_call_above_two_streams_per_cu_takes_two_chunks_by_itself():
    """2 CU + 8 streams of 0.5 to 1.0 s, no chunk setting: the call runs in two time chunks by the engine's own rule, which the
    host-only mode table replays.  A process in which spx_set_pipeline_chunks was ever called never takes that rule again (the
    setting is binding, 1 included), and other tests of this suite call it: so this case -- and it alone -- runs in a fresh
    process, which is what the test is about."""
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_time_map as t; t.throughput_rule_case()" % (os.path.dirname(here), here))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "throughput rule:" in r.stdout, r.returncode


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
