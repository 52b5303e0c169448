"""spx_batch_run_edits and spx_edit_replay on the MI355X.

Every comparison is exact.  A job's expected records are tests/edit_list_ref.py's (EditStream: the time-scale stage of tests/tsm_ref.py
with absolute positions; tests/test_edit_list_abi.py pins it against tsm_ref and the oracle on the CPU); out, n_out and the taps are
compared with spx_batch_run's on the same table, byte for byte; a replayed companion track with edit_list_ref.replay in Python
integers.  The directed jobs are tests/tsm_inputs.py's at 16 and 22.05 kHz with 1, 2 and 3 channels, and one 44.1 kHz job (its
steps reach outside the walk kernel's LDS window).  The definitions are computed once per process and shared."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_list_ref as E  # noqa: E402
import tsm_inputs as I  # noqa: E402
import tsm_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 0x5a5a
OP_CANARY = -1234567
_DEF = {}


def _linear_jobs(rate):
    """The directed linear jobs of one sample rate: 1, 2 and 3 channels at 16 and 22.05 kHz, the one 44.1 kHz job."""
    if rate == 44100:
        return [j for j in I.linear_jobs() if j[0] == "rates/44100Hz/1ch/13230/2"]
    return [j for j in I.linear_jobs() if j[1] == rate and j[2] in (1, 2, 3)]


def _nonlinear_jobs(rate):
    return [j for j in I.nonlinear_jobs() + I.nonlinear_map_jobs() if j[1] == rate and j[2] in (1, 2, 3)]


def _linear_def(job):
    name, rate, ch, x, speed = job
    if name not in _DEF:
        with E.shared_pitch_searches():
            _DEF[name] = E.linear_job(x, rate, ch, speed)
    return _DEF[name]


def _nonlinear_def(orc, job, mm):
    name, rate, ch, x, speed, nl = job
    if (name, mm) not in _DEF:
        tap = orc.compress_sound(x, rate, ch, speed, nl, 0.0, mm, chunk=1000, taps=True)["speed"]
        with E.shared_pitch_searches():
            _DEF[(name, mm)] = E.nonlinear_job(x, rate, ch, T.event_speeds(x.size // ch, rate, tap, speed), speed)
    return _DEF[(name, mm)]


def _sync_np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _caps(plan, jobs, defs):
    """spx_plan_edit_ops per job -- asserted to cover the definition's count wherever no step fails -- and the true count for the
    jobs whose steps fail (edit_list_ref.FAILED_STEP_JOBS)."""
    caps = []
    for job, e in zip(jobs, defs):
        nl = job[5] if len(job) == 6 else 0.0
        cap = plan.L.spx_plan_edit_ops(plan.h, job[3].size // job[2], float(job[4]), float(nl))
        assert cap >= 0, plan.L.spx_last_error()
        if e.failed_steps:
            assert job[0] in E.FAILED_STEP_JOBS and E.FAILED_STEP_JOBS[job[0]] == len(e.ops), job[0]
            cap = len(e.ops)
        else:
            assert cap >= len(e.ops), (job[0], cap, len(e.ops))
        caps.append(cap)
    return caps


def _run_family(plan, jobs, defs, taps):
    """spx_batch_run and spx_batch_run_edits on one table: everything the edits call shares with the plain call is byte-equal, the
    records are the definition's, the replay of every job's own input is the job's output, the walk form is 0."""
    from speedy_amd.batch import Batch
    lengths, chans = [j[3].size // j[2] for j in jobs], [j[2] for j in jobs]
    speeds, nls = [j[4] for j in jobs], [(j[5] if len(j) == 6 else 0.0) for j in jobs]
    streams = [j[3] for j in jobs]
    p = Batch(plan, lengths, chans, speeds, nls, taps=taps)
    p.upload(streams)
    p.run()
    nout, out = _sync_np(p.d_nout), _sync_np(p.d_out)
    tap = _sync_np(p.t_speed).tobytes() + _sync_np(p.t_tension).tobytes() + _sync_np(p.t_features).tobytes() if taps else b""
    assert (nout >= 0).all()
    b = Batch(plan, lengths, chans, speeds, nls, taps=taps, edits=True, ops_caps=_caps(plan, jobs, defs))
    b.upload(streams)
    b.d_ops.fill_(OP_CANARY)
    b.run()
    form = plan.L.spx_debug_last_walk_form()
    assert np.array_equal(_sync_np(b.d_nout), nout), "n_out differs from spx_batch_run's"
    assert np.array_equal(_sync_np(b.d_out), out), "out differs from spx_batch_run's"
    if taps:
        assert _sync_np(b.t_speed).tobytes() + _sync_np(b.t_tension).tobytes() + _sync_np(b.t_features).tobytes() == tap
    assert form == 0
    counts = b.op_counts()
    ops = _sync_np(b.d_ops)
    for i, (job, e) in enumerate(zip(jobs, defs)):
        assert nout[i] == e.out_n, (job[0], nout[i], e.out_n)
        assert counts[i] == len(e.ops), (job[0], counts[i], len(e.ops))
        got = ops[b.op_offs[i]:b.op_offs[i] + len(e.ops)]
        want = np.asarray(e.ops, np.int32).reshape(-1, 4)
        assert np.array_equal(got, want), (job[0], np.nonzero((got != want).any(axis=1))[0][:4])
        assert (ops[b.op_offs[i] + len(e.ops):b.op_offs[i + 1]] == OP_CANARY).all(), job[0]
    back = b.replay(streams, chans)
    res = p.results()
    for i, job in enumerate(jobs):
        assert np.array_equal(back[i], res[i]), "%s: the replay on the job's own input is not the job's output" % job[0]
    return b


@pytest.mark.parametrize("rate", [16000, 22050, 44100])
def test_linear_jobs_equal_the_definition_and_the_plain_call(rate):
    from speedy_amd.batch import Plan
    jobs = _linear_jobs(rate)
    assert len(jobs) == (1 if rate == 44100 else len(jobs)) and (rate == 44100 or len(jobs) > 15)
    if rate != 44100:
        assert {j[2] for j in jobs} >= ({1, 2} if rate == 16000 else {1, 2, 3})
        assert {j[4] for j in jobs} >= set(I.SPEEDS + I.EXTRA_SPEEDS)
    plan = Plan(rate, False)
    try:
        _run_family(plan, jobs, [_linear_def(j) for j in jobs], taps=False)
    finally:
        plan.close()


@pytest.mark.parametrize("mm", [False, True], ids=["plain", "matlab"])
@pytest.mark.parametrize("rate", [16000, 22050])
def test_nonlinear_jobs_equal_the_definition_and_the_plain_call(orc, rate, mm):
    from speedy_amd.batch import Plan
    jobs = _nonlinear_jobs(rate)
    assert len(jobs) >= 3 and (rate != 16000 or {j[2] for j in jobs} == {1, 2, 3})
    plan = Plan(rate, mm)
    try:
        _run_family(plan, jobs, [_nonlinear_def(orc, j, mm) for j in jobs], taps=True)
    finally:
        plan.close()


# ------------------------------------------------------------------ companion tracks ------------------------------------------------------------------

def _full_scale(n_values, seed):
    """Random int16 over the whole range, both ends planted."""
    y = np.random.default_rng(seed).integers(-32768, 32768, max(n_values, 2)).astype(np.int16)
    y[0::97] = -32768
    y[1::89] = 32767
    return y[:n_values]


class _Replay:
    """One spx_edit_replay call over a Batch(edits=True) that has run, with a track table of its own: in_off / out_off chosen by the
    test, guard values around every output region."""

    def __init__(self, b, chans, in_res, out_res, seed=5, tracks=None):
        """in_res / out_res: the residues modulo 8 of the streams' in_off / out_off, taken in turn (all odd in these tests): stream
        i's region begins at the first such offset behind stream i - 1's, so at least one guard value lies between two regions."""
        import torch
        from speedy_amd._lib import EditTrack
        self.b, self.chans = b, [int(c) for c in chans]
        self.tr = (EditTrack * b.n)()
        in_off = out_off = 0
        self.tracks = []
        for i in range(b.n):
            c = self.chans[i]
            in_off += 1 + (in_res[i % len(in_res)] - (in_off + 1)) % 8
            out_off += 1 + (out_res[i % len(out_res)] - (out_off + 1)) % 8
            assert in_off % 8 == in_res[i % len(in_res)] and out_off % 8 == out_res[i % len(out_res)]
            self.tr[i].in_off, self.tr[i].out_off, self.tr[i].channels, self.tr[i].reserved = in_off, out_off, c, 0
            self.tracks.append(_full_scale(int(b.lengths[i]) * c, seed + i) if tracks is None else tracks[i])
            assert self.tracks[i].size == int(b.lengths[i]) * c
            in_off += int(b.lengths[i]) * c
            out_off += int(b.out_caps[i]) * c
        host = np.full(in_off + 8, 12345, np.int16)          # (what lies between the tracks is not zero)
        for i, y in enumerate(self.tracks):
            host[self.tr[i].in_off:self.tr[i].in_off + y.size] = y
        self.d_y = torch.from_numpy(host).to(b.device)
        self.d_yout = torch.full((out_off + 8,), CANARY, dtype=torch.int16, device=b.device)

    def call(self, **kw):
        import torch
        b, L = self.b, self.b.plan.L
        a = dict(jobs=b.jobs, ops=b.d_ops.data_ptr(), caps=b._ops_cap_ptr(), nops=b.d_nops.data_ptr(), nout=b.d_nout.data_ptr(),
                 tracks=self.tr, y=self.d_y.data_ptr(), yout=self.d_yout.data_ptr())
        a.update(kw)
        rc = L.spx_edit_replay(b.plan.h, a["jobs"], b.n, a["ops"], a["caps"], a["nops"], a["nout"], a["tracks"], a["y"], a["yout"],
                               torch.cuda.current_stream().cuda_stream)
        msg = L.spx_last_error().decode() if rc != 0 else ""
        torch.cuda.synchronize()
        return rc, msg

    def check(self, want, written=None):
        """want[i]: the expected frames of stream i as a flat list (None: nothing may be written there); everything else is CANARY."""
        out = _sync_np(self.d_yout)
        mask = np.zeros(out.size, bool)
        for i in range(self.b.n):
            if want[i] is None:
                continue
            w = np.asarray(want[i], np.int64)
            o = self.tr[i].out_off
            got = out[o:o + w.size].astype(np.int64)
            assert np.array_equal(got, w), "stream %d (%d channels, out_off %d): first difference at value %d" % (
                i, self.chans[i], o, int(np.nonzero(got != w)[0][0]))
            mask[o:o + w.size] = True
        assert (out[~mask] == CANARY).all(), "values written outside the streams' output: %s" % np.nonzero(out[~mask] != CANARY)[0][:8]


def _want(e, y, c):
    return E.replay(e.ops, y, c, e.limit, e.out_n)


def test_companion_tracks_with_other_channel_counts_at_odd_offsets(orc):
    """A mono track under the 3-channel key, 3-channel tracks under mono keys, 2 under 2: full-scale random values with both ends
    of the range, in_off and out_off odd and congruent to 1, 3 and 7 modulo 8, guard values before and behind every region."""
    from speedy_amd.batch import Plan
    by = {j[0]: j for j in I.linear_jobs()}
    lin = [by["speeds/16000Hz/1ch/9001/3.5"], by["speeds/16000Hz/1ch/9001/0.7"], by["rates/16000Hz/2ch/4800/1.3"], by["speeds/16000Hz/1ch/9001/1.3"]]
    nl = [j for j in I.nonlinear_map_jobs() if j[0] == "map/16000Hz/3ch/6000/2/1"] + [j for j in I.nonlinear_jobs() if j[0] == "nonlinear/16000Hz/1ch/15000/3.5/1"]
    assert len(nl) == 2
    jobs = lin + nl
    defs = [_linear_def(j) for j in lin] + [_nonlinear_def(orc, j, False) for j in nl]
    plan = Plan(16000, False)
    try:
        b = _run_family(plan, jobs, defs, taps=False)
        chans = [3, 3, 2, 1, 1, 3]
        r = _Replay(b, chans, in_res=[1, 3, 7], out_res=[7, 1, 3])
        assert {int(r.tr[i].out_off) % 8 for i in range(b.n)} == {int(r.tr[i].in_off) % 8 for i in range(b.n)} == {1, 3, 7}
        rc, msg = r.call()
        assert rc == 0, msg
        r.check([_want(e, y, c) for e, y, c in zip(defs, r.tracks, chans)])
        for y in r.tracks:
            assert y.min() == -32768 and y.max() == 32767
    finally:
        plan.close()


# ------------------------------------------------------------------ shapes of the replay launch ------------------------------------------------------------------

def _edits_batch(plan, streams, chans, speeds, nls, caps=None):
    from speedy_amd.batch import Batch
    b = Batch(plan, [x.size // c for x, c in zip(streams, chans)], chans, speeds, nls, edits=True, ops_caps=caps)
    b.upload(streams)
    b.run()
    return b


def test_one_stream_and_streams_without_output():
    """One stream alone; then a stream of 0 frames, one shorter than maxRequired (its records come from the flush alone) and a unity
    job of 40 000 frames (one record across many blocks) in one call."""
    from speedy_amd.batch import Plan
    by = {j[0]: j for j in I.linear_jobs()}
    one = by["speeds/16000Hz/1ch/9001/3.5"]
    plan = Plan(16000, False)
    try:
        b = _run_family(plan, [one], [_linear_def(one)], taps=False)
        r = _Replay(b, [2], in_res=[3], out_res=[5])
        assert r.call()[0] == 0
        r.check([_want(_linear_def(one), r.tracks[0], 2)])
        mr = plan.max_required
        unity = I.rectangles(16000, 1, 16000)
        unity = np.concatenate([unity, unity, unity[:8000]])
        streams = [np.zeros(0, np.int16), I.rectangles(16000, 1, mr - 5), unity]
        speeds = [2.0, 2.0, 1.0]
        defs = [E.linear_job(x, 16000, 1, s) for x, s in zip(streams, speeds)]
        assert defs[0].ops == [] or defs[0].out_n == 0
        assert defs[1].out_n > 0 and defs[2].ops[0] == (0, 0, -1, 40000) and defs[2].out_n == 40000
        b = _edits_batch(plan, streams, [1, 1, 1], speeds, 0.0)
        assert b.op_counts().tolist() == [len(e.ops) for e in defs]
        for i, e in enumerate(defs):
            assert np.array_equal(b.edits(i), np.asarray(e.ops, np.int32).reshape(-1, 4)), i
        r = _Replay(b, [1, 3, 3], in_res=[1, 7, 3], out_res=[3, 1, 7])
        assert r.call()[0] == 0
        assert plan.L.spx_debug_last_replay_grid(None) >= 40000 * 3 // 4096
        r.check([None if e.out_n == 0 else _want(e, y, c) for e, y, c in zip(defs, r.tracks, [1, 3, 3])])
    finally:
        plan.close()


def test_three_hundred_streams():
    """300 streams of four kinds (speed 200 with its records of one frame among them), each replayed on a 2-channel track."""
    from speedy_amd.batch import Plan
    by = {j[0]: j for j in I.linear_jobs()}
    kinds = [by["speeds/22050Hz/1ch/7000/200"], by["speeds/22050Hz/1ch/7000/2"], by["speeds/22050Hz/1ch/7000/0.7"], by["lengths/22050Hz/1ch/679/2"]]
    defs4 = [_linear_def(j) for j in kinds]
    assert sum(1 for op in defs4[0].ops if op[3] == 1) >= 20
    pick = [(i * 7 + i // 4) % 4 for i in range(300)]
    jobs, defs = [kinds[k] for k in pick], [defs4[k] for k in pick]
    plan = Plan(22050, False)
    try:
        caps = [len(e.ops) + 3 for e in defs]
        b = _edits_batch(plan, [j[3] for j in jobs], [1] * 300, [j[4] for j in jobs], 0.0, caps)
        assert b.op_counts().tolist() == [len(e.ops) for e in defs]
        kind_tracks = [_full_scale(j[3].size * 2, 40 + k) for k, j in enumerate(kinds)]       # one random track per kind
        r = _Replay(b, [2] * 300, in_res=[1, 3, 7], out_res=[3, 7, 1], tracks=[kind_tracks[k] for k in pick])
        assert r.call()[0] == 0
        want4 = [_want(e, y, 2) for e, y in zip(defs4, kind_tracks)]
        r.check([want4[k] for k in pick])
    finally:
        plan.close()


def test_a_planted_list_of_one_and_two_frame_records():
    """A list nobody's job wrote -- 9 000 records of one and two frames, copies and cross-fades in turn, over a 1 s track of 3
    channels: a block of 4096 values holds far more records than it stages, and reads them where they lie."""
    import torch
    from speedy_amd.batch import Plan
    rate, n_in = 16000, 16000
    ops, at = [], 0
    for k in range(9000):
        n = 1 + k % 2
        a, bb = (k * 37) % (n_in - 4), (k * 101 + 5) % (n_in + 300)      # (some up-ramps reach behind L)
        ops.append((at, a, -1 if k % 3 == 0 else bb, n))
        at += n
    n_out = at - 1                                                       # the cut falls inside the last record
    plan = Plan(rate, False)
    try:
        b = _edits_batch(plan, [I.rectangles(rate, 1, n_in)], [1], [1.0], 0.0, [len(ops)])
        assert int(b.out_caps[0]) >= n_out
        b.d_ops.copy_(torch.from_numpy(np.asarray(ops, np.int32)).to(b.device))
        b.d_nops.fill_(len(ops))
        b.d_nout.fill_(n_out)
        r = _Replay(b, [3], in_res=[7], out_res=[1])
        assert r.call()[0] == 0
        r.check([E.replay(ops, r.tracks[0], 3, n_in, n_out)])
    finally:
        plan.close()


def test_the_frames_behind_L_of_a_nonlinear_job_read_as_zero(orc):
    """n_in = R B + 37: the 37 real frames behind L = R B are never handed over, and a companion's values there -- planted, far
    from zero -- must not show: with L = n_in the definition's replay differs."""
    from speedy_amd.batch import Plan
    rate, R = 16000, 50
    n_in = R * 160 + 37
    x = I.syllables(rate, 1, n_in)
    job = ("tail37", rate, 1, x, 3.5, 1.0)
    e = _nonlinear_def(orc, job, False)
    assert e.limit == R * 160
    plan = Plan(rate, False)
    try:
        b = _run_family(plan, [job], [e], taps=True)
        y = _full_scale(n_in, 9)
        y[e.limit:] = 30000
        r = _Replay(b, [1], in_res=[3], out_res=[1], tracks=[y])
        assert r.call()[0] == 0
        want = _want(e, y, 1)
        assert want != E.replay(e.ops, y, 1, n_in, e.out_n), "the job reads nothing behind L: the case shows nothing"
        r.check([want])
    finally:
        plan.close()


# ------------------------------------------------------------------ time chunks ------------------------------------------------------------------

def _chunk_streams(lengths):
    import time_map_ref as tm
    knobs = [(3.5, 1.0), (1.5, 0.5), (0.8, 1.0), (2.0, 0.0), (0.7, 0.0)]
    return [(tm.signal(16000, 1, n, seed=5100 + 13 * i),) + knobs[i % 5] for i, n in enumerate(lengths)]


def _edits_of(plan, streams, caps=None):
    b = _edits_batch(plan, [s[0] for s in streams], [1] * len(streams), [s[1] for s in streams], [s[2] for s in streams], caps)
    return b, plan.L.spx_debug_last_call_chunks(), plan.L.spx_debug_last_walk_form()


def _same_lists(b, ref):
    """(the capacities of these calls are explicit and generous: the speeds of a nonlinear job's events are the tension's)"""
    assert np.array_equal(_sync_np(b.d_nout), _sync_np(ref.d_nout)) and np.array_equal(_sync_np(b.d_out), _sync_np(ref.d_out))
    assert np.array_equal(b.op_counts(), ref.op_counts()) and (ref.op_counts() > 0).sum() >= b.n - 2
    for i in range(b.n):
        assert np.array_equal(b.edits(i), ref.edits(i)), "stream %d: the records differ from the one-chunk call's" % i


@pytest.mark.parametrize("chunks", [2, 3])
def test_an_edits_call_in_forced_time_chunks(chunks):
    """20 streams of 0.5 to 1.0 s (and one of 0 frames, one shorter than a ring buffer), linear and nonlinear, speed-up and
    slow-down, under spx_set_pipeline_chunks: every chunk but the first continues the stream's list from the count in n_ops."""
    from speedy_amd.batch import Plan
    streams = _chunk_streams([8000 + 421 * i for i in range(18)] + [0, 100])
    plan = Plan(16000, False)
    try:
        plan.L.spx_set_pipeline_chunks(1)
        ref, ran1, _ = _edits_of(plan, streams, 6000)
        plan.L.spx_set_pipeline_chunks(chunks)
        b, ran, form = _edits_of(plan, streams, 6000)
        assert (ran1, ran, form) == (1, chunks, 0), (ran1, ran, form)
        _same_lists(b, ref)
    finally:
        plan.L.spx_set_pipeline_chunks(1)
        plan.close()


def throughput_rule_case():
    """The body of the test below; runs in a process of its own (see there).  Raises on any difference."""
    import torch
    from speedy_amd.batch import Plan
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * cus + 8
    distinct = _chunk_streams([4000 + 333 * k for k in range(10)])
    streams = [distinct[(i * 3 + i // 10) % 10] for i in range(n)]
    plan = Plan(16000, False)
    try:
        b, ran, form = _edits_of(plan, streams, 4000)
        plan.L.spx_set_pipeline_chunks(1)
        ref, ran1, _ = _edits_of(plan, streams, 4000)
        print("throughput rule:", n, "streams on", cus, "CUs: the edits call ran in", ran, "chunks, walk form", form)
        assert (ran, ran1, form) == (2, 1, 0), (ran, ran1, form)
        _same_lists(b, ref)
    finally:
        plan.close()


def test_an_edits_call_above_two_streams_per_cu_takes_two_chunks_by_itself():
    """2 CU + 8 streams, no chunk setting: two time chunks by the engine's own rule.  A process in which spx_set_pipeline_chunks was
    ever called never takes that rule again, and other tests call it: this case runs in a fresh process (as
    tests/test_gpu_time_map.py arranges it)."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_edit_list as t; t.throughput_rule_case()" % (os.path.dirname(here), here))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "throughput rule:" in r.stdout, r.returncode


# ------------------------------------------------------------------ capacity ------------------------------------------------------------------

def test_capacities_at_below_and_far_below_the_count():
    """ops_cap = the true count, the count - 1, 0, and the count + 5: n_ops is the count, minus the count twice, the count; nothing
    is written behind a stream's region; out and n_out are what they were; the replay writes nothing for the two streams whose
    lists did not fit and replays their neighbours.  Then an out_cap that is too small: n_out negative, nothing replayed."""
    import torch
    from speedy_amd.batch import Plan
    by = {j[0]: j for j in I.linear_jobs()}
    jobs = [by["speeds/16000Hz/1ch/9001/3.5"], by["speeds/16000Hz/1ch/9001/0.7"], by["speeds/16000Hz/1ch/9001/1.3"], by["speeds/16000Hz/1ch/9001/2"]]
    defs = [_linear_def(j) for j in jobs]
    cnt = [len(e.ops) for e in defs]
    assert min(cnt) > 20
    plan = Plan(16000, False)
    try:
        streams, speeds = [j[3] for j in jobs], [j[4] for j in jobs]
        ref = _edits_batch(plan, streams, [1] * 4, speeds, 0.0, cnt)
        assert ref.op_counts().tolist() == cnt
        caps = [cnt[0], cnt[1] - 1, 0, cnt[3] + 5]
        from speedy_amd.batch import Batch
        b = Batch(plan, [x.size for x in streams], 1, speeds, 0.0, edits=True, ops_caps=caps)
        b.upload(streams)
        b.d_ops = torch.full((sum(caps) + 8, 4), OP_CANARY, dtype=torch.int32, device=b.device)      # 8 guard records behind the last region
        b.run()
        assert b.op_counts().tolist() == [cnt[0], -cnt[1], -cnt[2], cnt[3]]
        assert np.array_equal(_sync_np(b.d_nout), _sync_np(ref.d_nout)) and np.array_equal(_sync_np(b.d_out), _sync_np(ref.d_out))
        ops = _sync_np(b.d_ops)
        o = b.op_offs
        assert np.array_equal(ops[o[0]:o[1]], np.asarray(defs[0].ops, np.int32))
        assert np.array_equal(ops[o[1]:o[2]], np.asarray(defs[1].ops[:cnt[1] - 1], np.int32))     # what fits is stored, the rest counted
        assert o[2] == o[3] and np.array_equal(ops[o[3]:o[3] + cnt[3]], np.asarray(defs[3].ops, np.int32))
        assert (ops[o[3] + cnt[3]:] == OP_CANARY).all(), "records written behind a stream's region"
        r = _Replay(b, [2, 2, 2, 2], in_res=[1], out_res=[3])
        assert r.call()[0] == 0
        r.check([_want(defs[0], r.tracks[0], 2), None, None, _want(defs[3], r.tracks[3], 2)])
        # out_cap too small for stream 0: n_out negative, its records unspecified, nothing replayed; stream 3 as before
        small = Batch(plan, [x.size for x in streams], 1, speeds, 0.0, edits=True, ops_caps=[c + 8 for c in cnt])
        small.jobs[0].out_cap = 100
        small.upload(streams)
        small.run()
        nout = _sync_np(small.d_nout)
        assert nout[0] < 0 and (nout[1:] == [e.out_n for e in defs[1:]]).all()
        r = _Replay(small, [2, 2, 2, 2], in_res=[1], out_res=[3])
        assert r.call()[0] == 0
        r.check([None] + [_want(e, y, 2) for e, y in zip(defs[1:], r.tracks[1:])])
    finally:
        plan.close()


# ------------------------------------------------------------------ refusals ------------------------------------------------------------------

def test_refusals_launch_nothing_and_a_good_call_works_right_after():
    import torch
    from speedy_amd._lib import EditTrack
    from speedy_amd.batch import Batch, Plan
    by = {j[0]: j for j in I.linear_jobs()}
    jobs = [by["speeds/16000Hz/1ch/9001/3.5"], by["speeds/16000Hz/1ch/9001/0.7"]]
    defs = [_linear_def(j) for j in jobs]
    plan = Plan(16000, False)
    try:
        L = plan.L
        b = Batch(plan, [j[3].size for j in jobs], 1, [j[4] for j in jobs], 0.0, edits=True)
        b.upload([j[3] for j in jobs])
        hs = torch.cuda.current_stream().cuda_stream
        i64 = C.POINTER(C.c_int64)

        def run(**kw):
            b.d_out.fill_(CANARY); b.d_nout.fill_(-77); b.d_ops.fill_(OP_CANARY); b.d_nops.fill_(-78)
            a = dict(ops=b.d_ops.data_ptr(), caps=b._ops_cap_ptr(), nops=b.d_nops.data_ptr(), ws=b.d_ws.numel())
            a.update(kw)
            rc = L.spx_batch_run_edits(plan.h, b.jobs, b.n, b.d_in.data_ptr(), b.d_out.data_ptr(), b.d_nout.data_ptr(), a["ops"], a["caps"],
                                       a["nops"], b.d_ws.data_ptr(), a["ws"], None, hs)
            msg = L.spx_last_error().decode() if rc != 0 else ""
            torch.cuda.synchronize()
            untouched = (bool((b.d_out == CANARY).all()) and bool((b.d_nout == -77).all()) and bool((b.d_ops == OP_CANARY).all())
                         and bool((b.d_nops == -78).all()))
            return rc, msg, untouched

        for kw, word in (({"ops": None}, "NULL"), ({"caps": None}, "NULL"), ({"nops": None}, "NULL"),
                         ({"ops": b.d_ops.data_ptr() + 4}, "aligned"),
                         ({"caps": (C.c_int64 * 2)(5, -1)}, "negative capacity"),
                         ({"caps": (C.c_int64 * 2)(2 ** 31 - 1, 1)}, "2^31 - 1"),
                         ({"ws": L.spx_batch_workspace_bytes(plan.h, b.jobs, b.n) - 1}, "workspace")):
            rc, msg, untouched = run(**{k: (C.cast(v, i64) if k == "caps" and v is not None else v) for k, v in kw.items()})
            assert rc == -1 and word in msg and untouched, (kw, rc, msg, untouched)
        good = b.jobs[1].speed
        b.jobs[1].speed = float("nan")
        rc, msg, untouched = run()
        assert rc == -1 and "speed" in msg and untouched, (rc, msg, untouched)
        assert L.spx_batch_run(plan.h, b.jobs, b.n, b.d_in.data_ptr(), b.d_out.data_ptr(), b.d_nout.data_ptr(), b.d_ws.data_ptr(),
                               b.d_ws.numel(), None, hs) == -1 and L.spx_last_error().decode() == msg, "the message is spx_batch_run's"
        assert L.spx_plan_edit_ops(plan.h, 1000, float("nan"), 0.0) == -1 and L.spx_plan_edit_ops(plan.h, -1, 2.0, 0.0) == -1
        b.jobs[1].speed = good
        rc, msg, untouched = run()
        assert rc == 0 and not untouched, msg
        assert b.op_counts().tolist() == [len(e.ops) for e in defs]
        # ... and the replay's: a NULL pointer, channels < 1, a negative offset, a table spx_batch_run refuses
        r = _Replay(b, [2, 1], in_res=[1], out_res=[3])
        for key in ("ops", "caps", "nops", "nout", "tracks", "y", "yout"):
            rc, msg = r.call(**{key: None})
            assert rc == -1 and "NULL" in msg, (key, rc, msg)
        bad = (EditTrack * 2)()
        for k in range(2):
            bad[k].in_off, bad[k].out_off, bad[k].channels = r.tr[k].in_off, r.tr[k].out_off, r.tr[k].channels
        bad[1].channels = 0
        rc, msg = r.call(tracks=bad)
        assert rc == -1 and "channels" in msg, (rc, msg)
        bad[1].channels, bad[0].out_off = 1, -1
        rc, msg = r.call(tracks=bad)
        assert rc == -1 and "negative" in msg, (rc, msg)
        b.jobs[1].speed = float("nan")
        rc, msg = r.call()
        assert rc == -1 and "speed" in msg, (rc, msg)
        b.jobs[1].speed = good
        r.check([None, None])                                   # nothing was launched
        rc, msg = r.call()
        assert rc == 0, msg
        r.check([_want(e, y, c) for e, y, c in zip(defs, r.tracks, [2, 1])])
    finally:
        plan.close()


# ------------------------------------------------------------------ Python, and the C example ------------------------------------------------------------------

def test_python_round_trip_and_the_value_error():
    from speedy_amd.batch import Batch, Plan
    by = {j[0]: j for j in I.linear_jobs()}
    job = by["rates/16000Hz/2ch/4800/1.3"]
    e = _linear_def(job)
    plan = Plan(16000, False)
    try:
        with pytest.raises(ValueError):
            Batch(plan, [4800], 2, 1.3, 0.0, edits=True, rate=1.25)
        with pytest.raises(ValueError):
            Batch(plan, [4800], 2, 1.3, 0.0, edits=True, time_map=True)
        b = Batch(plan, [4800], 2, 1.3, 0.0, edits=True)
        b.upload([job[3]])
        b.run()
        ops = b.edits(0)
        assert ops.dtype == np.int32 and ops.shape == (len(e.ops), 4) and np.array_equal(ops, np.asarray(e.ops, np.int32))
        assert np.array_equal(b.replay([job[3]], 2)[0], b.results()[0])
        y = _full_scale(4800 * 5, 77)
        assert b.replay([y], 5)[0].tolist() == _want(e, y, 5)
        with pytest.raises(RuntimeError):
            b.run_ahead()
    finally:
        plan.close()


def test_c_edits_example(tmp_path):
    """tools/batch_edits_example.c: a key and a 2-channel track through the C ABI alone; both counts printed, both outputs the
    definition's."""
    exe = os.path.join(ROOT, "speedy_amd", "lib", "batch_edits_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "editsexample"])
    by = {j[0]: j for j in I.linear_jobs()}
    job = by["speeds/16000Hz/1ch/9001/3.5"]
    e = _linear_def(job)
    y = _full_scale(9001 * 2, 31)
    job[3].tofile(tmp_path / "key.raw")
    y.tofile(tmp_path / "track.raw")
    r = subprocess.run([exe, str(tmp_path / "key.raw"), str(tmp_path / "track.raw"), "16000", "1", "2", "3.5", "0", str(tmp_path / "ok.raw"),
                        str(tmp_path / "ot.raw")], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert r.stdout.split() == ["frames", str(e.out_n), "ops", str(len(e.ops))]
    assert np.fromfile(tmp_path / "ok.raw", np.int16).tolist() == _want(e, job[3], 1)
    assert np.fromfile(tmp_path / "ot.raw", np.int16).tolist() == _want(e, y, 2)
