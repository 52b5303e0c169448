"""spx_batch_run_twopass on the MI355X.

Every comparison is exact.  The call is defined by three others: n_probe is spx_batch_run's count on the probe table (every job at
(float)want, fully nonlinear), speeds is the numpy definition of tests/twopass_ref.py evaluated on those counts, and out / n_out /
taps are spx_batch_run's on the final table (the jobs at those speeds), byte for byte.  Two drivers of the reference's CLI are then
compared with the oracle's two passes sample for sample."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import twopass_ref as tp  # noqa: E402
from util import CANARY, read_wav  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "speedy_amd", "lib", "batch_twopass_example")

_WAV = {}


def _wav(name):
    if name not in _WAV:
        _WAV[name] = read_wav(name)
    return _WAV[name]


def _len(T, rate, factor):
    """LENGTH target in seconds that asks for a speed-up by `factor`."""
    return T / rate / factor


def _mix8(nonlinear):
    """16 kHz mono, eight streams: both modes, the tapestry segments, streams too short to measure (the probe emits nothing: the
    fallback), one analysis frame, feedback, a slow-down target.  Entries: (samples, seconds, speed, nonlinear, feedback)."""
    x, rate, ch = _wav("tapestry.wav")
    assert (rate, ch) == (16000, 1)
    seg = [tp.segment(x, s) for s in tp.SEGMENTS]
    nl = list(nonlinear) if isinstance(nonlinear, (list, tuple)) else [nonlinear] * 8
    t = [(seg[0], _len(seg[0].size, rate, 3.5), 1.0, nl[0], 0.0),
         (seg[1], 0.0, 2.0, nl[1], 0.0),
         (seg[2], _len(seg[2].size, rate, 1.5), 9.0, nl[2], 0.1),     # (the speed of a LENGTH job is ignored)
         (seg[3], _len(seg[3].size, rate, 0.8), 1.0, nl[3], 0.0),     # a slow-down target
         (x[:0], 0.0, 3.0, nl[4], 0.0),
         (x[:1], _len(1, rate, 2.0), 1.0, nl[5], 0.0),
         (x[:100], 0.0, 2.0, nl[6], 0.0),
         (x[:241], _len(241, rate, 2.0), 1.0, nl[7], 0.1)]
    return rate, 1, t


def _stereo():
    x, rate, ch = _wav("tapestry.wav")
    a = np.stack([x[:12000], x[8000:20000]], axis=1).ravel()
    b = np.stack([x[20000:26000], x[1000:7000]], axis=1).ravel()
    return rate, 2, [(a, _len(12000, rate, 2.0), 1.0, 1.0, 0.0), (b, 0.0, 3.0, 0.0, 0.0)]


def _k22():
    x, rate, ch = _wav("tapestry22050.wav")
    assert (rate, ch) == (22050, 1)
    return rate, 1, [(x[:9000], _len(9000, rate, 2.0), 1.0, 1.0, 0.1), (x[:22050], 0.0, 3.5, 0.5, 0.0),
                     (x[4000:20000], _len(16000, rate, 3.5), 1.0, 1.0, 0.0)]


def _many(nonlinear_of):
    """600 streams of 500 frames: more than two streams per CU -- a call of that size with an analysis of its own runs as two time
    chunks, and the patched speed must reach both copies of every stream's record."""
    x, rate, ch = _wav("tapestry.wav")
    t = []
    for i in range(600):
        s = x[37 * i:37 * i + 500]
        # (a slow-down target every twentieth stream: their capacities are 200 times the input)
        if i % 2:
            t.append((s, _len(500, rate, 0.8 if i % 40 == 1 else (1.5, 2.0, 3.5)[(i // 2) % 3]), 1.0, nonlinear_of(i), 0.0))
        else:
            t.append((s, 0.0, 0.9 if i % 40 == 0 else (2.0, 3.0)[(i // 2) % 2], nonlinear_of(i), 0.1 if i % 5 == 0 else 0.0))
    return rate, 1, t


BATCHES = {
    "mix8-nonlinear": lambda: _mix8(1.0),
    "mix8-finals-mixed": lambda: _mix8([1.0, 0.0, 0.5, 0.0, 1.0, 0.0, 0.5, 1.0]),
    "mix8-half": lambda: _mix8(0.5),
    "stereo": _stereo,
    "22k": _k22,
    "many-mixed": lambda: _many(lambda i: (1.0, 0.5, 0.0)[i % 3]),
    "many-nonlinear": lambda: _many(lambda i: (1.0, 0.5)[i % 2]),
}
REUSE = {"mix8-nonlinear": 1, "mix8-finals-mixed": 0, "mix8-half": 1, "stereo": 0, "22k": 1, "many-mixed": 0, "many-nonlinear": 1}


def _twopass(plan, table, ch, taps=False, out_caps=None):
    from speedy_amd.batch import TwoPassBatch
    b = TwoPassBatch(plan, [t[0].size // ch for t in table], ch, [t[2] for t in table], [t[3] for t in table], [t[4] for t in table],
                     taps=taps, spectrogram_taps=taps, seconds=[t[1] for t in table], out_caps=out_caps)
    b.upload([t[0] for t in table])
    return b


def _plain(plan, table, ch, speeds, nonlinear=None, taps=False):
    from speedy_amd.batch import Batch
    b = Batch(plan, [t[0].size // ch for t in table], ch, speeds, [t[3] for t in table] if nonlinear is None else nonlinear,
              [t[4] for t in table], taps=taps, spectrogram_taps=taps)
    b.upload([t[0] for t in table])
    return b


def _snap(b):
    """(n_out, the produced frames of every stream) after a synchronisation."""
    import torch
    torch.cuda.synchronize(b.device)
    nout = b.d_nout.cpu().numpy().copy()
    out = b.d_out.cpu().numpy()
    return nout, [out[b.out_offs[i]:b.out_offs[i] + max(0, int(nout[i])) * int(b.channels[i])].copy() for i in range(b.n)]


def _taps(b):
    import torch
    torch.cuda.synchronize(b.device)
    return [t.cpu().numpy().tobytes() for t in (b.t_tension, b.t_speed, b.t_features, b.t_spec, b.t_norm)]


def _check_definition(plan, name, taps=False):
    """One two-pass call against its definition; returns the two-pass batch (after the checks)."""
    rate, ch, table = BATCHES[name]()
    n = len(table)
    b = _twopass(plan, table, ch, taps=taps)
    b.d_out.fill_(CANARY)
    b.run()
    bit0 = plan.L.spx_debug_last_twopass() & 1
    n_probe, speeds = b.probe_counts(), b.final_speeds()
    nout, outs = _snap(b)
    tap_bytes = _taps(b) if taps else None
    # the probe table through spx_batch_run
    want = np.array([tp.want_of(t[0].size // ch, rate, t[1], t[2]) for t in table], np.float64)
    assert np.array_equal(want, b.want)
    p = _plain(plan, table, ch, want.astype(np.float32), nonlinear=[1.0] * n)
    p.run()
    p_nout, _ = _snap(p)
    assert np.array_equal(n_probe, p_nout), "n_probe %s, spx_batch_run on the probe table counts %s" % (n_probe, p_nout)
    # the formula
    ref = np.array([tp.second_speed(want[i], table[i][1] > 0, table[i][0].size // ch, n_probe[i]) for i in range(n)], np.float32)
    bad = np.nonzero(tp.bits(speeds) != tp.bits(ref))[0]
    assert bad.size == 0, "speeds differ from the definition at %s: %s against %s" % (bad[:8], speeds[bad][:8], ref[bad][:8])
    assert np.isfinite(speeds).all() and (speeds > 0).all()
    # the final table through spx_batch_run
    f = _plain(plan, table, ch, speeds, taps=taps)
    f.run()
    f_nout, f_outs = _snap(f)
    assert np.array_equal(nout, f_nout), "n_out %s, spx_batch_run on the final table counts %s" % (nout, f_nout)
    assert (nout >= 0).all()
    for i in range(n):
        assert np.array_equal(outs[i], f_outs[i]), "stream %d of %s: out differs from spx_batch_run on the final table" % (i, name)
    if taps:
        for k, (a, r) in enumerate(zip(tap_bytes, _taps(f))):
            assert a == r, "tap %d of %s differs from spx_batch_run's on the final table" % (k, name)
        assert np.frombuffer(tap_bytes[1], np.uint8).any() and np.frombuffer(tap_bytes[3], np.uint8).any()
    assert bit0 == REUSE[name], "spx_debug_last_twopass bit 0 is %d for %s" % (bit0, name)
    return b, n_probe, speeds, nout


@pytest.mark.parametrize("name", list(BATCHES))
def test_definition(name):
    from speedy_amd.batch import Plan
    rate = BATCHES[name]()[0]
    plan = Plan(rate)
    try:
        b, n_probe, speeds, nout = _check_definition(plan, name)
        if name.startswith("mix8"):
            # too short to measure: the probe emitted nothing and the final pass ran at the probe's speed
            assert (n_probe[4:7] == 0).all() and np.array_equal(tp.bits(speeds[4:7]), tp.bits(b.want[4:7].astype(np.float32)))
            assert speeds[3] < 1.0 < speeds[0]
        if name.startswith("many"):
            assert (n_probe > 0).all() and (speeds < 1.0).any() and (speeds > 1.0).any()
    finally:
        plan.close()


@pytest.mark.parametrize("name", ["mix8-nonlinear", "mix8-finals-mixed"])
def test_taps_are_the_final_tables(name):
    """All five taps, bitwise, where the second pass reuses the first pass's analysis and where it runs its own."""
    from speedy_amd.batch import Plan
    plan = Plan(16000)
    try:
        _check_definition(plan, name, taps=True)
    finally:
        plan.close()


def test_reference_semantics(orc):
    """--length 1.5 and --match_nonlinear --speed 3 (with --nonlinear 0.0, the flags of speedy_wave.cc:62) on tapestry.wav, as two
    streams of one call: the oracle's two passes, sample for sample.  compress_batch_to_length gives the first one too."""
    from speedy_amd.batch import Plan, compress_batch_to_length
    x, rate, ch = _wav("tapestry.wav")
    total = x.size // ch
    want = float(np.float32(total) / np.float32(rate)) / 1.5
    probe = orc.compress_sound(x, rate, ch, want, 1.0, 0.0, False, chunk=1000)
    got_speed = float(total) / float(probe["out"].size // ch)
    ref_len = orc.compress_sound(x, rate, ch, want * (want / got_speed), 1.0, 0.0, False, chunk=1000)["out"]
    probe3 = orc.compress_sound(x, rate, ch, 3.0, 1.0, 0.0, False, chunk=1000)
    achieved = float(total) / float(probe3["out"].size // ch)
    ref_match = orc.compress_sound(x, rate, ch, achieved, 0.0, 0.0, False, chunk=1000)["out"]
    plan = Plan(rate)
    try:
        b = _twopass(plan, [(x, 1.5, 1.0, 1.0, 0.0), (x, 0.0, 3.0, 0.0, 0.0)], ch)
        b.run()
        outs = b.results()
        assert np.array_equal(b.probe_counts(), [probe["out"].size // ch, probe3["out"].size // ch])
        assert np.array_equal(outs[0], ref_len), "--length 1.5 differs from the oracle's two passes"
        assert np.array_equal(outs[1], ref_match), "--match_nonlinear --speed 3 differs from the oracle's two passes"
        assert abs(outs[0].size / rate - 1.5) < 0.15    # what the flag is for
    finally:
        plan.close()
    outs, b2 = compress_batch_to_length([x], rate, ch, 1.5)
    try:
        assert np.array_equal(outs[0], ref_len)
    finally:
        b2.plan.close()


def test_walk_form_is_the_any_speed_one():
    """The second pass's walk kernel is chosen for "any speed", never from the placeholder in the host table: after a two-pass call
    spx_debug_last_walk_form() reads what it reads after a spx_batch_run of the same shape whose table mixes speeds 0.8 and 2.
    The plain call is made with its kernels in sequence (spx_set_concurrent(0)), as the second pass's always are: side by side
    with the analysis kernel a 16 kHz batch of eight such streams launches the same any-speed instantiation WITHOUT its output waves
    (the lean form: 64 where the second pass reads 68, measured), which is a launch order's choice and not another speed class.  The
    600-stream batch runs in sequence either way."""
    import torch
    from speedy_amd.batch import Plan
    plan = Plan(16000)
    try:
        L = plan.L
        for name in ("mix8-nonlinear", "many-nonlinear"):
            rate, ch, table = BATCHES[name]()
            b = _twopass(plan, table, ch)
            b.run()
            b.results()
            form = L.spx_debug_last_walk_form()
            m = _plain(plan, table, ch, [0.8 if i % 20 == 0 else 2.0 for i in range(len(table))])
            L.spx_set_concurrent(0)
            try:
                m.run()
                torch.cuda.synchronize()
            finally:
                L.spx_set_concurrent(1)
            mixed = L.spx_debug_last_walk_form()
            print("%s: walk form %d after the two-pass call, %d after a plain call mixing 0.8 and 2 (mode %d)"
                  % (name, form, mixed, L.spx_debug_last_call_concurrent()))
            assert form == mixed, (name, form, mixed)
            assert form != 0 or mixed == 0
    finally:
        plan.close()


def test_refusals_enqueue_nothing():
    """Every rule of the call: -1 with its text, and out, n_out, n_probe and speeds keep their sentinels."""
    import torch
    from speedy_amd._lib import StreamJob
    from speedy_amd.batch import Plan
    rate, ch, table = _mix8(1.0)
    table = table[:4]
    plan = Plan(rate)
    try:
        L = plan.L
        b = _twopass(plan, table, ch)
        hs = torch.cuda.current_stream().cuda_stream
        n = b.n
        need = L.spx_batch_workspace_bytes_twopass(plan.h, b.jobs, b._seconds_ptr(), n)
        assert need == b.d_ws.numel() and need > L.spx_batch_workspace_bytes(plan.h, b.jobs, n)

        def call(jobs=None, seconds="own", ws_bytes=None, probe=True, speeds=True):
            b.d_out.fill_(CANARY)
            b.d_nout.fill_(-77)
            b.d_probe.fill_(-78)
            b.d_speeds.fill_(-79.0)
            sec = b._seconds_ptr() if isinstance(seconds, str) else seconds
            rc = L.spx_batch_run_twopass(plan.h, b.jobs if jobs is None else jobs, sec, n, b.d_in.data_ptr(), b.d_out.data_ptr(),
                                         b.d_nout.data_ptr(), b.d_probe.data_ptr() if probe else None,
                                         b.d_speeds.data_ptr() if speeds else None, b.d_ws.data_ptr(),
                                         need if ws_bytes is None else ws_bytes, None, hs)
            msg = L.spx_last_error().decode() if rc != 0 else ""
            torch.cuda.synchronize()
            untouched = (bool((b.d_out == CANARY).all()) and bool((b.d_nout == -77).all()) and bool((b.d_probe == -78).all())
                         and bool((b.d_speeds == -79.0).all()))
            return rc, msg, untouched

        def jobs_with(i, **kw):
            j = (StreamJob * n)()
            for k in range(n):
                for f, _t in StreamJob._fields_:
                    setattr(j[k], f, getattr(b.jobs[k], f))
            for f, v in kw.items():
                setattr(j[i], f, v)
            return j

        def secs(i, v):
            s = b.seconds.copy()
            s[i] = v
            return s

        cases = [
            ("bad job", dict(jobs=jobs_with(n - 1, channels=0))),                      # spx_check_jobs, the probe table
            ("feedback", dict(jobs=jobs_with(n - 1, feedback=float("nan")))),
            ("nonlinear", dict(jobs=jobs_with(n - 1, nonlinear=1.5))),                 # ... the final table alone
            ("n_probe", dict(probe=False)),
            ("speeds", dict(speeds=False)),
            ("seconds", dict(seconds=secs(1, -1.0))),
            ("seconds", dict(seconds=secs(0, float("nan")))),
            ("seconds", dict(seconds=secs(2, float("inf")))),
            ("probe speed", dict(jobs=jobs_with(1, speed=0.0))),                       # match mode reads the job's speed
            ("probe speed", dict(jobs=jobs_with(1, speed=float("nan")))),
            ("probe speed", dict(jobs=jobs_with(0, n_in=0))),                          # length mode on an empty stream: want = 0
            ("probe speed", dict(seconds=secs(0, 1e-60))),                             # (float)want is infinite
            ("1e18", dict(jobs=jobs_with(1, speed=1e6, out_cap=10 ** 7))),
            ("workspace", dict(ws_bytes=need - 1)),
        ]
        for word, kw in cases:
            keep = [kw[k] for k in kw]   # (ctypes arrays and numpy buffers stay alive over the call)
            if "seconds" in kw:
                kw = dict(kw, seconds=kw["seconds"].ctypes.data_as(C.POINTER(C.c_double)))
            rc, msg, untouched = call(**kw)
            assert rc == -1 and word in msg and untouched, (word, rc, msg, untouched)
            del keep
        # the workspace query answers 0 for a refused table, and the speed of a LENGTH job is not judged
        assert L.spx_batch_workspace_bytes_twopass(plan.h, jobs_with(n - 1, nonlinear=1.5), b._seconds_ptr(), n) == 0
        assert "nonlinear" in L.spx_last_error().decode()
        assert L.spx_plan_out_capacity_twopass(plan.h, 1000, float("nan"), 1.0) == -1
        rc, msg, untouched = call(jobs=jobs_with(0, speed=float("nan")))
        assert rc == 0 and not untouched, msg
        rc, msg, untouched = call(ws_bytes=need)
        assert rc == 0 and not untouched, msg
        good = _snap(b)
        b.run()
        again = _snap(b)
        assert np.array_equal(good[0], again[0]) and all(np.array_equal(a, c) for a, c in zip(good[1], again[1]))
    finally:
        plan.close()


def test_capacity():
    """spx_plan_out_capacity_twopass is the larger of the two plain capacities; an out_cap that is too small gives the negative
    n_out spx_batch_run gives the final table, and nothing is written past the region."""
    import torch
    from speedy_amd.batch import Plan
    rate, ch, table = _mix8(1.0)
    table = table[:4]
    plan = Plan(rate)
    try:
        L = plan.L
        for n_in, want, nl in ((16000, 3.5, 1.0), (16000, 3.5, 0.0), (6000, 0.8, 1.0), (6000, 0.8, 0.0), (6000, 0.005, 0.0)):
            wf = float(np.float32(want))
            assert L.spx_plan_out_capacity_twopass(plan.h, n_in, want, nl) == max(L.spx_plan_out_capacity_for(plan.h, n_in, wf, 1.0),
                                                                               L.spx_plan_out_capacity_for(plan.h, n_in, wf, nl))
        full = _twopass(plan, table, ch)
        full.run()
        full_probe, full_speeds = full.probe_counts(), full.final_speeds()
        full_nout, _ = _snap(full)
        # stream 0: far too small for either pass; stream 2: the room the final pass needed in the full call -- the probe's frames
        # are more, its count comes back negative, and the final pass then runs at the probe's speed (the fallback) and overflows too
        assert full_nout[2] < full_probe[2]
        small = {0: 100, 2: int(full_nout[2])}
        b = _twopass(plan, table, ch)
        for i, cap in small.items():
            b.jobs[i].out_cap = cap
        b.d_out.fill_(CANARY)
        b.run()
        n_probe, speeds = b.probe_counts(), b.final_speeds()
        torch.cuda.synchronize()
        nout = b.d_nout.cpu().numpy().copy()
        out = b.d_out.cpu().numpy().copy()
        assert n_probe[0] < 0 and n_probe[2] < 0 and np.array_equal(n_probe[[1, 3]], full_probe[[1, 3]])
        assert np.array_equal(tp.bits(speeds[[0, 2]]), tp.bits(b.want[[0, 2]].astype(np.float32)))
        assert np.array_equal(tp.bits(speeds[[1, 3]]), tp.bits(full_speeds[[1, 3]]))
        f = _plain(plan, table, ch, speeds)
        for i, cap in small.items():
            f.jobs[i].out_cap = cap
        f.run()
        torch.cuda.synchronize()
        f_nout = f.d_nout.cpu().numpy()
        print("n_out", nout, "spx_batch_run on the final table", f_nout)
        assert np.array_equal(nout, f_nout) and nout[0] < 0
        for i, cap in small.items():
            end = b.out_offs[i] + cap * ch
            nxt = b.out_offs[i + 1]
            assert nxt > end and (out[end:nxt] == CANARY).all(), "stream %d: written past its region" % i
    finally:
        plan.close()


def test_back_to_back_calls():
    """Two calls on two buffer sets with no synchronisation between them give the bytes each gives alone."""
    from speedy_amd.batch import Plan
    plan = Plan(16000)
    try:
        pair = []
        for name in ("mix8-nonlinear", "mix8-finals-mixed"):
            rate, ch, table = BATCHES[name]()
            b = _twopass(plan, table, ch)
            b.run()
            alone = (_snap(b), b.probe_counts(), b.final_speeds())
            b.d_out.fill_(CANARY)
            b.d_nout.fill_(-77)
            pair.append((b, alone))
        for b, _ in pair:
            b.run()
        for b, (snap, n_probe, speeds) in pair:
            nout, outs = _snap(b)
            assert np.array_equal(nout, snap[0]) and np.array_equal(b.probe_counts(), n_probe)
            assert np.array_equal(tp.bits(b.final_speeds()), tp.bits(speeds))
            assert all(np.array_equal(a, c) for a, c in zip(outs, snap[1]))
    finally:
        plan.close()


def test_c_example(tmp_path):
    """tools/batch_twopass_example.c (plain C99 over include/speedy_hip.h): the counts, speeds and bytes of the Python call."""
    from speedy_amd.batch import Plan
    if not os.path.exists(EXAMPLE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "twopassexample"])
    x, rate, ch = _wav("tapestry.wav")
    x = x[:16000]
    raw = str(tmp_path / "in.raw")
    x.tofile(raw)
    r = subprocess.run([EXAMPLE, raw, str(rate), str(ch), "1", "l0.5", "m3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    plan = Plan(rate)
    try:
        b = _twopass(plan, [(x, 0.5, 1.0, 1.0, 0.0), (x, 0.0, 3.0, 1.0, 0.0)], ch)
        b.run()
        outs = b.results()
        n_probe, speeds = b.probe_counts(), b.final_speeds()
        lines = ["stream %d probe %d speed %08x frames %d crc32 %08x" % (i, n_probe[i], tp.bits(speeds[i]), outs[i].size // ch,
                                                                          zlib.crc32(outs[i].tobytes())) for i in range(2)]
        assert r.stdout.splitlines() == lines, (r.stdout, lines)
    finally:
        plan.close()
