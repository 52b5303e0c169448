"""spx_edit_replay_scaled on the MI355X: an edit list decided at the key's sample rate, replayed on int16 and float tracks at a
higher one.

Every check is against tests/edit_scaled_ref.py, bit for bit -- floats as their 32 bits -- with guard values around every output
region and in n_out_y (tests/edit_scaled_util.py).  The larger tracks are compared with the record-at-a-time form of the definition
(replay_scaled_np, held to the definition itself by tests/test_edit_scaled_definition.py), small ones with the definition directly.
The directed keys run once per module and are shared."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_list_ref as E  # noqa: E402
import edit_scaled_ref as SC  # noqa: E402
import edit_scaled_util as U  # noqa: E402
import tsm_inputs as I  # noqa: E402
import tsm_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

FORMATS = ["int16", "float"]


def _sync_np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _edits_batch(plan, streams, chans, speeds, nls, caps=None):
    from speedy_amd.batch import Batch
    b = Batch(plan, [x.size // c for x, c in zip(streams, chans)], chans, speeds, nls, edits=True, ops_caps=caps)
    b.upload(streams)
    b.run()
    return b


@pytest.fixture(scope="module")
def key(orc):
    """The directed keys, run once: two linear jobs (3.5x and 0.7x, 9001 frames) and one nonlinear job (15000 frames) at 16 kHz mono,
    with their definitions (tests/edit_list_ref.py) -- the device's records and counts are the definition's."""
    from speedy_amd.batch import Plan
    by = {j[0]: j for j in I.linear_jobs()}
    lin = [by["speeds/16000Hz/1ch/9001/3.5"], by["speeds/16000Hz/1ch/9001/0.7"]]
    nl = [j for j in I.nonlinear_jobs() if j[0] == "nonlinear/16000Hz/1ch/15000/3.5/1"]
    assert len(nl) == 1
    with E.shared_pitch_searches():
        defs = [E.linear_job(j[3], j[1], j[2], j[4]) for j in lin]
        name, rate, ch, x, speed, nlv = nl[0]
        tap = orc.compress_sound(x, rate, ch, speed, nlv, 0.0, False, chunk=1000, taps=True)["speed"]
        defs.append(E.nonlinear_job(x, rate, ch, T.event_speeds(x.size // ch, rate, tap, speed), speed))
    jobs = lin + nl
    plan = Plan(16000, False)
    try:
        b = _edits_batch(plan, [j[3] for j in jobs], [1, 1, 1], [j[4] for j in jobs], [0.0, 0.0, nl[0][5]])
        assert _sync_np(b.d_nout).tolist() == [e.out_n for e in defs]
        assert b.op_counts().tolist() == [len(e.ops) for e in defs]
        for i, e in enumerate(defs):
            assert np.array_equal(b.edits(i), np.asarray(e.ops, np.int32).reshape(-1, 4)), i
        assert defs[2].limit == 15000 // 160 * 160 < 15000
        yield b, defs
    finally:
        plan.close()


def _master_tracks(b, chans, p, q, fmt, seed, short=None):
    """One track per stream of the whole master length S(n_in) (`short`: that many frames fewer), and an odd number of values
    behind the last whole frame of every second one (any length is a track)."""
    frames = [SC.S(int(n), p, q) - (short[i] if short else 0) for i, n in enumerate(b.lengths)]
    return [U.track(fmt, f * c + (i % 2), seed + i) for i, (f, c) in enumerate(zip(frames, chans))], frames


def _want(defs, tracks, frames, chans, p, q, fmt):
    return [SC.replay_scaled_np(e.ops, y, c, e.limit, e.out_n, p, q, f, fmt) for e, y, f, c in zip(defs, tracks, frames, chans)]


# ------------------------------------------------------------------ directed jobs ------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("k", range(5), ids=["%d_%d" % r for r in SC.RATIOS])
def test_directed_jobs_at_every_ratio_in_both_formats(key, k, fmt):
    """The three keys' lists on tracks of 1, 2 and 3 channels (which stream has which turns with the ratio): full-scale int16 with
    both ends of the range, floats across -1 .. 1 with denormals and both zeros; in_off and out_off odd."""
    b, defs = key
    p, q = SC.RATIOS[k]
    chans = [1 + (i + k) % 3 for i in range(3)]
    tracks, frames = _master_tracks(b, chans, p, q, fmt, 700 + 10 * k)
    if fmt == "int16":
        assert all(y.min() == -32768 and y.max() == 32767 for y in tracks)
    else:
        assert all(y.min() == -1 and y.max() == 1 and (np.abs(y[y != 0]) < 1e-38).any() and np.signbit(y[y == 0]).any() for y in tracks)
    r = U.Scaled(b, chans, p, q, fmt, tracks, in_res=(1, 3, 7), out_res=(7, 1, 3))
    assert all(int(r.tr[i].in_off) % 4 and int(r.tr[i].out_off) % 4 for i in range(3))
    rc, msg = r.call()
    assert rc == 0, msg
    assert r.counts().tolist() == [SC.S(e.out_n, p, q) for e in defs]
    r.check(_want(defs, tracks, frames, chans, p, q, fmt))


def test_at_one_to_one_int16_is_spx_edit_replay_byte_for_byte(key):
    """The same lists, tracks and offsets through spx_edit_replay and through the new call at 1 / 1 (and at 7 / 7, which reduces
    to it): the two output buffers, guard values and all, are the same bytes."""
    import torch
    from speedy_amd._lib import EditTrack
    b, defs = key
    chans = [3, 1, 2]
    tracks, frames = _master_tracks(b, chans, 1, 1, "int16", 40)
    for p, q in ((1, 1), (7, 7)):
        r = U.Scaled(b, chans, p, q, "int16", tracks, in_res=(3, 7, 1), out_res=(1, 3, 7))
        rc, msg = r.call()
        assert rc == 0, msg
        old = (EditTrack * b.n)()
        for i in range(b.n):
            old[i].in_off, old[i].out_off, old[i].channels, old[i].reserved = r.tr[i].in_off, r.tr[i].out_off, chans[i], 0
        d_old = torch.full((r.size_out,), U.CANARY16, dtype=torch.int16, device=b.device)
        L = b.plan.L
        rc = L.spx_edit_replay(b.plan.h, b.jobs, b.n, b.d_ops.data_ptr(), b._ops_cap_ptr(), b.d_nops.data_ptr(), b.d_nout.data_ptr(), old,
                               r.d_y.data_ptr(), d_old.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, L.spx_last_error()
        assert _sync_np(d_old).tobytes() == r.out().tobytes()
        assert r.counts().tolist() == [e.out_n for e in defs]


# ------------------------------------------------------------------ planted lists, no walk call ------------------------------------------------------------------

def _planted(plan, lists):
    """A Batch(edits=True) that never runs: lists[i] = (key frames n_in, records, n_out).  The records, counts and output lengths
    are written where spx_batch_run_edits would have left them; out_cap is n_out."""
    import torch
    from speedy_amd.batch import Batch
    b = Batch(plan, [l[0] for l in lists], 1, 1.0, 0.0, edits=True, ops_caps=[len(l[1]) for l in lists])
    ops = np.full((max(1, b.op_offs[-1]), 4), U.OP_CANARY, np.int32)
    for i, (n_in, recs, n_out) in enumerate(lists):
        assert E.contiguous(recs)
        ops[b.op_offs[i]:b.op_offs[i] + len(recs)] = np.asarray(recs, np.int32).reshape(-1, 4)
        b.jobs[i].out_cap = n_out
        b.out_caps[i] = n_out
    b.d_ops.copy_(torch.from_numpy(ops).to(b.device))
    b.d_nops.copy_(torch.tensor([len(l[1]) for l in lists], dtype=torch.int64))
    b.d_nout.copy_(torch.tensor([l[2] for l in lists], dtype=torch.int64))
    return b


def _planted_lists():
    n_in = 16000
    tiny, at = [], 0
    for k in range(3000):               # records of one and two frames: at 3 / 1 a block of 4096 mono values holds about 900 of them
        n = 1 + k % 2
        a, bb = (k * 37) % (n_in - 4), (k * 101 + 5) % (n_in + 300)      # (some up-ramps reach behind L)
        tiny.append((at, a, -1 if k % 3 == 0 else bb, n))
        at += n
    straddle = [(0, 10, -1, 1300), (1300, 1310, 2400, 200), (1500, 2600, -1, 77), (1577, 5, 900, 1), (1578, 906, -1, 3)]
    big = [(0, 0, -1, 5), (5, 100, 20000, 21845), (21850, 41845, -1, 150)]
    return [(n_in, tiny, at - 1),                                        # the cut falls inside the last record
            (4000, straddle, 1581), (50000, big, 22000), (4000, straddle, 1581), (4000, straddle, 1500)]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("p,q", [(3, 1), (441, 160)])
def test_planted_lists(fmt, p, q):
    """Lists nobody's job wrote, five streams in one call:
      0  3 000 records of one and two frames, copies and cross-fades in turn, on a mono track: at 3 / 1 a block holds more records
         than it stages (512) and reads them where they lie; every record boundary falls inside some lane's group of four
      1  a cross-fade of 200 frames from key frame 1300: at 3 / 1 master frames 3900 .. 4500, across the first block boundary, on a
         mono track; a cross-fade of one frame (n' = 3: inside one group of four)
      2  a cross-fade with n' = 65535 at 3 / 1 (n = 21845), full-scale values: the quotient's last exact n'
      3  list 1 on a 2-channel track 40 frames shorter than S(L): the tail reads 0
      4  list 1 on a track with n_in = 0 (and not one value): every value 0 (+0.0f), the cut inside the cross-fade
    Stream 1 is compared with the definition itself, the others with its record-at-a-time form."""
    from speedy_amd.batch import Plan
    lists = _planted_lists()
    if (p, q) == (3, 1):
        assert SC.scaled_ops(lists[2][1], p, q)[1][3] == 65535
        assert SC.scaled_ops(lists[1][1], p, q)[1][0] < 4096 < SC.scaled_ops(lists[1][1], p, q)[2][0]
    chans = [1, 1, 1, 2, 3]
    plan = Plan(16000, False)
    try:
        b = _planted(plan, lists)
        frames = [SC.S(l[0], p, q) for l in lists]
        frames[3] -= 40
        frames[4] = 0
        tracks = [U.track(fmt, f * c, 900 + i) for i, (f, c) in enumerate(zip(frames, chans))]
        r = U.Scaled(b, chans, p, q, fmt, tracks, in_res=(7, 1, 3), out_res=(1, 7, 3))
        assert int(r.tr[4].n_in) == 0 and int(r.tr[3].n_in) < SC.S(lists[3][0], p, q)
        rc, msg = r.call()
        assert rc == 0, msg
        assert r.counts().tolist() == [SC.S(l[2], p, q) for l in lists]
        want = [SC.replay_scaled_np(l[1], y, c, l[0], l[2], p, q, f, fmt) for l, y, f, c in zip(lists, tracks, frames, chans)]
        want[1] = SC.replay_scaled(lists[1][1], tracks[1], 1, lists[1][0], lists[1][2], p, q, frames[1], fmt)
        assert None not in want[1]
        assert not U.as_bits(want[4], fmt).any() and U.as_bits(want[3], fmt).any()
        r.check(want)
        if (p, q) == (3, 1):
            assert plan.L.spx_debug_last_scaled_grid(None) == (22000 * 3 + 3 + 4095) // 4096
    finally:
        plan.close()


def test_planted_lists_at_one_to_one_through_both_calls():
    """The first three planted lists on mono int16 tracks through spx_edit_replay and through spx_edit_replay_scaled at 1 / 1 -- two
    instantiations of one kernel body (identity and multiply).  At 1 / 1 a block of 4096 values holds about 2 700 of list 0's
    records, so both kernels read them where they lie (the recorded lists of the equality test above always stage); list 1's
    cross-fade straddles no block here but its one-frame cross-fade and the odd offsets exercise the head and tail stores; list 2 is
    the n = 21 845 cross-fade.  The two output buffers are the same bytes, guard values included, each equals the definition, and
    the counts are n_out."""
    import torch
    from speedy_amd._lib import EditTrack
    from speedy_amd.batch import Plan
    lists = _planted_lists()[:3]
    assert sum(1 for r in lists[0][1] if r[0] < 4096) > 512
    plan = Plan(16000, False)
    try:
        b = _planted(plan, lists)
        tracks = [U.track("int16", l[0], 950 + i) for i, l in enumerate(lists)]
        r = U.Scaled(b, [1, 1, 1], 1, 1, "int16", tracks, in_res=(7, 1, 3), out_res=(1, 7, 3))
        rc, msg = r.call()
        assert rc == 0, msg
        old = (EditTrack * b.n)()
        for i in range(b.n):
            old[i].in_off, old[i].out_off, old[i].channels, old[i].reserved = r.tr[i].in_off, r.tr[i].out_off, 1, 0
        d_old = torch.full((r.size_out,), U.CANARY16, dtype=torch.int16, device=b.device)
        L = plan.L
        rc = L.spx_edit_replay(plan.h, b.jobs, b.n, b.d_ops.data_ptr(), b._ops_cap_ptr(), b.d_nops.data_ptr(), b.d_nout.data_ptr(), old,
                               r.d_y.data_ptr(), d_old.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, L.spx_last_error()
        assert _sync_np(d_old).tobytes() == r.out().tobytes()
        assert r.counts().tolist() == [l[2] for l in lists]
        want = [SC.replay_scaled_np(l[1], y, 1, l[0], l[2], 1, 1, l[0], "int16") for l, y in zip(lists, tracks)]
        r.check(want)                                   # (and so does the plain call's buffer: it is the same bytes)
    finally:
        plan.close()


# ------------------------------------------------------------------ counts------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_counts_of_streams_that_do_not_fit_or_have_nothing(key, fmt):
    """out_cap one frame short: -N', that region all guard values, the neighbours rendered.  A negative n_ops, an n_ops above the
    capacity, n_out = 0 and a negative n_out among good streams: 0, nothing written, the good ones rendered."""
    import torch
    b, defs = key
    p, q = 441, 160
    chans = [2, 1, 2]
    tracks, frames = _master_tracks(b, chans, p, q, fmt, 60)
    want = _want(defs, tracks, frames, chans, p, q, fmt)
    N = [SC.S(e.out_n, p, q) for e in defs]
    r = U.Scaled(b, chans, p, q, fmt, tracks, out_caps=[N[0], N[1] - 1, N[2]])
    rc, msg = r.call()
    assert rc == 0, msg
    assert r.counts().tolist() == [N[0], -N[1], N[2]] == [SC.count(e.out_n, int(b.out_caps[i]), len(e.ops), int(b.ops_caps[i]), p, q, int(r.tr[i].out_cap))
                                                          for i, e in enumerate(defs)]
    r.check([want[0], None, want[2]])
    nops, nout = b.op_counts(), _sync_np(b.d_nout)
    for bad_ops, bad_out, live in (([nops[0], -nops[1], nops[2]], [nout[0], nout[1], 0], [True, False, False]),
                                   ([nops[0], nops[1], int(b.ops_caps[2]) + 1], [-nout[0], nout[1], nout[2]], [False, True, False]),
                                   ([0, nops[1], nops[2]], list(nout), [False, True, True])):
        r = U.Scaled(b, chans, p, q, fmt, tracks)
        d_nops = torch.tensor([int(v) for v in bad_ops], dtype=torch.int64, device=b.device)
        d_nout = torch.tensor([int(v) for v in bad_out], dtype=torch.int64, device=b.device)
        rc, msg = r.call(nops=d_nops.data_ptr(), nout=d_nout.data_ptr())
        assert rc == 0, msg
        assert r.counts().tolist() == [N[i] if live[i] else 0 for i in range(3)]
        r.check([want[i] if live[i] else None for i in range(3)])


# ------------------------------------------------------------------ the grid ------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_three_hundred_streams_with_more_than_one_block_each(fmt):
    """300 keys of four kinds in one call, each with a 2-channel master at 3 / 1 of more than one block; the expected values are the
    definition applied to the records the device wrote (tests/test_gpu_edit_list.py holds those to their own definition)."""
    from speedy_amd.batch import Plan
    kinds = [(I.rectangles(16000, 1, 2000), 2.0), (I.syllables(16000, 1, 2400), 0.7), (I.rectangles(16000, 1, 3211), 3.5), (I.syllables(16000, 1, 1777), 1.3)]
    pick = [(i * 7 + i // 4) % 4 for i in range(300)]
    plan = Plan(16000, False)
    try:
        b = _edits_batch(plan, [kinds[k][0] for k in pick], [1] * 300, [kinds[k][1] for k in pick], 0.0)
        nout, nops = _sync_np(b.d_nout), b.op_counts()
        assert (nout > 0).all() and (nops > 0).all()
        first = [pick.index(k) for k in range(4)]
        for i, k in enumerate(pick):
            assert nout[i] == nout[first[k]] and nops[i] == nops[first[k]]
        kind_tracks = [U.track(fmt, kinds[k][0].size * 3 * 2, 40 + k) for k in range(4)]
        r = U.Scaled(b, [2] * 300, 3, 1, fmt, [kind_tracks[k] for k in pick], in_res=(1, 3, 7), out_res=(3, 7, 1))
        rc, msg = r.call()
        assert rc == 0, msg
        launches = C.c_int(0)
        gx = plan.L.spx_debug_last_scaled_grid(C.byref(launches))
        assert launches.value == 1 and gx == max((int(c) * 3 * 2 + 3 + 4095) // 4096 for c in b.out_caps) and gx >= 2
        assert min(nout) * 3 * 2 > 4096, "every stream has more than one block"
        want4 = [SC.replay_scaled_np(b.edits(first[k]).tolist(), kind_tracks[k], 2, kinds[k][0].size, int(nout[first[k]]), 3, 1,
                                     kinds[k][0].size * 3, fmt) for k in range(4)]
        assert r.counts().tolist() == [3 * int(v) for v in nout]
        r.check([want4[k] for k in pick])
    finally:
        plan.close()


# ------------------------------------------------------------------ refusals ------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_refusals_launch_nothing_and_a_good_call_works_right_after(key, fmt):
    from speedy_amd._lib import EditMaster
    b, defs = key
    p, q = 2, 1
    chans = [2, 1, 3]
    tracks, frames = _master_tracks(b, chans, p, q, fmt, 80)
    r = U.Scaled(b, chans, p, q, fmt, tracks)
    L = b.plan.L
    i64 = C.POINTER(C.c_int64)
    size = 4 if fmt == "float" else 2

    def table(**kw):
        t = (EditMaster * b.n)()
        for k in range(b.n):
            for f in ("in_off", "out_off", "n_in", "out_cap", "channels"):
                setattr(t[k], f, getattr(r.tr[k], f))
        for f, v in kw.items():
            setattr(t[1], f, v)
        return t

    cases = [({key_: None}, "NULL") for key_ in ("ops", "caps", "nops", "nout", "tracks", "y", "yout", "count")]
    cases += [({"tracks": table(channels=0)}, "channels"), ({"tracks": table(channels=65536)}, "channels"),
              ({"tracks": table(in_off=-1)}, "negative"), ({"tracks": table(out_off=-1)}, "negative"),
              ({"tracks": table(n_in=-1)}, "negative"), ({"tracks": table(out_cap=-1)}, "negative"),
              ({"ops": b.d_ops.data_ptr() + 4}, "aligned"),
              ({"y": r.d_y.data_ptr() + size // 2}, "aligned"), ({"yout": r.d_yout.data_ptr() + size // 2}, "aligned"),
              ({"caps": C.cast((C.c_int64 * 3)(5, -1, 5), i64)}, "negative capacity"),
              ({"caps": C.cast((C.c_int64 * 3)(2 ** 31 - 1, 1, 1), i64)}, "2^31 - 1"),
              ({"fmt": 2}, "sample_format"), ({"fmt": -1}, "sample_format")]
    cases += [({"p": pp, "q": qq}, "ratio") for pp, qq in ((1, 2), (33, 1), (0, 1), (3, 0), (-2, 1), (32769, 32768), (65538, 2))]
    for kw, word in cases:
        rc, msg = r.call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
        assert r.untouched(), kw
    # a table spx_batch_run refuses, with its message
    good = b.jobs[1].speed
    b.jobs[1].speed = float("nan")
    try:
        rc, msg = r.call()
        assert rc == -1 and "speed" in msg and r.untouched(), (rc, msg)
    finally:
        b.jobs[1].speed = good
    # positions at the master's rate that do not fit 2^31 - 1: S(out_cap) at 32 / 1, then S(L)
    cap, n_in = b.jobs[1].out_cap, b.jobs[1].n_in
    try:
        b.jobs[1].out_cap = 2 ** 26 + 1
        rc, msg = r.call(p=32, q=1)
        assert rc == -1 and "2^31 - 1" in msg and r.untouched(), (rc, msg)
        b.jobs[1].out_cap = cap
        b.jobs[1].n_in = 2 ** 26 + 1
        rc, msg = r.call(p=32, q=1)
        assert rc == -1 and "2^31 - 1" in msg and r.untouched(), (rc, msg)
    finally:
        b.jobs[1].out_cap, b.jobs[1].n_in = cap, n_in
    rc, msg = r.call()
    assert rc == 0, msg
    assert r.counts().tolist() == [SC.S(e.out_n, p, q) for e in defs]
    r.check(_want(defs, tracks, frames, chans, p, q, fmt))


# ------------------------------------------------------------------ Python, and the C example ------------------------------------------------------------------

def test_python_round_trip_and_its_exceptions(key):
    import torch
    b, defs = key
    y16 = [U.full_scale(SC.S(int(n), 3, 1) * 2, 20 + i) for i, n in enumerate(b.lengths)]
    got = b.replay_scaled(y16, 2, 3)
    for i, e in enumerate(defs):
        assert got[i].dtype == np.int16 and np.array_equal(got[i], SC.replay_scaled_np(e.ops, y16[i], 2, e.limit, e.out_n, 3, 1, y16[i].size // 2)), i
    chans = [1, 2, 1]
    yf = [U.float_track(SC.S(int(n), 441, 160) * c + 1, 30 + i) for i, (n, c) in enumerate(zip(b.lengths, chans))]
    got = b.replay_scaled([yf[0], torch.from_numpy(yf[1]), yf[2]], chans, (44100, 16000))
    for i, e in enumerate(defs):
        want = SC.replay_scaled_np(e.ops, yf[i], chans[i], e.limit, e.out_n, 441, 160, yf[i].size // chans[i], "float")
        assert got[i].dtype == np.float32 and np.array_equal(SC.bits(got[i]), SC.bits(want)), i
    with pytest.raises(ValueError):
        b.replay_scaled([y16[0], yf[1], y16[2]], 1, 3)
    with pytest.raises(ValueError):
        b.replay_scaled([y.astype(np.float64) for y in yf], 1, 3)
    with pytest.raises(RuntimeError):
        b.replay_scaled(y16, 2, (1, 2))
    with pytest.raises(RuntimeError):
        b.replay_scaled(y16, 0, 3)
    caps = list(b.out_caps)
    try:
        b.out_caps[1] = defs[1].out_n - 1            # the scaled capacity no longer holds stream 1: a negative count
        with pytest.raises(RuntimeError):
            b.replay_scaled(y16, 2, 3)
    finally:
        b.out_caps[:] = caps


def test_c_edit_scaled_example():
    """tools/batch_edit_scaled_example.c: a 16 kHz mono key decides, a 48 kHz stereo float master is rendered through the C ABI
    alone; the counts are printed, M = 3 N, and the program's own check of one cross-fade value against the formula passes."""
    exe = os.path.join(ROOT, "speedy_amd", "lib", "batch_edit_scaled_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "editscaledexample"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    w = r.stdout.split()
    assert w[0] == "frames" and w[2] == "ops" and w[4] == "master_frames" and w[6] == "xfade"
    assert int(w[1]) > 0 and int(w[3]) > 0 and int(w[5]) == 3 * int(w[1]) and 0 <= int(w[7]) < int(w[5])
