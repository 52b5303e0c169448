"""GPU: the int16 output and the frame count of every walk form, of the rate family, of the float call and of the drop-in stream
API against the exact integer definition of the time-scale modification (tests/tsm_ref.py) -- not against the oracle -- on the
full-scale, channel-distinct inputs of tests/tsm_inputs.py (what they reach: tests/test_oracle_tsm_definition.py,
profiles/tsm_definition.txt).  Every case also asserts the walk form it ran on.  Integer equality, no tolerance.

The drop-in API's rate stage (sonic2_api.hip, spx_rate_kernel) is held against tsm_ref.PlaybackStream call for call: rate changes
in mid-stream, both lives, a rate first set behind unread output, one nonlinear life on the events its own speed callback
reported, and the 16-channel limit.

The definition's outputs are computed once per module (_WANT) and left unchanged.
"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsm_inputs as I  # noqa: E402
import tsm_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

_WANT = {}


def want(job):
    """The definition's int16 output of a directed job (linear: 5 fields, with a rate: 6), once per module."""
    if job[0] not in _WANT:
        name, rate, ch, x, speed = job[:5]
        s = T.linear_job(x, rate, ch, speed) if len(job) == 5 else T.rate_job(x, rate, ch, speed, job[5])
        y = np.asarray(s.out, np.int64)
        assert y.size == 0 or (y.min() >= -32768 and y.max() <= 32767)
        _WANT[job[0]] = y.astype(np.int16)
        _WANT[job[0]].setflags(write=False)
    return _WANT[job[0]]


def differing(names, got, wants):
    """[(name, frames got, frames wanted, first differing value)] of the streams that are not the definition's."""
    bad = []
    for name, g, w in zip(names, got, wants):
        if g.size != w.size or not np.array_equal(g, w):
            k = min(g.size, w.size)
            d = np.nonzero(g[:k] != w[:k])[0]
            bad.append((name, g.size, w.size, int(d[0]) if d.size else k))
    return bad


def run_batch(rate, jobs, nonlinear=0.0, taps=False, time_map=False):
    """One batch call over directed jobs of one sample rate; returns (outputs, form, concurrent, batch, plan)."""
    from speedy_amd.batch import Batch, Plan
    plan = Plan(rate, False)
    b = Batch(plan, [j[3].size // j[2] for j in jobs], [j[2] for j in jobs], [j[4] for j in jobs], nonlinear, 0.0, taps=taps,
              rate=[j[5] for j in jobs] if len(jobs[0]) == 6 and nonlinear == 0.0 else None, time_map=time_map)
    b.upload([j[3] for j in jobs])
    b.run()
    outs = b.results()
    return outs, plan.L.spx_debug_last_walk_form(), plan.L.spx_debug_last_call_concurrent(), b, plan


def speedup_only(jobs):
    """The engine's own rule (include/speedy_hip.h): every job has a speed above 1."""
    return int(all(np.float32(j[4]) > np.float32(1.0) for j in jobs))


def walk_name(plan, jobs, lean=False):
    """The walk kernel that serves this batch, as spx_batch_kernel_names (_lean) gives it."""
    fn = plan.L.spx_batch_kernel_names_lean if lean else plan.L.spx_batch_kernel_names
    return fn(plan.h, len(jobs), max(j[2] for j in jobs), speedup_only(jobs)).decode().split(";")[2]


def form_of(kernel):
    """16 x search waves + output waves of a walk kernel's name; 0: the general kernel."""
    m = re.fullmatch(r"spx_walk_fast_kernel<(\d+), (\d+), \d+, \d+, \d+>", kernel)
    if m:
        return 16 * int(m.group(1)) + int(m.group(2))
    assert re.fullmatch(r"spx_walk_kernel<\d+, \d+>", kernel), kernel
    return 0


def prime_the_form_counter():
    """spx_debug_last_walk_form() starts at 0, which is also "the general kernel": before a case that expects 0, one small job on the
    speed-up kernel leaves 68 there, so that a 0 afterwards says that the general kernel was LAUNCHED."""
    jobs = [j for j in I.linear_jobs() if j[0] == "lengths/22050Hz/1ch/679/2"]
    outs, form, _, _, plan = run_batch(22050, jobs)
    plan.close()
    assert form == 68 and np.array_equal(outs[0], want(jobs[0]))


def _fam(name):
    return name.split("/")[0]


def linear(rate, channels=None, up=False, family=None):
    """The directed linear jobs of a sample rate.  channels: a count, "many" (more than one) or None (any).  up: the jobs with a
    speed above 1 only -- otherwise every job at a speed of 1 or less and, of the faster ones, those outside the two length families
    (which would only make the batch large)."""
    out = []
    for j in I.linear_jobs():
        name, r, c, _, s = j
        fast = np.float32(s) > np.float32(1.0)
        if r == rate and (channels is None or c == channels or (channels == "many" and c > 1)) and (family is None or _fam(name) == family) \
                and (fast if up else (not fast or _fam(name) not in ("run", "lengths"))):
            out.append(j)
    return out


# name: (sample rate, channels, speeds above 1 only, the form that must run: 16 x search waves + output waves (0: the general
# kernel), the walk kernel)
GROUPS = {
    # a CU per stream, speed-up only: the kernels in sequence, the walk kernel keeps its output waves
    "4+4 22k mono": (22050, 1, True, 68, "spx_walk_fast_kernel<4, 4, 22050, 1, 0>"),
    "4+4 16k mono": (16000, 1, True, 68, "spx_walk_fast_kernel<4, 4, 16000, 1, 0>"),
    "4+4 16k stereo": (16000, 2, True, 68, "spx_walk_fast_kernel<4, 4, 16000, 1, 1>"),
    "4+4 22k 2ch": (22050, 2, True, 68, "spx_walk_fast_kernel<4, 4, 22050, 1, 1>"),
    "4+4 22k 3ch": (22050, 3, True, 68, "spx_walk_fast_kernel<4, 4, 22050, 1, 1>"),
    "4+4 22k 5ch": (22050, 5, True, 68, "spx_walk_fast_kernel<4, 4, 22050, 1, 1>"),
    "4+4 22k 7ch": (22050, 7, True, 68, "spx_walk_fast_kernel<4, 4, 22050, 1, 1>"),
    "4+4 22k 8ch": (22050, 8, True, 68, "spx_walk_fast_kernel<4, 4, 22050, 1, 1>"),
    # the instantiation that also serves slow-down events (last template argument 2, multi-channel 3)
    "slow-down 22k mono": (22050, 1, False, 68, "spx_walk_fast_kernel<4, 4, 0, 0, 2>"),
    "slow-down 16k mono": (16000, 1, False, 68, "spx_walk_fast_kernel<4, 4, 0, 0, 2>"),
    "slow-down 22k many channels": (22050, "many", False, 68, "spx_walk_fast_kernel<4, 4, 0, 0, 3>"),
    "slow-down 16k stereo": (16000, 2, False, 68, "spx_walk_fast_kernel<4, 4, 0, 0, 3>"),
    "slow-down 48k": (48000, 1, False, 132, "spx_walk_fast_kernel<8, 4, 0, 0, 2>"),
    # eight search waves, two lags per lane in the refine select
    "wide 44.1k": (44100, 1, True, 132, "spx_walk_fast_kernel<8, 4, 0, 0, 0>"),
    "wide 48k mono": (48000, 1, True, 132, "spx_walk_fast_kernel<8, 4, 0, 0, 0>"),
    "wide 48k 2ch": (48000, 2, False, 132, "spx_walk_fast_kernel<8, 4, 0, 0, 3>"),
    "wide 48k 4ch": (48000, 4, True, 132, "spx_walk_fast_kernel<8, 4, 0, 0, 1>"),
    "wide 44.1k slow-down": (44100, 1, False, 132, "spx_walk_fast_kernel<8, 4, 0, 0, 2>"),
    # 72 coarse lags, two per lane in the coarse select
    "wide coarse 11k": (11025, 1, True, 68, "spx_walk_fast_kernel<4, 4, 0, 2, 0>"),
    "wide coarse 11k slow-down": (11025, 1, False, 68, "spx_walk_fast_kernel<4, 4, 0, 2, 2>"),
    # the general kernel: rates beyond the speed-up kernel's, skip x channels past 56
    "general 96k": (96000, 1, False, 0, None),
    "general 64k": (63999, 1, False, 0, None),
    "general 48k 5ch": (48000, 5, False, 0, None),
}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_linear_jobs_equal_the_definition_on_every_walk_form(group):
    rate, channels, up, form, kernel = GROUPS[group]
    jobs = linear(rate, channels, up)
    assert len(jobs) >= 2 and speedup_only(jobs) == int(up), group
    if form == 0:
        prime_the_form_counter()
    outs, ran, _, b, plan = run_batch(rate, jobs)
    try:
        bad = differing([j[0] for j in jobs], outs, [want(j) for j in jobs])
        name = walk_name(plan, jobs)
        print(group, len(jobs), "streams, form", ran, name, bad[:4])
        assert ran == form and form_of(name) == form, (group, ran, name)
        assert name == kernel or kernel is None, (group, name)
        assert bad == [], (group, bad[:8])
    finally:
        plan.close()


def test_the_throughput_form():
    """More than two streams per CU: two search waves, no output waves, the short window.  Six distinct jobs, each repeated at
    different places of the batch: the definition runs once per distinct job."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    distinct = [j for j in I.linear_jobs() if j[0] in ("run/22050Hz/1ch/2999/2", "run/22050Hz/1ch/3000/3.5", "run/22050Hz/1ch/3019/2",
                                                       "speeds/22050Hz/1ch/7000/1.3", "speeds/22050Hz/1ch/7000/2", "channels/22050Hz/1ch/6615/1.3")]
    assert len(distinct) == 6
    jobs = [distinct[(i * 5 + i // 6) % 6] for i in range(2 * cus + 8)]
    outs, form, _, b, plan = run_batch(22050, jobs)
    try:
        bad = differing([j[0] for j in jobs], outs, [want(j) for j in jobs])
        name = walk_name(plan, jobs)
        print("throughput", len(jobs), "streams, form", form, name, bad[:4])
        assert form == 16 * 2 + 0 and name == "spx_walk_fast_kernel<2, 0, 22050, 0, 0>", (form, name)
        assert bad == [], bad[:8]
    finally:
        plan.close()


def _nonlinear_case(orc, rate, channels, form, concurrent, kernel, lean=False):
    """Nonlinear jobs of one rate in one call with taps: the speed tap equals the oracle's, the output is the definition's on the
    events that the call's OWN speed tap gives, and the call ran the walk form, the launch mode and the kernel given."""
    jobs = [j for j in I.nonlinear_jobs() if j[1] == rate and j[2] == channels]
    assert jobs
    from speedy_amd.batch import Batch, Plan
    plan = Plan(rate, False)
    try:
        b = Batch(plan, [j[3].size // j[2] for j in jobs], [j[2] for j in jobs], [j[4] for j in jobs], [j[5] for j in jobs], 0.0, taps=True)
        b.upload([j[3] for j in jobs])
        b.run()
        outs = b.results()
        ran, mode, name = plan.L.spx_debug_last_walk_form(), plan.L.spx_debug_last_call_concurrent(), walk_name(plan, jobs, lean)
        print(rate, channels, "form", ran, "concurrent", mode, name)
        assert ran == form and form_of(name) == form and name == kernel, (ran, name)
        assert concurrent is None or mode == concurrent, mode
        for i, (job, _, ch, x, speed, nl) in enumerate(jobs):
            tap = b.tap_arrays(i)["speed"]
            ref = orc.compress_sound(x, rate, ch, speed, nl, 0.0, False, chunk=1000, taps=True)
            assert np.array_equal(tap, ref["speed"]), job
            n = x.size // ch
            speeds = T.event_speeds(n, rate, tap, speed)
            assert 10 < len(tap) < len(speeds) and len(set(speeds)) > 10, job
            key = (job, tap.tobytes())
            if key not in _WANT:
                _WANT[key] = np.asarray(T.nonlinear_job(x, rate, ch, speeds, speed).out, np.int64)
            print(job, "frames", outs[i].size // ch, _WANT[key].size // ch)
            assert outs[i].size == _WANT[key].size and np.array_equal(outs[i], _WANT[key]), (job, outs[i].size, _WANT[key].size)
    finally:
        plan.close()


def test_nonlinear_jobs_on_the_lean_form(orc):
    """22.05 kHz mono, nonlinear: the concurrent mode, where the walk kernel gives up its output waves."""
    _nonlinear_case(orc, 22050, 1, 16 * 4 + 0, 1, "spx_walk_fast_kernel<4, 0, 22050, 0, 0>", lean=True)


def test_nonlinear_jobs_on_the_16_khz_form(orc):
    _nonlinear_case(orc, 16000, 1, 16 * 4 + 4, None, "spx_walk_fast_kernel<4, 4, 16000, 1, 0>")


def test_a_nonlinear_stereo_slow_down_job(orc):
    """Event speeds on both sides of unity, two channels: the multi-channel instantiation that also serves slow-down events."""
    _nonlinear_case(orc, 16000, 2, 16 * 4 + 4, None, "spx_walk_fast_kernel<4, 4, 0, 0, 3>")


def _nonlinear_map_case(orc, rate):
    """Every nonlinear job of one sample rate (tsm_inputs.nonlinear_jobs and nonlinear_map_jobs; 1, 2, 3 and 8 channels side by side
    at 16 kHz) in ONE spx_batch_run_map call with taps: the speed tap equals the oracle's, the output is the definition's on the
    events the call's OWN speed tap gives, and the rows are the definition's rows (tsm_ref.nonlinear_job: frames_out immediately
    before each event's write, then the final count) -- the `if constexpr (MAP)` stores of walk_body against the header's text,
    not against the oracle.  The call runs the general kernel's map instantiation (form 0, the counter primed).

    A map call cannot meet run_impl's "no general walk kernel for this batch": it asks spx_walk_config without a speed class, and
    walk_mode then answers 0 for every channel count.  So every count is taken, and the test asserts that it is."""
    jobs = [j for j in I.nonlinear_jobs() + I.nonlinear_map_jobs() if j[1] == rate]
    assert jobs
    from speedy_amd.batch import Batch, Plan
    prime_the_form_counter()
    plan = Plan(rate, False)
    try:
        b = Batch(plan, [j[3].size // j[2] for j in jobs], [j[2] for j in jobs], [j[4] for j in jobs], [j[5] for j in jobs], 0.0, taps=True,
                  time_map=True)
        b.upload([j[3] for j in jobs])
        b.d_map.fill_(-12345)
        b.run()
        outs = b.results()
        form, chunks = plan.L.spx_debug_last_walk_form(), plan.L.spx_debug_last_call_chunks()
        print(rate, "Hz map call:", len(jobs), "jobs, channels", sorted({j[2] for j in jobs}), "form", form, "chunks", chunks)
        assert form == 0 and chunks == 1, (form, chunks)
        nout = b.d_nout.cpu().numpy()
        for i, (job, _, ch, x, speed, nl) in enumerate(jobs):
            tap = b.tap_arrays(i)["speed"]
            ref = orc.compress_sound(x, rate, ch, speed, nl, 0.0, False, chunk=1000, taps=True)
            assert np.array_equal(tap, ref["speed"]), job
            n = x.size // ch
            speeds = T.event_speeds(n, rate, tap, speed)
            key = ("map", job, tap.tobytes())
            if key not in _WANT:
                s = T.nonlinear_job(x, rate, ch, speeds, speed)
                _WANT[key] = (np.asarray(s.out, np.int64), list(s.rows))
            w_out, w_rows = _WANT[key]
            got = b.time_map(i)
            print(job, "frames", outs[i].size // ch, w_out.size // ch, "rows", got.size)
            assert outs[i].size == w_out.size and np.array_equal(outs[i], w_out), (job, outs[i].size, w_out.size)
            assert got.tolist() == w_rows, (job, [k for k, (a, c) in enumerate(zip(got.tolist(), w_rows)) if a != c][:4])
            assert got.size == n // plan.B + 1 and got[-1] == nout[i] and (n < plan.B or got[0] == 0) and (np.diff(got) >= 0).all(), job
        assert b.map_offs[-1] == b.d_map.numel()
    finally:
        plan.close()


@pytest.mark.parametrize("rate", sorted({j[1] for j in I.nonlinear_jobs() + I.nonlinear_map_jobs()}))
def test_the_rows_of_nonlinear_jobs_are_the_definitions(orc, rate):
    """11.025, 16, 22.05 and 48 kHz; at 16 kHz: n_in = R B, R B + B - 1, R = 1, n_in < B, a slow-down job, 1 / 2 / 3 / 8 channels."""
    _nonlinear_map_case(orc, rate)


def test_the_map_calls_walk_instantiation():
    """spx_batch_run_map: the general walk kernel's map instantiation writes the same int16 output.  (spx_batch_kernel_names speaks of
    the plain call only: the map kernel has no name to ask for; the form counter is primed instead.)"""
    jobs = linear(16000, 1, family="rates")
    assert len(jobs) == 3
    prime_the_form_counter()
    outs, form, _, b, plan = run_batch(16000, jobs, time_map=True)
    try:
        bad = differing([j[0] for j in jobs], outs, [want(j) for j in jobs])
        print("map form", form, bad[:4])
        assert form == 0, form
        assert bad == [], bad[:8]
        for i, j in enumerate(jobs):
            assert b.time_map(i).tolist() == [want(j).size // j[2]], j[0]        # a linear stream: the final count alone
    finally:
        plan.close()


@pytest.mark.parametrize("hz", sorted({j[1] for j in I.rate_jobs()}))
def test_the_rate_family(hz):
    """spx_batch_run_rate (the general walk kernel, then spx_rate_batch.hip's closed form) against the rational definition of the
    rate stage: rates either side of 1, a halving that drops a bit, streams shorter than 8 values, three channels beyond 2 048
    values, output offsets in the caller's buffer that are no multiple of 8 values.  (No kernel name exists for this call either: the
    form counter is primed.)"""
    jobs = [j for j in I.rate_jobs() if j[1] == hz]
    jobs = sorted(jobs, key=lambda j: j[3].size)          # the short streams first: the longer ones start at odd offsets
    prime_the_form_counter()
    outs, form, _, b, plan = run_batch(hz, jobs)
    try:
        bad = differing([j[0] for j in jobs], outs, [want(j) for j in jobs])
        print("rate", hz, "form", form, b.out_offs, bad[:4])
        assert form == 0, form
        if hz == 22050:
            assert sum(1 for off in b.out_offs if off % 8) >= 5, b.out_offs
        assert bad == [], bad[:8]
    finally:
        plan.close()


def test_the_float_batch_call_on_one_job():
    """spx_batch_run_float: the input conversion by its numpy definition, the definition's int16 work in between, every output value
    that int16 / 32767.0f."""
    from speedy_amd.batch import compress_batch_float
    from test_batch_float_abi import float_to_short_def
    name, rate, ch, x, speed = [j for j in I.linear_jobs() if j[0] == "channels/22050Hz/3ch/6615/1.3"][0]
    xf = (x.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    xi = float_to_short_def(xf, False)
    assert np.abs(xi.astype(np.int64)).max() >= 32700
    w = np.asarray(T.linear_job(xi, rate, ch, speed).out, np.int64).astype(np.int16)
    outs, b = compress_batch_float([xf], rate, ch, speed, 0.0, 0.0, False)
    try:
        print("float form", b.plan.L.spx_debug_last_walk_form(), outs[0].size, w.size)
        assert b.plan.L.spx_debug_last_walk_form() == 68
        wf = w.astype(np.float32) / np.float32(32767)
        assert outs[0].size == wf.size and np.array_equal(outs[0].view(np.uint32), wf.view(np.uint32))
    finally:
        b.plan.close()


def _events_def(rate, ch, events, playback=None):
    s = T.SpeedStream(rate, ch) if playback is None else T.RateStream(rate, ch, playback)
    counts = []
    for ev in events:
        s.write(ev[1], ev[2]) if ev[0] == "write" else s.flush(ev[1])
        counts.append(s.frames_out)
    return np.asarray(s.out, np.int64), counts


def _drain(s, cap=1 << 16):
    got = []
    while True:
        y = s.read_short(cap)
        if y.size == 0:
            return np.concatenate(got).astype(np.int64) if got else np.zeros(0, np.int64)
        got.append(y.copy())


@pytest.mark.parametrize("coalesce", [True, False])
def test_the_stream_api_call_for_call_on_the_planted_event_lists(coalesce):
    """The drop-in API, call for call: after every call the reads return exactly what the definition produced in that call --
    through both lives.  The event lists with speeds on both sides of 1 go through the TSM stage's own calls (sonicIntSetSpeed,
    sonicIntWriteShortToStream, sonicIntFlushStream), which the general kernel serves; the lists with speeds above 1 only go
    through the stream's calls with the nonlinear factor 0 (sonicSetSpeed, sonicWriteShortToStream, sonicFlushStream), where the
    handle stays on the speed-up kernel (4 + 4 waves, 8 + 4 at 48 kHz: one short job per launch has a CU to itself)."""
    from speedy_amd.sonic2 import SonicStream
    for name, rate, ch, events in I.planted_streams():
        key = ("stream", name)
        if key not in _WANT:
            _WANT[key] = _events_def(rate, ch, events)
        out, counts = _WANT[key]
        s = SonicStream(rate, ch, False, coalesce)
        fast = name.startswith("speedup")
        assert (fast == all(ev[-1] > 1.0 for ev in events)) or name.startswith("second_life")
        if not fast:
            prime_the_form_counter()
        try:
            s.enable_nonlinear(0.0)
            done = 0
            for k, ev in enumerate(events):
                if fast:
                    s.set_speed(ev[-1])
                    assert (s.write_short(ev[1]) if ev[0] == "write" else s.flush()) == 1
                else:
                    s.int_set_speed(ev[-1])
                    assert (s.int_write_short(ev[1]) if ev[0] == "write" else s.int_flush()) == 1
                got = _drain(s)
                end = counts[k] * ch
                assert got.size == end - done and np.array_equal(got, out[done:end]), (name, coalesce, k, ev[0], ev[-1], got.size, end - done)
                done = end
            assert done == out.size
            form = s.L.spx_debug_last_walk_form()
            print(name, coalesce, "form", form)
            assert form == ((132 if rate == 48000 else 68) if fast else 0), (name, coalesce, form)
        finally:
            s.close()


def _playback_want(p):
    """(the definition's final output, frames after each event) of a playback stream, once per module."""
    key = ("playback", p[0])
    if key not in _WANT:
        s, counts = T.playback_events(p[1], p[2], p[3])
        y = np.asarray(s.out, np.int64)
        assert y.min() >= -32768 and y.max() <= 32767
        y.setflags(write=False)
        _WANT[key] = (y, counts)
    return _WANT[key]


def _playback_case(p, coalesce, own, hold=False):
    """One playback stream through a fresh handle, event for event: ("rate", r) is sonicSetRate (own) / sonicIntSetRate, after which
    nothing may appear; a write or a flush is followed by reads until nothing is left, which return exactly what the definition
    produced in that event.  own: sonicSetSpeed / sonicWriteShortToStream / sonicFlushStream with the nonlinear factor 0; otherwise
    the sonicInt* calls.  hold: nothing is read before the first write or flush behind the first sonicSetRate -- the handle enters rate
    mode with everything it has produced so far unread."""
    from speedy_amd.sonic2 import SonicStream
    name, rate, ch, events = p
    out, counts = _playback_want(p)
    first_rate = [e[0] for e in events].index("rate")
    prime_the_form_counter()
    s = SonicStream(rate, ch, False, coalesce)
    try:
        s.enable_nonlinear(0.0)
        done = 0
        for k, ev in enumerate(events):
            if ev[0] == "rate":
                s.set_rate(ev[1]) if own else s.L.sonicIntSetRate(s.h, float(ev[1]))
            elif own:
                s.set_speed(ev[-1])
                assert (s.write_short(ev[1]) if ev[0] == "write" else s.flush()) == 1, (name, k)
            else:
                s.int_set_speed(ev[-1])
                assert (s.int_write_short(ev[1]) if ev[0] == "write" else s.int_flush()) == 1, (name, k)
            if hold and k <= first_rate:
                continue
            got = _drain(s)
            end = counts[k] * ch
            assert got.size == end - done and np.array_equal(got, out[done:end]), (name, coalesce, own, k, ev[0], ev[-1], got.size // ch, (end - done) // ch)
            done = end
        assert done == out.size, name
        assert s.L.spx_debug_last_walk_form() == 0, (name, coalesce, own)           # a handle with a rate: the general kernel
    finally:
        s.close()


def _both_sides_of_one(events):
    speeds = [e[-1] for e in events if e[0] != "rate"]
    return min(speeds) < 1.0 < max(speeds)


@pytest.mark.parametrize("coalesce", [True, False])
@pytest.mark.parametrize("plan", range(len(I.RATE_PLANS)))
def test_the_stream_api_with_rate_changes_through_both_lives(plan, coalesce):
    """The planted event lists under one rate plan (tests/tsm_inputs.py RATE_PLANS) against tsm_ref.PlaybackStream, call for call
    through BOTH lives: positions carried across the flush, sonicSetRate in mid-stream (to and from 1, to the value already set) with
    a frame waiting, the rate first set behind three writes.  Every list goes through the stream's own calls with the nonlinear
    factor 0; the lists with speeds on both sides of 1 go through the sonicInt* calls as well.  A handle with a rate leaves the
    pool, so `coalesce` must make no difference -- it decides only what the handle was before.

    Out of scope: a NONLINEAR second life with a rate -- the shim's partial ring buffer survives the flush, and the event list of
    such a life has no closed form in tests/tsm_ref.py."""
    streams = [p for p in I.playback_streams() if p[0].endswith("/plan%d" % plan)]
    assert len(streams) == 8
    through_int = 0
    for p in streams:
        _playback_case(p, coalesce, own=True)
        if _both_sides_of_one(p[3]):
            _playback_case(p, coalesce, own=False)
            through_int += 1
    assert through_int == 4, through_int


DIRECTED = ("one_frame_calls", "stale_return", "sixteen_channels", "unread_head", "3999Hz", "44100Hz", "96000Hz")


@pytest.mark.parametrize("coalesce", [True, False])
@pytest.mark.parametrize("name", DIRECTED)
def test_the_stream_api_on_the_directed_playback_streams(name, coalesce):
    """One frame per call (the frame that waits is all the state there is), a return from 1 with a stale frame, 16 channels, 3 999 Hz,
    44.1 kHz and 96 kHz -- through the stream's own calls and, where the speeds lie on both sides of 1, the sonicInt* calls."""
    p = [q for q in I.playback_streams() if q[0] == name][0]
    _playback_case(p, coalesce, own=True)
    if _both_sides_of_one(p[3]):
        _playback_case(p, coalesce, own=False)


@pytest.mark.parametrize("coalesce", [True, False])
def test_a_rate_first_set_behind_unread_output(coalesce):
    """enter_rate_mode's copy of the unread head: nothing is read before the call behind the first sonicSetRate, then everything
    produced so far must come out -- the speed stage's frames of the calls before the rate, unchanged, and the rate stage's behind
    them.  The directed stream and the planted lists under the plan that sets the rate before event 3."""
    streams = [p for p in I.playback_streams() if p[0] == "unread_head" or p[0].endswith("/plan1")]
    assert len(streams) == 9
    held = 0
    for p in streams:
        first = [e[0] for e in p[3]].index("rate")
        assert first == 3, p[0]
        held += int(_playback_want(p)[1][first] > 0)
        _playback_case(p, coalesce, own=True, hold=True)
    assert held == 7, held          # (the two speed-up lists have produced nothing by then: 320 frames, below maxRequired, no unity write)


def _shim_speeds(orc, x, rate, ch, speed, nl, rates, chunk):
    """The oracle shim under the same calls: the speeds its speed callback reported, per write."""
    L = orc.lib()
    spd = []
    cb = orc.TENSION_FN(lambda s, t, v: spd.append(float(np.float32(v))))
    h = L.orc_sonicCreateStream(rate, ch, 0)
    L.orc_sonicSetSpeed(h, speed); L.orc_sonicEnableNonlinearSpeedup(h, nl); L.orc_sonicSetDurationFeedbackStrength(h, 0.0)
    L.orc_sonicSpeedCallback(h, cb)
    per_write = []
    for w, pos in enumerate(range(0, x.size // ch, chunk)):
        if w in rates:
            L.orc_sonicSetRate(h, rates[w])
        seg = np.ascontiguousarray(x[pos * ch:(pos + chunk) * ch])
        before = len(spd)
        assert L.orc_sonicWriteShortToStream(h, orc.sptr(seg), seg.size // ch) == 1
        per_write.append(spd[before:])
    L.orc_sonicDestroyStream(h)
    return per_write


@pytest.mark.parametrize("coalesce", [True, False])
def test_a_nonlinear_stream_with_a_rate_and_a_rate_change(orc, coalesce):
    """One life of a nonlinear stream (syllables, 16 kHz, 3.5x) with a rate from the start and another from write 7 on.  The events
    of the definition are the shim's handoff list: buffer k (B frames) at the k-th speed that the stream's OWN speed callback
    reported, in the write that reported it; the buffers left at the flush at the last speed; the trailing partial buffer dropped.
    The speeds are asserted equal to the oracle shim's, write for write.  After every call the reads return what the definition
    produced on that call's events."""
    from speedy_amd.sonic2 import SonicStream
    name, rate, ch, x, speed, nl = [j for j in I.nonlinear_jobs() if (j[1], j[2], j[4]) == (16000, 1, 3.5)][0]
    B, chunk, rates = rate // 100, 1000, {0: 1.25, 7: 0.8}
    n = x.size // ch
    prime_the_form_counter()
    s = SonicStream(rate, ch, False, coalesce)
    spd, calls = [], []
    try:
        s.set_speed(speed); s.enable_nonlinear(nl); s.set_feedback(0.0)
        s.on_speed(lambda t, v: spd.append(float(np.float32(v))))
        for w, pos in enumerate(range(0, n, chunk)):
            if w in rates:
                s.set_rate(rates[w])
            before = len(spd)
            assert s.write_short(x[pos * ch:(pos + chunk) * ch]) == 1
            calls.append((spd[before:], _drain(s)))
        assert s.flush() == 1
        tail = _drain(s)
        assert s.L.spx_debug_last_walk_form() == 0
    finally:
        s.close()
    assert [c[0] for c in calls] == _shim_speeds(orc, x, rate, ch, speed, nl, rates, chunk)
    assert n % B != 0 and len(set(spd)) > 10 and 10 < sum(len(c[0]) for c in calls[:7]) < len(spd) - 10 and len(spd) < n // B
    p = T.PlaybackStream(rate, ch)
    k = 0
    for w, (speeds, got) in enumerate(calls):
        if w in rates:
            p.set_rate(rates[w])
        before = len(p.out)
        for sp in speeds:
            p.write(x[k * B * ch:(k + 1) * B * ch], sp)
            k += 1
        want_w = np.asarray(p.out[before:], np.int64)
        assert got.size == want_w.size and np.array_equal(got, want_w), (w, got.size, want_w.size)
    before = len(p.out)
    while k < n // B:
        p.write(x[k * B * ch:(k + 1) * B * ch], spd[-1])
        k += 1
    p.flush(spd[-1])
    want_t = np.asarray(p.out[before:], np.int64)
    print(name, "events", n // B, "frames", p.frames_out, p.census)
    assert tail.size == want_t.size and np.array_equal(tail, want_t), (tail.size, want_t.size)
    assert p.census["set_with_left"] == 1 and p.census["straddle"] >= 50 and p.frames_out > 2000, p.census


def test_seventeen_channels_with_a_rate_are_refused_and_sixteen_work_right_after():
    """SPX_RATE_MAX_CHANNELS: the write returns 0 and the error names the limit, again on the next write (nothing was half done);
    a fresh 16-channel handle then produces the definition's stream."""
    from speedy_amd.sonic2 import SonicStream
    x = I.rectangles(16000, 17, 700)
    s = SonicStream(16000, 17, False, False)
    try:
        s.enable_nonlinear(0.0)
        s.set_speed(2.0)
        s.set_rate(1.25)
        for _ in range(2):
            assert s.write_short(x) == 0
            assert b"at most 16 channels" in s.L.speedyHipLastError()
            assert s.read_short(64).size == 0
        assert s.flush() == 0 and b"at most 16 channels" in s.L.speedyHipLastError()
    finally:
        s.close()
    _playback_case([q for q in I.playback_streams() if q[0] == "sixteen_channels"][0], False, own=True)


@pytest.mark.parametrize("coalesce", [True, False])
def test_the_stream_api_with_a_rate_on_single_life_streams(coalesce):
    """sonicSetRate before the first write, linear speed changes from write to write, one flush (spx_rate.hip: the closed form with
    carried state), call for call."""
    from speedy_amd.sonic2 import SonicStream
    streams = [p for p in I.planted_streams() if not p[0].startswith("second_life")]
    assert len(streams) == 6
    for (name, rate, ch, events), playback in zip(streams, (1.25, 0.8, 3.0, 0.5, 2.0, 1.1)):
        events = events[:[e[0] for e in events].index("flush") + 1]
        key = ("stream", name, playback)
        if key not in _WANT:
            _WANT[key] = _events_def(rate, ch, events, playback)
        out, counts = _WANT[key]
        prime_the_form_counter()
        s = SonicStream(rate, ch, False, coalesce)
        try:
            s.enable_nonlinear(0.0)
            s.set_rate(playback)
            done = 0
            for k, ev in enumerate(events):
                s.set_speed(ev[-1])
                assert (s.write_short(ev[1]) if ev[0] == "write" else s.flush()) == 1
                got = _drain(s)
                end = counts[k] * ch
                assert got.size == end - done and np.array_equal(got, out[done:end]), (name, coalesce, playback, k, ev[0], ev[-1], got.size, end - done)
                done = end
            assert done == out.size
            assert s.L.spx_debug_last_walk_form() == 0, (name, coalesce)        # a handle with a rate: the general kernel
        finally:
            s.close()
