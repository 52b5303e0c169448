"""CPU: everything that turns a chosen period into int16 output -- cross-fade, copy-through and its cap, `remaining` carried across
a speed change, unity pass-through, a failed step, the flush, the whole rate stage -- against an exact integer definition
(tests/tsm_ref.py) on inputs that give it teeth (tests/tsm_inputs.py: full scale, channel-distinct).

The oracle's TSM API (orc_sonicInt*) equals the definition sample for sample after EVERY call; the oracle shim's nonlinear stream
hands the TSM stage the closed-form event list and its output is the definition's on that list; the census conditions are
requirements on the inputs, asserted from the definition alone; every switch of the definition (one mistake each) changes the
output of some directed input.  All comparisons are integer equality.

The rate stage as a stream (tsm_ref.PlaybackStream; tsm_inputs.playback_streams: sonicSetRate in mid-stream, second lives, a stale
frame, one-frame calls) has a section of its own: the oracle after every call, the census per stream, one named stream per switch,
and the one equivalent switch (no_wrap), which must change nothing.

The time map's rows (tsm_ref.nonlinear_job(...).rows: frames_out before each event's write, then the final count) have a section
too: the oracle's rows through its hand-off callback on every nonlinear job, in one piece and in pieces of 1000 frames; what the
rows reach, from the definition alone; two mutants of the row definition, each changing a named job.

SPX_TSM_CENSUS=<path> writes the census table (profiles/tsm_definition.txt), SPX_TIME_MAP_CENSUS=<path> the rows' table
(profiles/time_map_definition.txt).
"""
import os

import numpy as np
import pytest

import tsm_inputs as I
import tsm_ref as T


# ------------------------------------------------------------------ the definition, once ------------------------------------------------------------------

def _run_events(make, events):
    """A stream of the definition over an event list: (stream, frames produced after each call)."""
    s = make()
    counts = []
    for ev in events:
        if ev[0] == "write":
            s.write(ev[1], ev[2])
        else:
            s.flush(ev[1])
        counts.append(s.frames_out)
    return s, counts


def _first_life(events):
    k = [e[0] for e in events].index("flush")
    return events[:k + 1]


@pytest.fixture(scope="module")
def linear():
    """{name: the definition's stream} of every directed linear job; computed once, left unchanged."""
    return {name: T.linear_job(x, rate, ch, speed) for name, rate, ch, x, speed in I.linear_jobs()}


@pytest.fixture(scope="module")
def rated():
    return {name: T.rate_job(x, hz, ch, speed, rate) for name, hz, ch, x, speed, rate in I.rate_jobs()}


@pytest.fixture(scope="module")
def planted():
    return {name: _run_events(lambda: T.SpeedStream(rate, ch), ev) for name, rate, ch, ev in I.planted_streams()}


def _shim_stream(orc, x, rate, ch, speed, nl):
    """The oracle shim's stream in writes of 1000 frames: (output, [(speed, buffer)] of its handoff callback)."""
    L = orc.lib()
    events = []

    def on(s, t, sp, buf, frames):
        events.append((float(np.float32(sp)), np.ctypeslib.as_array(buf, shape=(frames * ch,)).copy()))
    cb = orc.HANDOFF_FN(on)
    h = L.orc_sonicCreateStream(rate, ch, 0)
    L.orc_sonicSetSpeed(h, speed); L.orc_sonicEnableNonlinearSpeedup(h, nl); L.orc_sonicSetDurationFeedbackStrength(h, 0.0)
    L.orc_sonicHandoffCallback(h, cb)
    buf, got = np.zeros((1 << 17) * ch, np.int16), []

    def drain():
        while True:
            k = L.orc_sonicReadShortFromStream(h, orc.sptr(buf), 1 << 17)
            if k <= 0:
                return
            got.append(buf[:k * ch].copy())
    n = x.size // ch
    for pos in range(0, n, 1000):
        seg = np.ascontiguousarray(x[pos * ch:(pos + 1000) * ch])
        assert L.orc_sonicWriteShortToStream(h, orc.sptr(seg), seg.size // ch) == 1
        drain()
    assert L.orc_sonicFlushStream(h) == 1
    drain()
    L.orc_sonicDestroyStream(h)
    return (np.concatenate(got) if got else np.zeros(0, np.int16)), events


@pytest.fixture(scope="module")
def nonlinear(orc):
    """{name: (shim output, handoff events, the definition's stream on those events)}"""
    out = {}
    for name, rate, ch, x, speed, nl in I.nonlinear_jobs():
        ref, events = _shim_stream(orc, x, rate, ch, speed, nl)
        s = T.nonlinear_job(x, rate, ch, [sp for sp, _ in events], speed)
        out[name] = (ref, events, s)
    return out


# ------------------------------------------------------------------ the inputs ------------------------------------------------------------------

def test_the_directed_inputs_are_full_scale_bounded_and_cover_every_speed():
    for name, rate, ch, x, speed in I.linear_jobs():
        assert x.dtype == np.int16 and x.size // ch <= 1.0 * rate, name
        if name.startswith(("channels", "rates", "speeds")):
            assert 0.3 * rate - 1 <= x.size // ch, name
            assert x.max() == 32767 and x.min() == -32768, name
    lo, hi = I.unity_neighbours()
    assert T.is_unity(lo) and not T.is_unity(hi) and np.nextafter(np.float32(lo), np.float32(2)) == np.float32(hi)
    assert T.is_unity(1.0) and not T.is_unity(1.00002) and not T.is_unity(0.99998)
    assert I.below(2.0) < 2.0 and np.float32(I.below(2.0)) == np.nextafter(np.float32(2), np.float32(0))
    for name, rate, ch, ev in I.planted_streams():
        kinds = [e[0] for e in ev]
        assert name.startswith("second_life") or sorted(set(e[-1] for e in ev)) == sorted(set(
            I.SEQUENCE if "near_unity" in name else I.SEQUENCE_UP if name.startswith("speedup") else I.SEQUENCE_FAR)), name                  # every speed of the sequence is used
        assert kinds.count("flush") == 2 and kinds[-1] == "flush" and "write" in kinds[kinds.index("flush"):], name     # a second life
        assert sum(e[1].size for e in ev if e[0] == "write") // ch <= rate, name


def test_no_two_channels_of_an_output_are_equal(linear, rated):
    """A permuted channel or a slipped e / C in a kernel cannot hide behind equal channels."""
    seen = 0
    for name, rate, ch, x, speed in I.linear_jobs():
        if ch > 1:
            y = np.asarray(linear[name].out, np.int64).reshape(-1, ch)
            assert y.shape[0] > 1000, name
            for a in range(ch):
                for b in range(a + 1, ch):
                    assert not np.array_equal(y[:, a], y[:, b]), (name, a, b)
            seen += 1
    assert seen >= 20
    for name, hz, ch, x, speed, rate in I.rate_jobs():
        if ch > 1 and x.size // ch > 100:            # (the three-frame stream lies inside every channel's first rectangle)
            y = np.asarray(rated[name].out, np.int64).reshape(-1, ch)
            for a in range(ch):
                for b in range(a + 1, ch):
                    assert not np.array_equal(y[:, a], y[:, b]), (name, a, b)


# ------------------------------------------------------------------ the oracle's TSM API ------------------------------------------------------------------

class _Int:
    """The oracle's orc_sonicInt* stream; read() drains it."""

    def __init__(self, orc, rate, ch, playback=None):
        self.orc, self.L, self.ch = orc, orc.lib(), ch
        self.h = self.L.orc_sonicIntCreateStream(rate, ch)
        assert self.h
        if playback is not None:
            self.L.orc_sonicIntSetRate(self.h, playback)
        self.buf = np.zeros((1 << 16) * ch, np.int16)

    def read(self):
        got = []
        while True:
            k = self.L.orc_sonicIntReadShortFromStream(self.h, self.orc.sptr(self.buf), 1 << 16)
            if k <= 0:
                return np.concatenate(got).astype(np.int64) if got else np.zeros(0, np.int64)
            got.append(self.buf[:k * self.ch].copy())

    def call(self, ev):
        if ev[0] == "rate":
            self.L.orc_sonicIntSetRate(self.h, ev[1])
            return self.read()
        self.L.orc_sonicIntSetSpeed(self.h, ev[-1])
        if ev[0] == "write":
            x = np.ascontiguousarray(ev[1], np.int16)
            assert self.L.orc_sonicIntWriteShortToStream(self.h, self.orc.sptr(x), x.size // self.ch) == 1
        else:
            assert self.L.orc_sonicIntFlushStream(self.h) == 1
        return self.read()

    def close(self):
        self.L.orc_sonicIntDestroyStream(self.h)


def _call_for_call(orc, rate, ch, events, out, counts, tag, playback=None):
    """The oracle stream's reads after every call equal the definition's output of that call."""
    o = _Int(orc, rate, ch, playback)
    want = np.asarray(out, np.int64)
    done = 0
    for k, ev in enumerate(events):
        got = o.call(ev)
        # (a flush may cut, but never below what the calls before it produced: expected >= out)
        end = counts[k] * ch
        assert got.size == end - done, (tag, k, ev[0], ev[-1], got.size // ch, (end - done) // ch)
        assert np.array_equal(got, want[done:end]), (tag, k, ev[0], ev[-1], int(np.nonzero(got != want[done:end])[0][0]))
        done = end
    o.close()
    assert done == want.size, tag


def test_oracle_equals_the_definition_on_every_directed_batch_job(orc, linear):
    for name, rate, ch, x, speed in I.linear_jobs():
        s = linear[name]
        _call_for_call(orc, rate, ch, [("write", x, speed), ("flush", speed)], s.out, [s.frames_after_write, s.frames_out], name)


def test_oracle_equals_the_definition_on_the_planted_event_lists(orc, planted):
    for name, rate, ch, ev in I.planted_streams():
        s, counts = planted[name]
        assert (s.steps > 15 or name.startswith("second_life") or "near_unity" in name) and counts[-1] > 0, (name, s.steps)
        _call_for_call(orc, rate, ch, ev, s.out, counts, name)


def test_oracle_equals_the_definition_on_the_rate_jobs(orc, rated):
    for name, hz, ch, x, speed, rate in I.rate_jobs():
        s = rated[name]
        _call_for_call(orc, hz, ch, [("write", x, speed), ("flush", speed)], s.out, [s.frames_after_write, s.frames_out], name, rate)


@pytest.mark.parametrize("rate", [1.25, 0.8, 3.0])
def test_oracle_equals_the_definition_on_a_planted_first_life_with_a_rate(orc, rate):
    """One life cycle of every planted event list (up to its first flush) with a playback rate, call for call."""
    for name, hz, ch, ev in I.planted_streams():
        ev = _first_life(ev)
        s, counts = _run_events(lambda: T.RateStream(hz, ch, rate), ev)
        assert counts[-1] > 1000 or name.startswith("second_life"), name
        _call_for_call(orc, hz, ch, ev, s.out, counts, (name, rate), rate)


# ------------------------------------------------------------------ the oracle shim's nonlinear stream ------------------------------------------------------------------

def test_the_shims_handoff_has_the_closed_form_shape_and_the_definition_gives_its_output(orc, nonlinear):
    """n_in // B events of B frames, x[k B : (k + 1) B], the trailing partial buffer dropped; the first K events at the K values of
    the speed tap, the later ones at the last of them (tsm_ref.event_speeds).  Every stream with an event below speed 2 has events
    that inherit a pending copy from an event of another speed."""
    for name, rate, ch, x, speed, nl in I.nonlinear_jobs():
        ref, events, s = nonlinear[name]
        B = rate // 100
        n = x.size // ch
        assert len(events) == n // B and n % B != 0, name
        for k, (_, b) in enumerate(events):
            assert np.array_equal(b, x[k * B * ch:(k + 1) * B * ch]), (name, k)
        speeds = [sp for sp, _ in events]
        assert len(set(speeds)) > 10, name
        # the speeds: the first K events carry the speed tap's K values, the later ones the last of them
        tap = orc.compress_sound(x, rate, ch, speed, nl, 0.0, False, chunk=1000, taps=True)["speed"]
        assert 10 < len(tap) < len(events), (name, len(tap), len(events))
        assert speeds == T.event_speeds(n, rate, tap, speed), name
        assert speeds[:len(tap)] == [float(v) for v in tap] and set(speeds[len(tap):]) == {float(tap[-1])}, name
        got = np.asarray(s.out, np.int64)
        assert got.size == ref.size and np.array_equal(got, ref.astype(np.int64)), name
        if min(speeds) < 2.0:          # (an event at 2 or more, or below 0.5, leaves no copy behind)
            assert s.census["inherits_copy"] >= 1, (name, s.census)
    assert sum(1 for _, ev, _ in nonlinear.values() if min(sp for sp, _ in ev) < 2.0) >= 4


# ------------------------------------------------------------------ the census ------------------------------------------------------------------

# the speeds at which a job cross-fades throughout (at 1.00002 and its like one period in 50 000 is cross-faded, the rest copied;
# at 2000 and 0.0001 every step fails; at 200 most do)
FULL_SPEEDS = tuple(s for s in I.SPEEDS if abs(s - 1.0) > 1e-3 and s not in (2000.0, 0.0001))


def _total(streams):
    t = dict.fromkeys(T.CENSUS, 0)
    for s in streams:
        for k, v in s.census.items():
            t[k] += v
    return t


def test_every_full_scale_job_has_the_delicate_numerators(linear):
    """Per full-scale job that runs cross-fades: at least 100 numerators that are negative and no multiple of n (floor and
    truncation differ there), at least 100 with |num| >= 32000 n (the last bits of a 16-bit reciprocal, the sign of a biased sample)."""
    for name, rate, ch, x, speed in I.linear_jobs():
        if name.startswith(("channels", "rates")) or (name.startswith("speeds") and speed in FULL_SPEEDS):
            c = linear[name].census
            assert c["xfade_neg_frac"] >= 100 and c["xfade_full"] >= 100, (name, c)


def test_every_census_condition_is_reached(linear, planted, rated):
    """Each count of the census is at least 1 somewhere in the directed set -- from the definition alone.

    Two conditions that are not obvious:
      * a KEPT cross-fade sample with exactly one operand in the flush padding: it survives the cut at every length of the run
        at speeds 2.0, 3.5 and 0.4, asserted below;
      * a flush that does NOT cut is reached only where a step fails: speeds 2000 and 0.0001 (every step fails) and 200 (23 steps
        run at 22.05 kHz before one fails) -- the write ends there, so the output stays short of `expected`.  No directed job
        without a failed step is uncut, asserted below over all of them.  An argument, not a proof, for why: the padded process
        call goes on while pos + maxRequired <= pending + 2 maxRequired, so it consumes all pending input and more than
        maxRequired frames of padding, and the steps on that padding usually produce more than the 0.5 frame that `expected`
        allows beyond pending / speed; it gives no bound per frame of padding (with maxRequired zeros instead of 2 maxRequired the
        output does fall short: the switch flush_pad_short, caught at lengths 678 and 679 at speed 0.7).  The mutant `flush_no_cut`
        needs no uncut flush: every job that cuts catches it."""
    lin = _total(linear.values())
    for k in ("xfade_neg_frac", "xfade_full", "pad_kept", "copy_capped", "failed_steps", "flush_cut", "flush_uncut", "flush_tie"):
        assert lin[k] >= 1, (k, lin)
    pl = _total(s for s, _ in planted.values())
    for k in ("inherits_copy", "unity_with_remaining", "copy_capped", "flush_cut"):
        assert pl[k] >= 1, (k, pl)
    for name, (s, _) in planted.items():
        if name.startswith("planted"):
            assert s.census["inherits_copy"] >= 1 and s.census["unity_with_remaining"] >= 1, (name, s.census)
        if name.startswith("speedup"):
            assert s.census["inherits_copy"] >= 1 and s.census["xfade_full"] >= 100, (name, s.census)
    rt = _total(rated.values())
    for k in ("rate_neg_frac", "halving_dropped"):
        assert rt[k] >= 1, (k, rt)
    assert rated["rate/44100Hz/2ch/13230/1.3/1.1"].census["halving_dropped"] >= 1
    for name, rate, ch, x, speed in I.linear_jobs():
        c = linear[name].census
        if name.startswith("run"):
            assert (c["pad_kept"] >= 1 or speed == 0.7) and c["flush_cut"] == 1 and c["flush_uncut"] == 0, (name, c)
        if speed in (1.3, 1.00002) and name.startswith("speeds"):
            # (at 16 kHz and 1.3 the periods this signal yields leave copies of 2.33 periods that stay below maxRequired)
            assert c["copy_capped"] >= 1 or rate == 16000 and speed == 1.3, (name, c)
        if speed in (2000.0, 0.0001):
            assert c["failed_steps"] == 2 and c["flush_uncut"] == 1, (name, c)
        assert c["flush_uncut"] == 0 or c["failed_steps"] >= 1, (name, c)           # uncut only where a step failed
    assert linear["speeds/22050Hz/1ch/7000/200"].steps > 20 and linear["speeds/22050Hz/1ch/7000/200"].census["flush_uncut"] == 1
    # the exact .5 tie of the flush count: speed 2.0 with an odd pending count -- every second length of the run
    ties = [x.size for name, rate, ch, x, speed in I.linear_jobs() if name.startswith("run") and speed == 2.0 and linear[name].census["flush_tie"]]
    assert len(ties) == len(I.RUN) // 2, ties


# ------------------------------------------------------------------ teeth ------------------------------------------------------------------

def _linear_differs(linear, names, switch):
    by = {j[0]: j for j in I.linear_jobs()}
    for name in names:
        _, rate, ch, x, speed = by[name]
        m = T.linear_job(x, rate, ch, speed, switch)
        if m.out != linear[name].out or m.frames_after_write != linear[name].frames_after_write:
            return name
    return None


def _planted_differs(planted, switch):
    for name, rate, ch, ev in I.planted_streams():
        m, counts = _run_events(lambda: T.SpeedStream(rate, ch, switch), ev)
        if m.out != planted[name][0].out or counts != planted[name][1]:
            return name
    return None


_J = "channels/22050Hz/%dch/6615/%s"
TEETH = {
    "xfade_floor": [_J % (2, "2"), _J % (1, "0.7")],
    "xfade_swapped": [_J % (2, "2"), _J % (1, "0.7")],
    "xfade_late": [_J % (2, "2"), _J % (1, "0.7")],
    "copy_uncapped": [_J % (1, "1.3"), "speeds/22050Hz/1ch/7000/1.00002"],
    "flush_floor": ["run/22050Hz/1ch/2981/2", "run/22050Hz/1ch/2981/0.4"],
    "flush_after_pad": [_J % (1, "2"), _J % (1, "0.7")],
    "flush_pad_short": ["lengths/22050Hz/1ch/678/0.7", "lengths/22050Hz/1ch/679/0.7", "run/22050Hz/1ch/3019/0.7"],
    "flush_no_cut": [_J % (1, "2"), _J % (1, "0.7")],
}


@pytest.mark.parametrize("switch", sorted(TEETH))
def test_every_speed_stage_switch_changes_a_batch_jobs_output(linear, switch):
    """Teeth: the mutant's final output (or what it had produced after the write) differs from the definition's on EVERY job
    listed for it: a kernel with that mistake cannot produce the definition's output there."""
    for name in TEETH[switch]:
        assert _linear_differs(linear, [name], switch) == name, (switch, name)


@pytest.mark.parametrize("switch", ["unity_clears_remaining", "flush_resets_prev", "copy_uncapped", "xfade_floor", "flush_floor"])
def test_the_stream_switches_change_a_planted_event_list(planted, switch):
    """A unity write that clears `remaining` and a flush that clears prevPeriod show only where a stream goes on: on the planted
    event lists (unity between two other speeds; a second life)."""
    assert _planted_differs(planted, switch) is not None, switch


def test_unity_clears_remaining_and_flush_resets_prev_cannot_show_in_a_linear_job(linear):
    """One write at one speed, one flush: a unity job never has a `remaining`, and nothing follows the flush.  These two switches
    are equivalent to the definition on every linear batch job -- they are pinned by the stream API alone."""
    names = [j[0] for j in I.linear_jobs() if j[0].startswith(("speeds", "lengths", "rates"))]
    assert _linear_differs(linear, names, "unity_clears_remaining") is None
    assert _linear_differs(linear, names, "flush_resets_prev") is None


@pytest.mark.parametrize("switch", T.CLOSED_FORM_SWITCHES)
def test_every_rate_stage_switch_changes_a_rate_jobs_output(rated, switch):
    caught = []
    for name, hz, ch, x, speed, rate in I.rate_jobs():
        m = T.rate_job(x, hz, ch, speed, rate, switch)
        if m.out != rated[name].out or m.frames_after_write != rated[name].frames_after_write:
            caught.append(name)
    assert caught, switch
    if switch == "rate_no_halving":          # shows exactly where halving dropped a bit
        assert "rate/44100Hz/2ch/13230/1.3/1.1" in caught
        assert all(rated[n].census["halving_dropped"] for n in caught), caught


def test_every_switch_has_a_test():
    covered = set(TEETH) | {"unity_clears_remaining", "flush_resets_prev"} | set(T.CLOSED_FORM_SWITCHES) | set(PLAYBACK_TEETH) | {"no_wrap"}
    assert covered == set(T.SWITCHES)


# ------------------------------------------------------------------ the rate stage as a stream ------------------------------------------------------------------

@pytest.fixture(scope="module")
def playback():
    """{name: (the definition's PlaybackStream, frames after each event)} of every playback stream; computed once, left unchanged."""
    return {name: T.playback_events(hz, ch, ev) for name, hz, ch, ev in I.playback_streams()}


N_PLAYBACK = 8 * 4 + 7          # the eight planted lists under the four rate plans, seven directed cases


def test_the_playback_streams_are_the_planted_lists_under_every_plan_and_the_directed_cases():
    streams = I.playback_streams()
    assert len(streams) == N_PLAYBACK == len(I.planted_streams()) * len(I.RATE_PLANS) + 7
    assert len({s[0] for s in streams}) == N_PLAYBACK
    for (name, hz, ch, ev), k in zip(streams, range(len(I.planted_streams()) * len(I.RATE_PLANS))):
        pname, phz, pch, pev = I.planted_streams()[k // len(I.RATE_PLANS)]
        plan = I.RATE_PLANS[k % len(I.RATE_PLANS)]
        assert name == "%s/plan%d" % (pname, k % len(I.RATE_PLANS)) and (hz, ch) == (phz, pch)
        assert [e for e in ev if e[0] != "rate"] == pev, name                                   # the planted events, in order
        rates = [e[1] for e in ev if e[0] == "rate"]
        assert rates == [float(plan[i]) for i in sorted(plan) if i < len(pev)] and rates, name
        assert len(rates) == len(plan) or pname != "planted22k", name    # (shorter lists: the later indices plant nothing)
    for name, hz, ch, ev in streams:
        kinds = [e[0] for e in ev]
        assert kinds.count("flush") == 2 and kinds[-1] == "flush" and "rate" in kinds, name
        assert sum(e[1].size for e in ev if e[0] == "write") // ch <= 30000, name
    by = {s[0]: s for s in streams}
    assert by["sixteen_channels"][2] == 16 and {by[n][1] for n in ("3999Hz", "44100Hz", "96000Hz")} == {3999, 44100, 96000}
    ev = by["one_frame_calls"][3]
    assert ev[0] == ("rate", 0.8) and [e[1].size // 2 for e in ev[1:41]] == [1] * 40 and all(e[2] == 1.0 for e in ev[1:41])
    ev = by["unread_head"][3]
    assert [e[0] for e in ev[:4]] == ["write", "write", "write", "rate"]


def test_the_playback_stream_with_one_life_is_the_closed_form(rated):
    """The rate set before the first write, one write, one flush: the sequential definition equals rate_stage's closed form on every
    directed rate job, after the write and after the flush."""
    for name, hz, ch, x, speed, rate in I.rate_jobs():
        s, counts = T.playback_events(hz, ch, [("rate", rate), ("write", x, speed), ("flush", speed)])
        assert counts[1:] == [rated[name].frames_after_write, rated[name].frames_out] and s.out == rated[name].out, name
        assert s.census["rate_neg_frac"] == rated[name].census["rate_neg_frac"], name


def test_oracle_equals_the_definition_on_every_playback_stream(orc, playback):
    """orc_sonicInt* after EVERY call -- orc_sonicIntSetRate included, after which nothing may appear -- in count and samples."""
    seen = 0
    for name, hz, ch, ev in I.playback_streams():
        s, counts = playback[name]
        assert counts[-1] > 0, name
        _call_for_call(orc, hz, ch, ev, s.out, counts, name)
        seen += 1
    assert seen == N_PLAYBACK


def test_the_shims_nonlinear_stream_with_a_rate_is_the_definition_on_its_handoff_list(orc):
    """One nonlinear life (syllables, 16 kHz, 3.5x) with a rate from the start and another from write 7 on: after every write the
    shim's reads are what PlaybackStream produces on the buffers handed over in that write (B frames each, at the speed handed with
    them), sonicSetRate falling between the same two events; at the flush the remaining whole buffers at the last speed."""
    L = orc.lib()
    name, rate, ch, x, speed, nl = [j for j in I.nonlinear_jobs() if (j[1], j[2], j[4]) == (16000, 1, 3.5)][0]
    B, rates, n = rate // 100, {0: 1.25, 7: 0.8}, x.size // ch
    handed = []
    cb = orc.HANDOFF_FN(lambda s, t, sp, buf, frames: handed.append((float(np.float32(sp)), np.ctypeslib.as_array(buf, shape=(frames * ch,)).copy())))
    h = L.orc_sonicCreateStream(rate, ch, 0)
    L.orc_sonicSetSpeed(h, speed); L.orc_sonicEnableNonlinearSpeedup(h, nl); L.orc_sonicSetDurationFeedbackStrength(h, 0.0)
    L.orc_sonicHandoffCallback(h, cb)
    buf = np.zeros((1 << 16) * ch, np.int16)

    def drain():
        got = []
        while True:
            k = L.orc_sonicReadShortFromStream(h, orc.sptr(buf), 1 << 16)
            if k <= 0:
                return np.concatenate(got).astype(np.int64) if got else np.zeros(0, np.int64)
            got.append(buf[:k * ch].copy())
    p = T.PlaybackStream(rate, ch)
    for w, pos in enumerate(list(range(0, n, 1000)) + [None]):
        if w in rates:
            L.orc_sonicSetRate(h, rates[w])
            p.set_rate(rates[w])
        before_ev, before_out = len(handed), len(p.out)
        if pos is None:
            assert L.orc_sonicFlushStream(h) == 1
        else:
            seg = np.ascontiguousarray(x[pos * ch:(pos + 1000) * ch])
            assert L.orc_sonicWriteShortToStream(h, orc.sptr(seg), seg.size // ch) == 1
        for sp, b in handed[before_ev:]:
            p.write(b, sp)
        if pos is None:
            p.flush(handed[-1][0])
        got, want = drain(), np.asarray(p.out[before_out:], np.int64)
        assert got.size == want.size and np.array_equal(got, want), (w, got.size, want.size)
    L.orc_sonicDestroyStream(h)
    assert len(handed) == n // B and all(np.array_equal(b, x[k * B * ch:(k + 1) * B * ch]) for k, (_, b) in enumerate(handed))
    assert p.census["set_with_left"] == 1 and p.census["straddle"] >= 50 and p.frames_out > 2000, p.census


# What each stream reaches, counted by the definition alone: (wraps, set_with_left, bypass_flush_with_left, stale_used,
# life_starts_off_zero, short_calls).  Wraps: 22.05 kHz needs the rates 3.0 and 1.1 (old = 11 025 input frames in one life), 48 kHz
# wraps at old = 12 000, 3 999 Hz at 3 999.
REACHES = {
    "planted22k/plan0": (0, 4, 0, 1, 1, 0), "planted22k/plan1": (0, 1, 1, 0, 0, 0),
    "planted22k/plan2": (1, 1, 1, 0, 1, 0), "planted22k/plan3": (1, 0, 0, 0, 1, 0),
    "planted16k_stereo/plan0": (0, 3, 1, 0, 0, 0), "planted16k_stereo/plan1": (0, 1, 1, 0, 0, 0),
    "planted16k_stereo/plan2": (0, 1, 1, 0, 1, 0), "planted16k_stereo/plan3": (0, 0, 0, 0, 1, 0),
    "planted16k_near_unity/plan0": (0, 1, 0, 0, 1, 0), "planted16k_near_unity/plan1": (0, 1, 1, 0, 0, 0),
    "planted16k_near_unity/plan2": (0, 0, 0, 0, 1, 0), "planted16k_near_unity/plan3": (0, 0, 0, 0, 1, 0),
    "planted48k/plan0": (0, 2, 0, 0, 0, 0), "planted48k/plan1": (1, 1, 1, 0, 0, 0),
    "planted48k/plan2": (2, 1, 1, 0, 1, 0), "planted48k/plan3": (2, 0, 0, 0, 1, 0),
    "speedup22k/plan0": (0, 3, 1, 0, 0, 0), "speedup22k/plan1": (0, 1, 1, 0, 0, 0),
    "speedup22k/plan2": (0, 1, 1, 0, 1, 0), "speedup22k/plan3": (1, 0, 0, 0, 1, 0),
    "speedup48k_stereo/plan0": (0, 2, 0, 0, 1, 0), "speedup48k_stereo/plan1": (1, 1, 1, 0, 0, 0),
    "speedup48k_stereo/plan2": (1, 0, 0, 0, 1, 0), "speedup48k_stereo/plan3": (1, 0, 0, 0, 1, 0),
    "second_life_hum22k/plan0": (0, 0, 0, 0, 1, 0), "second_life_hum22k/plan1": (0, 0, 0, 0, 0, 0),
    "second_life_hum22k/plan2": (0, 0, 0, 0, 1, 0), "second_life_hum22k/plan3": (0, 0, 0, 0, 1, 0),
    "second_life_hum16k/plan0": (0, 0, 0, 0, 1, 0), "second_life_hum16k/plan1": (0, 0, 0, 0, 0, 0),
    "second_life_hum16k/plan2": (0, 0, 0, 0, 1, 0), "second_life_hum16k/plan3": (0, 0, 0, 0, 1, 0),
    "one_frame_calls": (0, 0, 0, 0, 1, 2), "stale_return": (0, 4, 1, 1, 0, 0), "sixteen_channels": (0, 1, 0, 0, 1, 0),
    "unread_head": (0, 0, 0, 0, 1, 0), "3999Hz": (1, 1, 0, 0, 1, 0), "44100Hz": (1, 1, 0, 0, 1, 0), "96000Hz": (1, 0, 0, 0, 0, 0),
}


def test_what_every_playback_stream_reaches(playback):
    """Requirements on the INPUTS, from the definition alone.  Per stream the six structural counts, exactly; then what the directed
    cases are for."""
    keys = ("wraps", "set_with_left", "bypass_flush_with_left", "stale_used", "life_starts_off_zero", "short_calls")
    assert set(REACHES) == set(playback) and len(playback) == N_PLAYBACK
    for name, (s, _) in playback.items():
        assert s.census.keys() == dict.fromkeys(T.PLAYBACK_CENSUS).keys(), name
        assert tuple(s.census[k] for k in keys) == REACHES[name], (name, s.census)
    for k in T.PLAYBACK_CENSUS:                                                   # every count is reached somewhere
        assert sum(s.census[k] for s, _ in playback.values()) >= 1, k
    c = {name: s.census for name, (s, _) in playback.items()}
    # one frame per call: the first call of each life only sets the waiting frame; every output of a write has operands from two
    # calls (the flush's padded call, 2 maxRequired zero frames at once, emits the rest)
    s, counts = playback["one_frame_calls"]
    ev = {p[0]: p[3] for p in I.playback_streams()}["one_frame_calls"]
    writes = [k for k, e in enumerate(ev) if e[0] == "write"]
    assert c["one_frame_calls"]["short_calls"] == 2 and counts[writes[0]] == 0
    assert c["one_frame_calls"]["straddle"] >= sum(counts[k] - counts[k - 1] for k in writes[1:]) >= 55
    assert c["stale_return"]["stale_used"] == 1 and c["planted22k/plan0"]["stale_used"] == 1
    assert c["stale_return"]["bypass_flush_with_left"] == 1
    assert c["sixteen_channels"]["rate_neg_frac"] >= 1000 and c["sixteen_channels"]["straddle"] >= 2
    assert c["44100Hz"]["halving_dropped"] >= 1 and c["96000Hz"]["halving_dropped"] == 0 and c["96000Hz"]["wraps"] == 1
    assert c["planted48k/plan1"]["halving_dropped"] == 0          # (48 000 / 0.5, / 2.0: even all the way down)
    assert c["planted22k/plan3"]["halving_dropped"] >= 1          # 22 050 / 1.1 = 20 045: the halving drops a bit of `new`
    for name in playback:
        if name.startswith(("planted", "speedup")):
            assert c[name]["straddle"] >= 1, name
    # no two channels of the 16-channel output are equal
    y = np.asarray(playback["sixteen_channels"][0].out, np.int64).reshape(-1, 16)
    assert y.shape[0] > 5000 and len({y[:, a].tobytes() for a in range(16)}) == 16


# The stream that each switch is shown on (the others it changes: profiles/tsm_definition.txt)
PLAYBACK_TEETH = {
    "flush_resets_positions": "planted22k/plan3",          # the second life starts at positions != 0 and no sonicSetRate follows
    "flush_keeps_left": "unread_head",
    "set_rate_keeps_positions": "planted22k/plan0",
    "set_rate_drops_left": "stale_return",
    "same_rate_is_noop": "planted22k/plan0",               # 1.5 set again at event 27
    "unity_rate_drops_left": "stale_return",
    "flush_count_without_left": "one_frame_calls",
    "straddle_uses_new_left": "one_frame_calls",
}


def _playback_caught(playback, switch):
    """The streams whose output, or whose count after some event, the switch changes; every stream is visited."""
    caught, seen = [], 0
    for name, hz, ch, ev in I.playback_streams():
        m, counts = T.playback_events(hz, ch, ev, switch)
        if m.out != playback[name][0].out or counts != playback[name][1]:
            caught.append(name)
        seen += 1
    assert seen == N_PLAYBACK
    return caught


@pytest.mark.parametrize("switch", sorted(PLAYBACK_TEETH))
def test_every_playback_switch_changes_a_named_stream(playback, switch):
    assert PLAYBACK_TEETH[switch] in _playback_caught(playback, switch), switch


def test_no_wrap_is_equivalent_and_changes_nothing(playback):
    """In unbounded integers (o, k) and (o + old, k + new) give the same loop test (o + 1) new > k old and the same ratio
    (o + 1) new - k old, and k == new whenever o reaches old: a stage that never returns to 0 computes the same stream.  (In 32-bit
    arithmetic it would overflow after 2^31 / 2^14 input frames: the return to 0 is what keeps the products small.)  Shown on streams
    that do wrap."""
    assert len(set(PLAYBACK_TEETH) | {"no_wrap"}) == len(T.PLAYBACK_SWITCHES) == 9 and set(PLAYBACK_TEETH) | {"no_wrap"} == set(T.PLAYBACK_SWITCHES)
    assert sum(1 for s, _ in playback.values() if s.census["wraps"]) >= 10
    assert _playback_caught(playback, "no_wrap") == []


# ------------------------------------------------------------------ the time map's rows ------------------------------------------------------------------

@pytest.fixture(scope="module")
def mapped(orc, nonlinear):
    """{name: (job, event speeds from the oracle's speed tap, the definition's stream with its rows)} of every nonlinear job: the
    six above (their streams are the `nonlinear` fixture's) and tsm_inputs.nonlinear_map_jobs()."""
    out = {}
    for job in I.nonlinear_jobs() + I.nonlinear_map_jobs():
        name, rate, ch, x, speed, nl = job
        tap = orc.compress_sound(x, rate, ch, speed, nl, 0.0, False, chunk=1000, taps=True)["speed"]
        speeds = T.event_speeds(x.size // ch, rate, tap, speed)
        if name in nonlinear:
            s = nonlinear[name][2]
            assert speeds == [sp for sp, _ in nonlinear[name][1]], name
        else:
            s = T.nonlinear_job(x, rate, ch, speeds, speed)
        out[name] = (job, speeds, s)
    return out


def _census_of_rows(rows, B):
    """What a job's rows reach: the longest run of equal rows that does not start at row 0, whether the two rows directly before
    the last are equal, the largest rise between consecutive rows, and M[0] = M[1] = 0."""
    best = start = 0                    # maximal runs by the index they start at; the run that starts at row 0 does not count
    for k in range(1, len(rows) + 1):
        if k == len(rows) or rows[k] != rows[start]:
            if start > 0:
                best = max(best, k - start)
            start = k
    return dict(flat_run=best, flat_before_last=len(rows) >= 3 and rows[-3] == rows[-2],
                largest_rise=max([b - a for a, b in zip(rows, rows[1:])] or [0]), starts_flat=len(rows) >= 2 and rows[0] == rows[1] == 0)


MAP_JOB = "map/%dHz/%dch/%d/%g/%g"


def test_the_map_jobs_are_the_shapes_the_rows_are_defined_on():
    by = {j[0]: j for j in I.nonlinear_map_jobs()}
    assert len(by) == len(I.nonlinear_map_jobs()) == 9 and not set(by) & {j[0] for j in I.nonlinear_jobs()}
    shape = {name: (rate // 100, x.size // ch) for name, rate, ch, x, speed, nl in by.values()}
    for name, rate, ch, x, speed, nl in by.values():
        assert x.dtype == np.int16 and x.size // ch <= 1.5 * rate and nl != 0, name
    B, n = shape[MAP_JOB % (16000, 1, 8000, 3.5, 1)]
    assert n % B == 0 and n // B == 50                                         # n_in = R B exactly
    B, n = shape[MAP_JOB % (16000, 1, 6559, 1.2, 1)]
    assert n % B == B - 1                                                      # n_in = R B + B - 1
    B, n = shape[MAP_JOB % (16000, 1, 200, 3.5, 1)]
    assert B <= n < 2 * B                                                      # R = 1
    B, n = shape[MAP_JOB % (16000, 1, 100, 3.5, 1)]
    assert n < B                                                               # no complete buffer
    assert {j[2] for j in by.values()} >= {1, 3, 8} and {j[1] for j in by.values()} == {11025, 16000, 48000}
    assert by[MAP_JOB % (16000, 1, 9000, 0.5, 1)][4] == 0.5


@pytest.mark.parametrize("chunk", [None, 1000], ids=["one piece", "chunks of 1000"])
def test_the_definitions_rows_are_the_oracles(orc, mapped, chunk):
    """frames_out immediately before each event's write, then the final count behind the flush -- the header's text, stated over
    tests/tsm_ref.py's stream -- equals what the oracle stream reports through its hand-off callback (tests/time_map_ref.py), for
    every nonlinear job, written in one piece and in pieces of 1000 frames; the output too."""
    import time_map_ref as tm
    assert len(mapped) == 15
    for name, (job, speeds, s) in mapped.items():
        _, rate, ch, x, speed, nl = job
        B, n = rate // 100, x.size // ch
        rows, times, out = tm.oracle_map(orc, x, rate, ch, speed, nl, False, 0.0, chunk=chunk)
        assert len(s.rows) == n // B + 1 == tm.map_rows(B, n, nl), name
        assert s.rows == rows.tolist(), (name, [k for k, (a, b) in enumerate(zip(s.rows, rows.tolist())) if a != b][:4])
        assert s.rows[-1] == s.frames_out and np.array_equal(np.asarray(s.out, np.int64), out.astype(np.int64)), name
        assert all(a <= b for a, b in zip(s.rows, s.rows[1:])) and (n < B or s.rows[0] == 0), name
        if B <= n < 2 * B:                 # R = 1: no analysis frame, the event runs at the job's speed
            assert speeds == [float(np.float32(speed))], name


def test_linear_jobs_have_the_final_count_alone(linear):
    for name, rate, ch, x, speed in I.linear_jobs():
        assert linear[name].rows == [linear[name].frames_out] == T.linear_rows(linear[name]), name


# What the rows reach, from the definition alone: the job each condition is asserted on (all jobs: profiles/time_map_definition.txt)
ROWS_REACH = {
    "flat_run": MAP_JOB % (16000, 1, 8000, 3.5, 1),             # 3 or more equal rows, not from row 0
    "flat_before_last": MAP_JOB % (16000, 1, 6559, 1.2, 1),     # two equal rows directly before the last row
    "rise_above_B": MAP_JOB % (16000, 1, 9000, 0.5, 1),         # a segment that rises by more than B
    "starts_flat": MAP_JOB % (16000, 1, 6559, 1.2, 1),          # M[0] = 0 with M[1] = 0
}


def test_what_the_rows_reach(mapped):
    c = {name: _census_of_rows(s.rows, job[1] // 100) for name, (job, _, s) in mapped.items()}
    assert c[ROWS_REACH["flat_run"]]["flat_run"] >= 3, c[ROWS_REACH["flat_run"]]
    assert c[ROWS_REACH["flat_before_last"]]["flat_before_last"], mapped[ROWS_REACH["flat_before_last"]][2].rows[-4:]
    assert mapped[ROWS_REACH["flat_before_last"]][2].rows[-2] > 0          # (not the zeros the rows begin with)
    assert c[ROWS_REACH["rise_above_B"]]["largest_rise"] > 160, c[ROWS_REACH["rise_above_B"]]
    assert c[ROWS_REACH["starts_flat"]]["starts_flat"], mapped[ROWS_REACH["starts_flat"]][2].rows[:3]


ROW_TEETH = {"row_after_write": MAP_JOB % (16000, 1, 8000, 3.5, 1), "row_before_cut": MAP_JOB % (16000, 1, 8000, 3.5, 1)}


@pytest.mark.parametrize("switch", T.ROW_SWITCHES)
def test_every_row_mutant_changes_a_named_jobs_rows(mapped, switch):
    """Teeth: a count taken behind the event's write instead of before it, and a last row taken before the flush's cut, each
    change the rows of the job named -- a kernel with that mistake cannot write the definition's rows there."""
    assert set(ROW_TEETH) == set(T.ROW_SWITCHES)
    job, speeds, s = mapped[ROW_TEETH[switch]]
    _, rate, ch, x, speed, nl = job
    m = T.nonlinear_job(x, rate, ch, speeds, speed, row_switch=switch)
    assert m.rows != s.rows and len(m.rows) == len(s.rows), switch
    if switch == "row_before_cut":
        assert m.rows[:-1] == s.rows[:-1] and m.rows[-1] > s.rows[-1]
    else:
        assert m.rows[:-2] == s.rows[1:-1] and m.rows[-1] == s.rows[-1]        # every row but the last moves up by one event


def _rows_caught(mapped, switch):
    caught = []
    for name, (job, speeds, s) in mapped.items():
        _, rate, ch, x, speed, nl = job
        if T.nonlinear_job(x, rate, ch, speeds, speed, row_switch=switch).rows != s.rows:
            caught.append(name)
    return caught


def test_time_map_table(mapped):
    """The rows' census per job and what each mutant changes; written to SPX_TIME_MAP_CENSUS when that is set
    (profiles/time_map_definition.txt; lines that start with # -- the legend and the device's figures, noted by hand -- stay, in
    front of the table)."""
    path = os.environ.get("SPX_TIME_MAP_CENSUS")
    rows = []
    for name, (job, _, s) in mapped.items():
        B, n = job[1] // 100, job[3].size // job[2]
        c = _census_of_rows(s.rows, B)
        R = n // B
        rows.append((name, R, (n - (R - 1) * B) if R >= 1 else n, s.frames_out, c))
    assert len(rows) == 15
    if path:
        notes = [ln for ln in open(path)] if os.path.exists(path) else []
        with open(path, "w") as f:
            f.writelines(ln for ln in notes if ln.startswith("#"))      # the legend and the device's figures first
            f.write("\n%-36s %4s %5s %5s %7s %9s %16s %8s %11s\n" % ("job", "B", "R", "last", "frames", "flat_run", "flat_before_last", "max_rise", "starts_flat"))
            for name, R, last, frames, c in rows:
                f.write("%-36s %4d %5d %5d %7d %9d %16d %8d %11d\n" % (name, mapped[name][0][1] // 100, R, last, frames, c["flat_run"],
                                                                    c["flat_before_last"], c["largest_rise"], c["starts_flat"]))
            f.write("\n")
            for sw in T.ROW_SWITCHES:
                caught = _rows_caught(mapped, sw)
                f.write("%-16s changes %2d of %d (asserted on %s): %s\n" % (sw, len(caught), len(mapped), ROW_TEETH[sw], " ".join(caught)))


# ------------------------------------------------------------------ the table ------------------------------------------------------------------

def test_census_table(linear, planted, rated, nonlinear, playback):
    """The census of every directed input; written to SPX_TSM_CENSUS when that is set (profiles/tsm_definition.txt).  The playback
    streams follow in a table of their own (PLAYBACK_CENSUS), then the streams that each PlaybackStream switch changes."""
    rows = []
    for name, rate, ch, x, speed in I.linear_jobs():
        if not name.startswith("run"):
            rows.append((name, linear[name].frames_out, linear[name].steps, linear[name].census))
    for sp in I.RUN_SPEEDS:
        ss = [linear[j[0]] for j in I.linear_jobs() if j[0].startswith("run") and j[4] == sp]
        rows.append(("run/22050Hz/1ch/%d..%d/%g (sum of %d)" % (I.RUN[0], I.RUN[-1], sp, len(ss)), sum(s.frames_out for s in ss),
                     sum(s.steps for s in ss), _total(ss)))
    for name, (s, _) in planted.items():
        rows.append((name, s.frames_out, s.steps, s.census))
    for name, (_, _, s) in nonlinear.items():
        rows.append((name, s.frames_out, s.steps, s.census))
    for name, s in rated.items():
        rows.append((name, s.frames_out, s.speed_stage.steps, s.census))
    assert all(r[3].keys() == dict.fromkeys(T.CENSUS).keys() for r in rows)
    path = os.environ.get("SPX_TSM_CENSUS")
    if path:
        short = ("neg_frac", "full", "pad_kept", "capped", "inherit", "unity_rem", "failed", "cut", "uncut", "tie", "r_neg_frac", "halv_drop")
        notes = [ln for ln in open(path)] if os.path.exists(path) else []
        with open(path, "w") as f:
            f.write("%-44s %7s %5s " % ("input", "frames", "steps") + " ".join("%10s" % k for k in short) + "\n")
            for name, frames, steps, c in rows:
                f.write("%-44s %7d %5d " % (name, frames, steps) + " ".join("%10d" % c[k] for k in T.CENSUS) + "\n")
            pshort = ("wraps", "set_left", "byp_flush", "stale", "off_zero", "short", "straddle", "r_neg_frac", "halv_drop")
            f.write("\n%-44s %7s %5s " % ("playback stream", "frames", "steps") + " ".join("%10s" % k for k in pshort) + "\n")
            for name, (s, _) in playback.items():
                f.write("%-44s %7d %5d " % (name, s.frames_out, s.speed_stage.steps) + " ".join("%10d" % s.census[k] for k in T.PLAYBACK_CENSUS) + "\n")
            f.write("\n")
            for sw in T.PLAYBACK_SWITCHES:
                caught = _playback_caught(playback, sw)
                f.write("%-26s changes %2d of %d: %s\n" % (sw, len(caught), len(playback), " ".join(caught) if caught else "none (equivalent)"))
            f.writelines(ln for ln in notes if ln.startswith("#"))      # (the GPU file's wall time, noted by hand, stays)
