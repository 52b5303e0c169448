"""The time-scale modification behind the pitch decision as exact integers -- test infrastructure, CPU only.

Written from the algorithm's text (the anchors in oracle/orc_sonic.h; soniclib.c:354-371, 397-399, 529-552
for the order of events), not from the kernels and not from oracle/orc_sonic.c: what turns a chosen period into int16 output.
The decision itself is tests/pitch_ref.py's (find_pitch_period, step_lengths) and is not restated here.  Every sample and every
position is a Python integer.  The only floating point is float32, evaluated as written: the step lengths (pitch_ref), the two
flush counts and newSampleRate.

SpeedStream -- the speed stage as a stream: write(frames, speed), flush(speed), `out` (everything produced so far).  It fixes
  * unity: !(speed > 1.00001 || speed < 0.99999), asked in double of the float32 value; a unity write moves all pending input to
    the output and leaves `remaining` as it is;
  * no step below maxRequired pending frames; the loop's exit test pos + maxRequired <= n; copy-through in pieces of at most
    maxRequired;
  * the cross-fade (down[t] (n - t) + up[t] t) / n per channel, truncated toward zero; speed-up: down = the period at the position,
    up = the period behind it; slow-down: the period is copied through first and the ramps are exchanged;
  * a failed step (n == 0) ends the write and consumes nothing (the slow-down step has emitted its period by then);
  * the flush: expected = out + (int)(pending / speed + 0.5f) BEFORE the padding, 2 maxRequired zero frames, one process call, the
    output cut to `expected` only if it is longer, input and `remaining` cleared, prevPeriod and prevMinDiff kept.

linear_job / nonlinear_job -- what a batch job is in terms of that stream.  The event speeds of a nonlinear job are DATA here
(pinned by tests/features_ref.py and the bit-exact taps).  Both record `rows`, the job's TIME MAP as include/speedy_hip.h words it:
frames_out immediately before each event's write, then the final count behind the flush; a linear job, or a nonlinear one without
a complete buffer, has the final count alone.  ROW_SWITCHES are the two mistakes a kernel could make there.

rate_stage / rate_job -- the rate stage (sonicSetRate) of ONE life cycle -- the rate set before the first write, one flush -- in
closed form over the speed stage's uncut output.

PlaybackStream -- the rate stage as a stream, the sequential form of the same text (the dependency's adjustRate, interpolate,
sonicSetRate and sonicFlushStream; anchors in oracle/orc_sonic.h): set_rate(r) at any time, any number of lives.  It fixes
  * set_rate: the rate is stored and both positions return to 0, always -- also for the value already set; waiting frames stay;
  * after each process call the frames that call appended: at rate 1 straight to the output, positions and pitch buffer untouched
    (a frame waiting there goes stale); otherwise appended to the pitch buffer and, for pos in 0 .. M - 2: while (o + 1) new > k old
    emit (ratio p[pos] + (new - ratio) p[pos + 1]) / new per channel, truncated toward zero, ratio = (o + 1) new - k old, k += 1;
    then o += 1, and at o == old both positions return to 0; the consumed frames leave the buffer, one stays;
  * the flush: expected = out + (int)((pending / speed + waiting) / rate + 0.5f) in float32 BEFORE the padding, `waiting` the pitch
    buffer's frame count, a stale frame included; the padded call; the output cut to `expected` if it is longer; the pitch buffer
    emptied; the positions KEPT.
PINNED by it, on the CPU against the oracle and on the device against the drop-in API: second lives with a rate, rate changes in
the middle of a stream (to and from 1, to the value already set), a rate first set behind unread output, one-frame calls.  What
REMAINS outside: a NONLINEAR second life with a rate (the shim's partial ring buffer survives the flush; the event list of such a
life has no closed form here), and pitch / volume / chord pitch, which the project does not implement.

The switches make one mistake each (SWITCHES); the tests use them to show that the directed inputs have teeth:
  xfade_floor   floor for truncation          copy_uncapped           one piece of `remaining`
  xfade_swapped ramps exchanged               unity_clears_remaining  a unity write clears `remaining`
  xfade_late    weights (n - t - 1, t + 1)    flush_floor             no + 0.5
  flush_after_pad  `expected` from the padded input       flush_pad_short   maxRequired zeros
  flush_no_cut     the output is not cut                  flush_resets_prev the flush clears prevPeriod
  rate_floor    floor for truncation          rate_swapped      weights exchanged
  rate_no_halving  the rates are not halved   rate_keeps_last   emits while t <= M - 1, repeating the last frame
  rate_flush_floor no + 0.5 in the rate stage's flush count
and PlaybackStream's (PLAYBACK_SWITCHES):
  flush_resets_positions   the flush zeroes o and k        flush_keeps_left         the flush keeps the waiting frame
  set_rate_keeps_positions set_rate leaves o and k         set_rate_drops_left      set_rate empties the pitch buffer
  same_rate_is_noop        set_rate(the value set) does nothing                     unity_rate_drops_left    a call at rate 1 empties it
  flush_count_without_left `expected` without `waiting`    straddle_uses_new_left   a frame that straddles two calls takes its left
  no_wrap                  the positions never return to 0 at o == old              operand from the new call's first frame
no_wrap is EQUIVALENT in unbounded integers: (o, k) and (o + old, k + new) give the same loop test and the same ratio.
"""
import numpy as np

import pitch_ref as R

SPEED_SWITCHES = ("xfade_floor", "xfade_swapped", "xfade_late", "copy_uncapped", "unity_clears_remaining", "flush_floor",
                  "flush_after_pad", "flush_pad_short", "flush_no_cut", "flush_resets_prev")
CLOSED_FORM_SWITCHES = ("rate_floor", "rate_swapped", "rate_no_halving", "rate_keeps_last", "rate_flush_floor")     # rate_stage / RateStream
PLAYBACK_SWITCHES = ("flush_resets_positions", "flush_keeps_left", "set_rate_keeps_positions", "set_rate_drops_left", "same_rate_is_noop",
                     "unity_rate_drops_left", "flush_count_without_left", "straddle_uses_new_left", "no_wrap")           # PlaybackStream
RATE_SWITCHES = CLOSED_FORM_SWITCHES + PLAYBACK_SWITCHES
SWITCHES = SPEED_SWITCHES + RATE_SWITCHES

CENSUS = ("xfade_neg_frac", "xfade_full", "pad_kept", "copy_capped", "inherits_copy", "unity_with_remaining", "failed_steps",
          "flush_cut", "flush_uncut", "flush_tie", "rate_neg_frac", "halving_dropped")
# PlaybackStream's own counts.  halving_dropped: process calls at a rate != 1 whose (new, old) lost a bit to the halving
PLAYBACK_CENSUS = ("wraps", "set_with_left", "bypass_flush_with_left", "stale_used", "life_starts_off_zero", "short_calls", "straddle",
                   "rate_neg_frac", "halving_dropped")

_F = np.float32


def tdiv(a, b):
    """a / b truncated toward zero (b > 0)."""
    q = abs(a) // b
    return -q if a < 0 else q


def is_unity(speed):
    s = float(_F(speed))
    return not (s > 1.00001 or s < 0.99999)


class SpeedStream:
    def __init__(self, rate, channels, switch=None):
        assert switch is None or switch in SWITCHES, switch
        self.rate, self.C, self.switch = rate, channels, switch
        self.max_required = R.limits(rate)[2]
        self.inp, self.out = [], []            # interleaved Python integers
        self.remaining = 0
        self.prev_period = self.prev_min_diff = 0
        self.census = dict.fromkeys(CENSUS, 0)
        self.steps = 0
        self._remaining_speed = None           # the float32 speed of the step that left `remaining`
        self._pad_from = None                  # inside the flush: the first padding frame of the input
        self._pad_marks = []                   # output indices of cross-fade samples with exactly one operand in the padding

    @property
    def frames_out(self):
        return len(self.out) // self.C

    @property
    def pending(self):
        return len(self.inp) // self.C

    def _xfade(self, n, down, up):
        C, x, out, cen, sw = self.C, self.inp, self.out, self.census, self.switch
        if sw == "xfade_swapped":
            down, up = up, down
        pad = self._pad_from
        for t in range(n):
            wd, wu = (n - t - 1, t + 1) if sw == "xfade_late" else (n - t, t)
            one_in_pad = pad is not None and ((down + t >= pad) != (up + t >= pad))
            for c in range(C):
                num = x[(down + t) * C + c] * wd + x[(up + t) * C + c] * wu
                if num < 0 and num % n:
                    cen["xfade_neg_frac"] += 1
                if abs(num) >= 32000 * n:
                    cen["xfade_full"] += 1
                if one_in_pad:
                    self._pad_marks.append(len(out))
                out.append(num // n if sw == "xfade_floor" else tdiv(num, n))

    def _process(self, speed):
        C, x = self.C, self.inp
        sp = _F(speed)
        if is_unity(sp):
            self.out += x
            self.inp = []
            if self.switch == "unity_clears_remaining":
                self.remaining = 0
            return
        n_in = len(x) // C
        mr = self.max_required
        if n_in < mr:
            return
        pos = 0
        while True:
            if self.remaining > 0:
                n = min(self.remaining, mr)
                if self.remaining > mr:
                    self.census["copy_capped"] += 1
                    if self.switch == "copy_uncapped":
                        n = min(self.remaining, n_in - pos)
                self.out += x[pos * C:(pos + n) * C]
                self.remaining -= n
                pos += n
            else:
                period, ret, min_diff, _ = R.find_pitch_period(x[pos * C:(pos + mr) * C], self.rate, C, self.prev_period, self.prev_min_diff)
                self.prev_period, self.prev_min_diff = period, min_diff
                self.steps += 1
                n, rem, _, _ = R.step_lengths(ret, sp)
                self.remaining, self._remaining_speed = rem, sp
                if sp > 1:
                    if n == 0:
                        self.census["failed_steps"] += 1
                        return
                    self._xfade(n, pos, pos + ret)
                    pos += ret + n
                else:
                    self.out += x[pos * C:(pos + ret) * C]
                    if n == 0:
                        self.census["failed_steps"] += 1
                        return
                    self._xfade(n, pos + ret, pos)
                    pos += n
            if pos + mr > n_in:
                break
        self.inp = x[pos * C:]

    def write(self, frames, speed):
        """Append interleaved samples and process them at `speed`."""
        sp = _F(speed)
        if is_unity(sp):
            if self.remaining > 0 and self.inp:
                self.census["unity_with_remaining"] += 1
        elif self.remaining > 0 and sp != self._remaining_speed:
            self.census["inherits_copy"] += 1
        self.inp += frames.tolist() if isinstance(frames, np.ndarray) else [int(v) for v in frames]
        self._process(speed)

    def flush(self, speed, cut=True):
        """cut=False: the rate stage's view -- the padded process call without the cut; `uncut_from` / `flush_pending` tell it where
        the flush began."""
        sp = _F(speed)
        C, mr = self.C, self.max_required
        pending = self.pending
        self.flush_pending, self.uncut_from = pending, self.frames_out
        pad = (mr if self.switch == "flush_pad_short" else 2 * mr)
        counted = pending + pad if self.switch == "flush_after_pad" else pending
        v = _F(_F(counted) / sp) if self.switch == "flush_floor" else _F(_F(counted) / sp) + _F(0.5)
        if pending and float(v) == int(v):
            self.census["flush_tie"] += 1
        expected = self.frames_out + int(v)
        self.inp += [0] * (pad * C)
        self._pad_from, self._pad_marks = pending, []
        self._process(speed)
        self._pad_from = None
        if cut and self.switch != "flush_no_cut" and self.frames_out > expected:
            self.census["flush_cut"] += 1
            del self.out[expected * C:]
        elif cut:
            self.census["flush_uncut"] += 1
        self.census["pad_kept"] += sum(1 for i in self._pad_marks if i < len(self.out))
        self.inp = []
        self.remaining = 0
        if self.switch == "flush_resets_prev":
            self.prev_period = 0


def linear_rows(s):
    """The time-map rows of a linear job (include/speedy_hip.h "TIME MAP"): the final count alone."""
    return [s.frames_out]


def linear_job(x, rate, channels, speed, switch=None):
    """One write of everything at the job's speed, then the flush.  Returns the stream; `rows` beside it."""
    s = SpeedStream(rate, channels, switch)
    s.write(x, speed)
    s.frames_after_write = s.frames_out
    s.flush(speed)
    s.rows = linear_rows(s)
    return s


def event_speeds(n_in, rate, tap, job_speed):
    """The speeds of a nonlinear job's n_in // B events (B = rate // 100): the first len(tap) carry the speed tap's values, the later
    ones the last of them."""
    k = n_in // (rate // 100)
    tap = [float(_F(v)) for v in tap]
    return [tap[i] if i < len(tap) else (tap[-1] if tap else float(job_speed)) for i in range(k)]


ROW_SWITCHES = ("row_after_write", "row_before_cut")


def nonlinear_job(x, rate, channels, speeds, job_speed=1.0, switch=None, row_switch=None):
    """n_in // B events of B frames, x[k B : (k + 1) B], each at its speed; the flush at the last speed; the trailing partial buffer
    is dropped (soniclib.c:538-550).  Returns the stream.

    `rows` beside it: the time map's rows as include/speedy_hip.h words them ("the output frames the time-scale stage has produced
    when ring buffer k is about to be handed to it", then "the job's final count") -- frames_out immediately before each event's
    write, and the final frames_out behind the flush: n_in // B + 1 rows, the final count alone for a job shorter than one buffer.
    row_switch makes one mistake (ROW_SWITCHES): row_after_write counts behind the event's write, row_before_cut takes the last row
    before the flush cuts the output."""
    assert row_switch is None or row_switch in ROW_SWITCHES, row_switch
    B = rate // 100
    s = SpeedStream(rate, channels, switch)
    x = [int(v) for v in x]
    assert len(speeds) == len(x) // channels // B
    rows = []
    for k, sp in enumerate(speeds):
        if row_switch != "row_after_write":
            rows.append(s.frames_out)
        s.write(x[k * B * channels:(k + 1) * B * channels], sp)
        if row_switch == "row_after_write":
            rows.append(s.frames_out)
    s.flush(speeds[-1] if len(speeds) else job_speed, cut=row_switch != "row_before_cut")
    rows.append(s.frames_out)
    s.rows = rows
    return s


def rate_pair(rate_hz, rate, switch=None, census=None):
    """(new, old): newSampleRate = (int)(rate_hz / rate) in float32 and the stream's rate, halved together while either exceeds 2^14."""
    new, old = int(_F(rate_hz) / _F(rate)), rate_hz
    while switch != "rate_no_halving" and (new > 16384 or old > 16384):
        if census is not None and ((new | old) & 1):
            census["halving_dropped"] += 1
        new >>= 1
        old >>= 1
    return new, old


def rate_stage(y, channels, new, old, switch=None, census=None):
    """Output k exists while t = floor(k old / new) <= M - 2 and is ((new - w) y[t] + w y[t + 1]) / new, w = k old - t new, truncated
    toward zero, per channel.  y: interleaved Python integers, M frames."""
    C = channels
    M = len(y) // C
    out = []
    last = M - 1 if switch == "rate_keeps_last" else M - 2
    k = 0
    while M >= 2:
        t = k * old // new
        if t > last:
            break
        w = k * old - t * new
        a, b = (w, new - w) if switch == "rate_swapped" else (new - w, w)
        t1 = min(t + 1, M - 1)
        for c in range(C):
            num = a * y[t * C + c] + b * y[t1 * C + c]
            if census is not None and num < 0 and num % new:
                census["rate_neg_frac"] += 1
            out.append(num // new if switch == "rate_floor" else tdiv(num, new))
        k += 1
    return out


class RateStream:
    """SpeedStream with the rate stage behind it, for one life cycle: write, write, ..., flush.  `out` is the final output so far."""

    def __init__(self, rate_hz, channels, rate, switch=None):
        self.speed_stage = SpeedStream(rate_hz, channels, switch if switch in SPEED_SWITCHES else None)
        self.C, self.switch, self.playback = channels, switch, _F(rate)
        self.census = self.speed_stage.census
        self.new, self.old = rate_pair(rate_hz, rate, switch, self.census)
        self.out = []
        self.flushed = False

    @property
    def frames_out(self):
        return len(self.out) // self.C

    def write(self, frames, speed):
        assert not self.flushed, "one life cycle only"
        self.speed_stage.write(frames, speed)
        self.out = rate_stage(self.speed_stage.out, self.C, self.new, self.old, self.switch)

    def flush(self, speed):
        assert not self.flushed, "one life cycle only"
        self.flushed = True
        s = self.speed_stage
        before = self.frames_out
        s.flush(speed, cut=False)
        left = 1 if s.uncut_from >= 1 else 0          # the one frame the stage holds back
        v = _F(_F(_F(s.flush_pending) / _F(speed)) + _F(left)) / self.playback
        if self.switch != "rate_flush_floor":
            v = v + _F(0.5)
        expected = before + int(v)
        full = rate_stage(s.out, self.C, self.new, self.old, self.switch, self.census)
        self.out = full[:expected * self.C] if len(full) // self.C > expected else full


class PlaybackStream:
    """SpeedStream with the rate stage behind it AS A STREAM: set_rate(r) at any time, write(frames, speed), flush(speed), any number
    of lives.  `out` is the final output so far, `census` counts what the calls reached (PLAYBACK_CENSUS).

    The state is the float32 rate (1 at creation), the two positions o (input frames passed) and k (output frames emitted) since
    they were last zeroed, and the pitch buffer: the frames that wait for a right neighbour.  After every process call of the speed
    stage -- a write, or the flush's padded call -- the stage takes what that call appended (_take)."""

    def __init__(self, rate_hz, channels, switch=None):
        assert switch is None or switch in SWITCHES, switch
        self.speed_stage = SpeedStream(rate_hz, channels, switch if switch in SPEED_SWITCHES else None)
        self.rate_hz, self.C, self.switch = rate_hz, channels, switch
        self.playback = _F(1.0)
        self.o = self.k = 0
        self.pitch = []                        # waiting frames, each a list of C Python integers
        self.out = []
        self.census = dict.fromkeys(PLAYBACK_CENSUS, 0)
        self._stale = False                    # the waiting frame was passed by while the rate was 1
        self._life_begins = True               # no process call yet in this life

    @property
    def frames_out(self):
        return len(self.out) // self.C

    def set_rate(self, r):
        r = _F(r)
        if self.pitch:
            self.census["set_with_left"] += 1
        if self.switch == "same_rate_is_noop" and r == self.playback:
            return
        self.playback = r
        if self.switch != "set_rate_keeps_positions":
            self.o = self.k = 0
        if self.switch == "set_rate_drops_left":
            self.pitch, self._stale = [], False

    def _take(self, fresh):
        """fresh: what the speed stage appended in this process call, interleaved."""
        C, cen, sw = self.C, self.census, self.switch
        begins, self._life_begins = self._life_begins, False
        if self.playback == _F(1.0):
            self.out += fresh
            if self.pitch:
                self._stale = True
                if sw == "unity_rate_drops_left":
                    self.pitch, self._stale = [], False
            return
        if begins and (self.o or self.k):
            cen["life_starts_off_zero"] += 1
        new, old = rate_pair(self.rate_hz, self.playback, None, cen)
        had = len(self.pitch)                  # 0 or 1: the frame an earlier call left behind
        p = self.pitch
        p += [fresh[i:i + C] for i in range(0, len(fresh), C)]
        M = len(p)
        if M < 2:
            if fresh:
                cen["short_calls"] += 1
            return
        for pos in range(M - 1):
            across = pos == 0 and had > 0
            left, right = (p[1] if across and sw == "straddle_uses_new_left" else p[pos]), p[pos + 1]
            while (self.o + 1) * new > self.k * old:
                ratio = (self.o + 1) * new - self.k * old
                if across:
                    cen["straddle"] += 1
                    if self._stale:
                        cen["stale_used"] += 1
                for c in range(C):
                    num = ratio * left[c] + (new - ratio) * right[c]
                    if num < 0 and num % new:
                        cen["rate_neg_frac"] += 1
                    self.out.append(tdiv(num, new))
                self.k += 1
            self.o += 1
            if self.o == old and sw != "no_wrap":
                self.o = self.k = 0
                cen["wraps"] += 1
        del p[:M - 1]
        self._stale = False

    def write(self, frames, speed):
        s = self.speed_stage
        before = len(s.out)
        s.write(frames, speed)
        self._take(s.out[before:])

    def flush(self, speed):
        s = self.speed_stage
        waiting = 0 if self.switch == "flush_count_without_left" else len(self.pitch)
        v = _F(_F(_F(s.pending) / _F(speed)) + _F(waiting)) / self.playback + _F(0.5)
        expected = self.frames_out + int(v)
        if self.playback == _F(1.0) and self.pitch:
            self.census["bypass_flush_with_left"] += 1
        before = len(s.out)
        s.flush(speed, cut=False)
        self._take(s.out[before:])
        if self.frames_out > expected:
            del self.out[expected * self.C:]
        if self.switch != "flush_keeps_left":
            self.pitch, self._stale = [], False
        if self.switch == "flush_resets_positions":
            self.o = self.k = 0
        self._life_begins = True


def playback_events(rate_hz, channels, events, switch=None):
    """A PlaybackStream over [("rate", r) | ("write", samples, speed) | ("flush", speed)]: (stream, frames produced after each event)."""
    s = PlaybackStream(rate_hz, channels, switch)
    counts = []
    for ev in events:
        if ev[0] == "rate":
            s.set_rate(ev[1])
        elif ev[0] == "write":
            s.write(ev[1], ev[2])
        else:
            s.flush(ev[1])
        counts.append(s.frames_out)
    return s, counts


def rate_job(x, rate_hz, channels, speed, rate, switch=None):
    """A batch job with a playback rate: one write, the flush.  Returns the RateStream."""
    s = RateStream(rate_hz, channels, rate, switch)
    s.write(x, speed)
    s.frames_after_write = s.frames_out
    s.flush(speed)
    return s
