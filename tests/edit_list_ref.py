"""The edit list of a batch job as exact integers -- test infrastructure, CPU only.

include/speedy_hip.h "EDIT LIST" words what a job's list is; tests/tsm_ref.py states the time-scale stage as two operations on
Python integers, a copy and a cross-fade.  EditStream is the speed stage of tsm_ref.SpeedStream restated with ABSOLUTE positions --
the input is never shifted, `base` is the first frame still pending -- and, instead of computing samples, it writes down every
operation: (out_at, a, -1, n) for n frames copied from input frame a, (out_at, a, b, n) for n frames of cross-fade with the ramp
going down at a and the ramp coming up at b (SpeedStream._xfade's (down, up)).  The decision -- which period, how many frames -- is
tests/pitch_ref.py's, as in tsm_ref.

replay(ops, y, channels, L, n_out) applies a list to a track in Python integers: output frame o < n_out is the value of the record
that covers o; a source frame at or behind L reads as 0; the quotient truncates toward zero.  replay(list of a job, the job's own
input) is tsm_ref's output of the job -- tests/test_edit_list_abi.py asserts it on every directed job -- so the list is pinned by a
definition that is neither the kernel nor the oracle.

SWITCHES make one mistake each:
  ramps_swapped   a cross-fade is recorded as (b, a)
  limit_n_in      L = n_in on a nonlinear job (the trailing partial ring buffer read as if it had been handed over)
  floor           floor for truncation in the replay's quotient
  cut_drops_op    a record that reaches behind the flush's cut is dropped
"""
import contextlib
import hashlib

import numpy as np

import pitch_ref as R
import tsm_ref as T

SWITCHES = ("ramps_swapped", "limit_n_in", "floor", "cut_drops_op")
_F = np.float32
_MEMO = {}

# The directed linear jobs of tests/tsm_inputs.py with failed steps and their true record counts (the definition's:
# tests/test_edit_list_abi.py asserts them).  At 2000 and 0.0001 every step fails -- the write's and the flush's, two -- and at 200
# n = (int)(period / 199) is 1 for long periods and 0 for short ones.  spx_plan_edit_ops promises nothing for these.
FAILED_STEP_JOBS = {
    "speeds/22050Hz/1ch/7000/2000": 0, "speeds/22050Hz/1ch/7000/0.0001": 2, "speeds/22050Hz/1ch/7000/200": 22,
    "speeds/16000Hz/1ch/9001/2000": 0, "speeds/16000Hz/1ch/9001/0.0001": 2, "speeds/16000Hz/1ch/9001/200": 0,
}


@contextlib.contextmanager
def shared_pitch_searches():
    """Inside: pitch_ref.find_pitch_period remembers its answers.  EditStream asks exactly what tsm_ref.SpeedStream asked on the same
    job (the same window, the same previous period), so a test that runs both pays for each search once.  The answers are the
    function's own."""
    real, memo = R.find_pitch_period, _MEMO

    def find(window, rate, channels, prev_period, prev_min_diff, *more, **kw):
        if more or kw:
            return real(window, rate, channels, prev_period, prev_min_diff, *more, **kw)
        key = (hashlib.sha1(np.asarray(window, np.int64).tobytes()).digest(), rate, channels, prev_period, prev_min_diff)
        if key not in memo:
            memo[key] = real(window, rate, channels, prev_period, prev_min_diff)
        return memo[key]
    R.find_pitch_period = find
    try:
        yield
    finally:
        R.find_pitch_period = real


class EditStream:
    def __init__(self, rate, channels, switch=None):
        assert switch is None or switch in SWITCHES, switch
        self.rate, self.C, self.switch = rate, channels, switch
        self.max_required = R.limits(rate)[2]
        self.x = []                 # everything ever handed over, the flush's zeros included: interleaved Python integers
        self.base = 0               # first frame still pending
        self.avail = 0              # frames handed over
        self.out_n = 0              # frames produced
        self.ops = []
        self.remaining = 0
        self.prev_period = self.prev_min_diff = 0
        self.failed_steps = 0
        self.limit = None           # L: set by the flush

    def _copy(self, a, n):
        if n >= 1:
            self.ops.append((self.out_n, a, -1, n))
            self.out_n += n

    def _xfade(self, n, down, up):
        assert n >= 1
        self.ops.append((self.out_n, up, down, n) if self.switch == "ramps_swapped" else (self.out_n, down, up, n))
        self.out_n += n

    def _process(self, speed):
        C, mr = self.C, self.max_required
        sp = _F(speed)
        if T.is_unity(sp):
            self._copy(self.base, self.avail - self.base)
            self.base = self.avail
            return
        n_in = self.avail - self.base
        if n_in < mr:
            return
        pos = 0
        while True:
            if self.remaining > 0:
                n = min(self.remaining, mr)
                self._copy(self.base + pos, n)
                self.remaining -= n
                pos += n
            else:
                p = self.base + pos
                period, ret, min_diff, _ = R.find_pitch_period(self.x[p * C:(p + mr) * C], self.rate, C, self.prev_period, self.prev_min_diff)
                self.prev_period, self.prev_min_diff = period, min_diff
                n, rem, _, _ = R.step_lengths(ret, sp)
                self.remaining = rem
                if sp > 1:
                    if n == 0:
                        self.failed_steps += 1
                        return                      # nothing consumed
                    self._xfade(n, p, p + ret)
                    pos += ret + n
                else:
                    self._copy(p, ret)
                    if n == 0:
                        self.failed_steps += 1
                        return                      # the copy stays
                    self._xfade(n, p + ret, p)
                    pos += n
            if pos + mr > n_in:
                break
        self.base += pos

    def write(self, frames, speed):
        self.x += frames.tolist() if isinstance(frames, np.ndarray) else [int(v) for v in frames]
        self.avail = len(self.x) // self.C
        self._process(speed)

    def flush(self, speed):
        sp = _F(speed)
        mr = self.max_required
        pending = self.avail - self.base
        expected = self.out_n + int(_F(_F(pending) / sp) + _F(0.5))
        self.limit = self.avail
        self.x += [0] * (2 * mr * self.C)
        self.avail += 2 * mr
        self._process(speed)
        if self.out_n > expected:
            self.out_n = expected                   # the cut removes no record
            if self.switch == "cut_drops_op":
                self.ops = [op for op in self.ops if op[0] + op[3] <= expected]
        self.base = self.avail
        self.remaining = 0


def linear_job(x, rate, channels, speed, switch=None):
    """One write of everything at the job's speed, then the flush.  Returns the stream: ops, out_n (= n_out), limit (= L)."""
    s = EditStream(rate, channels, switch)
    s.write(x, speed)
    s.flush(speed)
    return s


def nonlinear_job(x, rate, channels, speeds, job_speed=1.0, switch=None):
    """n_in // B events of B frames each at its speed, the flush at the last; the trailing partial buffer is never handed over."""
    B = rate // 100
    s = EditStream(rate, channels, switch)
    x = [int(v) for v in x]
    assert len(speeds) == len(x) // channels // B
    for k, sp in enumerate(speeds):
        s.write(x[k * B * channels:(k + 1) * B * channels], sp)
    s.flush(speeds[-1] if len(speeds) else job_speed)
    if switch == "limit_n_in":
        s.limit = len(x) // channels
    return s


def limit_of(n_in, rate, nonlinear):
    """L as the header words it: n_in for a linear job, (n_in / B) * B for a nonlinear one."""
    B = rate // 100
    return n_in // B * B if nonlinear else n_in


def replay(ops, y, channels, L, n_out, switch=None):
    """The track y (interleaved, any channel count) under the list: n_out frames as a list of Python integers.  A frame no record
    covers stays None."""
    C = channels
    y = y.tolist() if isinstance(y, np.ndarray) else y
    out = [None] * (n_out * C)
    for out_at, a, b, n in ops:
        assert n >= 1
        for t in range(min(n, n_out - out_at)):
            for c in range(C):
                va = y[(a + t) * C + c] if a + t < L else 0
                if b < 0:
                    v = va
                else:
                    vb = y[(b + t) * C + c] if b + t < L else 0
                    num = va * (n - t) + vb * t
                    v = num // n if switch == "floor" else T.tdiv(num, n)
                out[(out_at + t) * C + c] = v
    return out


def contiguous(ops):
    """ops[0].out_at = 0 and ops[k + 1].out_at = ops[k].out_at + ops[k].n."""
    at = 0
    for op in ops:
        if op[0] != at or op[3] < 1:
            return False
        at += op[3]
    return True
