"""The directed inputs of the time-scale-modification tests (tests/test_oracle_tsm_definition.py on the CPU,
tests/test_gpu_tsm_definition.py on the device): generated, deterministic, no fixture files, 0.3 to 1.0 s.

Full-scale rectangles, every channel with its own period and phase and one value in seven drawn from the whole int16 range:
cross-fade numerators of both signs near +-32768 n, most of them no multiple of n, and channels that no permutation and no
slipped e / C leaves equal.  tests/tsm_ref.py's census (asserted by the CPU test) says what each input reaches.
"""
import numpy as np

import pitch_ref as R

_F = np.float32
_SIGNALS = {}


def rectangles(rate, channels, frames):
    """Interleaved int16: channel c is +32767 where (t + 13 c) mod P_c < D_c, else -32768, with P_c = rate // (150 + 20 c) and
    D_c = rate // (300 + 40 c) - c; every value whose (index + frame) is a multiple of 7 is random over the whole int16 range
    (so that with 7 channels the random values do not all fall on one channel).  Built once per (rate, channels), never modified;
    shorter signals are prefixes of the longest one asked for."""
    key = (rate, channels)
    if key not in _SIGNALS or _SIGNALS[key].size < frames * channels:
        n = max(frames, rate)
        t = np.arange(n)
        chans = [np.where(((t + 13 * c) % (rate // (150 + 20 * c))) < rate // (300 + 40 * c) - c, 32767, -32768) for c in range(channels)]
        x = np.stack(chans, axis=1).reshape(-1).astype(np.int16)
        rng = np.random.default_rng([rate, channels])
        idx = np.arange(x.size)
        pick = (idx + idx // channels) % 7 == 0
        x[pick] = rng.integers(-32768, 32768, int(pick.sum()))
        x.setflags(write=False)
        _SIGNALS[key] = x
    return _SIGNALS[key][:frames * channels]


def below(v):
    return float(np.nextafter(_F(v), _F(0)))


def unity_neighbours():
    """(the largest float32 that the unity test still takes for 1, the float32 above it): the neighbours of 1.00001."""
    a = _F(1.00001)
    if float(a) > 1.00001:
        a = np.nextafter(a, _F(0))
    b = np.nextafter(a, _F(2))
    assert float(a) <= 1.00001 < float(b)
    return float(a), float(b)


SPEEDS = (2.0, below(2.0), 1.3, 1.00002) + unity_neighbours() + (0.99998, 0.5, below(0.5), 0.7, 3.5, 2000.0, 0.0001)
EXTRA_SPEEDS = (200.0,)                 # n = (int)(period / 199) is 1 for long periods and 0 for short ones: a step fails AFTER others ran
RUN = tuple(range(2980, 3020))          # 40 consecutive lengths: the flush meets every phase of a step
RUN_SPEEDS = (2.0, 3.5, 0.4, 0.7)
_LINEAR = None


def linear_jobs():
    """[(name, rate, channels, int16 interleaved samples, speed)] -- every directed batch job without a playback rate."""
    global _LINEAR
    if _LINEAR is not None:
        return _LINEAR
    jobs = []

    def add(tag, rate, ch, frames, speeds):
        x = rectangles(rate, ch, frames)
        for s in speeds:
            jobs.append(("%s/%dHz/%dch/%d/%.9g" % (tag, rate, ch, frames, s), rate, ch, x, float(s)))

    for ch in (1, 2, 3, 5, 7, 8):                                   # the speed-up kernel serves skip x channels <= 56, C <= 8
        add("channels", 22050, ch, 6615, (2.0, 1.3, 0.7))
    for ch in (1, 2, 4, 5):                                         # 5 channels at 48 kHz: the general kernel
        add("channels", 48000, ch, 14400, (2.0, 1.3, 0.7))
    for rate in (11025, 16000, 44100, 63999, 96000, 3999):          # 3 999 Hz: skip == 1, the direct search
        add("rates", rate, 1, int({11025: 0.6, 16000: 0.6, 3999: 1.0}.get(rate, 0.3) * rate), (2.0, 1.3, 0.7))
    add("rates", 16000, 2, 4800, (2.0, 1.3, 0.4))
    add("speeds", 22050, 1, 7000, SPEEDS + EXTRA_SPEEDS)
    add("speeds", 16000, 1, 9001, SPEEDS + EXTRA_SPEEDS)
    mr = R.limits(22050)[2]
    for n in (0, 1, mr - 1, mr, mr + 1):
        add("lengths", 22050, 1, n, (2.0, 0.7, 1.0))
    for n in RUN:
        add("run", 22050, 1, n, RUN_SPEEDS)
    _LINEAR = jobs
    return jobs


SIZES = (1, 159, 160, 161, 1000, "mr", 700, "mr-1", 3, "2mr+3", 220)
SEQUENCE = (3.5, 1.3, 1.0, 0.4, 1.00002, 2.0, 0.7, 1.0, 1.9, 0.99998, 1.3, 1.3, 0.6, 3.5)
# ... and without the two speeds next to 1: one step at 1.00002 leaves a copy of 50 000 periods, and nothing but the flush ends it
SEQUENCE_FAR = (3.5, 1.3, 1.0, 0.4, 2.0, 0.7, 1.0, 1.9, 1.3, 1.3, 1.0, 0.6, 3.5, 0.55, 1.6)
# ... and speeds above 1 only: the drop-in API keeps such a stream on the speed-up kernel
SEQUENCE_UP = (3.5, 1.3, 2.0, 1.9, 1.3, 1.6, 2.5, 1.1, 1.3)
_PLANTED = None


def _events(rate, ch, frames, scale, flush_at, sequence=SEQUENCE_FAR):
    """Writes of irregular sizes at speeds that jump between the branches, a flush after write number `flush_at`, a second life, a
    last flush.  [("write", samples, speed) | ("flush", speed)]: the flush runs at the speed set last."""
    x = rectangles(rate, ch, frames)
    mr = R.limits(rate)[2]
    ev, pos, k, speed = [], 0, 0, 1.0
    while pos < frames:
        size = SIZES[k % len(SIZES)]
        size = {"mr": mr, "mr-1": mr - 1, "2mr+3": 2 * mr + 3}[size] if isinstance(size, str) else size * scale
        size = min(size, frames - pos)
        speed = sequence[k % len(sequence)]
        ev.append(("write", x[pos * ch:(pos + size) * ch], speed))
        pos += size
        k += 1
        if k == flush_at:
            ev.append(("flush", speed))
    ev.append(("flush", speed))
    return ev


def _second_life(name, split):
    """A quiet signal of tests/pitch_inputs.py cut where the first step of the second life keeps the previous period -- the one the
    FIRST life left: a flush that cleared prevPeriod would choose another."""
    import pitch_inputs
    rate, x = [(r, x) for n, r, c, x in pitch_inputs.directed() if n == name][0]
    mr = R.limits(rate)[2]
    return rate, 1, [("write", x[:split], 2.0), ("flush", 2.0), ("write", x[split:split + 3 * mr], 2.0), ("flush", 2.0)]


def planted_streams():
    """[(name, rate, channels, events)] for the stream APIs."""
    global _PLANTED
    if _PLANTED is None:
        _PLANTED = [("planted22k", 22050, 1, _events(22050, 1, 19000, 1, 23)),
                    ("planted16k_stereo", 16000, 2, _events(16000, 2, 12000, 1, 17)),
                    ("planted16k_near_unity", 16000, 1, _events(16000, 1, 9000, 1, 14, SEQUENCE)),
                    ("planted48k", 48000, 1, _events(48000, 1, 30000, 2, 15)),
                    ("speedup22k", 22050, 1, _events(22050, 1, 15000, 1, 19, SEQUENCE_UP)),
                    ("speedup48k_stereo", 48000, 2, _events(48000, 2, 24000, 2, 13, SEQUENCE_UP)),
                    ("second_life_hum22k",) + _second_life("hum22k", 1356),
                    ("second_life_hum16k",) + _second_life("hum16k", 984)]
    return _PLANTED


# Rate plans over the planted event lists: {index of the planted event BEFORE which sonicSetRate is called: the rate}.  An index past
# the end of a list (the two second_life lists have four events) plants nothing.
RATE_PLANS = ({0: 1.25, 9: 0.8, 16: 1.0, 20: 1.5, 27: 1.5},     # both sides of 1, back to 1 and away again, the value already set
              {3: 0.5, 12: 1.0, 25: 2.0},                        # the rate first set after three writes; through 1 in the middle
              {0: 3.0, 30: 1.0},
              {0: 1.1})
_PLAYBACK = None


def with_rates(events, plan):
    out = []
    for k, ev in enumerate(events):
        if k in plan:
            out.append(("rate", float(plan[k])))
        out.append(ev)
    return out


def _calls(rate, ch, calls):
    """[("rate", r) | ("flush", speed) | (frames, speed)] over consecutive pieces of the rectangles."""
    total = sum(c[0] for c in calls if c[0] not in ("rate", "flush"))
    x = rectangles(rate, ch, total)
    ev, pos = [], 0
    for c in calls:
        if c[0] in ("rate", "flush"):
            ev.append((c[0], float(c[1])))
        else:
            ev.append(("write", x[pos * ch:(pos + c[0]) * ch], float(c[1])))
            pos += c[0]
    return ev


def playback_streams():
    """[(name, rate_hz, channels, events)] for the rate stage as a stream: the planted event lists (two lives each) under every rate
    plan, then the directed cases.  Events: the planted ones and ("rate", r)."""
    global _PLAYBACK
    if _PLAYBACK is not None:
        return _PLAYBACK
    out = []
    for name, rate, ch, ev in planted_streams():
        for i, plan in enumerate(RATE_PLANS):
            out.append(("%s/plan%d" % (name, i), rate, ch, with_rates(ev, plan)))
    # one frame per call at speed 1: the first call of a life only sets the waiting frame, every later call emits one or two frames
    # whose operands come from two calls
    out.append(("one_frame_calls", 16000, 2, _calls(16000, 2, [("rate", 0.8)] + [(1, 1.0)] * 40 + [("flush", 1.0)] + [(1, 1.0)] * 9
                                                           + [("flush", 1.0)])))
    # back from 1 to a rate != 1 with a frame gone stale; a flush at 1 with that frame waiting; the value already set, set again
    out.append(("stale_return", 16000, 1, _calls(16000, 1, [("rate", 0.8), (300, 1.0), ("rate", 1.0), (200, 1.0), (1, 1.0), ("rate", 1.25),
                                                           (300, 1.0), (900, 2.0), ("rate", 1.25), (150, 1.0), ("rate", 1.0), (50, 1.0),
                                                           ("flush", 1.0), (100, 1.0), ("rate", 0.8), (700, 2.0), (120, 1.0),
                                                           ("flush", 1.0)])))
    # 16 channels, the most a rate != 1 supports; no two channels equal
    out.append(("sixteen_channels", 16000, 16, _calls(16000, 16, [("rate", 1.25), (2500, 2.0), (700, 1.0), ("rate", 0.8), (1500, 0.7),
                                                                  ("flush", 0.7), (900, 1.0), ("flush", 1.0)])))
    # the rate first set behind several writes: on the device nothing is read before the write that follows it
    out.append(("unread_head", 22050, 1, _calls(22050, 1, [(1500, 2.0), (700, 1.0), (2100, 1.3), ("rate", 1.25), (1800, 2.0), (400, 1.0),
                                                           ("flush", 1.0), (2000, 2.0), ("flush", 2.0)])))
    # 3 999 Hz (the direct search; old = 3 999 wraps inside the stream), 44.1 kHz (the halving drops a bit of `new`), 96 kHz
    out.append(("3999Hz", 3999, 1, _calls(3999, 1, [("rate", 1.1), (1000, 0.7), (1000, 0.7), (1000, 0.7), ("flush", 0.7), (500, 2.0),
                                                    ("rate", 0.8), (499, 2.0), ("flush", 2.0)])))
    out.append(("44100Hz", 44100, 2, _calls(44100, 2, [("rate", 1.1), (5000, 1.3), (4000, 1.0), (4230, 2.0), ("flush", 2.0), (6000, 1.3),
                                                       ("rate", 0.7), (6000, 1.0), ("flush", 1.0)])))
    out.append(("96000Hz", 96000, 1, _calls(96000, 1, [("rate", 0.8), (9000, 2.0), (10800, 1.0), ("flush", 1.0), ("rate", 1.25), (9000, 2.0),
                                                       ("flush", 2.0)])))
    _PLAYBACK = out
    return out


def syllables(rate, channels, frames):
    """The rectangles under a 4 Hz raised-cosine envelope (full scale at the crests, silence between them): the nonlinear
    speed-up's speed moves with it, so that consecutive 10 ms events carry different speeds."""
    x = rectangles(rate, channels, frames).astype(np.float64).reshape(-1, channels)
    env = 0.5 * (1.0 - np.cos(2.0 * np.pi * 4.0 * np.arange(frames) / rate))
    y = np.trunc(x * env[:, None]).astype(np.int16).reshape(-1)
    y.setflags(write=False)
    return y


# (rate, channels, frames, speed, nonlinear factor): speed-up around 3.5 and around 1.2 (both branches of the speed-up step), and
# a slow-down job whose events fall on both sides of unity
_NONLINEAR_SPECS = ((22050, 1, 19999, 3.5, 1.0), (22050, 1, 15000, 1.2, 1.0), (22050, 1, 12345, 2.0, 0.5),
                    (16000, 1, 15000, 3.5, 1.0), (16000, 1, 9000, 1.2, 1.0), (16000, 2, 9000, 0.8, 0.5))
_NONLINEAR = None


def nonlinear_jobs():
    """[(name, rate, channels, samples, speed, nonlinear factor)] -- the event speeds are the analysis side's (the speed tap)."""
    global _NONLINEAR
    if _NONLINEAR is None:
        _NONLINEAR = [("nonlinear/%dHz/%dch/%d/%g/%g" % spec, spec[0], spec[1], syllables(*spec[:3]), spec[3], spec[4])
                      for spec in _NONLINEAR_SPECS]
    return _NONLINEAR


# The time map's nonlinear jobs (a list of its own: the names above stay what they were).  B = rate // 100, R = frames // B:
# (rate, channels, frames, speed, nonlinear factor, what the job is for)
_MAP_SPECS = ((16000, 1, 8000, 3.5, 1.0, "n_in = R B exactly"),
              (16000, 1, 6559, 1.2, 1.0, "n_in = R B + B - 1"),
              (16000, 1, 200, 3.5, 1.0, "R = 1: no analysis frame, the one event runs at the job's speed"),
              (16000, 1, 100, 3.5, 1.0, "n_in < B: no event, the final count alone"),
              (16000, 3, 6000, 2.0, 1.0, "3 channels"),
              (16000, 8, 4000, 3.5, 1.0, "8 channels"),
              (16000, 1, 9000, 0.5, 1.0, "slow-down: rows that rise by more than B"),
              (11025, 1, 6000, 3.0, 1.0, "11.025 kHz"),
              (48000, 1, 24100, 2.0, 1.0, "48 kHz"))
_MAP_JOBS = None


def nonlinear_map_jobs():
    """[(name, rate, channels, samples, speed, nonlinear factor)] -- the jobs the time map's rows are defined on, in addition to
    nonlinear_jobs(): syllables, at most 1.5 s each."""
    global _MAP_JOBS
    if _MAP_JOBS is None:
        _MAP_JOBS = [("map/%dHz/%dch/%d/%g/%g" % spec[:5], spec[0], spec[1], syllables(*spec[:3]), spec[3], spec[4])
                     for spec in _MAP_SPECS]
    return _MAP_JOBS


_RATE = None


def rate_jobs():
    """[(name, rate_hz, channels, samples, speed, playback rate)] -- the directed jobs of the rate stage."""
    global _RATE
    if _RATE is not None:
        return _RATE
    jobs = []

    def add(rate_hz, ch, frames, speed, rate):
        jobs.append(("rate/%dHz/%dch/%d/%g/%.9g" % (rate_hz, ch, frames, speed, rate), rate_hz, ch, rectangles(rate_hz, ch, frames),
                     float(speed), float(rate)))

    for r in (1.25, 0.8, 2.0, 0.5, 3.0, 1.0000001):
        add(22050, 1, 6615, 2.0, r)
    add(44100, 2, 13230, 1.3, 1.1)          # halving drops a bit of `new`
    add(16000, 3, 4800, 1.0, 0.8)           # three channels, more than 2 048 output values: a block that begins inside a frame
    add(22050, 3, 6615, 0.7, 1.25)
    add(48000, 1, 14400, 2.0, 0.5)
    add(8000, 1, 2400, 0.7, 3.0)
    add(22050, 1, 3, 1.0, 2.0)              # streams shorter than 8 output values
    add(22050, 1, 1, 1.0, 1.25)
    add(22050, 1, 9, 1.0, 1.25)
    add(16000, 3, 3, 1.0, 0.8)
    _RATE = jobs
    return jobs
