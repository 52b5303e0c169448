"""A float64 definition of everything Speedy computes AFTER the spectrum -- the fifteen feature values, the tension and the
speed of every 10 ms frame -- written from the reference's text (speedy.c, soniclib.c, speedy.h) and not from oracle/: the
second, independent check the feature tests hold the oracle and the HIP kernels to.  Same standing as spectrum_ref.py.

The chain is full of gates and recurrences, so the definition does not run free against an implementation.  check() gives each
stage the implementation's OWN float32 outputs of the stage before (teacher forcing): no error crosses a gate or a recurrence
step, every gate compares float32 numbers that are in the taps and is decided exactly, and a stage's bound is a count of its
float32 roundings (u = 2^-24 each), written beside the stage.  No bound is fitted and none is loosened per case.

Time base.  The shim hands analysis frame j to Speedy stamped with its write index (soniclib.c:295-296), which is j + W/B =
j + 1 at every rate (W = floor(1.5 fs / 100), B = floor(fs / 100)): row j of the spectrogram callback, and of the batch
`spectrogram` tap (include/speedy_hip.h: "|DFT| of analysis frame j"), is the spectrum of Speedy time j + 1.  Time 0 is the
all-zero history row (speedy.c:242-247).  The tension of time k is computed once time k + F has been added (speedy.c:755) from
the spectra of times k and k - 1 (:756-757), i.e. callback rows k - 1 and k - 2; T spectrogram rows give K = T + 1 - F rows.
The unit-level loop of speedy_test.cc:911-935 stamps its first frame with time 0 instead: `t0` below is the time of
spectrogram row 0 (1 for the shim, 0 for the unit level).
Features 1 - 3 and 12 of row k were made when time k + F was added (speedy.c:517-522), the others at tension time k
(:672-728): f12 = k + F, f13 = k, and the energy that f1 / f2 of row k were made from is f0 of row k + F (speedy.c:515 and :636
are the same float32 sum over the same bins).

run()     the free-running chain from spectra alone (pinned by the reference's own data in the tests)
check()   every stage of every frame of an implementation's taps against (expected, bound); returns the table
"""
import math

import numpy as np

U = 2.0 ** -24                                    # unit roundoff of float32
ALPHA = float(np.float32(math.exp(-1.0 / 100.0)))  # speedy.c:67 with kFrameRateHz (:90,287,290), stored as float (:52)
MEAN_ENERGY = float(np.float32(2.14204))          # speedy.c:263, float fields (:158-162)
MEAN_DIFFERENCE = float(np.float32(123.837))      # :264
MEAN_LPF = float(np.float32(123.979))             # :265
MEAN_RELATIVE = float(np.float32(0.971975))       # :266
MAX_HYSTERESIS = float(np.float32(1.41421))       # :267
EPS = float(np.float32(2.2204e-16))               # :641,712 `const float eps`
LOW_THRESHOLD = float(np.float32(0.04 * MAX_HYSTERESIS))   # :682 double product stored in a float feature
CLAMP = 4.0 * MEAN_RELATIVE                       # :728, exact in float
FRAME_DURATION = float(np.float32(1.0 / 100.0))   # :783 `float frame_duration`
MIN_SPEED = 0.01                                  # :92 kMinimumSpeed, a double

STAGES = ["f0", "f1", "f2", "f3", "f4", "f5", "f6", "f7", "f8", "f9", "f10", "f11", "f12", "f13", "f14", "tension", "speed"]


def hysteresis_shape(matlab):
    """(future, past) frames, speedy.h:136-146."""
    return (8, 12) if matlab else (12, 8)


def taper(n):
    """speedy.c:597,604: (n - i) / (float)n, a float32 quotient, for i = 0 .. n."""
    return (np.arange(n, -1, -1, dtype=np.float32) / np.float32(n)).astype(np.float64)


# ---- stages: float64 in, (expected, bound) out ----------------------------------------------------------------------

def energy(spec, W):
    """f0, speedy.c:633-640 (= :513-516): sum_{i=1}^{W-1} S[i]^2.  The reference squares and adds W - 1 non-negative floats one
    after another: one rounding per square, one per addition, each at most u relative to a partial sum that never exceeds the
    total: (2 (W - 1)) u e would be the crude count; squares carry u each into a sum of non-negative terms (u e in all) and
    the W - 2 additions (W - 2) u e, the float64 sum here adds nothing visible: (W + 2) u e with room to spare."""
    s = np.asarray(spec, np.float64)[..., 1:W]
    e = (s * s).sum(axis=-1)
    return e, (W + 2) * U * e


def lowpass(x, prev):
    """f1 / f8, speedy.c:73-76: (1 - alpha) x + alpha state, all float.  1 - alpha is exact (alpha in [1/2, 1)); the two
    products and the sum round once each, the terms are non-negative: 3 u |value|."""
    v = (1.0 - ALPHA) * x + ALPHA * prev
    return v, 3 * U * np.abs(v)


def local_energy(e, f1):
    """f2, speedy.c:519: one float division: u |value|."""
    with np.errstate(divide="ignore", invalid="ignore"):
        v = e / f1
    return v, U * np.abs(v)


def compressed(f2):
    """f3, speedy.c:520: sqrt in double of min(f2, 2), stored as float: one rounding (the double square root's own error is
    2^-29 of that): u |value|."""
    v = np.sqrt(np.minimum(f2, 2.0))
    return v, U * v * (1 + 2.0 ** -28)


def hysteresis(c, bc, k, F, P):
    """f4, speedy.c:590-610: (max_{i<=F} c[k+i] (F-i)/(float)F + max_{i<=P} c[k-i] (P-i)/(float)P) / 2 with c = 0 before the
    first frame (:284).  c, bc: callables time -> compressed energy and its bound.  Each product rounds once, the maxima are
    exact (and 1-Lipschitz: no discontinuity), the sum rounds once, the halving is exact: 2 u value, plus the tapered bounds
    of the c that no feature row shows."""
    wf, wp = taper(F), taper(P)
    fut = max([0.0] + [c(k + i) * wf[i] for i in range(F + 1)])
    past = max([0.0] + [c(k - i) * wp[i] for i in range(P + 1)])
    carried = max(bc(k + i) * wf[i] for i in range(F + 1)) + max(bc(k - i) * wp[i] for i in range(P + 1))
    v = (fut + past) / 2.0
    return v, 2 * U * v + carried / 2.0


def bin_gate(cur, prev, W):
    """speedy.c:705-714: t = (float)(max_{i>=1} S[k][i] / 100.0) -- a double division stored in a float, which the float64
    division below followed by the cast reproduces bit for bit -- and bin i is kept iff S[k][i] > t && S[k-1][i] > t.  Decided
    exactly on the tap's float32 values."""
    t = float(np.float32(np.max(cur[1:W]) / 100.0))
    keep = np.zeros(cur.shape[0], bool)
    keep[1:W] = (cur[1:W] > t) & (prev[1:W] > t)
    return keep, t


def spectral_difference(cur, prev, W):
    """f6, speedy.c:628-647,711-719: sum over kept bins of |log((n_k[i] + eps) / (n_{k-1}[i] + eps))|, n = S / (sqrt(energy) +
    eps).  Count per kept bin, in units of u relative to the quotient: a normalised float has W/2 + 1 from its energy (the
    float sum of W - 1 squares, (W + 2) u, halved by the square root), 1 from the float inverse_norm and 1 from the float
    product: W/2 + 3, one below the W/2 + 4 of spectrum_ref.normalized_bound; the two of a bin make W + 6.  The two float
    additions of eps and the float quotient are 3 more: W + 9 <= W + 10.  |log| moves by what its argument moves by relatively
    (derivative 1 / argument), and the log itself is taken in double (error far below u).  The g terms are added in double and
    the sum is stored in the float feature after each one: g stores, (g + 1) u f6 with one to spare.
    Bound: g (W + 10) u + (g + 1) u f6."""
    keep, _ = bin_gate(cur, prev, W)
    g = int(keep.sum())
    if g == 0:
        return 0.0, 0.0, 0
    e1, _ = energy(cur, W)
    e0, _ = energy(prev, W)
    n1 = cur[keep] / (math.sqrt(e1) + EPS)
    n0 = prev[keep] / (math.sqrt(e0) + EPS)
    v = float(np.abs(np.log((n1 + EPS) / (n0 + EPS))).sum())
    return v, g * (W + 10) * U + (g + 1) * U * v, g


def weighted(f6, f4):
    """f7, speedy.c:720-721: one float product: u |value|."""
    v = f6 * f4
    return v, U * np.abs(v)


def relative(f7, f8):
    """f9, speedy.c:725-726: f7 / (f8 + 0.01 * mean_lpf); the sum and the quotient are double, the store rounds: 2 u |value|
    has one to spare."""
    v = f7 / (f8 + 0.01 * MEAN_LPF)
    return v, 2 * U * np.abs(v)


def speech_changes(f9):
    """f10, speedy.c:727-728: min(f9, 4 * mean): exact given f9; u |value| allowed."""
    v = np.minimum(f9, CLAMP)
    return v, U * np.abs(v)


def tension(f4, f10):
    """f11, speedy.c:754-761: a (f4 - M_E) + b (f10 - M_S) with float a = 1/2, b = 1/4, M_E = 0.7f, M_S = 1: two float
    differences and one sum round, the scalings are exact: 3 u (|f4| + 0.7 + |f10| + 1)."""
    m_e = float(np.float32(0.7))
    v = 0.5 * (f4 - m_e) + 0.25 * (f10 - 1.0)
    return v, 3 * U * (np.abs(f4) + 0.7 + np.abs(f10) + 1.0)


class SpeedState:
    """speedy.c:768-788 and soniclib.c:339-345 as a float64 recurrence with the bound carried along.

    Without feedback: R + (1 - R) T in float is a difference, a product and a sum, the max / min against 1 and 0.01 are exact and
    1-Lipschitz: 3 u (|R| (1 + |T|) + 1).
    With feedback the float duration sums enter.  After each frame current += frame / speed and desired += frame / R in float: one
    division (u of the term) and one addition (u of the new sum) each, and the term itself moves by frame / speed^2 times the
    speed's own error.  e_cur and e_des below accumulate exactly that, frame by frame, so after k frames they are at most
    k u max(sum) plus the propagated speed error.  The feedback term fmax(0.01, fb (current - desired)) (1-Lipschitz) then adds
    fb (e_cur + e_des) and three roundings (difference, product, the final sum): + 3 u (fb |excess| + |speed|).
    The interpolation speed nl + R (1 - nl) (soniclib.c:344-345) is exact for nl = 1 (the difference is 0, the products are
    speed and 0, the sum is speed): nothing is added there.  Otherwise the difference 1 - nl, the product R (1 - nl) (two
    roundings on that term), the product speed nl and the sum (two on that one, the sum's counted against both) round:
    + 3 u (|speed nl| + |R (1 - nl)|) has one to spare on each term, and the speed's own error arrives scaled by nl."""

    def __init__(self, R, nl, fb):
        self.R, self.nl, self.fb = float(np.float32(R)), float(np.float32(nl)), float(np.float32(fb))
        self.cur = self.des = self.e_cur = self.e_des = 0.0

    def step(self, T):
        R, nl, fb = self.R, self.nl, self.fb
        raw = R + (1.0 - R) * T
        if R > 1.0:
            s = max(1.0, raw)
        else:
            s = max(float(np.float32(MIN_SPEED)), min(1.0, R - (1.0 - R) * T))   # the double 0.01 lands in a float (:771,776)
        b = 3 * U * (abs(R) * (1 + abs(T)) + 1)
        if fb > 0:
            excess = self.cur - self.des
            s = s + max(MIN_SPEED, fb * excess)
            b += fb * (self.e_cur + self.e_des) + 3 * U * (fb * abs(excess) + abs(s))
        term_c, term_d = FRAME_DURATION / s, FRAME_DURATION / R
        self.cur += term_c
        self.des += term_d
        self.e_cur += U * self.cur + U * term_c + FRAME_DURATION / (s * max(s - b, 1e-300)) * b
        self.e_des += U * self.des + U * term_d
        if nl == 1.0:                       # 1 - nl = 0, R * 0 = 0, speed * 1 and speed + 0 are all exact: nothing is added
            return s, b
        v = s * nl + R * (1.0 - nl)
        return v, b * abs(nl) + 3 * U * (abs(s * nl) + abs(R * (1.0 - nl)))


# ---- the free-running chain -------------------------------------------------------------------------------------------

def run(S, R, nl, fb, matlab, t0=1):
    """The whole chain in float64 from spectra alone.  S: [T][>= W] magnitudes, row j = Speedy time j + t0; W bins are used.
    Returns dict(features [K][15], tension [K], speed [K]).  Not compared with an implementation frame by frame (gates may
    legitimately flip); the tests pin it with the reference's own data."""
    S = np.asarray(S, np.float64)
    T, W = S.shape[0], S.shape[1]
    F, P = hysteresis_shape(matlab)
    K = max(0, T + t0 - F)

    def at(t):
        return S[t - t0] if 0 <= t - t0 < T else np.zeros(W)

    e_all, _ = energy(S, W)
    lp, f2a, c = {}, {}, {}
    state = MEAN_ENERGY
    for t in range(t0, t0 + T):
        state, _ = lowpass(e_all[t - t0], state)
        lp[t] = state
        f2a[t] = float(local_energy(e_all[t - t0], state)[0])
        c[t] = float(compressed(f2a[t])[0])
    feat = np.zeros((K, 15))
    speed = np.zeros(K)
    f8 = MEAN_DIFFERENCE
    sp = SpeedState(R, nl, fb)
    for k in range(K):
        r = feat[k]
        r[0] = e_all[k - t0] if 0 <= k - t0 < T else 0.0
        r[1], r[2], r[3], r[12], r[13], r[14] = lp[k + F], f2a[k + F], c[k + F], k + F, k, LOW_THRESHOLD
        r[4], _ = hysteresis(lambda t: c.get(t, 0.0), lambda t: 0.0, k, F, P)
        low = r[0] <= r[14] or k == 0                      # speedy.c:683-692 with skip_frame_count = 1 at the start (:293)
        r[5] = float(low)
        if low:
            f8, _ = lowpass(0.0, f8)
        else:
            r[6] = spectral_difference(at(k), at(k - 1), W)[0]
            r[7] = r[6] * r[4]
            f8, _ = lowpass(r[7], f8)
            r[9] = relative(r[7], f8)[0]
            r[10] = min(r[9], CLAMP)
        r[8] = f8
        r[11] = tension(r[4], r[10])[0]
        speed[k] = sp.step(r[11])[0]
    return dict(features=feat, tension=feat[:, 11].copy(), speed=speed)


def unit_level_frames(x, rate):
    """The frames of the reference's unit-level loop (speedy_test.cc:911-935,483-500): float input, frame t starts at
    round(t * (float)(rate / 100.f)), pre-emphasis carried from window to window (speedy.c:416-425), Hamming window.
    NOT part of the definition and not held to anything by check(): it exists because the reference's tension KAT and its Matlab
    comparison feed Speedy through this loop (a step of 220.5 samples at 22 050 Hz, first frame at time 0), not through the
    shim's framing (spectrum_ref.analysis_frames: a step of 220, first frame at time 1).  The Matlab matrices were made with the
    220.5 step: through the shim's framing the frames drift by 0.7 of a frame over the file and start one later, every best
    delay lands one off and the SNRs fall below the reference's thresholds (spectrogram energy 43 against 2e5), as they would for
    the reference itself.  So the tests that pin run() stand where the reference's own test stands."""
    import spectrum_ref as sr
    x = np.asarray(x, np.float32)
    W = sr.window_size(rate)
    step = np.float32(rate / np.float32(100))
    count = int((x.size - W) / step + 1)
    win = sr.hamming(W)
    out = np.zeros((count, W), np.float32)
    state = np.float32(0.0)
    for t in range(count):
        start = int(math.floor(float(np.float32(t) * step) + 0.5))
        v = x[start:start + W]
        prev = np.concatenate([[state], v[:-1]]).astype(np.float32)
        e = (1.0 * v.astype(np.float64) - 0.97 * prev.astype(np.float64)).astype(np.float32)
        state = v[-1]
        out[t] = e * win
    return out


# ---- the teacher-forced check -----------------------------------------------------------------------------------------

class Table(dict):
    """stage -> dict(ratio = worst error / bound, frame, got, want, bound, n = values checked, low / kept where they apply)."""

    def worst(self):
        s = max(self, key=lambda k: self[k]["ratio"])
        return s, self[s]

    def failures(self):
        return {s: e for s, e in self.items() if not e["ratio"] <= 1.0}

    def checked(self):
        return sum(e["n"] for e in self.values())

    def describe(self, stage, what=""):
        e = self[stage]
        k = e["frame"]
        return "%s stage %s frame %d (mod 16 = %d, mod 512 = %d): got %r, want %r, %.3g bounds off" % (
            what, stage, k, k % 16, k % 512, e["got"], e["want"], e["ratio"])

    def lines(self):
        return ["%-8s %10.4g  at frame %d" % (s, self[s]["ratio"], self[s]["frame"]) for s in STAGES]


class Worst:
    """The worst error / bound per stage and sample rate over many tables, and the frames behind them."""

    def __init__(self):
        self.by_rate, self.frames = {}, {}

    def add(self, rate, table):
        row = self.by_rate.setdefault(rate, dict.fromkeys(STAGES, 0.0))
        for s in STAGES:
            row[s] = max(row[s], table[s]["ratio"])
        self.frames[rate] = self.frames.get(rate, 0) + table["f0"]["n"]

    def text(self):
        rates = sorted(self.by_rate)
        out = ["%-8s" % "stage" + "".join("%9d" % r for r in rates) + "%9s" % "all"]
        for s in STAGES:
            v = [self.by_rate[r][s] for r in rates]
            out.append("%-8s" % s + "".join("%9.3f" % x for x in v) + "%9.3f" % max(v + [0.0]))
        out.append("%-8s" % "frames" + "".join("%9d" % self.frames[r] for r in rates) + "%9d" % sum(self.frames.values()))
        return "\n".join(out)


def _ratio(got, want, bound):
    err = abs(got - want)
    if err == 0.0:
        return 0.0
    if not err <= bound:                  # nan included
        return math.inf if bound == 0.0 or err != err else err / bound
    return err / bound


def check(taps, rate, R, nl, fb, matlab, t0=1):
    """taps: dict(spectrogram [T][>= W], features [K][15], tension [K], speed [K]) of float32 values of ONE stream.  Every stage
    of every feature row is compared with the definition fed with the taps of the stage before.  Returns the Table; the caller
    asserts table.failures() == {} and table.checked() == K * len(STAGES).  Nothing is left out: rows whose inputs lie before
    the first feature row are computed from the spectrogram tap, free-running from the start states, with the bound of those
    few steps carried along."""
    import spectrum_ref as sr
    W = sr.window_size(rate)
    F, P = hysteresis_shape(matlab)
    spec = np.asarray(taps["spectrogram"], np.float32).astype(np.float64)
    f = np.asarray(taps["features"], np.float32).astype(np.float64)
    ten = np.asarray(taps["tension"], np.float32)
    spd = np.asarray(taps["speed"], np.float32).astype(np.float64)
    T = spec.shape[0]
    K = max(0, T + t0 - F)
    assert f.shape == (K, 15) and ten.shape == (K,) and spd.shape == (K,), (f.shape, ten.shape, spd.shape, T, K)
    zero = np.zeros(spec.shape[1] if T else W)

    def at(t):
        return spec[t - t0] if 0 <= t - t0 < T else zero

    e_sp, be_sp = energy(spec, W) if T else (np.zeros(0), np.zeros(0))

    # times t0 .. F - 1 lie before every feature row: the energy filter's state and the compressed energies of those times,
    # free-running from the spectrogram tap and the start state (speedy.c:287-289), bounds carried step by step
    state, b_state = MEAN_ENERGY, 0.0
    c_early, bc_early = {}, {}
    for t in range(t0, min(F, t0 + T)):
        e, be = e_sp[t - t0], be_sp[t - t0]
        state, b3 = lowpass(e, state)
        b_state = b3 + (1.0 - ALPHA) * be + ALPHA * b_state
        f2, b2 = local_energy(e, state)
        b2 = b2 + (be / state + f2 * b_state / state) * (1 + 1e-3)           # quotient rule, second order inside the 1e-3
        c_early[t], b3c = compressed(f2)
        # d sqrt(min(x, 2)) <= dx / (2 sqrt(x)); at x = 0 the value itself bounds the move: sqrt(b2)
        bc_early[t] = b3c + (min(b2 / (2 * c_early[t]), math.sqrt(b2)) if c_early[t] > 0 else math.sqrt(b2))

    def c(t):
        if t >= F:
            return f[t - F, 3]
        return c_early.get(t, 0.0)

    def bc(t):
        return 0.0 if t >= F else bc_early.get(t, 0.0)

    table = Table((s, dict(ratio=0.0, frame=0, got=None, want=None, bound=None, n=0)) for s in STAGES)
    table.low_frames, table.after_low, table.clamped, table.max_kept, table.f2_limited = 0, 0, 0, 0, 0

    def put(stage, k, got, want, bound):
        e = table[stage]
        e["n"] += 1
        r = _ratio(float(got), float(want), float(bound))
        if e["got"] is None or r > e["ratio"]:
            e.update(ratio=r, frame=k, got=float(got), want=float(want), bound=float(bound))

    sp = SpeedState(R, nl, fb)
    prev_low = False
    for k in range(K):
        r = f[k]
        # f0
        want, b = (e_sp[k - t0], be_sp[k - t0]) if 0 <= k - t0 < T else (0.0, 0.0)
        put("f0", k, r[0], want, b)
        # f1, f2, f3, time stamps: made at time k + F from that frame's energy
        if k + F < K:
            e, be = f[k + F, 0], 0.0
        else:
            e, be = e_sp[k + F - t0], be_sp[k + F - t0]
        prev, bprev = (f[k - 1, 1], 0.0) if k >= 1 else (state, b_state)
        want, b = lowpass(e, prev)
        put("f1", k, r[1], want, b + (1.0 - ALPHA) * be + ALPHA * bprev)
        want, b = local_energy(e, r[1])
        put("f2", k, r[2], want, b + (be / r[1] if be else 0.0))
        want, b = compressed(r[2])
        put("f3", k, r[3], want, b)
        table.f2_limited += r[2] > 2.0
        put("f12", k, r[12], k + F, 0.0)
        put("f13", k, r[13], k, 0.0)
        # f4
        want, b = hysteresis(c, bc, k, F, P)
        put("f4", k, r[4], want, b)
        # the low-energy gate, decided on the row's own float32 f0 and f14
        put("f14", k, r[14], LOW_THRESHOLD, 0.0)
        low = bool(r[0] <= r[14]) or k == 0
        put("f5", k, r[5], float(low), 0.0)
        prev8 = f[k - 1, 8] if k >= 1 else MEAN_DIFFERENCE
        if low:
            table.low_frames += 1
            for i in (6, 7, 9, 10):
                put("f%d" % i, k, r[i], 0.0, 0.0)
            want, b = lowpass(0.0, prev8)
            put("f8", k, r[8], want, b)
        else:
            table.after_low += prev_low
            want, b, g = spectral_difference(at(k), at(k - 1), W)
            table.max_kept = max(table.max_kept, g)
            put("f6", k, r[6], want, b)
            want, b = weighted(r[6], r[4])
            put("f7", k, r[7], want, b)
            want, b = lowpass(r[7], prev8)
            put("f8", k, r[8], want, b)
            want, b = relative(r[7], r[8])
            put("f9", k, r[9], want, b)
            want, b = speech_changes(r[9])
            put("f10", k, r[10], want, b)
            table.clamped += r[9] > CLAMP
        prev_low = low
        want, b = tension(r[4], r[10])
        put("f11", k, r[11], want, b)
        same = ten[k].tobytes() == np.float32(r[11]).tobytes()                # the tap IS f11 (soniclib.c:320-329)
        put("tension", k, float(ten[k]) if same else math.nan, r[11], 0.0)
        want, b = sp.step(float(ten[k]))
        put("speed", k, spd[k], want, b)
    return table
