"""The time map's definition, on the CPU (include/speedy_hip.h "TIME MAP"): the oracle's rows, and the lookups in numpy int64 and
-- ExactMap, forward_exact, inverse_exact -- in Python integers, written from the header's text and not from the numpy functions
(tests/test_time_map_lookup_definition.py asserts that the two agree inside the domain).  The rows' own definition, which reads
no oracle, is tests/tsm_ref.py's (nonlinear_job(...).rows).

Rows.  The oracle stream is observed, not changed: orc_sonicHandoffCallback fires when ring buffer k is about to be handed to the
time-scale stage, and inside the callback orc_sonicIntSamplesAvailable is the number of output frames produced so far (no audio is
read before the end, so the count is the running total).  After orc_sonicFlushStream the count is read once more: the last row."""
import bisect

import numpy as np

# the shapes the definition was pinned on: (sample rate, channels, speed, nonlinear, n_in)
SHAPES = [
    (16000, 1, 3.5, 1.0, 4000),
    (16000, 1, 0.5, 1.0, 8000),
    (22050, 2, 1.5, 1.0, 11025),
    (16000, 1, 2.0, 0.5, 3200),
    (11025, 1, 3.0, 1.0, 5512),
    (16000, 1, 3.0, 1.0, 159),
    (16000, 1, 3.0, 1.0, 160),
    (16000, 1, 2.0, 0.0, 4000),   # linear: no callback, one row
]


def signal(rate_hz, ch, n, seed=900):
    """n frames of speech-like audio, interleaved."""
    from speedy_amd.synth import speech_like
    if n == 0:
        return np.zeros(0, np.int16)
    return np.stack([speech_like(n, rate_hz, seed=seed + 7 * c) for c in range(ch)], axis=1).reshape(-1).astype(np.int16)


def oracle_map(orc, x, rate_hz, ch, speed, nl, mm=False, feedback=0.0, chunk=None):
    """(rows int64, callback times, output int16) of one job: written in pieces of `chunk` frames (None: one piece), flushed."""
    L = orc.lib()
    x = np.ascontiguousarray(x, np.int16)
    n = x.size // ch
    h = L.orc_sonicCreateStream(int(rate_hz), int(ch), int(bool(mm)))
    assert h
    L.orc_sonicSetSpeed(h, float(speed))
    L.orc_sonicEnableNonlinearSpeedup(h, float(nl))
    L.orc_sonicSetDurationFeedbackStrength(h, float(feedback))
    rows, times = [], []

    def on_handoff(s, t, _speed, _buf, _frames):
        times.append(int(t))
        rows.append(int(L.orc_sonicIntSamplesAvailable(s)))

    cb = orc.HANDOFF_FN(on_handoff)
    L.orc_sonicHandoffCallback(h, cb)
    step = n if not chunk else int(chunk)
    for pos in range(0, n, max(1, step)):
        seg = np.ascontiguousarray(x[pos * ch:(pos + step) * ch])
        assert L.orc_sonicWriteShortToStream(h, orc.sptr(seg), seg.size // ch) == 1
    assert L.orc_sonicFlushStream(h) == 1
    total = int(L.orc_sonicIntSamplesAvailable(h))
    rows.append(total)
    out = np.zeros(max(1, total) * ch, np.int16)
    got = L.orc_sonicReadShortFromStream(h, orc.sptr(out), total) if total else 0
    assert got == total
    L.orc_sonicDestroyStream(h)
    return np.asarray(rows, np.int64), times, out[:total * ch].copy()


def map_rows(B, n_in, nl):
    return n_in // B + 1 if nl != 0 else 1


def nodes(M, B, n_in, nl):
    """(X, Y) int64: the nodes the lookups interpolate between."""
    M = np.asarray(M, np.int64)
    R = n_in // B if nl != 0 else 0
    if R >= 1:
        assert M.size == R + 1
        return np.concatenate([np.arange(R, dtype=np.int64) * B, [n_in]]).astype(np.int64), M.copy()
    assert M.size == 1
    return np.asarray([0, n_in], np.int64), np.asarray([0, M[0]], np.int64)


class ExactMap:
    """The lookups in Python integers (unbounded; // on non-negative operands; bisect_right), written from the text of
    include/speedy_hip.h "TIME MAP" and from nothing else:
      Nodes: X = [0, B, .., (R-1)B, n_in], Y = M for R >= 1;  X = [0, n_in], Y = [0, M[0]] for R = 0.  L = the number of nodes.
      forward  t clamped to [0, n_in]; n_in = 0 gives 0; else j = min(t / B, L - 2) and
               Y[j] + (t - X[j]) * (Y[j+1] - Y[j]) / (X[j+1] - X[j])
      inverse  u clamped to [0, Y[L-1]]; u >= Y[L-1] gives n_in; else j = the largest index with Y[j] <= u and
               X[j] + (u - Y[j]) * (X[j+1] - X[j]) / (Y[j+1] - Y[j])
    R = n_in / B for a nonlinear job, 0 for a linear one.  The rows must not decrease and must not be negative."""

    def __init__(self, M, B, n_in, nl):
        M = [int(v) for v in M]
        self.B, self.n_in = int(B), int(n_in)
        R = self.n_in // self.B if nl != 0 else 0
        if R >= 1:
            assert len(M) == R + 1
            self.X, self.Y = [k * self.B for k in range(R)] + [self.n_in], M
        else:
            assert len(M) == 1
            self.X, self.Y = [0, self.n_in], [0, M[0]]
        assert all(a <= b for a, b in zip(self.Y, self.Y[1:])) and self.Y[0] >= 0, "rows outside the definition"
        self.L = len(self.X)

    def forward(self, t):
        t = min(max(int(t), 0), self.n_in)
        if self.n_in == 0:
            return 0
        X, Y = self.X, self.Y
        j = min(t // self.B, self.L - 2)
        return Y[j] + (t - X[j]) * (Y[j + 1] - Y[j]) // (X[j + 1] - X[j])

    def inverse(self, u):
        X, Y = self.X, self.Y
        u = min(max(int(u), 0), Y[-1])
        if u >= Y[-1]:
            return self.n_in
        j = bisect.bisect_right(Y, u) - 1
        return X[j] + (u - Y[j]) * (X[j + 1] - X[j]) // (Y[j + 1] - Y[j])

    def largest_product(self):
        """The largest value either product can take over all queries: max over segments of width x rise (the domain's bound)."""
        return max((self.X[j + 1] - self.X[j]) * (self.Y[j + 1] - self.Y[j]) for j in range(self.L - 1))


def forward_exact(M, B, n_in, nl, t):
    """Input frame -> output frame for every t of a sequence, as a list of Python integers."""
    m = ExactMap(M, B, n_in, nl)
    return [m.forward(v) for v in t]


def inverse_exact(M, B, n_in, nl, u):
    """Output frame -> input frame for every u of a sequence, as a list of Python integers."""
    m = ExactMap(M, B, n_in, nl)
    return [m.inverse(v) for v in u]


def forward(M, B, n_in, nl, t):
    """Input frame -> output frame, elementwise over t (int64, floor division)."""
    X, Y = nodes(M, B, n_in, nl)
    t = np.clip(np.asarray(t, np.int64), 0, n_in)
    if n_in == 0:
        return np.zeros_like(t)
    j = np.minimum(t // B, X.size - 2)
    return Y[j] + (t - X[j]) * (Y[j + 1] - Y[j]) // (X[j + 1] - X[j])


def inverse(M, B, n_in, nl, u):
    """Output frame -> input frame, elementwise over u."""
    X, Y = nodes(M, B, n_in, nl)
    u = np.clip(np.asarray(u, np.int64), 0, Y[-1])
    res = np.full(u.shape, n_in, np.int64)
    inside = u < Y[-1]
    ui = u[inside]
    j = np.searchsorted(Y, ui, side="right") - 1    # the largest index with Y[j] <= u (Y is non-decreasing, Y[0] = 0)
    dy = Y[j + 1] - Y[j]
    assert (dy > 0).all()
    res[inside] = X[j] + (ui - Y[j]) * (X[j + 1] - X[j]) // dy
    return res
