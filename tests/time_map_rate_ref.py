"""The time map of a call with playback rates, on the CPU (include/speedy_hip.h "TIME MAP", "WITH PLAYBACK RATES, AND ON FLOAT
SAMPLES"): rate_pair and F written from the header's text, and the oracle's rows -- time_map_ref.oracle_map's observer with
orc_sonicSetRate set before the first write, on int16 and on float input.

The header's words: (new, old) = (int)(sample rate / rate) computed in float and the sample rate, halved together until both fit
14 bits; F(m) = 0 for m < 2, else ((m - 1) * new + old - 1) / old -- the frames behind the rate stage after m frames of the speed
stage.  Row k < R of a job with a rate other than 1 is F(the row spx_batch_run_map writes), the last row is the job's final count."""
import numpy as np

import time_map_ref as tm

RATES = (0.5, 0.75, 1.3, 2.0, 3.0)
CHUNKINGS = (None, 160, 1000)
# time_map_ref.SHAPES' fields and the feedback strength: those shapes, a slow-down with feedback that has 301 rows, an empty job
SHAPES = [s + (0.0,) for s in tm.SHAPES] + [(16000, 1, 0.8, 1.0, 48000, 0.1), (16000, 1, 3.5, 1.0, 0, 0.0)]


def rate_pair(rate_hz, rate):
    """(new, old) of a playback rate: Python integers."""
    new, old = int(np.float32(rate_hz) / np.float32(rate)), int(rate_hz)
    while new > (1 << 14) or old > (1 << 14):
        new >>= 1
        old >>= 1
    return new, old


def F(m, new, old):
    """Frames behind the rate stage after m frames of the speed stage (Python integers)."""
    m = int(m)
    return 0 if m < 2 else ((m - 1) * new + old - 1) // old


def convert_rows(rows, rate_hz, rate, total):
    """The rows of a job with a rate other than 1, from the rows spx_batch_run_map writes for it and the job's final count."""
    new, old = rate_pair(rate_hz, rate)
    return np.asarray([F(m, new, old) for m in rows[:-1]] + [int(total)], np.int64)


def _observe(orc, x, rate_hz, ch, speed, nl, fb, rate, chunk, mm, as_float):
    L = orc.lib()
    n = x.size // ch
    h = L.orc_sonicCreateStream(int(rate_hz), int(ch), int(bool(mm)))
    assert h
    L.orc_sonicSetSpeed(h, float(speed))
    if rate is not None:
        L.orc_sonicSetRate(h, float(rate))
    L.orc_sonicEnableNonlinearSpeedup(h, float(nl))
    L.orc_sonicSetDurationFeedbackStrength(h, float(fb))
    rows, times = [], []

    def on_handoff(s, t, _speed, _buf, _frames):
        times.append(int(t))
        rows.append(int(L.orc_sonicIntSamplesAvailable(s)))

    cb = orc.HANDOFF_FN(on_handoff)
    L.orc_sonicHandoffCallback(h, cb)
    write, ptr = (L.orc_sonicWriteFloatToStream, orc.fptr) if as_float else (L.orc_sonicWriteShortToStream, orc.sptr)
    step = n if not chunk else int(chunk)
    for pos in range(0, n, max(1, step)):
        seg = np.ascontiguousarray(x[pos * ch:(pos + step) * ch])
        assert write(h, ptr(seg), seg.size // ch) == 1
    assert L.orc_sonicFlushStream(h) == 1
    total = int(L.orc_sonicIntSamplesAvailable(h))
    rows.append(total)
    L.orc_sonicDestroyStream(h)
    assert times == list(range(len(times)))
    return np.asarray(rows, np.int64)


def oracle_rate_map(orc, x, rate_hz, ch, speed, nl, fb, rate, chunk, mm=False):
    """The rows (int64) of one job at a playback rate: the oracle stream with orc_sonicSetRate set before the first write (rate None:
    never set), written in pieces of `chunk` frames (None: one piece), flushed; the count inside each hand-off callback, then the
    stream's total.  Final frames: what the stream offers its reader."""
    return _observe(orc, np.ascontiguousarray(x, np.int16), rate_hz, ch, speed, nl, fb, rate, chunk, mm, False)


def oracle_rate_map_float(orc, x, rate_hz, ch, speed, nl, fb, rate, chunk, mm=False):
    """The same observer on float input (orc_sonicWriteFloatToStream)."""
    return _observe(orc, np.ascontiguousarray(x, np.float32), rate_hz, ch, speed, nl, fb, rate, chunk, mm, True)
