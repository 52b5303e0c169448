"""The two-pass batch call's arithmetic (include/speedy_hip.h: spx_batch_run_twopass) as a numpy definition -- every operation one
IEEE operation on an explicit type, in the order of the two-pass drivers of tools/speedy_wave_hip.cpp:179-191 -- and the inputs the
tests of the call share: the segments of tapestry.wav and the targets."""
import numpy as np

# input segments of tapestry.wav (whole file, then slices) and the speed-ups the length targets are made of
SEGMENTS = [(None, None), (0, 16000), (8000, 20000), (0, 6000)]
FACTORS = [1.5, 2.0, 3.5]


def segment(x, seg):
    a, b = seg
    return x if a is None else x[a:b]


def want_of(n_in, rate, seconds, speed):
    """The probe pass's speed as a double: LENGTH (seconds > 0) (double)((float)T / (float)rate) / seconds, MATCH the job's float speed."""
    if seconds > 0:
        return np.float64(np.float32(int(n_in)) / np.float32(int(rate))) / np.float64(seconds)
    return np.float64(np.float32(speed))


def second_speed(want, length_mode, n_in, n_probe):
    """speeds[i] as a float32: n_probe <= 0 -> (float)want; got = (double)T / (double)n_probe; MATCH (float)got; LENGTH
    (float)(want * (want / got))."""
    want = np.float64(want)
    with np.errstate(all="ignore"):
        if int(n_probe) <= 0:
            return np.float32(want)
        got = np.float64(int(n_in)) / np.float64(int(n_probe))
        if not length_mode:
            return np.float32(got)
        return np.float32(want * (want / got))


def bits(v):
    return np.asarray(v, np.float32).view(np.uint32)
