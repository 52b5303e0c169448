"""The replay of an edit list on a track at a higher sample rate, as exact integers -- test infrastructure, CPU only.

include/speedy_hip.h "EDIT LIST, SCALED" words what spx_edit_replay_scaled computes; this file states it in Python integers (and, for
the float cross-fade, in np.float32 scalars one operation at a time), beside tests/edit_list_ref.py, whose records it takes.

With p / q the master's rate over the key's, reduced by its gcd, 1 <= q <= p <= 32 q and p <= 32768:
  S(x) = floor(x p / q)
  no = min(n_out, the key's out_cap),  N' = S(no),  L' = min(S(L), the track's own n_in)
  record (out_at, a, b, n) covers master frames [S(out_at), S(out_at + n)) cut at N':
      n' = S(out_at + n) - S(out_at) >= 1,  a' = S(a),  b' = S(b),  t = o - S(out_at)
  a source frame outside [0, L') reads as 0 (+0.0f)
  copy                 y[a' + t]
  cross-fade, int16    (y[a' + t] (n' - t) + y[b' + t] t) / n', truncated toward zero (tsm_ref.tdiv)
  cross-fade, float    ((ya * float(n' - t)) + (yb * float(t))) / float(n'), every operation rounded to float32

replay_scaled is the definition.  replay_scaled_np computes the same values a record at a time with numpy (int64 is exact here:
|y| <= 2^15 and n' < 2^31; float32 arrays round every operation as the scalars do); tests/test_edit_scaled_definition.py holds it to
the definition, and tests/test_gpu_edit_scaled.py uses it where the definition would take minutes.

SWITCHES make one mistake each:
  scale_n        n' = S(n): the length is scaled instead of the record's two ends
  shared_floor   b' = a' + S(b - a): one floor for both ramps instead of one each
  limit_no_min   L' = S(L), whatever the track's own length is
"""
import math

import numpy as np

import tsm_ref as T

SWITCHES = ("scale_n", "shared_floor", "limit_no_min")
RATIOS = ((1, 1), (2, 1), (3, 1), (441, 160), (320, 147))
MAX_P, MAX_RATIO = 32768, 32
_F = np.float32


def ratio(p, q):
    """(p, q) reduced by its gcd, or None for a ratio the call refuses."""
    if p < 1 or q < 1:
        return None
    g = math.gcd(p, q)
    p, q = p // g, q // g
    if p < q or p > MAX_RATIO * q or p > MAX_P:
        return None
    return p, q


def S(x, p, q):
    return x * p // q


def scale(x, p, q):
    """spx_edit_scale: S(x), -1 for a ratio that is refused or x < 0."""
    r = ratio(p, q)
    if r is None or x < 0:
        return -1
    return S(x, *r)


def scaled_ops(ops, p, q, switch=None):
    """The records at the master's rate: (S(out_at), a', b' or -1, n')."""
    assert switch is None or switch in SWITCHES, switch
    out = []
    for out_at, a, b, n in ops:
        at = S(out_at, p, q)
        n2 = S(n, p, q) if switch == "scale_n" else S(out_at + n, p, q) - at
        a2 = S(a, p, q)
        if b < 0:
            b2 = -1
        elif switch == "shared_floor":
            b2 = a2 + S(b - a, p, q)
        else:
            b2 = S(b, p, q)
        out.append((at, a2, b2, n2))
    return out


def tiles(ops, p, q, no):
    """The scaled extents, cut at N' = S(no), tile [0, N') and every n' is at least 1."""
    Np, at = S(no, p, q), 0
    for at2, _, _, n2 in scaled_ops(ops, p, q):
        if n2 < 1 or at2 != at:
            return False
        at += n2
    return at >= Np


def count(n_out, key_cap, n_ops, ops_cap, p, q, out_cap):
    """n_out_y of a stream: N', -N' where the track's capacity does not hold it, 0 where there is nothing to render."""
    if n_out <= 0 or n_ops <= 0 or n_ops > ops_cap:
        return 0
    Np = S(max(0, min(n_out, key_cap)), p, q)
    return -Np if Np > out_cap else Np


def limit(L, n_in, p, q, switch=None):
    return S(L, p, q) if switch == "limit_no_min" else min(S(L, p, q), n_in)


def replay_scaled(ops, y, channels, L, no, p, q, n_in, fmt="int16", switch=None):
    """The track y (interleaved; n_in frames of it count) under the list at p / q: N' = S(no) frames as a flat list -- Python integers
    for fmt "int16", np.float32 scalars for "float".  A value no record covers stays None."""
    assert fmt in ("int16", "float") and ratio(p, q) == (p, q)
    C, flt = channels, fmt == "float"
    Np, Lp = S(no, p, q), limit(L, n_in, p, q, switch)
    if flt:
        y = np.asarray(y, _F)
        zero = _F(0)
    else:
        y = y.tolist() if isinstance(y, np.ndarray) else y
        zero = 0
    out = [None] * (Np * C)
    with np.errstate(all="ignore"):
        for at, a, b, n in scaled_ops(ops, p, q, switch):
            for t in range(max(0, min(n, Np - at))):
                for c in range(C):
                    va = y[(a + t) * C + c] if 0 <= a + t < Lp else zero
                    if b < 0:
                        v = va
                    else:
                        vb = y[(b + t) * C + c] if 0 <= b + t < Lp else zero
                        if flt:
                            down = va * _F(n - t)
                            up = vb * _F(t)
                            v = (down + up) / _F(n)
                        else:
                            v = T.tdiv(va * (n - t) + vb * t, n)
                    out[(at + t) * C + c] = v
    return out


def replay_scaled_np(ops, y, channels, L, no, p, q, n_in, fmt="int16"):
    """replay_scaled's values, a record at a time: an int64 or float32 array of N' * channels values (a frame no record covers: 0)."""
    assert fmt in ("int16", "float") and ratio(p, q) == (p, q)
    C, flt = channels, fmt == "float"
    Np, Lp = S(no, p, q), limit(L, n_in, p, q)
    y = np.asarray(y, _F if flt else np.int64)
    Y = y[:y.size // C * C].reshape(-1, C)
    assert Y.shape[0] >= Lp
    out = np.zeros((Np, C), Y.dtype)

    def run(s, t):
        idx = s + t
        ok = (idx >= 0) & (idx < Lp)
        v = np.zeros((t.size, C), Y.dtype)
        v[ok] = Y[idx[ok]]
        return v

    with np.errstate(all="ignore"):
        for at, a, b, n in scaled_ops(ops, p, q):
            m = min(n, Np - at)
            if m <= 0:
                continue
            t = np.arange(m, dtype=np.int64)
            va = run(a, t)
            if b < 0:
                v = va
            else:
                vb = run(b, t)
                if flt:
                    down = va * (n - t).astype(_F)[:, None]
                    up = vb * t.astype(_F)[:, None]
                    v = (down + up) / _F(n)
                    assert v.dtype == _F
                else:
                    num = va * (n - t)[:, None] + vb * t[:, None]
                    v = np.sign(num) * (np.abs(num) // n)
            out[at:at + m] = v
    return out.reshape(-1)


def bits(values):
    """Float values as their 32 bits (uint32): what the comparisons with the device compare."""
    return np.asarray(values, _F).view(np.uint32)
