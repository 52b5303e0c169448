"""Row tracks through an edit list -- labels, flags and feature rows warped to the output's time and back -- as exact integers and
np.float32 scalars: test infrastructure, CPU only.

include/speedy_hip.h "EDIT LIST, ROW TRACKS" words what spx_edit_rows, spx_edit_warp_rows and spx_edit_unwarp_rows compute; this file
states it on Python integers, beside tests/edit_lookup_ref.py, whose L, n_out, src, forward and inverse it takes.

A row track has hop H >= 1 key frames per row and a phase 0 <= phi < H: row j describes key frames [j H, (j + 1) H) and frame
j H + phi stands for it.
  rows(x) = (x - phi + H - 1) // H for x > phi, else 0: the rows whose representative frame lies below x
  row_of(s) = s // H, or ZERO (a row of zero bytes) where s < 0, s >= L or s // H >= the track's n_rows

  warp     no = min(n_out, the key's out_cap); rows(no) rows.  Row j: u = j H + phi, k = the largest k with out_at(k) <= u,
           t = u - out_at(k).
             NEAREST   row_of(src(record k, t))
             BLEND     a copy record: NEAREST.  A cross-fade: ra = row_of(a + t), rb = row_of(b + t); ra == rb (the same row, or ZERO
                       twice): that row, bit for bit; else per element ((ya * f32(n - t)) + (yb * f32(t))) / f32(n), every operation
                       rounded to float32
  unwarp   rows(L) rows.  Row r: p = r H + phi, (o, k) = forward(p); ZERO where k = -1, else row o // H of the track, ZERO where that
           is >= n_rows.

warp_plan / unwarp_plan are the definition: per output row, what it is made of -- (ra, rb, t, n), ra and rb row indices or -1 for
ZERO, rb None where the row is not a blend.  render applies a plan to a track with numpy (a gather; float32 arrays round every
operation as the scalars do); blend_scalar is the cross-fade one np.float32 scalar at a time, and
tests/test_edit_rows_definition.py holds render to it.

SWITCHES make one mistake each:
  phase_ignored     u = j H (and p = r H): the phase plays no part in the position
  round_to_row      a source is rounded to the nearest row, (s + H // 2) // H, instead of floored
  pad_clamped       a source at or behind L, or a row at or behind n_rows, reads the track's last row instead of zeros
  no_same_row       ra == rb goes through the cross-fade arithmetic
  fma               the cross-fade's sum takes the product ya * (n - t) unrounded (a fused multiply-add)
  rows_plus_one     rows(x) counts the rows whose representative lies at or below x: one more at x = phi + m H
"""
import bisect

import numpy as np

import edit_lookup_ref as K

SWITCHES = ("phase_ignored", "round_to_row", "pad_clamped", "no_same_row", "fma", "rows_plus_one")
MAX_HOP, MAX_DIM = 1 << 20, 65536
_F = np.float32


def rows(x, H, phi, switch=None):
    if switch == "rows_plus_one":
        return (x - phi) // H + 1 if x >= phi else 0
    return (x - phi + H - 1) // H if x > phi else 0


def rows_api(x, H, phi):
    """spx_edit_rows: rows(x), -1 for arguments that are refused."""
    if x < 0 or H < 1 or H > MAX_HOP or phi < 0 or phi >= H:
        return -1
    return rows(x, H, phi)


def row_of(s, H, L, n_rows, switch=None):
    """The track's row that holds source frame s, -1 for a row of zeros."""
    r = (s + H // 2) // H if switch == "round_to_row" else s // H
    if s < 0:
        return -1
    if s >= L or r >= n_rows:
        return n_rows - 1 if switch == "pad_clamped" and n_rows > 0 else -1
    return r


def count(unwarp, n_out, key_cap, n_ops, ops_cap, L, H, phi, out_cap):
    """n_rows_out of a stream: the rows written, minus that where the track's capacity does not hold them, 0 for a dead stream."""
    if n_ops <= 0 or n_ops > ops_cap or (n_out < 0 if unwarp else n_out <= 0):
        return 0
    R = rows(L if unwarp else max(0, min(n_out, key_cap)), H, phi)
    return -R if R > out_cap else R


def warp_plan(ops, no, L, H, phi, n_rows, blend=False, switch=None):
    """[(ra, rb, t, n)] for the rows(no) output rows of a warp."""
    assert switch is None or switch in SWITCHES, switch
    ops = [tuple(int(v) for v in op) for op in ops]
    out_at = [op[0] for op in ops]
    plan = []
    for j in range(rows(no, H, phi, switch)):
        u = j * H + (0 if switch == "phase_ignored" else phi)
        k = max(bisect.bisect_right(out_at, u) - 1, 0)
        _, a, b, n = ops[k]
        t = u - out_at[k]
        if not blend or b < 0:
            plan.append((row_of(K.src(ops[k], t), H, L, n_rows, switch), None, 0, 1))
            continue
        ra, rb = row_of(a + t, H, L, n_rows, switch), row_of(b + t, H, L, n_rows, switch)
        plan.append((ra, None, 0, 1) if ra == rb and switch != "no_same_row" else (ra, rb, t, n))
    return plan


def unwarp_plan(ops, no, L, H, phi, n_rows, switch=None):
    """[(ra, None, 0, 1)] for the rows(L) output rows of an unwarp."""
    assert switch is None or switch in SWITCHES, switch
    m = K.Lookup(ops, no, L)
    plan = []
    for r in range(rows(L, H, phi, switch)):
        o, k = m.forward(r * H + (0 if switch == "phase_ignored" else phi))
        if k < 0:
            plan.append((-1, None, 0, 1))
            continue
        q = (o + H // 2) // H if switch == "round_to_row" else o // H
        if q >= n_rows:
            q = n_rows - 1 if switch == "pad_clamped" and n_rows > 0 else -1
        plan.append((q, None, 0, 1))
    return plan


def blend_scalar(ya, yb, t, n, switch=None):
    """One element of a cross-fade row, np.float32 scalars, one operation at a time."""
    with np.errstate(all="ignore"):
        ya, yb = _F(ya), _F(yb)
        up = yb * _F(t)
        if switch == "fma":
            return _F(_F(np.float64(ya) * np.float64(_F(n - t)) + np.float64(up)) / _F(n))
        down = ya * _F(n - t)
        return (down + up) / _F(n)


def render(plan, track, dim, switch=None):
    """The plan applied to a (n_rows, >= dim) array: a (len(plan), dim) array of the track's dtype."""
    track = np.asarray(track)
    out = np.zeros((len(plan), dim), track.dtype)
    if not plan:
        return out
    ra = np.asarray([p[0] for p in plan], np.int64)
    plain = np.asarray([p[1] is None for p in plan])
    pick = plain & (ra >= 0)
    out[pick] = track[ra[pick], :dim]
    mix = np.nonzero(~plain)[0]
    if mix.size:
        assert track.dtype == _F
        rb = np.asarray([plan[i][1] for i in mix], np.int64)
        t = np.asarray([plan[i][2] for i in mix], np.int64)
        n = np.asarray([plan[i][3] for i in mix], np.int64)
        ya, yb = np.zeros((mix.size, dim), _F), np.zeros((mix.size, dim), _F)
        ya[ra[mix] >= 0] = track[ra[mix][ra[mix] >= 0], :dim]
        yb[rb >= 0] = track[rb[rb >= 0], :dim]
        with np.errstate(all="ignore"):
            up = yb * t.astype(_F)[:, None]
            if switch == "fma":
                v = (ya.astype(np.float64) * (n - t).astype(_F).astype(np.float64)[:, None] + up.astype(np.float64)).astype(_F)
            else:
                v = ya * (n - t).astype(_F)[:, None] + up
            v = v / n.astype(_F)[:, None]
        assert v.dtype == _F
        out[mix] = v
    return out


def warp(ops, no, L, H, phi, track, dim, blend=False, switch=None):
    return render(warp_plan(ops, no, L, H, phi, len(track), blend, switch), track, dim, switch)


def unwarp(ops, no, L, H, phi, track, dim, switch=None):
    return render(unwarp_plan(ops, no, L, H, phi, len(track), switch), track, dim, switch)
