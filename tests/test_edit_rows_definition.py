"""CPU-only: the definition of row tracks through an edit list (tests/edit_rows_ref.py: spx_edit_rows, spx_edit_warp_rows,
spx_edit_unwarp_rows), and its C ABI.

The lists: the planted ones of tests/test_gpu_edit_lookup.py (SHAPES in its five streams, the six synthetic kinds -- imported, not
copied) and tests/edit_list_ref.py's lists of the directed linear jobs of tests/tsm_inputs.py at 16 and 22.05 kHz.  For every row of
every list the plan of edit_rows_ref is held to the answer derived from an ENUMERATION of the source of every output frame
(edit_lookup_ref.Lookup.brute_inverse_all / brute_forward_all); its numpy rendering is held to np.float32 scalars; every switch of
edit_rows_ref (one mistake each) changes an answer on these inputs; and two identities tie the definition to entry points that are
already pinned: at hop 1 the NEAREST warp is a gather by Lookup.inverse, and the BLEND warp is edit_scaled_ref's float replay at
p = q = 1."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_list_ref as E  # noqa: E402
import edit_lookup_ref as K  # noqa: E402
import edit_rows_ref as W  # noqa: E402
import edit_scaled_ref as S  # noqa: E402
import test_gpu_edit_lookup as GL  # noqa: E402  (SHAPES, synthetic, kinds: the planted lists, imported)
import tsm_inputs as I  # noqa: E402

NEW = ["spx_edit_rows", "spx_edit_warp_rows", "spx_edit_unwarp_rows", "spx_debug_last_rows_grid"]
HOPS = [(1, 0), (2, 0), (2, 1), (3, 1), (7, 6), (160, 0), (160, 80), (160, 159), (320, 160)]


def planted():
    """{name: (ops, no, L)}: SHAPES in the streams of the lookup's record-shape test, and its six synthetic kinds."""
    ops = np.asarray(GL.SHAPES, np.int32)
    total = int(ops[-1][0] + ops[-1][3])
    out = {}
    for name, s in [("shapes", GL.stream(ops, 4000, total)), ("shapes_cut_inside", GL.stream(ops, 4000, 60)),
                    ("shapes_cut_before", GL.stream(ops, 4000, 65)), ("shapes_L_below", GL.stream(ops, 1999, total, nl=1.0))] + GL.kinds():
        m = GL.ref(s)
        out[name] = (m.ops, m.n_out, m.L)
    return out


@pytest.fixture(scope="module")
def real():
    """{name: (ops, no, L)} of the directed linear jobs: computed once, left unchanged."""
    out = {}
    with E.shared_pitch_searches():
        for name, rate, ch, x, speed in I.linear_jobs():
            if rate in (16000, 22050):
                e = E.linear_job(x, rate, ch, speed)
                out[name] = (e.ops, e.out_n, e.limit)
    return out


@pytest.fixture(scope="module")
def lists(real):
    out = dict(planted())
    out.update(real)
    assert len(out) > 200
    return out


def hops_for(name, no):
    """Every hop on the planted lists; on a job's list four of them, where they leave it at least a few rows."""
    return HOPS if "/" not in name else [h for h in ((1, 0), (3, 1), (160, 80), (320, 160)) if h[0] <= max(1, no // 3)]


def track_rows(L, H, short):
    """Rows of a track that covers [0, L) -- or, short, one row fewer than the sources reach."""
    return max(0, -(-L // H) - (1 if short else 0))


def test_rows_counts_the_representatives_below_x():
    for H, phi in HOPS + [(5, 4), (1 << 20, 17)]:
        for x in list(range(0, 40)) + [H - 1, H, H + 1, 3 * H + phi, 3 * H + phi + 1, 10 ** 9]:
            want = sum(1 for j in range(0, min(x // H + 2, 200)) if j * H + phi < x) if x < 150 * H else (x - phi + H - 1) // H
            assert W.rows(x, H, phi) == W.rows_api(x, H, phi) == want, (x, H, phi)
    assert W.rows(80, 160, 80) == 0 and W.rows(81, 160, 80) == 1 and W.rows(240, 160, 80) == 1 and W.rows(241, 160, 80) == 2
    assert [W.rows_api(*a) for a in ((-1, 1, 0), (5, 0, 0), (5, (1 << 20) + 1, 0), (5, 4, 4), (5, 4, -1))] == [-1] * 5


def test_every_row_is_the_enumerations(lists):
    """NEAREST warp: row j is the row of the source the enumeration gives output frame j H + phi.  Unwarp: row r is the row of the
    first output frame whose source is at or above r H + phi.  BLEND: a copy record is NEAREST, and the NEAREST row is one of the two."""
    checked = 0
    for name, (ops, no, L) in lists.items():
        m = K.Lookup(ops, no, L)
        inv, fwd = m.brute_inverse_all(), m.brute_forward_all()
        assert all(v >= 0 for v, _ in m.sources()), name
        for H, phi in hops_for(name, no):
            for short in ((False, True) if no < 50000 or H > 3 else (True,)):      # (the 300 000-frame list at small hops: once)
                n_rows = track_rows(L, H, short)
                want = []
                for j in range(W.rows(no, H, phi)):
                    sv, k = inv[j * H + phi]
                    assert k >= 0
                    want.append(-1 if sv >= L or sv // H >= n_rows else sv // H)
                near = W.warp_plan(ops, no, L, H, phi, n_rows)
                assert [p[0] for p in near] == want and all(p[1] is None for p in near), (name, H, phi, short)
                mix = W.warp_plan(ops, no, L, H, phi, n_rows, blend=True)
                assert len(mix) == len(near)
                for j, (p, q) in enumerate(zip(near, mix)):
                    k = inv[j * H + phi][1]
                    if ops[k][2] < 0:
                        assert p == q, (name, H, phi, j)
                    else:
                        assert p[0] in (q[0], q[1]) and (q[1] is None or (q[0] != q[1] and q[3] == ops[k][3] and 0 <= q[2] < q[3])), (name, j)
                # the unwarp reads a track on the OUTPUT timeline: rows(no) rows, or one fewer
                o_rows = max(0, -(-no // H) - (1 if short else 0))
                want = []
                for r in range(W.rows(L, H, phi)):
                    o, k = fwd[r * H + phi]
                    want.append(-1 if k < 0 or o // H >= o_rows else o // H)
                got = W.unwarp_plan(ops, no, L, H, phi, o_rows)
                assert [p[0] for p in got] == want, (name, H, phi, short)
                checked += len(near) + len(got)
    assert checked > 200000


def _float_track(n_rows, dim, seed):
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal((max(n_rows, 1), dim)) * 1000).astype(np.float32)
    return y[:n_rows]


def test_the_rendering_is_the_scalars(lists):
    """edit_rows_ref.render against blend_scalar, one np.float32 operation at a time, a NaN and an infinity in one row."""
    for name in ("shapes", "shapes_L_below", "down", "up"):
        ops, no, L = lists[name]
        for H, phi in ((1, 0), (3, 1), (7, 6)):
            n_rows = track_rows(L, H, True)
            y = _float_track(n_rows, 3, 5)
            y[n_rows // 4, 0], y[n_rows // 4, 2] = np.nan, np.inf
            plan = W.warp_plan(ops, no, L, H, phi, n_rows, blend=True)
            got = W.render(plan, y, 3)
            assert any(p[1] is not None for p in plan)
            zero = np.zeros(3, np.float32)
            for j, (ra, rb, t, n) in enumerate(plan):
                ya = y[ra] if ra >= 0 else zero
                if rb is None:
                    want = ya
                else:
                    yb = y[rb] if rb >= 0 else zero
                    want = np.asarray([W.blend_scalar(ya[c], yb[c], t, n) for c in range(3)], np.float32)
                assert np.array_equal(S.bits(got[j]), S.bits(want)), (name, H, phi, j)


_GOOD = {}      # the definition's own outputs on the switch test's inputs: computed once, shared by its cases


@pytest.mark.parametrize("switch", W.SWITCHES)
def test_every_switch_changes_an_answer(lists, switch):
    caught = []
    for name in list(planted()) + ["speeds/16000Hz/1ch/9001/3.5", "rates/16000Hz/2ch/4800/0.4"]:
        ops, no, L = lists[name]
        for H, phi in ((1, 0), (3, 1), (160, 80)):
            n_rows = track_rows(L, H, True)
            y = _float_track(n_rows, 2, 9)
            if n_rows > 8:
                y[n_rows // 2, 1] = np.inf
            z = _float_track(max(0, -(-no // H) - 1), 2, 10)
            if (name, H, phi) not in _GOOD:
                _GOOD[name, H, phi] = (W.warp(ops, no, L, H, phi, y, 2), W.warp(ops, no, L, H, phi, y, 2, blend=True),
                                       W.unwarp(ops, no, L, H, phi, z, 2))
            good = _GOOD[name, H, phi]
            bad = (W.warp(ops, no, L, H, phi, y, 2, switch=switch), W.warp(ops, no, L, H, phi, y, 2, blend=True, switch=switch),
                   W.unwarp(ops, no, L, H, phi, z, 2, switch=switch))
            if any(g.shape != b.shape or not np.array_equal(S.bits(g), S.bits(b)) for g, b in zip(good, bad)):
                caught.append((name, H, phi))
    assert caught, switch
    if switch == "phase_ignored":
        assert all(H > 1 and phi > 0 for _, H, phi in caught), caught
    if switch in ("no_same_row",):
        assert all(H > 1 for _, H, _ in caught), caught       # (at hop 1 the two ramps never share a row)


def test_at_hop_one_the_nearest_warp_is_a_gather_by_inverse(lists):
    for name, (ops, no, L) in lists.items():
        m = K.Lookup(ops, no, L)
        plan = W.warp_plan(ops, no, L, 1, 0, L)
        assert len(plan) == no == W.rows(no, 1, 0), name
        assert [p[0] for p in plan] == [(-1 if s == L else s) for s, _ in (m.inverse(u) for u in range(no))], name


def test_at_hop_one_the_blend_warp_is_the_float_replay(real):
    """H = 1, phi = 0, BLEND, dim = channels, a track of L frames: edit_scaled_ref's float replay at p = q = 1, bit for bit, on every
    real list -- whose cross-fades all have a != b (asserted), so the same-row rule plays no part."""
    fades = 0
    for name, (ops, no, L) in real.items():
        assert all(a != b for _, a, b, _ in ops if b >= 0), name
        fades += sum(1 for op in ops if op[2] >= 0)
        C = 2
        y = _float_track(L, C, 21)
        if L > 10:
            y[L // 3, 0], y[L // 2, 1] = np.inf, np.nan
        want = S.replay_scaled_np(ops, y.reshape(-1), C, L, no, 1, 1, L, "float").reshape(-1, C)
        got = W.warp(ops, no, L, 1, 0, y, C, blend=True)
        assert got.shape == want.shape == (no, C) and np.array_equal(S.bits(got), S.bits(want)), name
    assert fades > 3000


def test_the_count_of_a_stream():
    assert W.count(False, 1000, 1000, 5, 5, 3000, 160, 80, 6) == 6 and W.count(False, 1000, 1000, 5, 5, 3000, 160, 80, 5) == -6
    assert W.count(False, 1000, 500, 5, 5, 3000, 160, 80, 6) == 3                                  # (the key's out_cap cuts)
    assert W.count(True, 1000, 1000, 5, 5, 3000, 160, 80, 99) == 19 and W.count(True, 0, 1000, 5, 5, 3000, 160, 80, 99) == 19
    assert [W.count(u, *a) for u in (False, True) for a in ((1000, 1000, 0, 5, 3000, 160, 80, 99), (1000, 1000, 6, 5, 3000, 160, 80, 99),
                                                             (1000, 1000, -7, 5, 3000, 160, 80, 99), (-1, 1000, 5, 5, 3000, 160, 80, 99))] == [0] * 8
    assert W.count(False, 0, 1000, 5, 5, 3000, 160, 80, 99) == 0


def test_the_abi_has_the_row_calls():
    """The header declares the four functions and the struct, the binding lists them, the library exports them; the ABI version is
    still 1; the scaled replay no longer lists tracks below the key's rate as out of scope."""
    import speedy_amd
    from speedy_amd._lib import SYMBOLS, EditRowsTrack
    hdr = open(os.path.join(ROOT, "include", "speedy_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in include/speedy_hip.h"
        assert name in SYMBOLS, name + " is missing from speedy_amd._lib.SYMBOLS"
    assert len(SYMBOLS["spx_edit_warp_rows"][1]) == 19 and len(SYMBOLS["spx_edit_unwarp_rows"][1]) == 19
    assert ctypes.sizeof(EditRowsTrack) == 32 and re.search(r"int64_t in_off, out_off, n_rows, out_cap; \} spx_edit_rows_track;", code)
    assert "#define SPX_ROWS_NEAREST 0" in code and "#define SPX_ROWS_BLEND 1" in code
    assert "they need record compaction" not in hdr and "EDIT LIST, ROW TRACKS" in hdr
    speedy_amd.build()
    raw = ctypes.CDLL(os.path.join(ROOT, "speedy_amd", "lib", "libspeedy_hip.so"))
    assert not [n for n in NEW if not hasattr(raw, n)]
    raw.spx_abi_version.restype = ctypes.c_int
    assert raw.spx_abi_version() == 1
    fn = raw.spx_edit_rows
    fn.restype, fn.argtypes = ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    for x, H, phi in ((0, 1, 0), (81, 160, 80), (80, 160, 80), (10 ** 12, 7, 6), (-1, 1, 0), (5, 0, 0), (5, (1 << 20) + 1, 0), (5, 4, 4), (5, 4, -1)):
        assert fn(x, H, phi) == W.rows_api(x, H, phi), (x, H, phi)


def test_the_c_example_builds():
    """tools/batch_edit_rows_example.c builds with gcc -std=c99 -pedantic -Wall -Wextra -Werror (make editrowsexample)."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "editrowsexample"])
    assert os.path.exists(os.path.join(ROOT, "speedy_amd", "lib", "batch_edit_rows_example"))
