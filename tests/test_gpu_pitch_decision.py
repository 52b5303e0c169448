"""GPU: the walk kernels' pitch decision against the exact integer definition (tests/pitch_ref.py).

First half: the three lag selectors (fast_select, fast_select2 of spx_walk_fast.hip; select_fold / select_finish of spx_walk.hip)
run on vectors of sums built on the host (spx_debug_select_check, spx_debug_select_fold_check) -- every returned lag and every
quotient equals the sequential scan with exact rational comparisons, first lag wins.  No tolerance.

Second half: the directed signals of tests/pitch_inputs.py (quiet hum in a nearly silent recording: lags of equal key and unequal
ratio, minDiff / maxDiff on the edges of the previous-period rule -- asserted from the census in
tests/test_oracle_pitch_decision.py) through every form of the walk kernels, bit-compared with the oracle.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pitch_inputs  # noqa: E402
import pitch_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ the selectors ------------------------------------------------------------------

def _log_uniform_int(rng, hi, n):
    return np.minimum(hi, np.floor(np.exp(rng.uniform(0.0, math.log(hi + 2.0), n)) - 1.0)).astype(np.int64)


def _planted(rng, p0, nl, m, n, side, straddle=None, tie_keys=False):
    """n rows with a chain of m lags p1 < p1 + s < ... whose sums lie in arithmetic progression with d_a p_b - d_b p_a = e (b - a)
    for a < b, e in {-1, 0, +1} (for m = 2: exactly the near-tie d1 p2 - d2 p1 = e), at an integer part k of the ratio between 0
    and 65 530; every other lag is worse by 3 or more in d / p (side "min"; "max": smaller by 3 or more, and k >= 4).  e = +1: each
    later lag has the strictly smaller ratio, e = -1 the larger -- the scan must switch on one side and must not on the other;
    e = 0: equal ratios, the first wins.
    straddle: the chain's first lag index below it and its last at or above it (a lane pair i / 64 + j, a fold boundary).
    tie_keys (the speed-up selector, ranges whose lag products exceed 2^16): the chain's last two lags have a product above 2^16,
    and in the vectors with e = +1 the lags are drawn again until two keys floor(d 2^16 / p) of the chain coincide -- unequal ratios
    under one key, the exact winner not the first of them.  The vectors with e = 0 or -1 are right on the first key by themselves,
    so the share of vectors where the first minimal key is not the exact answer is the share of e = +1: three in five."""
    rows = np.empty((n, nl), np.int64)
    lags = p0 + np.arange(nl, dtype=np.int64)
    ks = _log_uniform_int(rng, 65530, n)
    for v in range(n):
        e = int(rng.choice([1, 1, 1, 0, -1])) * (1 if side == "min" else -1)   # three in five: the scan has to move on
        k = int(ks[v])
        if side == "max":
            k = max(k, 4)
        for attempt in range(100000):
            s = int(rng.integers(1, max(2, (nl - 1) // (m - 1) + 1)))
            if straddle is None:
                i1 = int(rng.integers(0, nl - (m - 1) * s)) if nl - (m - 1) * s > 0 else -1
            else:
                lo, hi = max(0, straddle - (m - 1) * s), min(straddle, nl - (m - 1) * s)
                i1 = int(rng.integers(lo, hi)) if hi > lo else -1
            p1 = p0 + i1
            if i1 < 0 or math.gcd(p1, s) != 1:
                continue
            d1 = (e * pow(s, -1, p1)) % p1 + k * p1 if p1 > 1 else k
            t = (d1 * s - e) // p1
            assert t * p1 == d1 * s - e and t >= 0
            if tie_keys:       # (which keys coincide depends on the lags alone: the chain's ratios are k + c / p1 - j / (p1 p_j), c fixed by them)
                keys = [((d1 + j * t) << 16) // (p1 + j * s) for j in range(m)]
                if (p1 + (m - 2) * s) * (p1 + (m - 1) * s) <= 68000 or (e == 1 and keys.index(min(keys)) == m - 1):
                    continue
            break
        else:
            raise AssertionError("no place for the chain", p0, nl, m, straddle)
        if side == "min":
            rows[v] = (k + 3) * lags + rng.integers(0, lags)
        else:
            rows[v] = (k - 3) * lags - rng.integers(0, lags)
        for j in range(m):
            rows[v, i1 + j * s] = d1 + j * t
    assert (rows >= 0).all() and (rows <= 65535 * lags).all()
    return rows


def _families(rng, p0, nl, side="min", n=600, tie_keys=False):
    """{family: rows} for the lags p0 .. p0 + nl - 1."""
    lags = p0 + np.arange(nl, dtype=np.int64)
    F = {}
    F["1 constant"] = np.repeat(np.arange(9, dtype=np.int64)[:, None], nl, axis=1)
    if nl >= 2:
        F["2 pairs"] = _planted(rng, p0, nl, 2, n, side, tie_keys=tie_keys)
    if nl >= 9:
        F["3 triples"] = _planted(rng, p0, nl, 3, n // 2, side, tie_keys=tie_keys)
        F["3 quadruples"] = _planted(rng, p0, nl, 4, n // 2, side, tie_keys=tie_keys)
    for b in range(64, nl, 64):
        F["4 across %d" % b] = _planted(rng, p0, nl, 2, n // 2, side, straddle=b, tie_keys=tie_keys)
    full = np.repeat((65535 * lags)[None, :], 6, axis=0)
    for r, j in enumerate((0, nl // 2, nl - 1)):
        full[1 + r, j] -= 1
    full[4, nl // 3] = 0
    full[5, nl - 1] = 65534 * lags[-1]
    F["5 full scale"] = full
    F["6 random small"] = rng.integers(0, 3 * lags + 1, size=(n, nl))
    return F


def _pack(rng, D, width):
    """uint32 rows of `width` words: the sums, then garbage in the invalid lanes (zeros, all ones, random words)."""
    n, nl = D.shape
    out = rng.integers(0, 1 << 32, size=(n, width), dtype=np.uint64).astype(np.uint32)
    out[::3, nl:] = 0
    out[1::3, nl:] = 0xffffffff
    out[:, :nl] = D.astype(np.uint32)
    return np.ascontiguousarray(out)


def _first_in_window(D, p0, ext, p_ext, side):
    """The first lag of every row inside the general selector's ratio window around the exact extremum (d, lag) = (ext, p_ext)."""
    lags = p0 + np.arange(D.shape[1], dtype=np.int64)
    if side == "min":
        inside = D * p_ext[:, None] * 65536 <= ext[:, None] * lags[None, :] * 65537
    else:
        inside = D * p_ext[:, None] * 65536 >= ext[:, None] * lags[None, :] * 65535
    return p0 + inside.argmax(axis=1)


# rate, p0, lags, maxPeriod, two lags per lane -- the refine ranges that occur (bottom, middle, top of the period range), the coarse
# ranges (needResolve false in the kernel: maxPeriod = the coarse search's own last lag), 16 kHz (246^2 < 2^16: the keys alone), and
# rows shorter than the wave (clamped ranges).  The rows labelled 63999 are SYNTHETIC for this selector: 121 and 128 lags are what two
# lags per lane can hold, but the engine serves that rate with the general kernel (97 lags at 48 kHz is the most the speed-up kernel sees).
FAST_CONFIGS = [
    (22050, 55, 41, 339, 0), (22050, 180, 41, 339, 0), (22050, 299, 41, 339, 0),
    (44100, 110, 89, 678, 1), (44100, 350, 89, 678, 1), (44100, 590, 89, 678, 1),
    (48000, 120, 97, 738, 1), (48000, 380, 97, 738, 1), (48000, 642, 97, 738, 1),
    (63999, 500, 121, 984, 1), (63999, 864, 121, 984, 1),
    (22050, 11, 57, 67, 0), (48000, 10, 52, 61, 0), (11025, 13, 72, 84, 1), (63999, 10, 56, 65, 0),
    (16000, 40, 33, 246, 0), (16000, 120, 33, 246, 0), (16000, 214, 33, 246, 0),
    (44100, 634, 45, 678, 1), (48000, 700, 39, 738, 1), (22050, 338, 2, 339, 0), (22050, 339, 1, 339, 0), (48000, 674, 65, 738, 1),
    (22050, 276, 64, 339, 0), (63999, 857, 128, 984, 1),
]


def test_selectors_against_exact_rationals():
    """spx_debug_select_check (the speed-up kernel's selector, one and two lags per lane) and spx_debug_select_fold_check (the general
    kernel's, 64 lags per fold, minimum and maximum, both forms of the first fold) on the vector families below: every returned lag,
    key and quotient equals tests/pitch_ref.py select_rows.

    Per family and configuration the test also asserts that the vectors are what the generator meant them to be -- the share of
    vectors where "the first lag with the minimal key" (speed-up selector) or "the first lag inside the ratio window" (general
    selector) is NOT the exact answer.  Intended shares, from the construction (_planted):
      * speed-up selector, every configuration is of one of two kinds.  Largest lag squared below 2^16 (the coarse ranges, 16 kHz, the
        lower part of the other ranges): the keys order exactly like the rationals, the share is 0 in every family.  Otherwise the
        planted chains are placed where lag products exceed 2^16, the e = +1 ones where keys coincide: the share is
        the share of e = +1, 0.6, asserted as 0.45 .. 0.75 (five standard deviations of 300 draws) in families 2 - 4 -- at both
        one lag per lane (22.05 kHz, where only the top of the range reaches 2^16) and two;
      * the general selector's window is RELATIVE (2^-16 of the ratio): a near-tie lies inside it whenever the ratio is at least
        2^16 / (p1 p2), which most of the log-uniform ratios are: at least a quarter in every configuration."""
    from speedy_amd._lib import lib
    L = lib()
    rng = np.random.default_rng(20261019)
    u32p, i32p = C.POINTER(C.c_uint), C.POINTER(C.c_int)
    shares = []
    tied_seen = {0: 0, 1: 0}      # configurations with planted key ties, by lags per lane - 1
    for rate, p0, nl, max_p, two in FAST_CONFIGS:
        last = p0 + nl - 1
        exact_keys = last * last < 65536
        assert exact_keys or (last - 1) * last > 68000, (rate, p0, nl)     # one kind or the other
        fam = _families(rng, p0, nl, tie_keys=not exact_keys)
        names = list(fam)
        D = np.concatenate([fam[k] for k in names])
        owner = np.concatenate([np.full(fam[k].shape[0], i) for i, k in enumerate(names)])
        best, min_diff, _, _ = R.select_rows(D, p0)
        d_best = D[np.arange(D.shape[0]), best - p0]
        first, _ = R.first_key_rows(D, p0)
        packed = _pack(rng, D, 128 if two else 64)
        idx = np.full(D.shape[0], -1, np.int32)
        kmin = np.zeros(D.shape[0], np.uint32)
        assert L.spx_debug_select_check(packed.ctypes.data_as(u32p), D.shape[0], p0, nl, max_p, two, idx.ctypes.data_as(i32p),
                                        kmin.ctypes.data_as(u32p)) == 0
        bad = np.nonzero(idx != best - p0)[0]
        assert bad.size == 0, (rate, p0, nl, two, names[owner[bad[0]]], D[bad[0]].tolist(), int(idx[bad[0]]), int(best[bad[0]] - p0))
        assert np.array_equal(kmin.astype(np.int64), (d_best << 16) // best), (rate, p0, nl)
        assert np.array_equal(kmin.astype(np.int64) >> 16, min_diff), (rate, p0, nl)
        if not exact_keys:
            assert max_p * max_p >= 65536        # the kernel rescans ties there
            tied_seen[two] += nl >= 9
        for i, k in enumerate(names):
            share = float(np.mean(first[owner == i] != best[owner == i]))
            shares.append(("fast", rate, p0, nl, k, round(share, 3)))
            if exact_keys:
                assert share == 0.0, (rate, p0, nl, k, share)           # the keys order exactly like the rationals
            elif k[0] in "234":
                assert 0.45 <= share <= 0.75, (rate, p0, nl, k, share)
            if k == "1 constant":
                sel = owner == i
                assert np.array_equal(best[sel][1:], np.full(8, p0 + nl - 1)) and best[sel][0] == p0
    assert tied_seen[0] >= 2 and tied_seen[1] >= 8, tied_seen     # fast_select's own tie scan and fast_select2's, both exercised

    # the general selector: rate, p0, lags -- refine ranges of 96 kHz (four folds), of the rates whose multi-channel batches fall
    # to it, a coarse range, the direct search of a 4 kHz stream, short rows
    for rate, p0, nl in [(96000, 240, 193), (96000, 700, 193), (96000, 1284, 193), (44100, 350, 89), (63999, 864, 121), (48000, 642, 97),
                         (22050, 180, 41), (96000, 10, 52), (4000, 10, 52), (96000, 1412, 65), (96000, 1476, 1), (48000, 600, 64), (96000, 1300, 128)]:
        for side in ("min", "max"):
            fam = _families(rng, p0, nl, side, n=400)
            names = list(fam)
            D = np.concatenate([fam[k] for k in names])
            owner = np.concatenate([np.full(fam[k].shape[0], i) for i, k in enumerate(names)])
            best, min_diff, worst, max_diff = R.select_rows(D, p0)
            rows = np.arange(D.shape[0])
            d_best = D[rows, best - p0]
            nz = D.max(axis=1) > 0
            d_worst = np.where(nz, D[rows, np.where(nz, worst - p0, 0)], 0)
            first_min = _first_in_window(D, p0, d_best, best, "min")
            first_max = _first_in_window(D, p0, d_worst, np.where(nz, worst, 1), "max")
            packed = _pack(rng, D, (nl + 63) // 64 * 64)
            for want_max in (1, 0):
                for fresh in (0, 1):
                    out = np.full((D.shape[0], 3), -1, np.int32)
                    assert L.spx_debug_select_fold_check(packed.ctypes.data_as(u32p), D.shape[0], p0, nl, want_max, fresh,
                                                         out.ctypes.data_as(i32p)) == 0
                    want = np.stack([best, min_diff, max_diff if want_max else np.zeros_like(max_diff)], axis=1)
                    bad = np.nonzero((out != want).any(axis=1))[0]
                    assert bad.size == 0, (rate, p0, nl, side, want_max, fresh, names[owner[bad[0]]], D[bad[0]].tolist(),
                                           out[bad[0]].tolist(), want[bad[0]].tolist())
            for i, k in enumerate(names):
                sel = owner == i
                share = float(np.mean((first_min[sel] != best[sel]) if side == "min" else (first_max[sel] != worst[sel]) & nz[sel]))
                shares.append(("general " + side, rate, p0, nl, k, round(share, 3)))
                if k[0] in "234":
                    assert share >= 0.25, (rate, p0, nl, side, k, share)
                if k == "1 constant":
                    assert out[sel][0].tolist() == [p0, 0, 0]                    # all zero: worst = 255, maxDiff = 0
                    assert np.array_equal(worst[sel][1:], np.full(8, p0)) and worst[sel][0] == 255
    if os.environ.get("SPX_PITCH_SHARES"):      # the table of profiles/pitch_decision.txt
        with open(os.environ["SPX_PITCH_SHARES"], "w") as f:
            for s in shares:
                f.write("%-12s %6d Hz  p0 %4d  lags %3d  %-14s %.3f\n" % s)


# ------------------------------------------------------------------ end to end ------------------------------------------------------------------

def _oracle(orc, x, rate, ch, speed, nl=0.0, taps=False):
    n = x.size // ch
    return orc.compress_sound(x, rate, ch, speed, nl, 0.0, False, chunk=1000 if nl != 0 else max(n, 1), taps=taps)


def _oracle_steps(orc, x, rate, ch, speed, nl=0.0, playback_rate=None):
    L = orc.lib()
    h = L.orc_sonicCreateStream(rate, ch, 0)
    L.orc_sonicSetSpeed(h, speed); L.orc_sonicEnableNonlinearSpeedup(h, nl); L.orc_sonicSetDurationFeedbackStrength(h, 0.0)
    if playback_rate is not None:
        L.orc_sonicSetRate(h, playback_rate)
    x = np.ascontiguousarray(x, np.int16)
    n = x.size // ch
    chunk = 1000 if nl != 0 else max(n, 1)
    for pos in range(0, n, chunk):
        seg = np.ascontiguousarray(x[pos * ch:(pos + chunk) * ch])
        L.orc_sonicWriteShortToStream(h, orc.sptr(seg), seg.size // ch)
    L.orc_sonicFlushStream(h)
    k = int(L.orc_sonicIntStepCount(h))
    L.orc_sonicDestroyStream(h)
    return k


def _by_rate(rate, ch=1):
    return [(name, x) for name, r, c, x in pitch_inputs.directed() if r == rate and c == ch]


def _run(orc, rate, chs, xs, speeds, nls=0.0, taps=False, batch_rate=None):
    """One batch call; every stream's int16 output and step count against the oracle.  Returns (form, batch, plan)."""
    from speedy_amd.batch import Batch, Plan
    n = len(xs)
    chs = np.broadcast_to(np.asarray(chs, np.int32), (n,))
    speeds = np.broadcast_to(np.asarray(speeds, np.float64), (n,))
    nls = np.broadcast_to(np.asarray(nls, np.float64), (n,))
    plan = Plan(rate, False)
    b = Batch(plan, [x.size // int(c) for x, c in zip(xs, chs)], chs, speeds, nls, 0.0, taps=taps, rate=batch_rate)
    b.upload(xs)
    b.run()
    outs = b.results()
    form = plan.L.spx_debug_last_walk_form()
    steps = b.step_counts()
    memo = {}
    for i, x in enumerate(xs):
        key = (x.tobytes(), int(chs[i]), float(speeds[i]), float(nls[i]))
        if key not in memo:
            if batch_rate is None:
                memo[key] = (_oracle(orc, x, rate, int(chs[i]), float(speeds[i]), float(nls[i]), taps=taps),
                             _oracle_steps(orc, x, rate, int(chs[i]), float(speeds[i]), float(nls[i])))
            else:
                from test_batch_rate_abi import oracle_rate_stream
                memo[key] = ({"out": oracle_rate_stream(orc, x, rate, int(chs[i]), float(speeds[i]), float(nls[i]), batch_rate)},
                             _oracle_steps(orc, x, rate, int(chs[i]), float(speeds[i]), float(nls[i]), batch_rate))
        ref, ref_steps = memo[key]
        assert outs[i].size == ref["out"].size and np.array_equal(outs[i], ref["out"]), (rate, i, int(chs[i]), float(speeds[i]), form)
        assert int(steps[i]) == ref_steps and ref_steps > 0, (rate, i, float(speeds[i]), int(steps[i]), ref_steps)
        if taps and nls[i] != 0:
            got = b.tap_arrays(i)
            for k in ("tension", "speed", "features"):
                assert np.array_equal(got[k], ref[k]), (rate, i, k)
    return form, b, plan


SPEEDS = (2.0, 1.3, 3.5)


def test_directed_signals_on_the_4_plus_4_form(orc):
    """Linear jobs, a CU per stream: the kernels run in sequence and the walk kernel keeps its output waves."""
    for rate in (22050, 16000):
        sig = _by_rate(rate)
        xs = [x for _, x in sig for _ in SPEEDS]
        form, _, _ = _run(orc, rate, 1, xs, [s for _ in sig for s in SPEEDS])
        assert form == 16 * 4 + 4, (rate, form)
    sig = _by_rate(22050, 2)          # duplicated stereo: the multi-channel instantiation
    form, _, _ = _run(orc, 22050, 2, [x for _, x in sig for _ in SPEEDS], [s for _ in sig for s in SPEEDS])
    assert form == 16 * 4 + 4, form


def test_directed_signals_on_the_lean_form_with_taps(orc):
    """Nonlinear jobs (factor 1.0) at 22.05 kHz mono: the concurrent mode, where the walk kernel gives up its output waves -- and the
    analysis side on inputs this quiet: tension, speed and features equal the oracle's."""
    from speedy_amd._lib import lib
    sig = _by_rate(22050)
    xs = [x for _, x in sig for _ in SPEEDS]
    form, _, _ = _run(orc, 22050, 1, xs, [s for _ in sig for s in SPEEDS], nls=1.0, taps=True)
    assert lib().spx_debug_last_call_concurrent() == 1
    assert form == 16 * 4 + 0, form


def test_directed_signals_on_the_throughput_form(orc):
    """More than two streams per CU: two search waves, no output waves, the 1536-frame window.  The signals repeated at
    different phases fill the batch."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sig = _by_rate(22050)
    n0 = 9000
    count = 2 * cus + 8
    xs = [np.ascontiguousarray(sig[i % len(sig)][1][37 * (i // len(sig)) % 4000:][:n0]) for i in range(count)]
    form, _, _ = _run(orc, 22050, 1, xs, [SPEEDS[(i // len(sig)) % 3] for i in range(count)])
    assert form == 16 * 2 + 0, form


@pytest.mark.parametrize("rate", [44100, 48000])
def test_directed_signals_on_the_wide_form(orc, rate):
    """Eight search waves and two lags per lane in the refine select (89 and 97 lags); the stereo variant at 48 kHz."""
    sig = _by_rate(rate)
    form, _, _ = _run(orc, rate, 1, [x for _, x in sig for _ in SPEEDS], [s for _ in sig for s in SPEEDS])
    assert form == 16 * 8 + 4, (rate, form)
    sig = _by_rate(rate, 2)
    if sig:
        form, _, _ = _run(orc, rate, 2, [x for _, x in sig for _ in SPEEDS], [s for _ in sig for s in SPEEDS])
        assert form == 16 * 8 + 4, (rate, form)


def test_directed_signals_on_the_wide_coarse_form(orc):
    """11.025 kHz: 72 coarse lags, two per lane in the coarse select, and every lag product below 2^16 -- the keys alone decide."""
    sig = _by_rate(11025)
    form, _, plan = _run(orc, 11025, 1, [x for _, x in sig for _ in SPEEDS], [s for _ in sig for s in SPEEDS])
    assert form == 16 * 4 + 4, form
    names = plan.L.spx_batch_kernel_names(plan.h, len(sig) * 3, 1, 1).decode()
    assert names.split(";")[2] == "spx_walk_fast_kernel<4, 4, 0, 2, 0>", names      # SPEC = 2: the wide coarse select


def test_a_slow_down_job_on_the_speed_up_kernel(orc):
    """Speeds 0.7 and 0.4 beside 2.0 and 1.3 in one batch: the speed-up kernel's instantiation that also serves slow-down events
    (last template argument 2), 4 + 4 waves at 22.05 kHz and 8 + 4 at 48 kHz."""
    for rate, want, name in ((22050, 16 * 4 + 4, "spx_walk_fast_kernel<4, 4, 0, 0, 2>"), (48000, 16 * 8 + 4, "spx_walk_fast_kernel<8, 4, 0, 0, 2>")):
        sig = _by_rate(rate)
        speeds = [0.7, 2.0, 0.4, 1.3]
        form, _, plan = _run(orc, rate, 1, [x for _, x in sig for _ in speeds], [s for _ in sig for s in speeds])
        assert form == want, (rate, form)
        names = plan.L.spx_batch_kernel_names(plan.h, len(sig) * len(speeds), 1, 0).decode()
        assert names.split(";")[2] == name, names


def test_directed_signals_on_the_general_kernel(orc):
    """Reached three ways: a rate beyond the speed-up kernel's (96 kHz, 193 refine lags: four folds of the selector; 63 999 Hz,
    121 lags, whose ragged refine tasks do not fit eight search waves -- rect64k has lags of equal key and unequal ratio on both
    sides of the first fold boundary), a channel count past skip x channels = 56 (48 kHz x 5 channels), and a batch with a playback
    rate (spx_batch_run_rate)."""
    for rate in (96000, 63999):
        sig = _by_rate(rate)
        form, _, _ = _run(orc, rate, 1, [x for _, x in sig for _ in SPEEDS], [s for _ in sig for s in SPEEDS])
        assert form == 0, (rate, form)
    x48 = dict(_by_rate(48000))["rect48k"]
    x5 = np.ascontiguousarray(np.repeat(x48[:, None], 5, axis=1).reshape(-1))
    form, _, _ = _run(orc, 48000, 5, [x5] * 3, list(SPEEDS))
    assert form == 0, form
    x22 = dict(_by_rate(22050))["rect22k"]
    form, _, _ = _run(orc, 22050, 1, [x22], [2.0], batch_rate=1.25)
    assert form == 0, form


@pytest.mark.parametrize("coalesce", [True, False])
def test_streaming_in_writes_of_1000_frames(orc, coalesce):
    """One 22.05 kHz and one 48 kHz signal through the drop-in stream API, call for call against the oracle shim."""
    from speedy_amd.sonic2 import SonicStream
    L = orc.lib()
    for name, rate, speed, want in (("rect22k", 22050, 2.0, 16 * 4 + 4), ("rect48k", 48000, 1.3, 16 * 8 + 4)):
        x = dict(_by_rate(rate))[name]
        h = L.orc_sonicCreateStream(rate, 1, 0)
        s = SonicStream(rate, 1, False, coalesce)
        L.orc_sonicSetSpeed(h, speed); s.set_speed(speed)
        L.orc_sonicEnableNonlinearSpeedup(h, 0.0); s.enable_nonlinear(0.0)
        buf = np.zeros(8192, np.int16)
        for pos in range(0, x.size, 1000):
            seg = np.ascontiguousarray(x[pos:pos + 1000])
            assert L.orc_sonicWriteShortToStream(h, orc.sptr(seg), seg.size) == 1
            assert s.write_short(seg) == 1
            k = L.orc_sonicReadShortFromStream(h, orc.sptr(buf), 8192)
            got = s.read_short(8192)
            assert got.size == k and np.array_equal(got, buf[:k]), (name, coalesce, pos)
        L.orc_sonicFlushStream(h)
        assert s.flush() == 1
        while True:
            k = L.orc_sonicReadShortFromStream(h, orc.sptr(buf), 8192)
            got = s.read_short(8192)
            assert got.size == k and np.array_equal(got, buf[:k]), (name, coalesce, "drain")
            if k == 0:
                break
        assert s.L.spx_debug_last_walk_form() == want, (name, coalesce, s.L.spx_debug_last_walk_form())   # one short job per launch: a CU to itself
        L.orc_sonicDestroyStream(h)
        s.close()


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_low_level_fuzz(orc, seed):
    """Ten cases per seed over the low-level rectangular family: level 1 .. 30 LSB, the period within 1 % of an integer or a
    half-integer anywhere in the search range, 1 - 2 channels, every rate of this file, speeds either side of 1 and 2."""
    from speedy_amd.batch import compress_batch
    rng = np.random.default_rng([20261019, seed])
    for i in range(10):
        rate = int(rng.choice([11025, 16000, 22050, 44100, 48000, 63999, 96000]))
        ch = int(rng.choice([1, 1, 2]))
        a = int(rng.integers(1, 31))
        per = (int(rng.integers(rate // 400, rate // 65 + 1)) + 0.5 * int(rng.integers(0, 2))) * (1.0 + rng.uniform(-0.01, 0.01))
        x = pitch_inputs.rect(rate, a, per, float(rng.uniform(0.1, 0.9)), bool(rng.integers(0, 2)), 0.5)
        if ch == 2:
            x = pitch_inputs.duplicated_stereo(x) if rng.integers(0, 2) else pitch_inputs.one_sided_stereo(x)
        speed = float(rng.choice([2.0, 1.3, 3.5, 0.7]))
        ref = _oracle(orc, x, rate, ch, speed)
        outs, b = compress_batch([x], rate, ch, speed, 0.0, 0.0, False, taps=False)
        tag = (seed, i, rate, ch, a, per, speed)
        assert np.array_equal(outs[0], ref["out"]), tag
        # one linear job: the kernels in sequence, the full form of its rate -- 4 + 4 waves (wide coarse select at 11.025 kHz), 8 + 4
        # from 24 kHz, the general kernel where the ragged refine tasks do not fit eight search waves
        want = {11025: 68, 16000: 68, 22050: 68, 44100: 132, 48000: 132, 63999: 0, 96000: 0}[rate]
        assert b.plan.L.spx_debug_last_walk_form() == want, tag + (b.plan.L.spx_debug_last_walk_form(),)
        assert int(b.step_counts()[0]) == _oracle_steps(orc, x, rate, ch, speed), tag
