"""CPU: the pitch decision -- which lag wins the AMDF search, minDiff, maxDiff, whether the previous period is kept -- against
an exact integer definition (tests/pitch_ref.py), on inputs that reach its delicate part (tests/pitch_inputs.py).

The existing signals (tests/test_gpu_fuzz.py) never produce two lags with the same key floor(d 2^16 / p) and different ratios,
and never sit on an edge of the previous-period rule (profiles/pitch_decision.txt); the directed ones do, and this file asserts
that they do, from the definition's own census: the conditions below are requirements on the chosen inputs, not measurements.
Then: the oracle's period log equals the definition's, and every mutant of the definition (a selector without its tie scan, a
`>` for a `>=` in the rule ...) changes the period log of some directed input, so that a kernel with that mistake would change
its int16 output (tests/test_gpu_pitch_decision.py compares it with the oracle's).
"""
import ctypes

import numpy as np
import pytest

import pitch_inputs
import pitch_ref as R

SPEEDS = (2.0, 1.3)


@pytest.fixture(scope="module")
def walks():
    """{(name, speed): walk of the definition with its census}, computed once and left unchanged."""
    return {(name, s): R.walk(x, rate, ch, s) for name, rate, ch, x in pitch_inputs.directed() for s in SPEEDS}


@pytest.fixture(scope="module")
def tallies(walks):
    out = {}
    for name, rate, ch, _ in pitch_inputs.directed():
        t = dict.fromkeys(R.COUNTS, 0)
        for s in SPEEDS:
            for k, v in R.tally(walks[(name, s)]["census"]).items():
                t[k] += v
        out[name] = (rate, ch, t)
    return out


def test_directed_signals_are_quiet_and_short():
    for name, rate, ch, x in pitch_inputs.directed():
        assert x.dtype == np.int16 and 0.4 * rate <= x.size // ch <= 1.0 * rate, name
        assert np.abs(x.astype(np.int64)).max() <= 80, name      # the suite had nothing between silence / DC and amplitude 20 000


@pytest.mark.parametrize("rate", [22050, 44100, 48000, 96000])
def test_the_first_minimal_key_is_not_the_exact_choice(tallies, rate):
    """At each of these rates some directed signal has at least five steps where the first lag holding the minimal key
    floor(d 2^16 / p) is NOT the lag the sequential scan picks: a selector without the exact rescan of the ties, or with it
    slightly wrong, chooses another period there."""
    best = max(t["key_first_wrong"] for r, _, t in tallies.values() if r == rate)
    assert best >= 5, (rate, best)


def test_a_tie_crosses_the_64_lag_boundary(tallies):
    """Lags of equal key and unequal ratio on both sides of lag index 64 of a refine search.  Reached end to end at 63 999 Hz
    (121 refine lags; the general kernel serves that rate, so this is select_fold's running result across its first fold
    boundary).  NOT reached end to end: such a tie at 44.1 / 48 kHz (the two halves of fast_select2), or one inside the general
    selector's 1 + 2^-16 window across a fold boundary at 96 kHz -- searches of several hundred random low-level signals found
    none; those cases are left to the device check, tests/test_gpu_pitch_decision.py family 4 (profiles/pitch_decision.txt)."""
    assert sum(t["key_tie_unequal_cross64"] for _, _, t in tallies.values()) >= 1
    assert tallies["rect64k"][2]["key_tie_unequal_cross64"] >= 1


def test_the_general_selectors_window_is_reached(tallies):
    """Lags inside the general selector's ratio window (1 + 2^-16 of the minimum, 1 - 2^-16 of the maximum) whose first member is not
    the exact choice, on each side."""
    assert sum(t["win_min_first_wrong"] for _, _, t in tallies.values()) >= 1
    assert sum(t["win_max_first_wrong"] for _, _, t in tallies.values()) >= 1


def test_every_edge_of_the_rule_is_reached(tallies):
    """Each inequality of the previous-period rule at equality and at the nearest attainable value on the other side (maxDiff =
    3 minDiff + 1; 2 minDiff is even, so 3 prevMinDiff + 1 or + 2; minDiff = 0 below minDiff >= 1), on steps with a previous period.
    With the previous period both taken and not taken wherever the edge leaves that open: maxDiff = 3 minDiff + 1 is "a clear
    match", 2 minDiff = 3 prevMinDiff is "not much worse" and minDiff = 0 ends the rule, so those three exclude the previous period
    by themselves."""
    tot = dict.fromkeys(R.COUNTS, 0)
    for _, _, t in tallies.values():
        for k, v in t.items():
            tot[k] += v
    for k in ("A_eq", "A_above", "B_eq", "B_above", "C_eq", "C_below"):
        assert tot[k] >= 1, (k, tot)
    for k in ("A_eq", "B_above", "C_eq"):
        assert tot[k + "_taken"] >= 1 and tot[k] - tot[k + "_taken"] >= 1, (k, tot)
    for k in ("decisive_A_ge", "decisive_B_lt", "decisive_C_gt"):     # steps where the strictness of that inequality decides
        assert tot[k] >= 1, (k, tot)


def test_stereo_variants_decide_like_their_mono_signal(walks):
    """Duplicated stereo and (2 a, 0) stereo have the mono signal's channel mean and decimated sums exactly."""
    for s in SPEEDS:
        assert walks[("rect22k_dup", s)]["periods"] == walks[("rect22k", s)]["periods"]
        assert walks[("rect48k_left", s)]["periods"] == walks[("rect48k", s)]["periods"]


def _oracle_single_write(orc, x, rate, ch, speed):
    L = orc.lib()
    h = L.orc_sonicIntCreateStream(rate, ch)
    L.orc_sonicIntSetSpeed(h, speed)
    n = x.size // ch
    log = (ctypes.c_int * (n // 8 + 16))()
    L.orc_sonicIntSetPeriodLog(h, log, len(log))
    x = np.ascontiguousarray(x, np.int16)
    L.orc_sonicIntWriteShortToStream(h, orc.sptr(x), n)
    steps, frames = int(L.orc_sonicIntStepCount(h)), int(L.orc_sonicIntSamplesAvailable(h))
    L.orc_sonicIntDestroyStream(h)
    assert steps <= len(log)
    return list(log[:steps]), steps, frames


def test_oracle_period_log_equals_the_definition_on_the_directed_signals(orc, walks):
    for name, rate, ch, x in pitch_inputs.directed():
        for speed in SPEEDS + (3.5, 0.7, 0.4, 2000.0, 0.0001):      # the last two: the first step yields nothing and ends the write
            w = walks[(name, speed)] if (name, speed) in walks else R.walk(x, rate, ch, speed, census=False)
            log, steps, frames = _oracle_single_write(orc, x, rate, ch, speed)
            assert steps == len(w["periods"]) and steps > 0, (name, speed, steps, len(w["periods"]))
            assert log == w["periods"], (name, speed, [(i, a, b) for i, (a, b) in enumerate(zip(log, w["periods"])) if a != b][:5])
            assert frames == w["frames_out"], (name, speed, frames, w["frames_out"])
            if speed in (2000.0, 0.0001):
                assert steps == 1 and w["consumed"] == 0 and frames == (0 if speed > 1 else log[0]), (name, speed, steps, frames)


@pytest.mark.parametrize("rate", [16000, 22050])
def test_oracle_period_log_equals_the_definition_on_the_fuzz_kinds(orc, rate):
    """One short signal of each kind of tests/test_gpu_fuzz.py, mono and with three channels."""
    import test_gpu_fuzz as F
    rng = np.random.default_rng(rate)
    for i, kind in enumerate(F.KINDS):
        ch = 3 if i % 3 == 2 else 1
        x = F._signal(kind, rate // 2, rate, ch, rng)
        for speed in (2.0, 1.5, 0.6):
            w = R.walk(x, rate, ch, speed, census=False)
            log, steps, frames = _oracle_single_write(orc, x, rate, ch, speed)
            assert steps == len(w["periods"]) and steps > 0, (kind, speed)
            assert log == w["periods"], (kind, ch, speed)
            assert frames == w["frames_out"], (kind, ch, speed)


def test_the_ballot_form_of_the_clear_match_is_the_inequality(walks):
    """The speed-up kernel asks "some lag has d_p >= (3 minDiff + 1) p" instead of maxDiff > 3 minDiff (max_p floor(d_p / p) =
    floor(max_p d_p / p)): the same decision on every step of every directed signal."""
    for name, rate, ch, x in pitch_inputs.directed():
        for s in SPEEDS:
            assert R.walk(x, rate, ch, s, rule="ballot", census=False)["periods"] == walks[(name, s)]["periods"], (name, s)


MUTANTS = [("first_key", "exact"), ("last_tie", "exact"), ("exact", "A_ge"), ("exact", "B_lt"), ("exact", "C_gt"), ("exact", "ballot_3m")]


@pytest.mark.parametrize("sel,rule", MUTANTS)
def test_every_mutant_changes_a_period_log(walks, sel, rule):
    """Teeth: the mutant's period log differs from the exact one on at least one directed signal -- and at speed 2.0, where a step
    is as long as its period, so do the positions of the later steps and the number of frames produced: a kernel with that mistake
    cannot produce the oracle's output."""
    caught, caught_frames = [], []
    for name, rate, ch, x in pitch_inputs.directed():
        for s in SPEEDS:
            m = R.walk(x, rate, ch, s, select=sel, rule=rule, census=False)
            e = walks[(name, s)]
            if m["periods"] != e["periods"]:
                caught.append((name, s))
                if s == 2.0:
                    assert m["positions"] != e["positions"] or m["frames_out"] != e["frames_out"], (name, sel, rule)
                    if m["frames_out"] != e["frames_out"]:
                        caught_frames.append(name)
    assert caught, (sel, rule)
    assert caught_frames, (sel, rule, caught)


def test_the_last_maximal_lag_gives_the_same_quotient(walks):
    """The one switch of the definition that CANNOT show: maxDiff taken at the last instead of the first maximal lag.  Equal ratios
    d / p have equal floors, and only the quotient maxDiff leaves the search -- so this mutant is equivalent, on these signals as on
    any other, and no test of the output can pin which of the tied worst lags a selector holds."""
    for name, rate, ch, x in pitch_inputs.directed():
        m = R.walk(x, rate, ch, 2.0, select="max_last", census=False)
        e = walks[(name, 2.0)]
        assert m["periods"] == e["periods"] and m["max_diff"] == e["max_diff"], name


def test_select_rows_equals_the_scan():
    """The vectorised form of the scan that the device test uses (int64 rows) against the Python-integer one."""
    rng = np.random.default_rng(7)
    for p0, nl in ((55, 41), (290, 89), (640, 97), (20, 193), (10, 64)):
        D = rng.integers(0, 4, size=(200, nl)) * rng.integers(1, 3 * (p0 + nl), size=(200, nl))
        D[:20] = 0
        D[20:40] = 5
        best, mn, worst, mx = R.select_rows(D, p0)
        for v in range(D.shape[0]):
            assert (int(best[v]), int(mn[v]), int(worst[v]), int(mx[v])) == R.select([int(t) for t in D[v]], p0), (p0, nl, v)
