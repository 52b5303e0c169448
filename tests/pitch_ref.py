"""The pitch decision of the time-scale modification as exact integers -- test infrastructure, CPU only.

Written from the algorithm's text (the anchors in oracle/orc_sonic.h), not from the kernels and not
from oracle/orc_sonic.c: which lag wins the AMDF search, what minDiff and maxDiff are, whether the previous period is
kept, and where the position walk of ONE write goes with it.  Everything is Python integers; numpy int64 only for the sums
d_p = sum |x[i] - x[i + p]| (at most 65535 p, p < 2^12: no overflow) and, in select_rows, for products d p' < 2^16 2^12 2^12.
The only floating point is the float32 step length, evaluated as written in skip_pitch_period / insert_pitch_period.

What the definition fixes:
  * select: a sequential scan over ascending lags with d best < minD p (the minimum) and d worst > maxD p (the maximum), so
    the FIRST lag wins among equal ratios on both sides; start values best = 0 (the first lag is taken), maxDiff = 0,
    worst = 255; minDiff and maxDiff are the floor quotients of the winners.
  * the previous-period rule as three inequalities: minDiff >= 1 (and a previous period exists), maxDiff > 3 minDiff
    ("a clear match"), 2 minDiff <= 3 prevMinDiff ("not much worse than last time").

The switches (`select=` / `rule=`) are the mutants the tests use to show that the directed inputs have teeth:
  select "first_key"   the first lag with the minimal key floor(d 2^16 / p)   (a fast selector without its tie scan)
         "last_tie"    the last lag among exact ties                          (<= for <)
         "max_last"    maxDiff from the last instead of the first maximal lag (>= for >)
  rule   "A_ge"        maxDiff >= 3 minDiff      for >
         "B_lt"        2 minDiff <  3 prevMinDiff for <=
         "C_gt"        minDiff > 1               for >= 1
         "ballot"      NO mutant: the speed-up kernel's form of inequality A, "some lag has d_p >= (3 minDiff + 1) p"
         "ballot_3m"   that form with 3 minDiff + 1 written as 3 minDiff
"""
import numpy as np

MIN_PITCH, MAX_PITCH, AMDF_FREQ = 65, 400, 4000
SELECTS = ("exact", "first_key", "last_tie", "max_last")
RULES = ("exact", "A_ge", "B_lt", "C_gt", "ballot", "ballot_3m")


def limits(rate):
    """minPeriod, maxPeriod, maxRequired, skip of a sample rate."""
    min_p, max_p = rate // MAX_PITCH, rate // MIN_PITCH
    return min_p, max_p, 2 * max_p, (rate // AMDF_FREQ if rate > AMDF_FREQ else 1)


def down_sample(frames, skip, channels, count):
    """Mean of `skip` frames over all channels, C division (truncating toward zero).  frames: interleaved samples."""
    per = skip * channels
    s = np.asarray(frames[: count * per], np.int64).reshape(count, per).sum(axis=1)
    return np.where(s < 0, -((-s) // per), s // per)


def amdf(x, lo, hi):
    """d_p = sum_{i < p} |x[i] - x[i + p]| for p = lo .. hi, as a list of Python integers."""
    x = np.asarray(x, np.int64)
    return [int(np.abs(x[:p] - x[p:2 * p]).sum()) for p in range(lo, hi + 1)]


def select(d, p0, variant="exact"):
    """The scan over lags p0, p0 + 1, ... with sums d.  Returns (best, minDiff, worst, maxDiff)."""
    if variant == "first_key":
        keys = [(di << 16) // (p0 + i) for i, di in enumerate(d)]
        i = keys.index(min(keys))
        best, min_d = p0 + i, d[i]
    else:
        best, min_d = 0, 1
        for i, di in enumerate(d):
            p = p0 + i
            if best == 0 or (di * best <= min_d * p if variant == "last_tie" else di * best < min_d * p):
                best, min_d = p, di
    worst, max_d = 255, 0
    for i, di in enumerate(d):
        p = p0 + i
        if di * worst >= max_d * p if variant == "max_last" else di * worst > max_d * p:
            worst, max_d = p, di
    return best, min_d // best, worst, max_d // worst


def select_rows(D, p0):
    """select() on every row of the int64 array D (vectors x lags) at once: the same scan, one lag at a time over all rows.
    d <= 65535 p and p < 2^12, so no product exceeds 2^40.  Returns arrays (best, minDiff, worst, maxDiff)."""
    D = np.asarray(D, np.int64)
    n = D.shape[0]
    best, min_d = np.zeros(n, np.int64), np.ones(n, np.int64)
    worst, max_d = np.full(n, 255, np.int64), np.zeros(n, np.int64)
    for j in range(D.shape[1]):
        p, d = p0 + j, D[:, j]
        take = (best == 0) | (d * best < min_d * p)
        best, min_d = np.where(take, p, best), np.where(take, d, min_d)
        take = d * worst > max_d * p
        worst, max_d = np.where(take, p, worst), np.where(take, d, max_d)
    return best, min_d // best, worst, max_d // worst


def first_key_rows(D, p0):
    """The first lag holding the minimal key floor(d 2^16 / p) of every row, and that key."""
    D = np.asarray(D, np.int64)
    keys = (D << 16) // (p0 + np.arange(D.shape[1], dtype=np.int64))
    i = keys.argmin(axis=1)
    return p0 + i, keys[np.arange(D.shape[0]), i]


def prev_period_taken(min_diff, max_diff, prev_period, prev_min_diff, rule="exact", d=None, p0=0):
    """True where the previous period is returned instead of the new one."""
    if prev_period == 0:
        return False
    if not (min_diff > 1 if rule == "C_gt" else min_diff >= 1):
        return False
    if rule in ("ballot", "ballot_3m"):
        need = 3 * min_diff + (1 if rule == "ballot" else 0)
        clear = any(di >= need * (p0 + i) for i, di in enumerate(d))
    else:
        clear = max_diff >= 3 * min_diff if rule == "A_ge" else max_diff > 3 * min_diff
    if clear:
        return False
    if 2 * min_diff < 3 * prev_min_diff if rule == "B_lt" else 2 * min_diff <= 3 * prev_min_diff:
        return False
    return True


def search_census(d, p0):
    """What an approximate selector would have to get right in this search (d: the sums of lags p0 ...)."""
    n = len(d)
    best, _, worst, _ = select(d, p0)
    keys = [(di << 16) // (p0 + i) for i, di in enumerate(d)]
    kmin = min(keys)
    tied = [i for i in range(n) if keys[i] == kmin]
    f = tied[0]
    c = {"lags": n}
    c["key_tie"] = len(tied) > 1
    c["key_tie_unequal"] = any(d[i] * (p0 + f) != d[f] * (p0 + i) for i in tied)
    c["key_first_wrong"] = p0 + f != best
    c["key_tie_cross64"] = tied[0] // 64 != tied[-1] // 64
    c["key_tie_unequal_cross64"] = c["key_tie_unequal"] and c["key_tie_cross64"]
    # the general selector: every lag whose ratio lies within 1 + 2^-16 of the minimum (1 - 2^-16 of the maximum) is rescanned
    db, pb = d[best - p0], best
    wmin = [i for i in range(n) if d[i] * pb * 65536 <= db * (p0 + i) * 65537]
    c["win_min_unequal"] = any(d[i] * pb != db * (p0 + i) for i in wmin)
    c["win_min_first_wrong"] = p0 + wmin[0] != best
    c["win_min_cross64"] = len(wmin) > 1 and wmin[0] // 64 != wmin[-1] // 64
    if worst == 255 and all(di == 0 for di in d):
        c["all_zero"] = True
        c["win_max_unequal"] = c["win_max_first_wrong"] = c["win_max_cross64"] = False
    else:
        c["all_zero"] = False
        dw, pw = d[worst - p0], worst
        wmax = [i for i in range(n) if d[i] * pw * 65536 >= dw * (p0 + i) * 65535]
        c["win_max_unequal"] = any(d[i] * pw != dw * (p0 + i) for i in wmax)
        c["win_max_first_wrong"] = p0 + wmax[0] != worst
        c["win_max_cross64"] = len(wmax) > 1 and wmax[0] // 64 != wmax[-1] // 64
    return c


def rule_census(min_diff, max_diff, prev_period, prev_min_diff):
    """Which edge of the three inequalities the step sits on, whether the previous period is taken, and which strictness flips would
    change that.  A (maxDiff > 3 minDiff) and B (2 minDiff <= 3 prevMinDiff): "eq", "above" = the first attainable value above, or None.
    C (minDiff >= 1): "eq" at minDiff = 1, "below" at minDiff = 0, or None."""
    c = {"live": prev_period != 0}
    # (A and B are asked only behind minDiff >= 1: with minDiff = 0 the step sits on 0 = 0 trivially)
    c["A"] = {0: "eq", 1: "above"}.get(max_diff - 3 * min_diff) if min_diff else None
    c["B"] = {0: "eq", 1: "above", 2: "above"}.get(2 * min_diff - 3 * prev_min_diff) if min_diff else None   # 2 minDiff is even: 3 q + 1 or 3 q + 2
    c["C"] = {1: "eq", 0: "below"}.get(min_diff)
    c["taken"] = prev_period_taken(min_diff, max_diff, prev_period, prev_min_diff)
    c["decisive"] = [r for r in ("A_ge", "B_lt", "C_gt")
                     if prev_period_taken(min_diff, max_diff, prev_period, prev_min_diff, r) != c["taken"]]
    return c


def find_pitch_period(window, rate, channels, prev_period, prev_min_diff, select_variant="exact", rule="exact", census=None):
    """The two-stage search on `window` (interleaved, at least maxRequired frames) and the previous-period rule.
    Returns (period, returned period, minDiff, maxDiff)."""
    min_p, max_p, max_req, skip = limits(rate)
    if channels == 1 and skip == 1:
        d, lo = amdf(window, min_p, max_p), min_p
    else:
        dn = down_sample(window, skip, channels, max_req // skip)
        lo = min_p // skip
        d = amdf(dn, lo, max_p // skip)
        if skip != 1:
            if census is not None:
                census["coarse"] = search_census(d, lo)
            period = select(d, lo, select_variant)[0] * skip
            lo, hi = max(period - 4 * skip, min_p), min(period + 4 * skip, max_p)
            mono = window if channels == 1 else down_sample(window, 1, channels, max_req)
            d = amdf(mono, lo, hi)
    period, min_diff, _, max_diff = select(d, lo, select_variant)
    taken = prev_period_taken(min_diff, max_diff, prev_period, prev_min_diff, rule, d, lo)
    if census is not None:
        census["final"] = search_census(d, lo)
        census["rule"] = rule_census(min_diff, max_diff, prev_period, prev_min_diff)
    return period, (prev_period if taken else period), min_diff, max_diff


def step_lengths(period, speed):
    """(frames cross-faded, frames copied through afterwards, input frames consumed, output frames produced) of one step;
    float32 arithmetic as written."""
    f, one, two = np.float32, np.float32(1.0), np.float32(2.0)
    s, p = f(speed), f(period)
    if s > one:
        if s >= two:
            n, rem = int(p / (s - one)), 0
        else:
            n, rem = period, int(p * (two - s) / (s - one))
        return n, rem, period + n, n
    if s < f(0.5):
        n, rem = int(p * s / (one - s)), 0
    else:
        n, rem = period, int(p * (two * s - one) / (one - s))
    return n, rem, n, period + n


def walk(x, rate, channels, speed, select="exact", rule="exact", census=True):
    """The position walk of ONE write of the interleaved samples x, before any flush.  Returns a dict: `periods` (the period
    each step returned), `chosen` (the search's own winner), `positions` (the input frame of each step), `frames_out`, `consumed`
    and, with census=True, `census` (one dict per step: search_census of the searches, rule_census)."""
    x = np.asarray(x, np.int64)
    n_in = x.size // channels
    _, _, max_req, _ = limits(rate)
    out = {"periods": [], "chosen": [], "positions": [], "min_diff": [], "max_diff": [], "census": [], "frames_out": 0, "consumed": 0}
    if n_in < max_req:
        return out
    pos, remaining, prev_period, prev_min_diff, frames = 0, 0, 0, 0, 0
    while True:
        if remaining > 0:
            n = min(remaining, max_req)
            remaining -= n
            pos += n
            frames += n
        else:
            cen = {} if census else None
            period, ret, min_diff, max_diff = find_pitch_period(x[pos * channels:(pos + max_req) * channels], rate, channels,
                                                                prev_period, prev_min_diff, select, rule, cen)
            prev_period, prev_min_diff = period, min_diff
            out["periods"].append(ret); out["chosen"].append(period); out["positions"].append(pos)
            out["min_diff"].append(min_diff); out["max_diff"].append(max_diff)
            if census:
                out["census"].append(cen)
            n, remaining, used, made = step_lengths(ret, speed)
            frames += made
            if n == 0:
                break     # a failed step: the write ends and consumes nothing (a slow-down step has emitted its period by then)
            pos += used
        if pos + max_req > n_in:
            out["consumed"] = pos
            break
    out["frames_out"] = frames
    return out


COUNTS = ("steps", "key_tie", "key_tie_unequal", "key_first_wrong", "key_tie_unequal_cross64", "coarse_key_tie_unequal",
          "win_min_unequal", "win_min_first_wrong", "win_max_unequal", "win_max_first_wrong", "win_cross64", "all_zero",
          "A_eq", "A_above", "B_eq", "B_above", "C_eq", "C_below", "A_eq_taken", "B_above_taken", "C_eq_taken", "taken", "decisive_A_ge", "decisive_B_lt", "decisive_C_gt")


def tally(census):
    """Counts over the steps of one walk (keys: COUNTS); the rule's edges are counted on steps with a previous period only."""
    t = dict.fromkeys(COUNTS, 0)
    for c in census:
        t["steps"] += 1
        f, r = c["final"], c["rule"]
        for k in ("key_tie", "key_tie_unequal", "key_first_wrong", "key_tie_unequal_cross64", "win_min_unequal",
                  "win_min_first_wrong", "win_max_unequal", "win_max_first_wrong", "all_zero"):
            t[k] += bool(f[k])
        t["win_cross64"] += bool((f["win_min_unequal"] and f["win_min_cross64"]) or (f["win_max_unequal"] and f["win_max_cross64"]))
        t["coarse_key_tie_unequal"] += bool("coarse" in c and c["coarse"]["key_tie_unequal"])
        if r["live"]:
            for k in "ABC":
                if r[k]:
                    t[k + "_" + r[k]] += 1
                    if r["taken"] and k + "_" + r[k] + "_taken" in t:   # (the other edges exclude the previous period by themselves)
                        t[k + "_" + r[k] + "_taken"] += 1
            t["taken"] += bool(r["taken"])
            for m in r["decisive"]:
                t["decisive_" + m] += 1
    return t
