"""Census of the pitch decision (tests/pitch_ref.py) over the signals of tests/test_gpu_fuzz.py::_cases, seeds 1 - 6, and over the
directed signals of tests/pitch_inputs.py -- the tables of profiles/pitch_decision.txt.  CPU only:  python tools/pitch_census.py

Per sample rate: the pitch steps of ONE write of each signal at its case's speed (a nonlinear job is walked at its global speed) and
how many of them have lags of equal key floor(d 2^16 / p) and unequal ratio, have another lag than the exact choice first among
those, reach the general selector's ratio window likewise, or sit on an edge of the previous-period rule.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pitch_inputs  # noqa: E402
import pitch_ref as R  # noqa: E402

COLS = ("steps", "key_tie", "key_tie_unequal", "key_first_wrong", "key_tie_unequal_cross64", "coarse_key_tie_unequal", "win_min_first_wrong",
        "win_max_first_wrong", "all_zero", "A_eq", "A_above", "B_eq", "B_above", "C_eq", "taken", "decisive_A_ge", "decisive_B_lt",
        "decisive_C_gt")


def show(title, rows):
    print(title)
    print("%-14s" % "" + " ".join("%9s" % c[:9] for c in COLS))
    for key in sorted(rows):
        print("%-14s" % str(key) + " ".join("%9d" % rows[key][c] for c in COLS))
    print()


def add(rows, key, t):
    r = rows.setdefault(key, dict.fromkeys(R.COUNTS, 0))
    for k, v in t.items():
        r[k] += v


def main():
    print("columns: " + ", ".join(COLS) + "\n")
    import test_gpu_fuzz as F
    rows, kinds = {}, {}
    for seed in range(1, 7):
        for i, rate, ch, kind, n, speed, nl, fb, mm, rng in F._cases(seed, 21):
            x = F._signal(kind, n, rate, ch, rng)
            if abs(speed - 1.0) < 1e-5:
                continue
            t = R.tally(R.walk(x, rate, ch, speed)["census"])
            add(rows, rate, t)
            add(kinds, kind, t)
    show("tests/test_gpu_fuzz.py::_cases, seeds 1 - 6, by sample rate", rows)
    show("... by kind of signal", kinds)
    rows, names = {}, {}
    for name, rate, ch, x in pitch_inputs.directed():
        for speed in (2.0, 1.3):
            t = R.tally(R.walk(x, rate, ch, speed)["census"])
            add(rows, rate, t)
            add(names, name, t)
    show("tests/pitch_inputs.py directed(), speeds 2.0 and 1.3, by sample rate", rows)
    show("... by signal", names)


if __name__ == "__main__":
    main()
