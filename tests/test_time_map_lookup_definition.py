"""CPU: the time map's lookups as numpy states them (tests/time_map_ref.py forward / inverse, int64) against the same text in Python
integers (ExactMap: unbounded, // on non-negative operands, bisect_right) on every planted map of tests/time_map_planted.py, and
the properties include/speedy_hip.h claims of them.  Integer equality; nothing is skipped."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_map_planted as P  # noqa: E402
import time_map_ref as tm  # noqa: E402


def _all():
    return P.streams() + [P.long_stream()]


def test_the_planted_maps_are_what_they_are_planted_for():
    by = {s[0]: s for s in _all()}
    assert len(by) == len(_all())
    for name, n_in, nl, rows in _all():
        assert len(rows) == tm.map_rows(P.B, n_in, nl), name
        m = tm.ExactMap(rows, P.B, n_in, nl)                      # (asserts rows that never decrease, Y[0] >= 0)
        assert m.largest_product() <= P.I64_MAX, name             # inside the domain
        assert 0 <= n_in < 1 << 30, name
    last = lambda n: (lambda m: m.X[-1] - m.X[-2])(tm.ExactMap(by[n][3], P.B, by[n][1], by[n][2]))   # noqa: E731
    assert (last("flat_runs"), last("last_B_plus_1"), last("last_2B_minus_1")) == (P.B, P.B + 1, 2 * P.B - 1)
    rows = by["flat_runs"][3]
    assert rows[-3] == rows[-2] < rows[-1] and rows[3:7] == [130] * 4
    assert by["flat_then_step"][3][:-1] == [0] * 20
    assert by["one_buffer"][1] // P.B == 1 and by["short_nonlinear"][1] == 159 and by["empty"][1] == 0
    assert by["linear_2_30"][1] == (1 << 30) - 1 and by["linear_2_30"][3] == [1 << 32]
    # the domain's edge: this product fits, one more output frame does not
    name, n, nl, rows = by["largest_product"]
    assert n * rows[0] <= P.I64_MAX < n * (rows[0] + 1)
    assert len(P.long_stream()[3]) == 100001 and (100001 - 1).bit_length() == 17      # 17 halvings of [0, L - 1]
    slope = {n: tm.ExactMap(by[n][3], P.B, by[n][1], by[n][2]) for n in ("slope_1_2000", "slope_1", "slope_200")}
    assert slope["slope_1_2000"].Y[-1] * 2000 == slope["slope_1_2000"].n_in
    assert slope["slope_1"].Y[-1] == slope["slope_1"].n_in and slope["slope_200"].Y[-1] == 200 * slope["slope_200"].n_in
    assert slope["slope_200"].Y[1] - slope["slope_200"].Y[0] == 200 * P.B


def test_numpy_lookups_equal_the_python_integer_lookups_on_every_planted_map():
    seen = 0
    for name, n_in, nl, rows in _all():
        t, u = P.queries(name, n_in, nl, rows, spread=20000)
        assert t.size >= 9 and u.size >= 9
        fw = tm.forward(np.asarray(rows, np.int64), P.B, n_in, nl, t)
        iv = tm.inverse(np.asarray(rows, np.int64), P.B, n_in, nl, u)
        assert fw.tolist() == tm.forward_exact(rows, P.B, n_in, nl, t.tolist()), name
        assert iv.tolist() == tm.inverse_exact(rows, P.B, n_in, nl, u.tolist()), name
        seen += 1
    assert seen == 15


def test_the_headers_properties_hold_of_the_definition():
    """Both directions non-decreasing in the query, forward(inverse(u)) <= u, inverse(Y[-1]) = n_in, forward(n_in) = Y[-1]."""
    for name, n_in, nl, rows in _all():
        m = tm.ExactMap(rows, P.B, n_in, nl)
        t, u = P.queries(name, n_in, nl, rows, spread=20000)
        ts, us = sorted(t.tolist()), sorted(u.tolist())
        fw, iv = [m.forward(v) for v in ts], [m.inverse(v) for v in us]
        assert all(a <= b for a, b in zip(fw, fw[1:])), name
        assert all(a <= b for a, b in zip(iv, iv[1:])), name
        assert all(m.forward(x) <= min(max(v, 0), m.Y[-1]) for v, x in zip(us, iv)), name
        assert m.inverse(m.Y[-1]) == n_in and m.forward(n_in) == (m.Y[-1] if n_in else 0), name


def test_beyond_the_domain_int64_differs_from_the_definition():
    """Teeth for the domain sentence: one output frame above the planted edge the int64 product wraps and numpy's answer is no
    longer the definition's -- the bound is tight, not merely sufficient."""
    name, n, nl, rows = [s for s in P.streams() if s[0] == "largest_product"][0]
    over = [rows[0] + 1]
    assert n * over[0] > P.I64_MAX
    with np.errstate(over="ignore"):
        got = tm.forward(np.asarray(over, np.int64), P.B, n, nl, np.asarray([n], np.int64))
    assert got.tolist() != tm.forward_exact(over, P.B, n, nl, [n]) == [over[0]]
