"""Planted time maps for spx_map_lookup (tests/test_gpu_map_lookup.py on the device, tests/test_time_map_lookup_definition.py on
the CPU): job tables and rows that the test writes itself -- the lookup kernel reads n_in, nonlinear and the rows and nothing else,
so no audio is processed.  B = 160 (a plan of 16 kHz).  Generated, deterministic, no fixture files.

A planted stream is (name, n_in, nonlinear factor, rows as Python integers); what each is for stands beside it."""
import numpy as np

B = 160
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def _steps(n, rise):
    return [k * rise for k in range(n)]


def streams():
    """[(name, n_in, nonlinear, rows)] -- every stream inside the lookups' domain (include/speedy_hip.h "TIME MAP")."""
    s = []
    # all flat except the last step: every inverse query lands in the last segment, every forward one before it gives 0
    s.append(("flat_then_step", 20 * B + 37, 1.0, [0] * 20 + [5000]))
    # flat runs in the middle, a flat pair directly before the last node; the last segment is exactly B long
    s.append(("flat_runs", 12 * B, 1.0, [0, 0, 0, 130, 130, 130, 130, 400, 520, 640, 811, 811, 1000]))
    s.append(("one_buffer", 200, 1.0, [0, 57]))                       # R = 1: nodes [0, n_in]
    s.append(("short_nonlinear", 159, 1.0, [45]))                     # R = 0, nonlinear: nodes [0, n_in] x [0, M[0]]
    s.append(("empty", 0, 1.0, [0]))                                  # n_in = 0
    s.append(("linear_one_frame", 1, 0.0, [1]))
    s.append(("linear", 4000, 0.0, [1143]))
    # last segments of length B + 1 and 2 B - 1 (length B: flat_runs)
    s.append(("last_B_plus_1", 5 * B + 1, 1.0, [0, 0, 71, 140, 233, 317]))
    s.append(("last_2B_minus_1", 6 * B - 1, 1.0, [0, 0, 71, 140, 233, 317]))
    # slopes 1 / 2000 (a row rises by 1 every 12.5 segments), 1 and 200
    s.append(("slope_1_2000", 100 * B, 1.0, [k * B // 2000 for k in range(101)]))
    s.append(("slope_1", 40 * B + 80, 1.0, _steps(40, B) + [40 * B + 80]))
    s.append(("slope_200", 50 * B + 77, 1.0, _steps(50, 200 * B) + [200 * (50 * B + 77)]))
    # the longest linear job the call takes, a count beyond 32 bits
    s.append(("linear_2_30", (1 << 30) - 1, 0.0, [1 << 32]))
    # the largest in-domain product: n_in * Y[-1] just below 2^63 (one segment, as wide as n_in and as high as Y[-1])
    n = (1 << 30) - 1
    s.append(("largest_product", n, 0.0, [I64_MAX // n]))
    return s


def long_stream():
    """100 001 rows: a binary search 17 levels deep.  Rises of 0 .. 6 frames in an irregular pattern (flat runs of every length up
    to 4), so that neighbouring nodes are told apart."""
    R = 100000
    rng = np.random.default_rng(20240)
    rise = rng.integers(0, 7, R).astype(np.int64)
    rise[rng.integers(0, R, R // 5)] = 0
    rows = np.concatenate([[0], np.cumsum(rise)])
    rows[-1] += 9
    return ("long", R * B, 1.0, [int(v) for v in rows])


def queries(name, n_in, nl, rows, spread=0, seed=7):
    """(t, u) int64 arrays for one stream: every node, each node +- 1, both ends out of range, INT64_MIN and INT64_MAX; every
    position of a short stream; of a long one `spread` positions drawn with a fixed seed.  Values are clipped to int64."""
    R = n_in // B if nl != 0 else 0
    X = [k * B for k in range(R)] + [n_in] if R >= 1 else [0, n_in]
    Y = list(rows) if R >= 1 else [0, rows[0]]
    ends_t = [-5, -1, n_in + 1, n_in + 1000, I64_MIN, I64_MAX]
    ends_u = [-5, -1, Y[-1] + 1, Y[-1] + 77, I64_MIN, I64_MAX]
    t = X + [v - 1 for v in X] + [v + 1 for v in X] + ends_t
    u = Y + [v - 1 for v in Y] + [v + 1 for v in Y] + ends_u
    rng = np.random.default_rng([seed, len(rows), n_in % 9973])
    if n_in <= 20000:
        t += list(range(n_in + 1))
    elif spread:
        t += [int(v) for v in rng.integers(0, n_in + 1, spread)]
    if Y[-1] <= 20000:
        u += list(range(Y[-1] + 1))
    elif spread:
        u += [int(v) for v in rng.integers(0, Y[-1] + 1, spread)]
    clip = lambda v: min(max(v, I64_MIN), I64_MAX)   # noqa: E731
    return np.asarray([clip(v) for v in t], np.int64), np.asarray([clip(v) for v in u], np.int64)
