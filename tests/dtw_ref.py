"""The definition of batch dynamic time warping (include/speedy_hip.h "BATCH DTW"): Python and numpy float32 SCALARS only, one
operation and one rounding at a time -- no GPU, no oracle, no vectorised sum whose order numpy chooses.  Written from the
reference: EuclideanDistance (sonic_test.cc:200-209), DynamicTimeWarping::ComputeFromCostMatrix and BestPathSequence
(dynamic_time_warping.cc:76-132), LinearSlope, LinearSlopeEverywhere, VectorMean and VectorStandardDeviation
(sonic_test.cc:86-133).  tests/test_dtw_definition.py pins it; tests/test_gpu_dtw.py holds spx_batch_dtw to it bit for bit.

Domain: finite inputs whose accumulated costs stay finite.  A zero denominator (n_path = 1, a window in which `a` does not
advance, n_local = 0) gives what IEEE arithmetic gives -- NaN or an infinity; compare bit patterns, any NaN equal to any NaN
(same_bits)."""
import numpy as np

F = np.float32

# the mutants of tests/test_dtw_definition.py: the tie rule made non-strict, up and left swapped in the direction test
STRICT, NONSTRICT_TIES, SWAPPED_UP_LEFT = 0, 1, 2


def local_cost(ra, rb):
    """d = sqrtf(sum over k, in order, of (a[k] - b[k])^2): every operation rounded to float32, no fused multiply-add."""
    s = F(0.0)
    for x, y in zip(ra, rb):
        t = F(x - y)
        s = F(s + F(t * t))
    return F(np.sqrt(s))


def direction(up, left, diag, rule=STRICT):
    """ArgMin(up, diag, left), dynamic_time_warping.cc:66-74: -1 up, +1 left, 0 diagonal; strict, so ties go along the diagonal."""
    if rule == NONSTRICT_TIES:
        if up <= diag and up <= left:
            return -1
        if left <= up and left <= diag:
            return 1
        return 0
    if rule == SWAPPED_UP_LEFT:
        up, left = left, up
    if up < diag and up < left:
        return -1
    if left < up and left < diag:
        return 1
    return 0


def forward(a, b, rule=STRICT, d_matrix=None):
    """(cost, directions): the recurrence over the local costs, float32.  d_matrix: the local costs if the caller has them
    already (tests/dtw_cases.py local_costs: the same operations in the same order, a whole matrix per operation)."""
    n_a, n_b = len(a), len(b)
    rows_a = [[F(v) for v in r] for r in a] if d_matrix is None else None
    rows_b = [[F(v) for v in r] for r in b] if d_matrix is None else None
    dirs = np.zeros((n_a, n_b), np.int8)
    prev = None
    for i in range(n_a):
        cur = [None] * n_b
        for j in range(n_b):
            d = local_cost(rows_a[i], rows_b[j]) if d_matrix is None else F(d_matrix[i][j])
            if i == 0 and j == 0:
                cur[j] = d
            elif i == 0:
                cur[j] = F(d + cur[j - 1])
                dirs[i, j] = 1
            elif j == 0:
                cur[j] = F(d + prev[j])
                dirs[i, j] = -1
            else:
                up, left, diag = prev[j], cur[j - 1], prev[j - 1]
                cur[j] = F(d + min(min(up, left), diag))
                dirs[i, j] = direction(up, left, diag, rule)
        prev = cur
    return prev[n_b - 1], dirs


def back_trace(dirs):
    """BestPathSequence: [(i, j)] from (0, 0) to (n_a - 1, n_b - 1)."""
    i, j = dirs.shape[0] - 1, dirs.shape[1] - 1
    path = []
    while i >= 0 and j >= 0:
        path.append((i, j))
        d = dirs[i, j]
        if d <= 0:
            i -= 1
        if d >= 0:
            j -= 1
    return path[::-1]


def linear_slope(path):
    """LinearSlope with x = the a indices, y = the b indices: four float32 sums in path order, x*y and x*x exact integers."""
    n = F(len(path))
    sx, sy, sxy, sx2 = F(0), F(0), F(0), F(0)
    for x, y in path:
        x, y = int(x), int(y)
        sx = F(sx + F(x))
        sy = F(sy + F(y))
        sxy = F(sxy + F(x * y))
        sx2 = F(sx2 + F(x * x))
    with np.errstate(all="ignore"):
        return F(F(F(n * sxy) - F(sx * sy)) / F(F(n * sx2) - F(sx * sx)))


def local_slopes(path, half_width):
    """LinearSlopeEverywhere: window p covers entries p - h .. p + h - 1, p = h .. n_path - h - 1."""
    h = int(half_width)
    return [linear_slope(path[p - h:p + h]) for p in range(h, len(path) - h)]


def mean_std(slopes):
    """VectorMean and VectorStandardDeviation: ordered sums in a double, rounded to float32, divided by (float)n."""
    n = F(len(slopes))
    with np.errstate(all="ignore"):
        acc = np.float64(0.0)
        for s in slopes:
            acc = np.float64(acc + np.float64(s))
        mean = F(F(acc) / n)
        acc = np.float64(0.0)
        for s in slopes:
            diff = F(s - mean)
            acc = np.float64(acc + np.float64(F(diff * diff)))
        return mean, F(np.sqrt(F(F(acc) / n)))


def dtw(a, b, half_width=10, rule=STRICT, d_matrix=None):
    """Everything spx_batch_dtw leaves for one pair: dict(cost, slope, local_mean, local_std: float32; n_path, n_local: int;
    path: (n_path, 2) int32 of (a index, b index))."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    if a.ndim == 1:
        a = a[:, None]
    if b.ndim == 1:
        b = b[:, None]
    assert a.shape[1] == b.shape[1] and a.shape[0] >= 1 and b.shape[0] >= 1 and half_width >= 1
    with np.errstate(all="ignore"):
        cost, dirs = forward(a, b, rule, d_matrix)
    path = back_trace(dirs)
    slopes = local_slopes(path, half_width)
    mean, std = mean_std(slopes)
    return dict(cost=cost, slope=linear_slope(path), local_mean=mean, local_std=std, n_path=len(path), n_local=len(slopes),
                path=np.asarray(path, np.int32).reshape(len(path), 2))


def bits(v):
    return int(np.asarray(v, np.float32).view(np.uint32))


def same_bits(x, y):
    """Equal bit patterns; any NaN equals any NaN."""
    x, y = F(x), F(y)
    return bool((np.isnan(x) and np.isnan(y)) or bits(x) == bits(y))
