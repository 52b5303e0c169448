"""GPU: spx_map_lookup on PLANTED maps (tests/time_map_planted.py) against the header's text in Python integers
(tests/time_map_ref.py ExactMap) -- integer equality, both directions, nothing skipped.

The call gets a job table and a `map` tensor that the test writes itself: the kernel reads n_in, nonlinear and the rows and nothing
else, so no audio is processed and every shape of map can be planted -- flat runs, a last segment of every length, R = 1 and R = 0,
slopes from 1 / 2000 to 200, counts beyond 32 bits, 100 001 rows, and the job whose product lies just below 2^63 (the edge of the
domain the header states).  The launch shapes reach what real batches never did: a thread that strides over its stream's queries,
both clamps of the block count, the second launch behind 65 535 streams.  Every case prints and asserts the block count per stream
the call chose (spx_debug_last_lookup_grid) and how many queries each thread served; `r` is pre-filled with a canary, so an
unanswered query is seen."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_map_planted as P  # noqa: E402
import time_map_ref as tm  # noqa: E402

pytestmark = pytest.mark.gpu

R_CANARY = -0x5a5a5a5a5a5a5a5a
THREADS = 256           # SPX_MAP_THREADS
_EXACT = {}


def exact(s):
    """The Python-integer map of a planted stream, once per module."""
    if s[0] not in _EXACT:
        _EXACT[s[0]] = tm.ExactMap(s[3], P.B, s[1], s[2])
    return _EXACT[s[0]]


@pytest.fixture(scope="module")
def plan():
    from speedy_amd.batch import Plan
    p = Plan(16000, False)
    assert p.B == P.B == 160
    yield p
    p.close()


class Planted:
    """A job table and a map tensor over planted streams [(name, n_in, nonlinear, rows)]."""

    def __init__(self, plan, streams):
        import torch
        from speedy_amd._lib import StreamJob
        self.plan, self.n = plan, len(streams)
        self.jobs = (StreamJob * self.n)()
        for j, (_, n_in, nl, _) in zip(self.jobs, streams):
            j.n_in, j.channels, j.speed, j.nonlinear = n_in, 1, 2.0, nl
        rows = np.concatenate([np.asarray(s[3], np.int64) for s in streams])
        counts = [plan.L.spx_plan_map_rows(plan.h, s[1], s[2]) for s in streams] if self.n <= 4096 else [1] * self.n
        assert counts == [len(s[3]) for s in streams] and rows.size == sum(counts)
        self.d_map = torch.from_numpy(rows).cuda()

    def lookup(self, queries, inverse):
        """One spx_map_lookup over per-stream int64 query arrays: (answers per stream, blocks per stream, launches)."""
        import torch
        L = self.plan.L
        assert len(queries) == self.n
        offs = np.zeros(self.n + 1, np.int64)
        offs[1:] = np.cumsum([q.size for q in queries])
        total = int(offs[-1])
        d_off = torch.from_numpy(offs).cuda()
        d_q = torch.from_numpy(np.concatenate(queries) if total else np.zeros(1, np.int64)).cuda()
        d_r = torch.full_like(d_q, R_CANARY)
        rc = L.spx_map_lookup(self.plan.h, self.jobs, self.n, self.d_map.data_ptr(), d_off.data_ptr(), d_q.data_ptr(), d_r.data_ptr(),
                              1 if inverse else 0, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, L.spx_last_error().decode()
        torch.cuda.synchronize()
        launches = C.c_int(0)
        gx = L.spx_debug_last_lookup_grid(C.byref(launches))
        r = d_r.cpu().numpy()
        return [r[int(offs[i]):int(offs[i + 1])] for i in range(self.n)], gx, launches.value


def rounds(gx, most):
    """How many queries the busiest thread of a stream served: it starts at one and strides gx * 256 at a time."""
    return -(-most // (gx * THREADS))


def check_stream(s, t, u, fw, iv, tag):
    """Exact answers, no canary left, both directions non-decreasing in the query, the ends."""
    m = exact(s)
    assert fw.size == t.size and iv.size == u.size, tag
    assert not (fw == R_CANARY).any() and not (iv == R_CANARY).any(), (tag, "unanswered queries")
    want_f, want_i = [m.forward(v) for v in t.tolist()], [m.inverse(v) for v in u.tolist()]
    bad = [k for k, (a, b) in enumerate(zip(fw.tolist(), want_f)) if a != b]
    assert bad == [], (tag, "forward", [(int(t[k]), int(fw[k]), want_f[k]) for k in bad[:4]])
    bad = [k for k, (a, b) in enumerate(zip(iv.tolist(), want_i)) if a != b]
    assert bad == [], (tag, "inverse", [(int(u[k]), int(iv[k]), want_i[k]) for k in bad[:4]])
    assert (np.diff(fw[np.argsort(t, kind="stable")]) >= 0).all() and (np.diff(iv[np.argsort(u, kind="stable")]) >= 0).all(), tag


def test_one_stream_of_600000_queries_strides_three_times_at_1024_blocks(plan):
    """n = 1: the upper clamp of the block count, 262 144 threads for 600 000 queries; 100 001 rows, a search 17 levels deep.  The
    queries: every node and its two neighbours, both ends out of range, INT64_MIN / INT64_MAX, and a fixed-seed spread."""
    s = P.long_stream()
    t, u = P.queries(*s, spread=600000 - 3 * 100001 - 6)
    assert t.size == u.size == 600000
    pl = Planted(plan, [s])
    (fw,), gx, launches = pl.lookup([t], False)
    (iv,), gx_i, _ = pl.lookup([u], True)
    print("n = 1: blocks per stream", gx, "threads", gx * THREADS, "queries per thread", rounds(gx, t.size), "launches", launches)
    assert gx == gx_i == 1024 and launches == 1 and rounds(gx, t.size) == 3
    check_stream(s, t, u, fw, iv, "long")


def test_eight_streams_300000_queries_in_one_and_none_in_another(plan):
    """n = 8: 512 blocks per stream, 131 072 threads.  The stream with 300 000 queries is the linear job of 2^30 - 1 frames and a
    count of 2^32 (two nodes: all but twelve of its queries are the fixed-seed spread); one stream asks nothing."""
    by = {x[0]: x for x in P.streams()}
    streams = [by[k] for k in ("linear_2_30", "flat_runs", "one_buffer", "short_nonlinear", "empty", "slope_200", "last_2B_minus_1",
                               "slope_1_2000")]
    assert len(streams) == 8
    qs = [P.queries(*x, spread=300000 - 12) for x in streams]
    silent = 3
    empty = np.zeros(0, np.int64)
    qs[silent] = (empty, empty)
    assert qs[0][0].size == qs[0][1].size == 300000
    pl = Planted(plan, streams)
    fw, gx, launches = pl.lookup([q[0] for q in qs], False)
    iv, gx_i, _ = pl.lookup([q[1] for q in qs], True)
    print("n = 8: blocks per stream", gx, "threads", gx * THREADS, "queries per thread", rounds(gx, 300000), "launches", launches)
    assert gx == gx_i == 512 and launches == 1 and rounds(gx, 300000) == 3
    assert fw[silent].size == 0 and iv[silent].size == 0
    for i, x in enumerate(streams):
        check_stream(x, qs[i][0], qs[i][1], fw[i], iv[i], x[0])


def test_every_planted_map_and_the_headers_properties(plan):
    """All fifteen planted maps in one call, every query of tests/time_map_planted.py: exact answers; both directions
    non-decreasing; forward(inverse(u)) <= u, the inner lookup's answers fed back through the device; inverse(Y[-1]) = n_in and
    forward(n_in) = Y[-1].  Among them the job with n_in * Y[-1] just below 2^63: the edge of the domain include/speedy_hip.h states."""
    streams = P.streams() + [P.long_stream()]
    assert len(streams) == 15
    qs = [P.queries(*x, spread=20000) for x in streams]
    pl = Planted(plan, streams)
    fw, gx, launches = pl.lookup([q[0] for q in qs], False)
    iv, _, _ = pl.lookup([q[1] for q in qs], True)
    back, _, _ = pl.lookup(iv, False)
    print("n = 15: blocks per stream", gx, "launches", launches, "queries", sum(q[0].size + q[1].size for q in qs))
    assert gx == 4096 // 15 and launches == 1
    for i, x in enumerate(streams):
        m = exact(x)
        check_stream(x, qs[i][0], qs[i][1], fw[i], iv[i], x[0])
        assert m.largest_product() < 1 << 63, x[0]
        assert (back[i] <= np.clip(qs[i][1], 0, m.Y[-1])).all(), (x[0], "forward(inverse(u)) > u")
        L = m.L                                        # (the queries begin with the nodes: index L - 1 holds the last one)
        assert int(qs[i][0][L - 1]) == x[1] and int(fw[i][L - 1]) == (m.Y[-1] if x[1] else 0), x[0]        # forward(n_in) = Y[-1]
        assert int(qs[i][1][L - 1]) == m.Y[-1] and int(iv[i][L - 1]) == x[1], x[0]                          # inverse(Y[-1]) = n_in
    big = [m for m in (exact(x) for x in streams) if m.largest_product() > (1 << 63) - (1 << 31)]
    assert len(big) == 1 and big[0].n_in * big[0].Y[-1] == big[0].largest_product()


def test_2048_streams_of_2500_queries_at_four_blocks(plan):
    """The lower clamp: 4 096 / 2 048 = 2 blocks would be asked for, 4 are launched; 1 024 threads stride over 2 500 queries.  The
    fourteen planted maps round-robin, each with its own queries: a stream served with a neighbour's table or rows shows."""
    kinds = P.streams()
    per = {x[0]: tuple(np.resize(q, 2500) for q in P.queries(*x, spread=2500)) for x in kinds}
    want = {x[0]: ([exact(x).forward(v) for v in per[x[0]][0].tolist()], [exact(x).inverse(v) for v in per[x[0]][1].tolist()]) for x in kinds}
    streams = [kinds[(i * 5 + i // 14) % 14] for i in range(2048)]
    assert len({x[0] for x in streams}) == 14
    pl = Planted(plan, streams)
    fw, gx, launches = pl.lookup([per[x[0]][0] for x in streams], False)
    iv, gx_i, _ = pl.lookup([per[x[0]][1] for x in streams], True)
    print("n = 2048: blocks per stream", gx, "threads", gx * THREADS, "queries per thread", rounds(gx, 2500), "launches", launches)
    assert gx == gx_i == 4 and launches == 1 and rounds(gx, 2500) == 3
    bad = [(i, x[0]) for i, x in enumerate(streams) if fw[i].tolist() != want[x[0]][0] or iv[i].tolist() != want[x[0]][1]]
    assert bad == [], bad[:8]


def test_65600_one_row_streams_take_a_second_launch(plan):
    """More streams than the grid's second dimension holds: 65 535 in the first launch, 65 in the second.  Linear jobs, every one
    with its own length and its own row, three queries each: a slip in stream0 + blockIdx.y, or a stream served twice or never,
    changes an answer or leaves the canary."""
    n = 65600
    streams = [("row%d" % i, 1000 + i, 0.0, [500 + 3 * i]) for i in range(n)]
    t = [np.asarray([0, (1000 + i) // 2 + i % 7, 1000 + i], np.int64) for i in range(n)]
    u = [np.asarray([0, (500 + 3 * i) // 2 + i % 5, 500 + 3 * i], np.int64) for i in range(n)]
    pl = Planted(plan, streams)
    fw, gx, launches = pl.lookup(t, False)
    iv, gx_i, launches_i = pl.lookup(u, True)
    print("n = 65600: blocks per stream", gx, "launches", launches, "queries per thread", rounds(gx, 3))
    assert gx == gx_i == 4 and launches == launches_i == 2
    fw, iv = np.concatenate(fw), np.concatenate(iv)
    assert not (fw == R_CANARY).any() and not (iv == R_CANARY).any()
    want_f, want_i = [], []
    for i, (name, n_in, nl, rows) in enumerate(streams):
        m = tm.ExactMap(rows, P.B, n_in, nl)
        want_f += [m.forward(v) for v in t[i].tolist()]
        want_i += [m.inverse(v) for v in u[i].tolist()]
    bad = np.nonzero((fw != np.asarray(want_f, np.int64)) | (iv != np.asarray(want_i, np.int64)))[0]
    assert bad.size == 0, ("first differing streams", (bad[:8] // 3).tolist())
    assert len(set(want_f[1::3])) > 30000 and len(set(want_i[1::3])) > 30000           # the answers tell the streams apart


def test_a_stream_with_unspecified_rows_harms_no_other(plan):
    """Rows that decrease and rows that are negative (a job whose count came back negative has such) in ONE stream of a batch.
    Read in spx_map_lookup_kernel before this was run: the forward segment index is clamped to [0, L - 2] and the inverse search
    keeps 0 <= lo < mid < hi <= L - 1, so every load lies inside the stream's own rows whatever they hold; the forward divisor is
    a segment's width (at least B, or n_in > 0 where R = 0 -- n_in = 0 returns before it), the inverse one is used only where
    y1 > y0.  So: return code 0, a clean synchronise, exact answers for every other stream.  Nothing is asserted of the answers
    of the stream itself but that each query got one."""
    import torch
    odd = ("unspecified", 10 * P.B + 40, 1.0, [0, 500, 200, -7, 300, 300, 100, -40000, 900, 10, 5])
    good = [x for x in P.streams() if x[0] in ("flat_runs", "slope_1", "one_buffer", "linear")]
    streams = good[:2] + [odd] + good[2:]
    qs = [P.queries(*x) for x in good]
    odd_q = (np.arange(-10, odd[1] + 10, dtype=np.int64), np.arange(-50000, 2000, 7, dtype=np.int64))
    qs = qs[:2] + [odd_q] + qs[2:]
    pl = Planted(plan, streams)
    fw, gx, _ = pl.lookup([q[0] for q in qs], False)
    iv, _, _ = pl.lookup([q[1] for q in qs], True)
    torch.cuda.synchronize()
    print("unspecified rows: blocks per stream", gx)
    for i, x in enumerate(streams):
        if x[0] == "unspecified":
            assert not (fw[i] == R_CANARY).any() and not (iv[i] == R_CANARY).any()
        else:
            check_stream(x, qs[i][0], qs[i][1], fw[i], iv[i], x[0])
