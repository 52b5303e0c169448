"""spx_edit_index and spx_edit_lookup on the MI355X: every answer and every record compared for equality.

The expected answers are tests/edit_lookup_ref.py's (Python integers; tests/test_edit_lookup_definition.py holds its searched form to
an enumeration on the CPU).  Two kinds of lists:
  planted   records the test writes itself -- the kernels read ops, n_ops, n_out and the job table's n_in and nonlinear, nothing else,
            so no audio is processed and every shape of list and launch can be set up: the index over streams of 0 to 5 000 records,
            records of one to three frames, cuts inside and before a record, 600 000 queries in a stream, 65 600 streams
  real      the lists spx_batch_run_edits writes for the directed jobs of tests/tsm_inputs.py, queried at EVERY input frame and
            EVERY output frame, and held against the time map of the same table by an exact inequality.
r, rec and the index are pre-filled with canaries, so an unanswered query or a store outside a range is seen."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_list_ref as E  # noqa: E402
import edit_lookup_ref as K  # noqa: E402
import test_gpu_edit_list as GE  # noqa: E402  (its jobs, and its definitions of their lists: computed once per process, shared)
import tsm_inputs as I  # noqa: E402

pytestmark = pytest.mark.gpu

R_CANARY = -0x5a5a5a5a5a5a5a5a
REC_CANARY = -0x5a5a5a5
IDX_CANARY = 0x5b5b5b5
OP_CANARY = -1234567
GUARD = 8
THREADS = 256           # SPX_ELOOK_THREADS
_TABLES = {}


@pytest.fixture(scope="module")
def plan():
    from speedy_amd.batch import Plan
    p = Plan(16000, False)
    assert p.B == 160
    yield p
    p.close()


# ------------------------------------------------------------------ planted lists ------------------------------------------------------------------

def stream(ops, n_in, n_out, nl=0.0, cap=None, n_ops=None):
    ops = np.asarray(ops, np.int32).reshape(-1, 4)
    return dict(ops=ops, n_in=int(n_in), n_out=int(n_out), nl=float(nl), cap=len(ops) if cap is None else int(cap),
                n_ops=len(ops) if n_ops is None else int(n_ops))


def ref(s):
    """The definition over a planted stream: the records the device may read are the first min(n_ops, cap)."""
    k = max(0, min(s["n_ops"], s["cap"]))
    return K.Lookup(s["ops"][:k].tolist(), s["n_out"], K.limit_of(s["n_in"], 16000, s["nl"] != 0.0), n_ops=s["n_ops"])


def tables(s, key):
    """(forward(p) for p = 0 .. L, inverse(u) for u = 0 .. n_out), answers and records as int64 arrays: once per key."""
    if key not in _TABLES:
        m = ref(s)
        _TABLES[key] = (np.asarray([m.forward(p) for p in range(m.L + 1)], np.int64).reshape(-1, 2),
                        np.asarray([m.inverse(u) for u in range(max(m.n_out, 0) + 1)], np.int64).reshape(-1, 2))
    return _TABLES[key]


def expected(s, key, q, inverse):
    """The definition's answers to the queries q: both clamps are the definition's (edit_lookup_ref.Lookup.forward / .inverse; the
    record-shape test asks Lookup itself about queries outside the range)."""
    t = tables(s, key)[1 if inverse else 0]
    return t[np.clip(q, 0, len(t) - 1)]


class Planted:
    """A job table, the records, counts and an index region over planted streams; guard values behind everything."""

    def __init__(self, plan, streams):
        import torch
        from speedy_amd._lib import StreamJob
        self.plan, self.streams, self.n = plan, streams, len(streams)
        self.jobs = (StreamJob * self.n)()
        for j, s in zip(self.jobs, streams):
            j.n_in, j.channels, j.speed, j.nonlinear = s["n_in"], 1, 2.0, s["nl"]
        self.caps = np.ascontiguousarray([s["cap"] for s in streams], np.int64)
        self.offs = np.concatenate([[0], np.cumsum(self.caps)]).astype(np.int64)
        host = np.full((int(self.offs[-1]) + GUARD, 4), OP_CANARY, np.int32)
        for s, o in zip(streams, self.offs):
            k = min(len(s["ops"]), s["cap"])
            host[o:o + k] = s["ops"][:k]
        self.d_ops = torch.from_numpy(host).cuda()
        self.d_nops = torch.from_numpy(np.asarray([s["n_ops"] for s in streams], np.int64)).cuda()
        self.d_nout = torch.from_numpy(np.asarray([s["n_out"] for s in streams], np.int64)).cuda()
        self.d_index = torch.full((int(self.offs[-1]) + GUARD,), IDX_CANARY, dtype=torch.int32).cuda()

    def caps_ptr(self):
        return self.caps.ctypes.data_as(C.POINTER(C.c_int64))

    def index(self):
        """spx_edit_index; returns the whole index buffer, guard included."""
        import torch
        L = self.plan.L
        rc = L.spx_edit_index(self.plan.h, self.jobs, self.n, self.d_ops.data_ptr(), self.caps_ptr(), self.d_nops.data_ptr(),
                              self.d_index.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, L.spx_last_error().decode()
        torch.cuda.synchronize()
        return self.d_index.cpu().numpy()

    def lookup(self, queries, inverse, **kw):
        """One spx_edit_lookup over per-stream int64 query arrays: (answers, records, blocks per stream, launches)."""
        import torch
        L = self.plan.L
        assert len(queries) == self.n
        offs = np.zeros(self.n + 1, np.int64)
        offs[1:] = np.cumsum([q.size for q in queries])
        total = int(offs[-1])
        d_off = torch.from_numpy(offs).cuda()
        d_q = torch.from_numpy(np.concatenate(queries + [np.zeros(GUARD, np.int64)])).cuda()
        d_r = torch.full_like(d_q, R_CANARY)
        d_rec = torch.full((total + GUARD,), REC_CANARY, dtype=torch.int32).cuda()
        a = dict(ops=self.d_ops.data_ptr(), caps=self.caps_ptr(), nops=self.d_nops.data_ptr(), nout=self.d_nout.data_ptr(),
                 index=None if inverse else self.d_index.data_ptr(), qoff=d_off.data_ptr(), q=d_q.data_ptr(), r=d_r.data_ptr(),
                 rec=d_rec.data_ptr(), jobs=self.jobs)
        a.update(kw)
        rc = L.spx_edit_lookup(self.plan.h, a["jobs"], self.n, a["ops"], a["caps"], a["nops"], a["nout"], a["index"], a["qoff"], a["q"],
                               a["r"], a["rec"], 1 if inverse else 0, torch.cuda.current_stream().cuda_stream)
        self.msg = L.spx_last_error().decode() if rc != 0 else ""
        torch.cuda.synchronize()
        r, rec = d_r.cpu().numpy(), d_rec.cpu().numpy()
        if rc != 0:
            return rc, r, rec
        launches = C.c_int(0)
        gx = L.spx_debug_last_edit_lookup_grid(C.byref(launches))
        assert (r[total:] == R_CANARY).all() and (a["rec"] is None or (rec[total:] == REC_CANARY).all()), "answers written behind the last range"
        assert not (r[:total] == R_CANARY).any() and (a["rec"] is None or not (rec[:total] == REC_CANARY).any()), "unanswered queries"
        cut = lambda x: [x[int(offs[i]):int(offs[i + 1])] for i in range(self.n)]  # noqa: E731
        return cut(r), cut(rec), gx, launches.value


def numpy_index(ops):
    """R and its running maximum in numpy, from the header's words."""
    ops = ops.astype(np.int64)
    a, b, n = ops[:, 1], ops[:, 2], ops[:, 3]
    h = (n + 1) // 2
    ra, rb = a + h - 1, b + n - 1
    R = np.where(b < 0, a + n - 1, np.where(n > h, np.maximum(ra, rb), ra))
    return np.maximum.accumulate(R) if len(R) else R


def records_for(R, seed):
    """Contiguous records whose largest sources are the sequence R: copies, cross-fades whose maximum lies on ramp a (n = 1, or b
    far below), cross-fades whose maximum lies on ramp b -- taken in turn."""
    rng = np.random.default_rng(seed)
    ops, at = [], 0
    for k, r in enumerate(R):
        n = int(rng.integers(1, 90))
        kind = k % 3
        if kind == 0:
            op = (at, r - n + 1, -1, n)
        elif kind == 1:
            h = (n + 1) // 2
            op = (at, r - h + 1, 0, n) if r - h + 1 > n + 5 else (at, r - n + 1, -1, n)     # b + n - 1 = n - 1 stays below
        else:
            op = (at, 3, r - n + 1, n) if n > 1 and r - n + 1 >= 0 and r > 3 + n else (at, r - n + 1, -1, n)
        ops.append(op)
        at += n
    return np.asarray(ops, np.int32).reshape(-1, 4), at


def planted_R(count, shape, seed):
    rng = np.random.default_rng(seed)
    if shape == "descending":
        return (200000 - 7 * np.arange(count)).tolist()
    if shape == "last_lane":                 # the maximum so far on lanes 63, 127, .. and on the last record of every 256
        R = rng.integers(1000, 2000, count)
        for k in range(63, count, 64):
            R[k] = 5000 + 10 * k + (100000 if k % 256 == 255 else 0)
        return R.tolist()
    R = np.cumsum(rng.integers(-40, 60, count)) + 20000      # a walk that rises on the whole and falls often
    return R.tolist()


def test_the_index_of_planted_lists_is_numpys_running_maximum(plan):
    """Streams of 0, 1, 63, 64, 65, 255, 256, 257, 1 024, 1 025 and 5 003 records: below, at and above a wave and a pass of the
    kernel.  A one-record stream between two long ones; capacities above the counts; a stream with n_ops = -(count), whose region
    keeps its canary, like everything behind a stream's count."""
    counts = [5003, 1, 1025, 0, 63, 64, 65, 255, 256, 257, 1024, 700, 512]
    shapes = ["last_lane", "walk", "descending", "walk", "last_lane", "last_lane", "descending", "walk", "last_lane", "descending",
              "walk", "walk", "last_lane"]
    streams = []
    for i, (c, sh) in enumerate(zip(counts, shapes)):
        ops, at = records_for(planted_R(c, sh, 100 + i), 200 + i)
        assert numpy_index(ops).tolist() == np.maximum.accumulate(planted_R(c, sh, 100 + i)).tolist() if c else True
        streams.append(stream(ops, 400000, at, cap=c + (i % 3) * 5))
    streams[11]["n_ops"] = -700
    g = numpy_index(streams[0]["ops"])
    assert (np.diff(numpy_index(streams[2]["ops"])) == 0).all() and g[255] > g[254] and g[63] > g[62] and g[5002] == g[4991]
    pl = Planted(plan, streams)
    got = pl.index()
    for i, s in enumerate(streams):
        o, c = int(pl.offs[i]), s["n_ops"]
        if c < 0:
            assert (got[o:o + s["cap"]] == IDX_CANARY).all(), "the stream with a negative count was indexed"
            continue
        want = numpy_index(s["ops"])
        bad = np.nonzero(got[o:o + c] != want)[0]
        assert bad.size == 0, (i, c, shapes[i], bad[:6], got[o:o + c][bad[:6]], want[bad[:6]])
        assert want.tolist() == ref(s).G, i
        assert (got[o + c:o + s["cap"]] == IDX_CANARY).all(), (i, "values written behind the stream's count")
    assert (got[int(pl.offs[-1]):] == IDX_CANARY).all()


SHAPES = [(0, 100, -1, 1), (1, 500, 530, 1), (2, 531, 561, 2), (4, 563, 600, 3), (7, 603, -1, 2), (9, 605, -1, 3),
          (12, 608, -1, 40), (52, 648, 608, 13), (65, 621, -1, 40), (105, 661, 621, 1), (106, 622, -1, 40), (146, 662, 622, 2),
          (148, 624, -1, 40), (188, 664, 624, 39), (227, 663, -1, 31), (258, 694, 663, 30), (288, 693, 800, 6), (294, 900, 2000, 7),
          (301, 2007, -1, 5)]


def test_record_shapes_cuts_and_queries_out_of_range(plan):
    """Records of one, two and three frames, slow-down-shaped cross-fades (b < a, n below the period, n = 1, 2, 39 of 40), a jump
    ahead.  Every output frame and every input frame is asked, with its record, in five streams over the same records: the whole
    list, the cut inside a record, the cut before a record, n_out = 0, and L below the largest source (a nonlinear job whose
    trailing partial buffer was dropped: frames that play padding answer L).  Queries below 0 and far above, INT64_MIN and
    INT64_MAX: asked of edit_lookup_ref itself, not of a table."""
    ops = np.asarray(SHAPES, np.int32)
    assert E.contiguous([tuple(o) for o in ops.tolist()])
    total = int(ops[-1][0] + ops[-1][3])
    streams = [stream(ops, 4000, total), stream(ops, 4000, 60), stream(ops, 4000, 65), stream(ops, 4000, 0),
               stream(ops, 1999, total, nl=1.0), stream(ops, 4000, total - 2)]
    assert ref(streams[4]).L == 1920 and ref(streams[0]).forward(2012) == (total, -1)
    far = [-(1 << 63), -(1 << 40), -1, (1 << 31) - 1, 1 << 31, (1 << 40) + 3, (1 << 63) - 1]
    t = np.asarray(list(range(-3, 4010)) + far, np.int64)
    u = np.asarray(list(range(-3, total + 6)) + far, np.int64)
    pl = Planted(plan, streams)
    pl.index()
    fw, fw_rec, _, _ = pl.lookup([t] * 6, False)
    iv, iv_rec, _, _ = pl.lookup([u] * 6, True)
    for i, s in enumerate(streams):
        m = ref(s)
        want = [m.forward(v) for v in t.tolist()]
        got = list(zip(fw[i].tolist(), fw_rec[i].tolist()))
        bad = [k for k in range(t.size) if got[k] != want[k]]
        assert bad == [], (i, "forward", [(int(t[k]), got[k], want[k]) for k in bad[:5]])
        want = [m.inverse(v) for v in u.tolist()]
        got = list(zip(iv[i].tolist(), iv_rec[i].tolist()))
        bad = [k for k in range(u.size) if got[k] != want[k]]
        assert bad == [], (i, "inverse", [(int(u[k]), got[k], want[k]) for k in bad[:5]])
    # what the shapes are there for: a tie goes to the ramp coming up; the slow-down plays input twice
    m = ref(streams[0])
    assert m.inverse(2) == (531, 2) and m.inverse(3) == (562, 2) and m.inverse(1) == (500, 1)
    assert m.inverse(52 + 6) == (654, 7) and m.inverse(52 + 7) == (615, 7) and m.forward(648) == (52, 7) and m.forward(655) == (99, 8)
    assert m.forward(700) == (264, 15) and m.forward(709) == (291, 16) and m.R[16] > m.G[15] > 695      # (ramp a of record 16 alone would not do)


def synthetic(n_in, seed, slow, periods=(40, 200)):
    """A list shaped like a job's: speed-up steps (a cross-fade that skips a period, now and then a copy) or slow-down steps (a copy
    of a period, then a cross-fade back over it that advances by less than half of it: input played more than twice)."""
    rng = np.random.default_rng(seed)
    ops, at, pos = [], 0, 0
    while pos + 500 < n_in:
        period = int(rng.integers(*periods))
        if slow:
            n = int(rng.integers(1, period))
            ops += [(at, pos, -1, period), (at + period, pos + period, pos, n)]
            at += period + n
            pos += n
        else:
            n = int(rng.integers(1, period + 1))
            ops.append((at, pos, pos + period, n))
            at += n
            pos += period + n
            if rng.random() < 0.3:
                c = int(rng.integers(1, 300))
                ops.append((at, pos, -1, c))
                at += c
                pos += c
    return np.asarray(ops, np.int32), at


def kinds():
    """Six planted streams, each with a name for its tables."""
    out = []
    for name, n_in, seed, slow, cut in (("up_long", 300000, 1, False, 5), ("down", 6000, 2, True, 40), ("up", 30000, 3, False, 0),
                                        ("down_nl", 9037, 4, True, 3), ("up_short", 2000, 5, False, 1), ("down_long", 12000, 6, True, 100)):
        ops, at = synthetic(n_in, seed, slow)
        out.append((name, stream(ops, n_in, at - cut, nl=1.0 if name.endswith("_nl") else 0.0)))
    return out


def spread(s, count, seed, inverse):
    """Every position of the range and its surroundings, then a fixed-seed spread, `count` queries in all."""
    hi = s["n_out"] if inverse else s["n_in"]
    base = np.arange(-50, hi + 50, dtype=np.int64)
    rng = np.random.default_rng(seed)
    q = np.concatenate([base, rng.integers(-1000, hi + 1000, max(count - base.size, 0))])
    return q[:count]


def check(s, key, q, inverse, ans, rec, tag):
    want = expected(s, key, q, inverse)
    bad = np.nonzero((ans != want[:, 0]) | (rec != want[:, 1]))[0]
    assert bad.size == 0, (tag, "inverse" if inverse else "forward", [(int(q[k]), int(ans[k]), int(rec[k]), want[k].tolist()) for k in bad[:5]])


def rounds(gx, most):
    return -(-most // (gx * THREADS))


def test_one_stream_of_600000_queries_strides_three_times_at_1024_blocks(plan):
    """n = 1: the upper clamp of the block count, 262 144 threads for 600 000 queries over a list of about 1 700 records."""
    name, s = kinds()[0]
    assert 1300 < len(s["ops"]) < 2500
    pl = Planted(plan, [s])
    pl.index()
    t, u = spread(s, 600000, 11, False), spread(s, 600000, 12, True)
    (fw,), (fr,), gx, launches = pl.lookup([t], False)
    (iv,), (ir,), gx_i, _ = pl.lookup([u], True)
    print("n = 1: blocks per stream", gx, "threads", gx * THREADS, "queries per thread", rounds(gx, t.size), "launches", launches)
    assert t.size == u.size == 600000 and gx == gx_i == 1024 and launches == 1 and rounds(gx, t.size) == 3
    check(s, name, t, False, fw, fr, name)
    check(s, name, u, True, iv, ir, name)


def test_eight_streams_300000_queries_in_one_and_none_in_another(plan):
    """n = 8: 512 blocks per stream.  One stream asks 300 000 times, one nothing; slow-downs among them, whose forward search
    needs the running maximum (asserted: their R falls below it)."""
    ks = kinds()
    streams = [ks[1], ks[0], ks[2], ks[3], ks[4], ks[5], ("zero", stream(np.zeros((0, 4), np.int32), 500, 0)), ks[1]]
    m = ref(ks[1][1])
    assert sum(1 for r, g in zip(m.R, m.G) if r < g) > 20
    pl = Planted(plan, [s for _, s in streams])
    pl.index()
    counts = [300000, 20000, 0, 12000, 3000, 20000, 700, 9000]
    qs = [(spread(s, c, 20 + i, False), spread(s, c, 40 + i, True)) for i, ((_, s), c) in enumerate(zip(streams, counts))]
    fw, fr, gx, launches = pl.lookup([q[0] for q in qs], False)
    iv, ir, gx_i, _ = pl.lookup([q[1] for q in qs], True)
    print("n = 8: blocks per stream", gx, "queries per thread", rounds(gx, 300000), "launches", launches)
    assert gx == gx_i == 512 and launches == 1 and rounds(gx, 300000) == 3 and fw[2].size == 0 and iv[2].size == 0
    for i, (name, s) in enumerate(streams):
        check(s, name, qs[i][0], False, fw[i], fr[i], (i, name))
        check(s, name, qs[i][1], True, iv[i], ir[i], (i, name))


def test_lists_at_and_above_the_size_a_block_stages(plan):
    """The lookup kernel searches a list of at most 4 096 records in LDS and a longer one where it lies: slow-down lists of 4 095,
    4 096, 4 097 and about 6 000 records of two to eleven frames, every input frame and every output frame asked."""
    ops, _ = synthetic(11000, 9, True, periods=(2, 12))
    assert len(ops) > 5500 and E.contiguous([tuple(o) for o in ops.tolist()])
    streams = []
    for k in (4096, 4097, len(ops), 4095):
        end = int(ops[k - 1][0] + ops[k - 1][3])
        streams.append(("staged_%d" % k, stream(ops[:k], 11000, end - 3)))
    pl = Planted(plan, [s for _, s in streams])
    got = pl.index()
    for i, (_, s) in enumerate(streams):
        assert np.array_equal(got[int(pl.offs[i]):int(pl.offs[i + 1])], numpy_index(s["ops"])), i
    qs = [(np.arange(-5, s["n_in"] + 6, dtype=np.int64), np.arange(-5, s["n_out"] + 6, dtype=np.int64)) for _, s in streams]
    fw, fr, _, _ = pl.lookup([q[0] for q in qs], False)
    iv, ir, _, _ = pl.lookup([q[1] for q in qs], True)
    for i, (name, s) in enumerate(streams):
        assert sum(1 for r, g in zip(ref(s).R, ref(s).G) if r < g) > 500, name
        check(s, name, qs[i][0], False, fw[i], fr[i], name)
        check(s, name, qs[i][1], True, iv[i], ir[i], name)


def test_2048_streams_at_four_blocks(plan):
    """The lower clamp: 4 blocks per stream, 1 024 threads stride over 2 500 queries.  Five kinds of list round-robin, each with
    its own queries: a stream served with a neighbour's table, records or index shows."""
    ks = kinds()[1:]
    per = {name: (np.resize(spread(s, 2500, 60, False), 2500), np.resize(spread(s, 2500, 61, True), 2500)) for name, s in ks}
    pick = [(i * 3 + i // 5) % 5 for i in range(2048)]
    streams = [ks[k] for k in pick]
    pl = Planted(plan, [s for _, s in streams])
    pl.index()
    fw, fr, gx, launches = pl.lookup([per[name][0] for name, _ in streams], False)
    iv, ir, gx_i, _ = pl.lookup([per[name][1] for name, _ in streams], True)
    print("n = 2048: blocks per stream", gx, "queries per thread", rounds(gx, 2500), "launches", launches)
    assert gx == gx_i == 4 and launches == 1 and rounds(gx, 2500) == 3
    want = {name: (expected(s, name, per[name][0], False), expected(s, name, per[name][1], True)) for name, s in ks}
    bad = [i for i, (name, _) in enumerate(streams)
           if not (np.array_equal(fw[i], want[name][0][:, 0]) and np.array_equal(fr[i], want[name][0][:, 1])
                   and np.array_equal(iv[i], want[name][1][:, 0]) and np.array_equal(ir[i], want[name][1][:, 1]))]
    assert bad == [], bad[:8]


def test_65600_one_record_streams_take_a_second_launch(plan):
    """More streams than the grid's second dimension holds: 65 535 in the first launch, 65 in the second.  Every stream has its own
    record, length and count, three queries each way: a slip in stream0 + blockIdx.y, or a stream served twice or never, changes
    an answer or leaves the canary.  The index call covers them in one launch."""
    n = 65600
    streams = [stream([(0, 7 + i, -1, 40 + i % 50)] if i % 3 else [(0, 7 + i, 3 + i, 40 + i % 50)], 70000 + i, 30 + i % 40) for i in range(n)]
    t = [np.asarray([0, 7 + i + i % 37, 70000 + i], np.int64) for i in range(n)]
    u = [np.asarray([0, i % 41, 30 + i % 40], np.int64) for i in range(n)]
    pl = Planted(plan, streams)
    got = pl.index()
    assert np.array_equal(got[:n], np.asarray([ref(s).G[0] for s in streams], np.int32)) and (got[n:] == IDX_CANARY).all()
    fw, fr, gx, launches = pl.lookup(t, False)
    iv, ir, gx_i, launches_i = pl.lookup(u, True)
    print("n = 65600: blocks per stream", gx, "launches", launches)
    assert gx == gx_i == 4 and launches == launches_i == 2
    want_f, want_i = [], []
    for i, s in enumerate(streams):
        m = ref(s)
        want_f += [m.forward(v) for v in t[i].tolist()]
        want_i += [m.inverse(v) for v in u[i].tolist()]
    got_f = np.stack([np.concatenate(fw), np.concatenate(fr)], axis=1)
    got_i = np.stack([np.concatenate(iv), np.concatenate(ir)], axis=1)
    bad = np.nonzero((got_f != np.asarray(want_f, np.int64)).any(axis=1) | (got_i != np.asarray(want_i, np.int64)).any(axis=1))[0]
    assert bad.size == 0, ("first differing streams", (bad[:8] // 3).tolist())
    assert len({w[0] for w in want_f[1::3]}) > 30 and len({w[0] for w in want_i[1::3]}) > 30000


def test_a_stream_with_a_negative_count_answers_minus_one_and_harms_no_other(plan):
    """n_ops = -(count) (the list did not fit) and n_out negative (the output did not) between good streams: -1 for every answer
    and every record, exact neighbours, the index of the first untouched.  Read in the kernels before this was run: a negative
    n_ops or n_out leaves nk = 0 and takes the branch that loads nothing."""
    ks = kinds()
    a, b, c = ks[1], ks[4], ks[3]
    dead1 = stream(a[1]["ops"], a[1]["n_in"], a[1]["n_out"], n_ops=-len(a[1]["ops"]), cap=len(a[1]["ops"]) - 1)
    dead2 = stream(b[1]["ops"], b[1]["n_in"], -1)
    streams = [a, ("dead1", dead1), b, ("dead2", dead2), c]
    pl = Planted(plan, [s for _, s in streams])
    got = pl.index()
    o = int(pl.offs[1])
    assert (got[o:o + dead1["cap"]] == IDX_CANARY).all()
    qs = [(spread(s, 3000, 70 + i, False), spread(s, 3000, 80 + i, True)) for i, (_, s) in enumerate(streams)]
    fw, fr, _, _ = pl.lookup([q[0] for q in qs], False)
    iv, ir, _, _ = pl.lookup([q[1] for q in qs], True)
    for i, (name, s) in enumerate(streams):
        if name.startswith("dead"):
            assert ref(s).forward(5) == ref(s).inverse(5) == (-1, -1)
            assert (fw[i] == -1).all() and (fr[i] == -1).all() and (iv[i] == -1).all() and (ir[i] == -1).all(), name
        else:
            check(s, name, qs[i][0], False, fw[i], fr[i], name)
            check(s, name, qs[i][1], True, iv[i], ir[i], name)


def test_refusals_launch_nothing_and_a_good_call_works_right_after(plan):
    import torch
    ks = kinds()
    streams = [ks[4], ks[1]]
    pl = Planted(plan, [s for _, s in streams])
    L = plan.L
    i64 = C.POINTER(C.c_int64)
    qs = [spread(s, 2000, 90 + i, False) for i, (_, s) in enumerate(streams)]
    hs = torch.cuda.current_stream().cuda_stream

    def index(**kw):
        a = dict(ops=pl.d_ops.data_ptr(), caps=pl.caps_ptr(), nops=pl.d_nops.data_ptr(), index=pl.d_index.data_ptr(), jobs=pl.jobs)
        a.update(kw)
        rc = L.spx_edit_index(plan.h, a["jobs"], pl.n, a["ops"], a["caps"], a["nops"], a["index"], hs)
        msg = L.spx_last_error().decode() if rc != 0 else ""
        torch.cuda.synchronize()
        return rc, msg, bool((pl.d_index == IDX_CANARY).all())

    bad_caps = [C.cast((C.c_int64 * 2)(5, -1), i64), C.cast((C.c_int64 * 2)(2 ** 31 - 1, 1), i64)]
    for kw, word in (({"ops": None}, "NULL"), ({"caps": None}, "NULL"), ({"nops": None}, "NULL"), ({"index": None}, "NULL"),
                     ({"ops": pl.d_ops.data_ptr() + 4}, "aligned"), ({"caps": bad_caps[0]}, "negative capacity"),
                     ({"caps": bad_caps[1]}, "2^31 - 1")):
        rc, msg, untouched = index(**kw)
        assert rc == -1 and word in msg and untouched, ("index", list(kw), rc, msg, untouched)
    good = pl.jobs[1].speed
    pl.jobs[1].speed = float("nan")
    rc, msg, untouched = index()
    assert rc == -1 and "speed" in msg and untouched, (rc, msg)
    rc, r, rec = pl.lookup(qs, True)
    assert rc == -1 and "speed" in pl.msg and (r == R_CANARY).all() and (rec == REC_CANARY).all()
    pl.jobs[1].speed = good
    for inverse in (False, True):
        cases = [({"ops": None}, "NULL"), ({"caps": None}, "NULL"), ({"nops": None}, "NULL"), ({"nout": None}, "NULL"),
                 ({"qoff": None}, "NULL"), ({"q": None}, "NULL"), ({"r": None}, "NULL"),
                 ({"ops": pl.d_ops.data_ptr() + 8}, "aligned"), ({"caps": bad_caps[0]}, "negative capacity"),
                 ({"caps": bad_caps[1]}, "2^31 - 1")]
        if not inverse:
            cases.append(({"index": None}, "index"))
        for kw, word in cases:
            got = pl.lookup(qs, inverse, **kw)
            assert len(got) == 3 and got[0] == -1 and word in pl.msg, (inverse, list(kw), got[0], pl.msg)
            assert (got[1] == R_CANARY).all() and (got[2] == REC_CANARY).all(), (inverse, list(kw), "something was launched")
    # ... and a good call right after: the index, both directions, with and without rec, the inverse one without an index
    rc, msg, untouched = index()
    assert rc == 0 and not untouched, msg
    fw, fr, _, _ = pl.lookup(qs, False)
    iv, ir, _, _ = pl.lookup(qs, True, index=None)
    iv2, ir2, _, _ = pl.lookup(qs, True, rec=None)
    for i, (name, s) in enumerate(streams):
        check(s, name, qs[i], False, fw[i], fr[i], name)
        check(s, name, qs[i], True, iv[i], ir[i], name)
        assert np.array_equal(iv2[i], iv[i]) and (ir2[i] == REC_CANARY).all(), name


# ------------------------------------------------------------------ real lists ------------------------------------------------------------------

def _every_position(b, jobs, nonlinear, defs=None):
    """forward for every p in [0, L], inverse for every o in [0, n_out] of every stream of a Batch(edits=True) that has run: against
    the definition applied to the list the GPU wrote -- and to the definition's own list where one is given."""
    nout = GE._sync_np(b.d_nout)
    ms = []
    for i, job in enumerate(jobs):
        L = K.limit_of(job[3].size // job[2], job[1], nonlinear)
        ms.append(K.Lookup(b.edits(i).tolist(), int(nout[i]), L))
        if defs is not None:
            assert defs[i].ops == ms[i].ops and defs[i].out_n == ms[i].n_out and defs[i].limit == L, job[0]
    fw, fr = b.locate_all([np.arange(m.L + 1) for m in ms], records=True)
    iv, ir = b.locate_all([np.arange(m.n_out + 1) for m in ms], inverse=True, records=True)
    assert np.array_equal(b.locate_all([np.arange(0, m.L + 1, 7) for m in ms])[-1], fw[-1][::7])          # (records=False: the answers alone)
    for i, (job, m) in enumerate(zip(jobs, ms)):
        want = np.asarray([m.forward(p) for p in range(m.L + 1)], np.int64).reshape(-1, 2)
        bad = np.nonzero((fw[i] != want[:, 0]) | (fr[i] != want[:, 1]))[0]
        assert bad.size == 0, (job[0], "forward", [(int(k), int(fw[i][k]), int(fr[i][k]), want[k].tolist()) for k in bad[:4]])
        want = np.asarray([m.inverse(o) for o in range(m.n_out + 1)], np.int64).reshape(-1, 2)
        bad = np.nonzero((iv[i] != want[:, 0]) | (ir[i] != want[:, 1]))[0]
        assert bad.size == 0, (job[0], "inverse", [(int(k), int(iv[i][k]), int(ir[i][k]), want[k].tolist()) for k in bad[:4]])
    return ms, fw, iv


def _edits_batch(plan, jobs, defs=None):
    from speedy_amd.batch import Batch
    caps = GE._caps(plan, jobs, defs) if defs is not None else None
    b = Batch(plan, [j[3].size // j[2] for j in jobs], [j[2] for j in jobs], [j[4] for j in jobs],
              [(j[5] if len(j) == 6 else 0.0) for j in jobs], edits=True, ops_caps=caps)
    b.upload([j[3] for j in jobs])
    b.run()
    return b


@pytest.mark.parametrize("rate", [16000, 22050, 44100])
def test_every_position_of_the_linear_jobs(rate):
    """The jobs tests/test_gpu_edit_list.py pins, speeds 0.4, just below 0.5, 200 and 0.0001 among them: the list is the
    definition's, and every answer over it too."""
    from speedy_amd.batch import Plan
    jobs = GE._linear_jobs(rate)
    assert len(jobs) == 1 if rate == 44100 else len(jobs) > 15
    plan = Plan(rate, False)
    try:
        defs = [GE._linear_def(j) for j in jobs]
        _every_position(_edits_batch(plan, jobs, defs), jobs, False, defs)
    finally:
        plan.close()


@pytest.mark.parametrize("rate", [16000, 22050])
def test_every_position_of_the_nonlinear_jobs(orc, rate):
    from speedy_amd.batch import Plan
    jobs = GE._nonlinear_jobs(rate)
    assert len(jobs) >= 3
    plan = Plan(rate, False)
    try:
        defs = [GE._nonlinear_def(orc, j, False) for j in jobs]
        ms, _, _ = _every_position(_edits_batch(plan, jobs, defs), jobs, True, defs)
        assert any(m.L < j[3].size // j[2] for m, j in zip(ms, jobs)), "no job with a trailing partial buffer"
    finally:
        plan.close()


@pytest.mark.parametrize("rate", [16000, 11025, 48000])
def test_the_exact_lookup_against_the_time_map(rate):
    """The same table through spx_batch_run_map and spx_batch_run_edits (tests/tsm_inputs.py nonlinear_map_jobs).  Nothing emitted
    before ring buffer k is handed over can read frame k B, so for every k < R: forward(k B) >= M[k], and inverse(o) < k B for every
    o < M[k] -- an exact inequality, no tolerance.  Prints how late the 10 ms map is: the largest forward(k B) - M[k]."""
    from speedy_amd.batch import Batch, Plan
    jobs = [j for j in I.nonlinear_map_jobs() if j[1] == rate]
    assert len(jobs) == (7 if rate == 16000 else 1)
    plan = Plan(rate, False)
    try:
        B = plan.B
        args = ([j[3].size // j[2] for j in jobs], [j[2] for j in jobs], [j[4] for j in jobs], [j[5] for j in jobs])
        mp = Batch(plan, *args, time_map=True)
        mp.upload([j[3] for j in jobs])
        mp.run()
        b = _edits_batch(plan, jobs)
        assert np.array_equal(GE._sync_np(b.d_nout), GE._sync_np(mp.d_nout)) and (b.op_counts() >= 0).all()
        nout = GE._sync_np(b.d_nout)
        Rs = [a // B for a in args[0]]
        fw = b.locate_all([np.arange(R, dtype=np.int64) * B for R in Rs])
        iv = b.locate_all([np.arange(max(int(n), 0)) for n in nout], inverse=True)
        for i, job in enumerate(jobs):
            M, R = mp.time_map(i), Rs[i]
            assert M.size == R + 1 and M[R] == nout[i], job[0]
            late = fw[i] - M[:R]
            assert (late >= 0).all(), (job[0], "forward(k B) < M[k] at k =", np.nonzero(late < 0)[0][:5])
            top = np.maximum.accumulate(np.concatenate([[-1], iv[i]]))           # top[m] = the largest inverse(o), o < m
            ahead = [k for k in range(R) if top[M[k]] >= k * B]
            assert ahead == [], (job[0], "a frame before M[k] plays input at or behind k B, k =", ahead[:5])
            if R:
                held = np.arange(R) * B - 1 - top[M[:R]]                          # input frames handed over and not yet heard at M[k]
                print("%s: forward(k B) - M[k] at most %d output frames; at M[k] at most %d input frames before k B are not yet heard; "
                      "max_required %d" % (job[0], int(late.max()), int(held.max()), plan.max_required))
    finally:
        plan.close()


# ------------------------------------------------------------------ Python, and the C example ------------------------------------------------------------------

def test_python_round_trip_and_the_value_error():
    from speedy_amd.batch import Batch, Plan
    by = {j[0]: j for j in I.linear_jobs()}
    job = by["rates/16000Hz/2ch/4800/0.4"]
    e = GE._linear_def(job)
    m = K.Lookup(e.ops, e.out_n, e.limit)
    plan = Plan(16000, False)
    try:
        plain = Batch(plan, [4800], 2, 0.4, 0.0)
        with pytest.raises(ValueError, match="edits=True"):
            plain.locate(0, [1, 2])
        with pytest.raises(ValueError, match="edits=True"):
            plain.locate_all([[1, 2]], inverse=True)
        b = Batch(plan, [4800], 2, 0.4, 0.0, edits=True)
        b.upload([job[3]])
        b.run()
        cues = [0, 1, 777, 2400, 4799, 4800, 9999, -4]
        out = b.locate(0, cues)
        assert out.dtype == np.int64 and out.tolist() == [m.forward(p)[0] for p in cues]
        out, rec = b.locate(0, cues, records=True)
        assert rec.dtype == np.int32 and list(zip(out.tolist(), rec.tolist())) == [m.forward(p) for p in cues]
        back, rec = b.locate(0, out, inverse=True, records=True)
        assert list(zip(back.tolist(), rec.tolist())) == [m.inverse(o) for o in out.tolist()]
        assert all(p2 >= min(max(p, 0), 4800) for p, p2 in zip(cues, back.tolist()))
        ops = b.edits(0)
        k = int(rec[2])
        assert ops[k][0] <= out[2] < ops[k][0] + ops[k][3]                       # the record the caller reads the ramps from
        b.run()                                                                  # a second run: the index is built again
        assert b._index_built is False and b.locate(0, cues).tolist() == [m.forward(p)[0] for p in cues] and b._index_built
    finally:
        plan.close()


def test_c_edit_lookup_example(tmp_path):
    """tools/batch_edit_lookup_example.c: a job, its index, five cues forward and back through the C ABI alone."""
    exe = os.path.join(ROOT, "speedy_amd", "lib", "batch_edit_lookup_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "editlookupexample"])
    by = {j[0]: j for j in I.linear_jobs()}
    job = by["speeds/16000Hz/1ch/9001/3.5"]
    e = GE._linear_def(job)
    m = K.Lookup(e.ops, e.out_n, e.limit)
    job[3].tofile(tmp_path / "key.raw")
    cues = [0, 1234, 4500, 8999, 9001]
    r = subprocess.run([exe, str(tmp_path / "key.raw"), "16000", "1", "3.5", "0"] + [str(c) for c in cues], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    lines = r.stdout.strip().splitlines()
    assert lines[0].split() == ["frames", str(e.out_n), "ops", str(len(e.ops))]
    for line, p in zip(lines[1:], cues):
        o, k = m.forward(p)
        assert line.split() == ["cue", str(p), "out", str(o), "rec", str(k), "back", str(m.inverse(o)[0])], line
    assert len(lines) == 1 + len(cues)
