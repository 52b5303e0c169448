"""GPU: spx_batch_dtw (speedy_amd/csrc/spx_dtw.hip) against the definition, tests/dtw_ref.py -- the floats as uint32 patterns (any
NaN equals any NaN), the path as exact integers.  The kernel's tile edge is 64: the shapes sit on and around 1, 2 and 3 tiles."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dtw_cases
import dtw_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES = [1, 2, 63, 64, 65, 129]
SHAPES = [(n_a, n_b) for n_a in EDGES for n_b in EDGES] + [(257, 100), (100, 257), (600, 257)]
CANARY = -77


@pytest.fixture(scope="module")
def plan():
    from speedy_amd.batch import Plan
    p = Plan(16000)
    yield p
    p.close()


def _flat(seqs, ld, dim, fill=0.0):
    """The sequences one behind the other, rows ld floats apart, `fill` in every column at or behind dim."""
    out = []
    for s in seqs:
        m = np.full((s.shape[0], ld), fill, np.float32)
        m[:, :dim] = s
        out.append(m.ravel())
    return np.concatenate(out)


def run_pairs(plan, pairs, dim, ld_a=None, ld_b=None, half_width=10, fill=0.0):
    """One spx_batch_dtw call over `pairs` [(a, b)]: (results, [paths], DtwBatch), path and results canary-filled first."""
    import torch
    from speedy_amd import DtwBatch
    ld_a, ld_b = ld_a or dim, ld_b or dim
    b = DtwBatch(plan, [p[0].shape[0] for p in pairs], [p[1].shape[0] for p in pairs], dim, ld_a, ld_b, half_width)
    d_a = torch.from_numpy(_flat([p[0] for p in pairs], ld_a, dim, fill)).cuda()
    d_b = torch.from_numpy(_flat([p[1] for p in pairs], ld_b, dim, fill)).cuda()
    b.d_path.fill_(CANARY)
    b.d_results.fill_(0xA5)
    b.run(d_a, d_b)
    res = b.results()
    torch.cuda.synchronize()
    path = b.d_path.cpu().numpy().reshape(-1, 2)
    paths = []
    for i, (x, y) in enumerate(pairs):
        region = path[b.path_offs[i]:b.path_offs[i] + x.shape[0] + y.shape[0] - 1]
        n_path = int(res["n_path"][i])
        assert 1 <= n_path <= region.shape[0], (i, n_path)
        assert (region[n_path:] == CANARY).all(), "pair %d: written behind n_path" % i
        paths.append(region[:n_path].copy())
    return res, paths, b


def check(res, path, want, what):
    for f in ("cost", "slope", "local_mean", "local_std"):
        assert dtw_ref.same_bits(res[f], want[f]), "%s: %s %r (0x%08x), the definition %r (0x%08x)" % (
            what, f, float(res[f]), dtw_ref.bits(res[f]), float(want[f]), dtw_ref.bits(want[f]))
    assert int(res["n_path"]) == want["n_path"] and int(res["n_local"]) == want["n_local"], (what, res, want["n_path"], want["n_local"])
    assert np.array_equal(path, want["path"]), (what, np.nonzero((path != want["path"]).any(axis=1))[0][:4])


def _random_pair(rng, n_a, n_b, dim):
    return (rng.standard_normal((n_a, dim)).astype(np.float32), rng.standard_normal((n_b, dim)).astype(np.float32))


@pytest.mark.parametrize("dim", [1, 3, 60, 240])
def test_single_pair_shapes(plan, dim):
    """Every shape as a call of its own, one pair each; half width 3 so that short paths have windows too.  The three long shapes
    run at every dim as well: the definition's recurrence is what costs time, not the local costs (dtw_cases.local_costs)."""
    rng = np.random.default_rng(100 + dim)
    for n_a, n_b in SHAPES:
        a, b = _random_pair(rng, n_a, n_b, dim)
        res, paths, _ = run_pairs(plan, [(a, b)], dim, half_width=3)
        check(res[0], paths[0], dtw_cases.answer(a, b, 3), "%d x %d, dim %d" % (n_a, n_b, dim))


def test_scalar_definition_directly(plan):
    """A few shapes against dtw_ref.dtw with its own scalar local costs, no helper in between."""
    rng = np.random.default_rng(7)
    for n_a, n_b, dim in [(65, 63, 3), (1, 64, 1), (64, 1, 60), (20, 70, 33), (2, 2, 240)]:
        a, b = _random_pair(rng, n_a, n_b, dim)
        res, paths, _ = run_pairs(plan, [(a, b)], dim, half_width=2)
        check(res[0], paths[0], dtw_ref.dtw(a, b, 2), "%d x %d, dim %d" % (n_a, n_b, dim))


def test_ties(plan):
    """dim = 1 and values from {0, 1, 2}: most cells tie, and ties go along the diagonal.  Constant sequences of unequal length: the
    diagonal back from the end, then the border."""
    rng = np.random.default_rng(11)
    pairs = []
    for n_a, n_b in [(64, 64), (65, 129), (129, 63), (200, 70), (3, 130)]:
        pairs.append((rng.integers(0, 3, (n_a, 1)).astype(np.float32), rng.integers(0, 3, (n_b, 1)).astype(np.float32)))
    for n_a, n_b in [(70, 130), (130, 70), (64, 65)]:
        pairs.append((np.full((n_a, 1), 5.0, np.float32), np.full((n_b, 1), 5.0, np.float32)))
    res, paths, _ = run_pairs(plan, pairs, 1, half_width=4)
    for i, (a, b) in enumerate(pairs):
        want = dtw_ref.dtw(a, b, 4)
        check(res[i], paths[i], want, "pair %d" % i)
    p = paths[5]   # 70 x 130 constant: along the first row, then the diagonal
    assert p[:61].tolist() == [[0, j] for j in range(61)] and p[61:].tolist() == [[k, 60 + k] for k in range(1, 70)]


def test_strides(plan):
    """ld_a = 480, ld_b = 960, dim = 120, NaN in every column at or behind dim: the results of packed rows."""
    rng = np.random.default_rng(13)
    pairs = [_random_pair(rng, 70, 40, 120), _random_pair(rng, 64, 130, 120)]
    packed, ppaths, _ = run_pairs(plan, pairs, 120)
    strided, spaths, _ = run_pairs(plan, pairs, 120, ld_a=480, ld_b=960, fill=np.nan)
    for i, (a, b) in enumerate(pairs):
        want = dtw_cases.answer(a, b)
        check(strided[i], spaths[i], want, "strided pair %d" % i)
        check(packed[i], ppaths[i], want, "packed pair %d" % i)


def test_batch_of_300_ragged_pairs(plan):
    """More pairs than the chip has CUs in one call, a 1 x 1 and a 1 x n pair in the middle, gaps of canaries between the pairs'
    path regions: nothing is written behind n_path or outside a region; the launch rule is one workgroup per pair, two launches."""
    import torch
    from speedy_amd import DtwBatch
    rng = np.random.default_rng(17)
    n, dim, gap = 300, 5, 7
    shapes = [(int(rng.integers(1, 90)), int(rng.integers(1, 90))) for _ in range(n)]
    shapes[150], shapes[151], shapes[152] = (1, 1), (1, 37), (41, 1)
    pairs = [_random_pair(rng, n_a, n_b, dim) for n_a, n_b in shapes]
    b = DtwBatch(plan, [s[0] for s in shapes], [s[1] for s in shapes], dim, half_width=5)
    offs = []
    for i in range(n):   # the regions spread out, `gap` entries in front of each
        offs.append(b.path_offs[i] + gap * (i + 1))
        b.jobs[i].path_off = offs[i]
    total = offs[-1] + sum(shapes[-1]) - 1 + gap
    b.d_path = torch.full((total * 2,), CANARY, dtype=torch.int32, device="cuda")
    b.d_results.fill_(0xA5)
    b.run(torch.from_numpy(_flat([p[0] for p in pairs], dim, dim)).cuda(), torch.from_numpy(_flat([p[1] for p in pairs], dim, dim)).cuda())
    res = b.results()
    assert b.grid() == (n, 2)
    path = b.d_path.cpu().numpy().reshape(-1, 2)
    written = np.zeros(total, bool)
    for i, (x, y) in enumerate(pairs):
        want = dtw_cases.answer(x, y, 5)
        n_path = int(res["n_path"][i])
        check(res[i], path[offs[i]:offs[i] + n_path], want, "pair %d (%d x %d)" % (i, x.shape[0], y.shape[0]))
        written[offs[i]:offs[i] + n_path] = True
    assert (path[~written] == CANARY).all(), "an entry outside every pair's path was written"
    assert int(res["n_path"][150]) == 1 and np.isnan(res["slope"][150]) and int(res["n_local"][150]) == 0


def _taps_of(plan, x, speed, nonlinear):
    from speedy_amd.batch import Batch
    b = Batch(plan, [x.size], 1, speed, nonlinear, 0.0, taps=True, spectrogram_taps=True)
    b.upload([x])
    b.run()
    return b.results()[0], b


def test_taps_in_place(plan):
    """A 16 kHz tapestry job with the spectrogram tap, its output analysed the same way, the two tap tensors handed to DtwBatch where
    they lie (ld = N, dim = N / 4): the definition on the same rows copied to the host.  No bound on this slope: nobody has
    measured it on 10 ms pre-emphasised rows."""
    from speedy_amd import DtwBatch
    from util import read_wav
    x, rate, ch = read_wav("tapestry.wav")
    assert rate == 16000 and ch == 1
    y, ba = _taps_of(plan, x, 3.0, 1.0)
    _, bb = _taps_of(plan, y, 3.0, 1.0)
    N, dim = plan.N, plan.N // 4
    rows_a, rows_b = ba.tap_arrays(0)["spectrogram"], bb.tap_arrays(0)["spectrogram"]
    assert rows_a.shape == (ba.frames[0], N) and rows_b.shape == (bb.frames[0], N) and rows_b.shape[0] > 20
    d = DtwBatch(plan, [rows_a.shape[0]], [rows_b.shape[0]], dim, ld_a=N, ld_b=N)
    d.d_path.fill_(CANARY)
    d.run(ba.t_spec, bb.t_spec)
    res = d.results()
    want = dtw_cases.answer(rows_a[:, :dim], rows_b[:, :dim])
    print("taps in place: %d x %d rows, cost %r slope %r mean %r std %r" % (rows_a.shape[0], rows_b.shape[0], float(res["cost"][0]),
          float(res["slope"][0]), float(res["local_mean"][0]), float(res["local_std"][0])))
    check(res[0], d.path(0), want, "taps")


@pytest.mark.parametrize("name", ["linear", "nonlinear"])
def test_reference_measuring_device(plan, name):
    """The oracle's ComputeSpectrogram rows of the reference's own test pair, uploaded: the definition's results bit for bit, and
    therefore the reference's thresholds (sonic_test.cc:669-721)."""
    rows = dtw_cases.tapestry_rows()
    a, b = rows["original"], rows[name]
    dim = a.shape[1]
    res, paths, _ = run_pairs(plan, [(a, b)], dim, half_width=dtw_cases.HALF_WIDTH)
    want = dtw_cases.tapestry_answer(name)
    check(res[0], paths[0], want, name)
    got = {k: res[0][k] for k in ("cost", "slope", "local_mean", "local_std")}
    got["path"] = paths[0]
    dtw_cases.reference_thresholds(name, got)


def test_refusals(plan):
    """Every rule of the header: -1, a message, nothing written."""
    import torch
    from speedy_amd._lib import DtwJob
    L = plan.L
    dim, n_a, n_b = 4, 6, 5
    d_a = torch.zeros(n_a * dim, dtype=torch.float32, device="cuda")
    d_b = torch.zeros(n_b * dim, dtype=torch.float32, device="cuda")
    d_res = torch.full((24,), 0xA5, dtype=torch.uint8, device="cuda")
    d_path = torch.full((2 * (n_a + n_b - 1),), CANARY, dtype=torch.int32, device="cuda")

    def job(**kw):
        j = (DtwJob * 1)()
        j[0].a_off, j[0].b_off, j[0].path_off, j[0].n_a, j[0].n_b = 0, 0, 0, n_a, n_b
        for k, v in kw.items():
            setattr(j[0], k, v)
        return j
    ws_bytes = L.spx_dtw_workspace_bytes(job(), 1, dim)
    assert ws_bytes > 0
    d_ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
    good = dict(plan=plan.h, jobs=job(), n=1, dim=dim, ld_a=dim, ld_b=dim, h=10, a=d_a.data_ptr(), b=d_b.data_ptr(),
                res=d_res.data_ptr(), path=d_path.data_ptr(), ws=d_ws.data_ptr(), wsb=ws_bytes)

    def call(**kw):
        g = dict(good, **kw)
        return L.spx_batch_dtw(g["plan"], g["jobs"], g["n"], g["dim"], g["ld_a"], g["ld_b"], g["h"], g["a"], g["b"], g["res"], g["path"],
                               g["ws"], g["wsb"], None)
    bad = [dict(plan=None), dict(jobs=None), dict(a=None), dict(b=None), dict(res=None), dict(path=None), dict(ws=None),
           dict(n=0), dict(n=-1), dict(dim=0), dict(dim=(1 << 20)), dict(ld_a=dim - 1), dict(ld_b=dim - 1), dict(h=0),
           dict(jobs=job(n_a=0)), dict(jobs=job(n_b=0)), dict(jobs=job(n_a=-3)), dict(jobs=job(n_a=1 << 16, n_b=(1 << 14) + 1)),
           dict(jobs=job(a_off=-1)), dict(jobs=job(b_off=-1)), dict(jobs=job(path_off=-1)), dict(wsb=ws_bytes - 1), dict(wsb=0)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert L.spx_last_error(), kw
    assert L.spx_dtw_workspace_bytes(job(n_a=0), 1, dim) == 0 and L.spx_last_error()
    assert L.spx_dtw_workspace_bytes(job(), 1, 0) == 0
    torch.cuda.synchronize()
    assert (d_res.cpu().numpy() == 0xA5).all() and (d_path.cpu().numpy() == CANARY).all()
    # ... and the good call is taken: n_a * n_b = 2^30 exactly is inside the rule (sizes only, nothing is run at that size)
    assert L.spx_dtw_workspace_bytes(job(n_a=1 << 16, n_b=1 << 14), 1, dim) > 0
    assert call() == 0
    torch.cuda.synchronize()
    assert (d_path.cpu().numpy()[:2] == 0).all()


def test_timing_events(plan):
    """Under spx_set_timing the call's two launches are timed as DTW time -- not as analysis, walk or tension time -- and the tail's
    share is part of the whole."""
    import torch
    L = plan.L
    rng = np.random.default_rng(23)
    pairs = [_random_pair(rng, 130, 70, 8)]
    L.spx_timing_collect(None, None, None)   # whatever earlier tests left pending
    L.spx_set_timing(1)
    try:
        run_pairs(plan, pairs, 8)
        torch.cuda.synchronize()
        an, walk, calls = C.c_double(-1), C.c_double(-1), C.c_int(-1)
        assert L.spx_timing_collect(C.byref(an), C.byref(walk), C.byref(calls)) == 0
    finally:
        L.spx_set_timing(0)
    assert L.spx_timing_last_dtw_ms() > 0.0
    assert 0.0 < L.spx_timing_last_dtw_tail_ms() < L.spx_timing_last_dtw_ms()
    assert an.value == 0.0 and walk.value == 0.0 and L.spx_timing_last_tension_ms() == 0.0
    L.spx_timing_collect(None, None, None)
    assert L.spx_timing_last_dtw_ms() == 0.0


def test_c_example(plan, tmp_path):
    """tools/batch_dtw_example.c runs and prints what DtwBatch gives for the same input."""
    from speedy_amd import DtwBatch
    from util import read_wav
    exe = os.path.join(ROOT, "speedy_amd", "lib", "batch_dtw_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "dtwexample"])
    x, rate, _ = read_wav("tapestry.wav")
    raw = tmp_path / "in.raw"
    x.astype(np.int16).tofile(str(raw))
    out = subprocess.run([exe, str(raw), str(rate), "3.0", "1.0", "10"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = dict(line.split(None, 1) for line in out.stdout.strip().splitlines())
    y, ba = _taps_of(plan, x, 3.0, 1.0)
    _, bb = _taps_of(plan, y, 3.0, 1.0)
    assert got["rows"].split() == [str(ba.frames[0]), str(bb.frames[0])]
    d = DtwBatch(plan, [ba.frames[0]], [bb.frames[0]], plan.N // 4, ld_a=plan.N, ld_b=plan.N)
    d.run(ba.t_spec, bb.t_spec)
    res = d.results()[0]
    for f in ("cost", "slope", "local_mean", "local_std"):
        assert dtw_ref.same_bits(np.float32(float(got[f])), res[f]), (f, got[f], float(res[f]))
    assert int(got["n_path"]) == int(res["n_path"]) and int(got["n_local"]) == int(res["n_local"])
