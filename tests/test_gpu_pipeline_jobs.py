"""spx_pipeline_submit_jobs / spx_pipeline_jobs_fit (include/speedy_hip.h): one pipeline object, a DIFFERENT job table with every
batch -- lengths, speeds, nonlinear factors, empty lanes.  Whatever shapes are in flight beside a batch, every stream of it must be
what spx_batch_run gives for the same job and samples (CRC-32 per stream), and that is checked against the oracle on the first,
the middle and the last stream of every distinct table."""
import os
import subprocess
import zlib

import numpy as np
import pytest

from util import read_wav

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEEDS = (1.5, 2.0, 3.5)


def _crc(outs):
    return [zlib.crc32(np.ascontiguousarray(o).tobytes()) for o in outs]


def _bases(rate, ch, lane, seeds):
    from speedy_amd.synth import speech_like
    return [[speech_like(lane, rate, seed=1000 * s + i, channels=ch) for i in range(10)] for s in seeds]


def _content(bases, k, ch, lens):
    """Fresh content for submit k: lane i reads the front of a signal that no other submit gave it."""
    base = bases[k % len(bases)]
    return [base[(i + k) % len(base)][: lens[i] * ch] for i in range(len(lens))]


def _oracle_crc(orc, x, rate, ch, speed, nl):
    if x.size == 0:
        return zlib.crc32(b"")
    ref = orc.compress_sound(x, rate, ch, float(speed), float(nl), 0.0, False, chunk=1000, taps=False)
    return zlib.crc32(np.ascontiguousarray(ref["out"]).tobytes())


def _tables(rate, n, lane, seed):
    """The four tables of the ragged test as (lengths, speeds, nonlinear): A the creation shape at 3.5x nonlinear; B random lengths
    in [0.2 s, lane], a speed of 1.5 / 2.0 / 3.5 per lane, nonlinear; C every lane linear at 2x (no analysis frames at all);
    D the lengths of B reversed with a third of the lanes empty."""
    rng = np.random.default_rng(seed)
    lb = [int(v) for v in rng.integers(int(0.2 * rate), lane + 1, n)]
    sb = [SPEEDS[int(v)] for v in rng.integers(0, 3, n)]
    lc = [int(v) for v in rng.integers(int(0.2 * rate), lane + 1, n)]
    ld = [0 if i % 3 == 1 else v for i, v in enumerate(lb[::-1])]
    return [([lane] * n, [3.5] * n, 1.0), (lb, sb, 1.0), (lc, [2.0] * n, 0.0), (ld, sb[::-1], 1.0)]


def _batch_crcs(plan, ch, table, xs):
    from speedy_amd.batch import Batch
    lens, speeds, nl = table
    b = Batch(plan, lens, ch, speeds, nl, 0.0)
    b.upload(xs)
    b.run()
    return _crc(b.results())


def _check_oracle(orc, crcs, xs, rate, ch, table, what):
    lens, speeds, nl = table
    for i in (0, len(lens) // 2, len(lens) - 1):
        assert crcs[i] == _oracle_crc(orc, xs[i], rate, ch, speeds[i], nl), (what, i)


def _host_outs(pipe, t, lens):
    """One wait: the per-stream outputs, with what the packed layout promises checked on the way."""
    out, offsets, counts = pipe.wait(t)
    assert all(int(o) % 32 == 0 for o in offsets), t
    assert (counts >= 0).all(), t
    res = []
    for i in range(pipe.n):
        c = int(pipe.channels[i])
        if lens[i] == 0:
            assert int(counts[i]) == 0 and int(offsets[i + 1]) == int(offsets[i]), (t, i)   # an empty lane takes no room at all
        assert int(offsets[i + 1]) - int(offsets[i]) == (int(counts[i]) * c + 31) // 32 * 32, (t, i)
        res.append(out[int(offsets[i]):int(offsets[i]) + int(counts[i]) * c].copy())
    return res


@pytest.mark.parametrize("rate,ch,n,depth", [(16000, 1, 256, 4), (16000, 1, 61, 2), (22050, 1, 256, 3), (16000, 2, 128, 3),
                                             (16000, 1, 400, 3)])   # (256 x mono: pipelined order, lean walk kernels; 400: run_split)
def test_ragged_batches_with_tickets_lagging(orc, rate, ch, n, depth):
    """Twelve submits cycling four tables, each with content no earlier submit had, waited for depth - 1 submits later."""
    import torch
    from speedy_amd.batch import Pipeline, Plan
    plan = Plan(rate, False)
    lane = int(1.1 * rate)
    tables = _tables(rate, n, lane, n * 7 + depth)
    bases = _bases(rate, ch, lane, (11, 12, 13))
    pipe = Pipeline(plan, [lane] * n, ch, 3.5, 1.0, 0.0, depth=depth)
    want, packed = [], []
    for k in range(12):
        tab = tables[k % 4]
        xs = _content(bases, k, ch, tab[0])
        want.append(_batch_crcs(plan, ch, tab, xs))
        if k < 4:
            _check_oracle(orc, want[k], xs, rate, ch, tab, k)
        packed.append(torch.from_numpy(pipe.pack(xs, tab[0])).pin_memory())
    assert len({tuple(w) for w in want}) == 12
    modes = []
    tickets = []
    lag = depth - 1

    def check(k):
        tab = tables[k % 4]
        outs = _host_outs(pipe, tickets[k], tab[0])
        assert _crc(outs) == want[k], (k, tickets[k])

    for k in range(12):
        lens, speeds, nl = tables[k % 4]
        assert pipe.fits(lens, speeds, nl)
        tickets.append(pipe.submit_jobs(packed[k], lens, speed=speeds, nonlinear=nl))
        assert tickets[k] == k
        modes.append((plan.L.spx_debug_last_call_concurrent(), plan.L.spx_debug_last_walk_form()))
        if k >= lag:
            check(k - lag)
    for k in range(12 - lag, 12):
        check(k)
    print("launch order / walk form per submit (A B C D ...), rate %d ch %d n %d depth %d: %s" % (rate, ch, n, depth, modes))
    pipe.close()
    plan.close()


def test_fixed_and_varying_submits_interleaved(orc):
    """spx_pipeline_submit and spx_pipeline_submit_jobs taking turns on one pipeline: the fixed-shape tickets give the bytes they
    give on a pipeline that never sees a varying batch."""
    import torch
    from speedy_amd.batch import Pipeline, Plan
    rate, ch, n, depth = 16000, 1, 256, 3
    plan = Plan(rate, False)
    lane = int(1.1 * rate)
    ta, tb = _tables(rate, n, lane, 5)[:2]
    bases = _bases(rate, ch, lane, (21, 22))
    xa = [_content(bases, k, ch, ta[0]) for k in range(3)]
    xb = [_content(bases, 5 + k, ch, tb[0]) for k in range(2)]
    want_a = [_batch_crcs(plan, ch, ta, x) for x in xa]
    want_b = [_batch_crcs(plan, ch, tb, x) for x in xb]
    _check_oracle(orc, want_a[0], xa[0], rate, ch, ta, "A")
    _check_oracle(orc, want_b[0], xb[0], rate, ch, tb, "B")
    only_fixed = Pipeline(plan, ta[0], ch, 3.5, 1.0, 0.0, depth=depth)
    pa = [torch.from_numpy(only_fixed.pack(x)).pin_memory() for x in xa]
    ts = [only_fixed.submit(pa[k % 3]) for k in range(6)]
    fixed_bytes = {}
    for k in (3, 4, 5):
        fixed_bytes[k % 3] = _crc(only_fixed.results(ts[k]))
        assert fixed_bytes[k % 3] == want_a[k % 3]
    only_fixed.close()
    pipe = Pipeline(plan, ta[0], ch, 3.5, 1.0, 0.0, depth=depth)
    pb = [torch.from_numpy(pipe.pack(x, tb[0])).pin_memory() for x in xb]
    ts = []
    for k in range(12):
        if k % 2 == 0:
            ts.append((pipe.submit(pa[(k // 2) % 3]), fixed_bytes[(k // 2) % 3]))
        else:
            ts.append((pipe.submit_jobs(pb[(k // 2) % 2], tb[0], speed=tb[1]), want_b[(k // 2) % 2]))
        if k >= 2:
            t, w = ts[k - 2]
            assert _crc(pipe.results(t)) == w, (k, t)
    for t, w in ts[-2:]:
        assert _crc(pipe.results(t)) == w, t
    pipe.close()
    plan.close()


def test_device_input_and_device_output(orc):
    """SPX_PIPELINE_DEVICE_OUT with a device tensor as input: offsets stay the static capacity layout whatever the table, the counts
    are read from the device."""
    import torch
    from speedy_amd.batch import Pipeline, Plan
    rate, ch, n, depth = 16000, 1, 256, 4
    plan = Plan(rate, False)
    lane = int(1.1 * rate)
    tabs = _tables(rate, n, lane, 9)[:2]
    bases = _bases(rate, ch, lane, (31,))
    pipe = Pipeline(plan, [lane] * n, ch, 3.5, 1.0, 0.0, depth=depth, device_out=True)
    cap = (plan.out_capacity(lane, 3.5, 1.0) * ch + 31) // 32 * 32
    static = [i * cap for i in range(n + 1)]
    want, d_in = [], []
    for c, tab in enumerate(tabs):
        xs = _content(bases, c, ch, tab[0])
        want.append(_batch_crcs(plan, ch, tab, xs))
        _check_oracle(orc, want[c], xs, rate, ch, tab, c)
        d = torch.zeros(pipe.total_in + 64, dtype=torch.int16, device="cuda")
        d[: pipe.total_in].copy_(torch.from_numpy(pipe.pack(xs, tab[0])))
        d_in.append(d)
    torch.cuda.synchronize()
    ts = []
    for k in range(9):
        lens, speeds, nl = tabs[k % 2]
        ts.append(pipe.submit_jobs(d_in[k % 2], lens, speed=speeds, nonlinear=nl))
        if k >= depth - 1:
            j = k - (depth - 1)
            assert [int(v) for v in pipe.wait(ts[j])[1]] == static, j
            assert _crc(pipe.results(ts[j])) == want[j % 2], j
    for j in range(9 - (depth - 1), 9):
        assert [int(v) for v in pipe.wait(ts[j])[1]] == static, j
        assert _crc(pipe.results(ts[j])) == want[j % 2], j
    pipe.close()
    plan.close()


def test_mixed_rates(orc):
    """A 16 kHz + 22.05 kHz pipeline, two tables that differ in lengths and speeds, against the plain mixed call."""
    import torch
    from speedy_amd.batch import MixedBatch, Pipeline, Plan
    from speedy_amd.synth import speech_like
    rates = [16000, 22050]
    plans = [Plan(r, False) for r in rates]
    n, depth = 90, 3
    pidx = [i % 2 for i in range(n)]
    chs = [1 if (i // 2) % 2 == 0 else 2 for i in range(n)]
    lanes = [int(1.1 * rates[pidx[i]]) for i in range(n)]
    rng = np.random.default_rng(90)
    tabs = [(lanes, [1.5 if (i // 4) % 2 == 0 else 3.5 for i in range(n)]),
            ([int(rng.integers(int(0.2 * rates[pidx[i]]), lanes[i] + 1)) for i in range(n)], [SPEEDS[int(v)] for v in rng.integers(0, 3, n)])]
    pipe = Pipeline(plans, lanes, chs, tabs[0][1], 1.0, 0.0, depth=depth, plan_index=pidx)
    want, packed = [], []
    for c, (lens, speeds) in enumerate(tabs):
        xs = [speech_like(lens[i], rates[pidx[i]], seed=4100 + 100 * c + (i % 12), channels=chs[i]) for i in range(n)]
        mb = MixedBatch(plans, pidx, lens, chs, speeds, 1.0, 0.0)
        mb.upload(xs)
        mb.run()
        want.append(mb.crcs())
        for i in (0, n // 2, n - 1):
            assert want[c][i] == _oracle_crc(orc, xs[i], rates[pidx[i]], chs[i], speeds[i], 1.0), (c, i)
        packed.append(torch.from_numpy(pipe.pack(xs, lens)).pin_memory())
    ts = []
    for k in range(8):
        lens, speeds = tabs[k % 2]
        ts.append(pipe.submit_jobs(packed[k % 2], lens, speed=speeds))
        if k >= 2:
            assert _crc(_host_outs(pipe, ts[k - 2], tabs[k % 2][0])) == want[k % 2], k
    for k in (6, 7):
        assert _crc(_host_outs(pipe, ts[k], tabs[k % 2][0])) == want[k % 2], k
    # a lane keeps the capacity it was created with: a 16 kHz lane does not take the frames of a 22.05 kHz one
    longer = list(tabs[0][0])
    longer[0] = lanes[1]
    assert not pipe.fits(longer) and b"lane 0" in pipe.L.spx_last_error()
    pipe.close()
    for p in plans:
        p.close()


def test_refusals_leave_the_pipeline_as_it_was(orc):
    """Every table that does not fit is refused with the lane named, spx_pipeline_jobs_fit says the same, no ticket is used up, the
    batch in flight during the refusal delivers its bytes and the next valid submit works."""
    import math
    from speedy_amd.batch import Pipeline, Plan
    rate, ch, n = 16000, 1, 8
    plan = Plan(rate, False)
    L = plan.L
    lane = int(1.1 * rate)
    full = ([lane] * n, [3.5] * n, 1.0)
    short = ([lane - 700 * (i + 1) for i in range(n)], [SPEEDS[i % 3] for i in range(n)], 1.0)
    lin = ([lane - 500 * i for i in range(n)], [2.0] * n, 0.0)
    bases = _bases(rate, ch, lane, (51,))
    x_full, x_short, x_lin = (_content(bases, k, ch, t[0]) for k, t in enumerate((full, short, lin)))
    w_full, w_short, w_lin = (_batch_crcs(plan, ch, t, x) for t, x in ((full, x_full), (short, x_short), (lin, x_lin)))
    _check_oracle(orc, w_full, x_full, rate, ch, full, "full")
    _check_oracle(orc, w_short, x_short, rate, ch, short, "short")
    _check_oracle(orc, w_lin, x_lin, rate, ch, lin, "linear")
    pipe = Pipeline(plan, full[0], ch, 3.5, 1.0, 0.0, depth=3)
    linear_pipe = Pipeline(plan, full[0], ch, 2.0, 0.0, 0.0, depth=3)      # created LINEAR: no analysis frames in its workspace
    in_full, in_short = pipe.pack(x_full), pipe.pack(x_short, short[0])
    in_lin = linear_pipe.pack(x_lin, lin[0])

    def bad(lane_i, **change):
        """The short table with one lane changed."""
        kw = dict(lengths=list(short[0]), speed=list(short[1]), nonlinear=[1.0] * n, feedback=[0.0] * n, in_offs=list(pipe.in_offs))
        for key, v in change.items():
            kw[key][lane_i] = v
        return kw

    cases = [("a lane longer than created", 3, pipe, bad(3, lengths=lane + 1), None),
             ("past the input extent", 7, pipe, bad(7, lengths=lane, in_offs=pipe.in_offs[7] + 1), None),
             ("a slow-down on a lane created at 3.5x", 2, pipe, bad(2, speed=0.5), None),
             ("another channel count", 5, pipe, bad(5), 2),
             ("nonlinear jobs on a pipeline created linear", 0, linear_pipe, dict(lengths=lin[0], nonlinear=[1.0] * n), None),
             ("speed 0", 1, pipe, bad(1, speed=0.0), None),
             ("feedback not a number", 6, pipe, bad(6, feedback=math.nan), None)]
    for what, lane_i, p, kw, channels in cases:
        live_in, live_want = (in_lin, w_lin) if p is linear_pipe else (in_full, w_full)
        ok_in, ok_tab, ok_want = (in_lin, lin, w_lin) if p is linear_pipe else (in_short, short, w_short)
        live = p.submit_jobs(live_in, lin[0]) if p is linear_pipe else p.submit(live_in)       # in flight during the refusal
        jobs = p.table(**kw)
        if channels is not None:
            jobs[lane_i].channels = channels
        assert L.spx_pipeline_jobs_fit(p.h, jobs) == -1, what
        msg_fit = L.spx_last_error().decode()
        assert L.spx_pipeline_submit_jobs(p.h, jobs, ok_in.ctypes.data, 0) == -1, what
        msg = L.spx_last_error().decode()
        assert msg and ("lane %d" % lane_i) in msg and msg == msg_fit, (what, msg, msg_fit)
        if channels is None:
            assert not p.fits(**kw)
            with pytest.raises(RuntimeError, match="lane %d" % lane_i):
                p.submit_jobs(ok_in, **kw)
        assert p.fits(ok_tab[0], ok_tab[1], ok_tab[2])
        nxt = p.submit_jobs(ok_in, ok_tab[0], speed=ok_tab[1], nonlinear=ok_tab[2])
        assert nxt == live + 1, (what, live, nxt)                                                # no ticket was used up
        assert _crc(p.results(live)) == live_want, what
        assert _crc(_host_outs(p, nxt, ok_tab[0])) == ok_want, what
    # a table of another length than the pipeline's n_streams cannot be told from outside; a missing one can
    assert L.spx_pipeline_jobs_fit(pipe.h, None) == -1 and L.spx_pipeline_submit_jobs(pipe.h, None, in_full.ctypes.data, 0) == -1
    pipe.close()
    linear_pipe.close()
    plan.close()


def test_host_copy_reaches_this_batchs_extent_only(orc):
    """A short batch, its lanes packed densely, from a pageable array that ends where the batch ends is accepted and gives the
    right bytes.  (That the copy in stops there too is the library's promise; a copy that read on would rarely fault, so this test
    does not prove it.)"""
    from speedy_amd.batch import Pipeline, Plan
    rate, ch, n = 16000, 2, 16
    plan = Plan(rate, False)
    lane = int(1.1 * rate)
    lens = [int(0.2 * rate) + 97 * i for i in range(n)]
    speeds = [SPEEDS[i % 3] for i in range(n)]
    offs = [int(v) for v in np.concatenate(([0], np.cumsum(np.asarray(lens) * ch)[:-1]))]      # packed densely: a small extent
    extent = offs[-1] + lens[-1] * ch
    bases = _bases(rate, ch, lane, (61,))
    xs = _content(bases, 0, ch, lens)
    want = _batch_crcs(plan, ch, (lens, speeds, 1.0), xs)
    _check_oracle(orc, want, xs, rate, ch, (lens, speeds, 1.0), "short")
    pipe = Pipeline(plan, [lane] * n, ch, 3.5, 1.0, 0.0, depth=2)
    assert extent * 4 < pipe.total_in
    host = np.concatenate(xs)
    assert host.size == extent
    full = pipe.submit(np.zeros(pipe.total_in, np.int16))                 # the lanes hold something else first
    t = pipe.submit_jobs(host, lens, speed=speeds, in_offs=offs)
    assert (full, t) == (0, 1)
    assert _crc(_host_outs(pipe, t, lens)) == want
    pipe.close()
    plan.close()


def test_c_example_prints_the_oracles_counts_and_crcs(orc, tmp_path):
    """tools/pipeline_jobs_example.c (plain C99 over include/speedy_hip.h): three batches of different lengths and speeds through
    one pipeline, every line of its output against the oracle."""
    exe = os.path.join(ROOT, "speedy_amd", "lib", "pipeline_jobs_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "speedy_amd", "csrc"), "pipejobsexample"])
    x, rate_hz, ch = read_wav("tapestry.wav")
    x = x[: 2 * rate_hz * ch]
    raw = str(tmp_path / "in.raw")
    x.astype("<i2").tofile(raw)
    lanes = 4
    r = subprocess.run([exe, raw, str(rate_hz), str(ch), str(lanes), "3"], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    assert "refused as expected" in r.stderr and "lane %d" % (lanes - 1) in r.stderr, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("ticket ")]
    assert len(lines) == 3 * lanes, r.stdout
    shapes = set()
    for k, f in enumerate(lines):
        assert (int(f[1]), int(f[3])) == (k // lanes, k % lanes), f
        n_in, speed, nl = int(f[5]), float(f[7]), float(f[9])
        shapes.add((k // lanes, n_in, speed, nl))
        ref = orc.compress_sound(x[: n_in * ch], rate_hz, ch, speed, nl, 0.0, False, chunk=1000, taps=False)["out"] if n_in else np.zeros(0, np.int16)
        assert int(f[11]) == ref.size // ch, (f, ref.size // ch)
        assert int(f[13], 16) == zlib.crc32(ref.astype("<i2").tobytes()), f
    assert len({s[1:] for s in shapes}) >= 2 * lanes       # the batches really differ in lengths and speeds
