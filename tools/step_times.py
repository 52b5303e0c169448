"""GPU box: one line of profiles/analysis_first.txt per process -- the loop KIND timed for the library SPEEDY_HIP_LIB names (the
shipped one when unset).

    python3 tools/step_times.py KIND
      pipe16 / pipe22   256 streams x 10 s mono at 16 / 22.05 kHz through the pipeline object, depth 4, outputs left on the device:
                        two untimed windows, then one with the library's event timing (ms per launch)
      plain             the plain call (spx_batch_run) of the bench batch, two windows
      config4           the configs[4] shard (speedy_amd/config4.py) through the mixed pipeline object, two windows
      big               2 048 streams x 10 s in one plain call, two windows of 10 calls behind 3

60 batches per window behind 12 warm-up batches, as in profiles/tension_sequence.txt."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
from speedy_amd.batch import Batch, Pipeline, Plan  # noqa: E402

kind = sys.argv[1]
STEPS, WARM = 60, 12


def window(fn, steps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def tail(L):
    return "[mode %d]" % L.spx_debug_last_call_concurrent()


if kind in ("pipe16", "pipe22"):
    rate = 16000 if kind == "pipe16" else 22050
    n = rate * bench.SECONDS
    plan = Plan(rate, False)
    b = Batch(plan, [n] * bench.STREAMS_PER_GPU, 1, bench.SPEED, 1.0, 0.0)
    if rate == bench.RATE:
        b.upload(bench.make_streams(bench.STREAMS_PER_GPU, n, 0))
    else:
        from speedy_amd.synth import speech_like
        base = [speech_like(n, rate, seed=900 + i) for i in range(16)]
        b.upload([base[i % 16] for i in range(bench.STREAMS_PER_GPU)])
    pipe = Pipeline(plan, [n] * bench.STREAMS_PER_GPU, 1, bench.SPEED, 1.0, 0.0, depth=4, device_out=True)
    L = plan.L
    fn = lambda: pipe.submit(b.d_in)  # noqa: E731
    w = [window(fn, STEPS, WARM), window(fn, STEPS, WARM)]
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    L.spx_set_timing(1)
    t0 = time.perf_counter()
    for _ in range(STEPS):
        fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / STEPS * 1e3
    L.spx_set_timing(0)
    sa, sw, nc = C.c_double(0), C.c_double(0), C.c_int(0)
    L.spx_timing_collect(C.byref(sa), C.byref(sw), C.byref(nc))
    k = max(1, nc.value)
    print("%d Hz step %.4f / %.4f ms (untimed windows); with event timing: step %.4f, analysis %.4f, tension %.4f, lean walk %.4f ms per launch  %s"
          % (rate, w[0], w[1], dt, sa.value / k, L.spx_timing_last_tension_ms() / k, sw.value / k, tail(L)))
    pipe.close()
elif kind == "plain":
    n = bench.RATE * bench.SECONDS
    plan = Plan(bench.RATE, False)
    b = Batch(plan, [n] * bench.STREAMS_PER_GPU, 1, bench.SPEED, 1.0, 0.0)
    b.upload(bench.make_streams(bench.STREAMS_PER_GPU, n, 0))
    w = [window(b.run, STEPS, WARM), window(b.run, STEPS, WARM)]
    print("plain call (unpipelined) %.4f / %.4f ms per step  %s" % (w[0], w[1], tail(plan.L)))
elif kind == "big":
    n = bench.RATE * bench.SECONDS
    plan = Plan(bench.RATE, False)
    b = Batch(plan, [n] * 2048, 1, bench.SPEED, 1.0, 0.0)
    b.upload(bench.make_streams(bench.STREAMS_PER_GPU, n, 0) * 8)
    w = [window(b.run, 10, 3), window(b.run, 10, 3)]
    print("2 048 streams per call %.3f / %.3f ms per call  %s" % (w[0], w[1], tail(plan.L)))
elif kind == "config4":
    from speedy_amd import config4 as C4
    ids = C4.rank_ids(0, 8)
    plans = [Plan(r, False) for r in C4.RATES]
    xs = C4.make_streams(ids)
    lens = [C4.SECONDS * C4.cfg(i)[0] for i in ids]
    pipe = Pipeline(plans, lens, [C4.cfg(i)[1] for i in ids], [C4.cfg(i)[2] for i in ids], 1.0, 0.0, depth=4, device_out=True,
                    plan_index=[C4.RATES.index(C4.cfg(i)[0]) for i in ids])
    d = torch.zeros(pipe.total_in + 64, dtype=torch.int16, device="cuda")
    d[: pipe.total_in] = torch.from_numpy(pipe.pack(xs)).cuda()
    torch.cuda.synchronize()
    fn = lambda: pipe.submit(d)  # noqa: E731
    w = [window(fn, STEPS, WARM), window(fn, STEPS, WARM)]
    print("configs[4] shard through the mixed pipeline object %.4f / %.4f ms per step  %s" % (w[0], w[1], tail(plans[0].L)))
    pipe.close()
else:
    raise SystemExit(__doc__)
