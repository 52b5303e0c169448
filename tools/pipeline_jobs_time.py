"""Times behind profiles/pipeline_jobs.txt: the pipeline object with a job table per batch (spx_pipeline_submit_jobs).
Device-resident input, outputs left on the device (SPX_PIPELINE_DEVICE_OUT), 16 kHz mono, bench.py's own streams.

  python tools/pipeline_jobs_time.py fixed     BASELINE configs[3] (256 x 10 s, 3.5x nonlinear, depth 4) through spx_pipeline_submit and,
                                               where the library has it, through spx_pipeline_submit_jobs handed the creation table:
                                               ms per batch over windows of 100 submits (SPEEDY_HIP_LIB selects the build: the parent
                                               commit's for the record -- run the builds in turns, one process each)
  python tools/pipeline_jobs_time.py ragged    100 batches of 256 lanes, lengths uniform in [2, 10] s, a speed of 1.5 / 2.0 / 3.5 per
                                               lane, nonlinear: through spx_pipeline_submit_jobs on ONE pipeline; through
                                               spx_batch_run_overlapped with three caller-owned buffer sets (the best a caller of a
                                               library without the call could do); through a pipeline created per shape
  python tools/pipeline_jobs_time.py modes RATE CHANNELS
                                               eight ragged submits of 256 lanes of 2 .. 4 s at RATE / CHANNELS and what
                                               spx_debug_last_call_concurrent says behind each (SPX_DEBUG_MODE=1 prints the engine's
                                               own line per call on stderr)
Every figure is a host clock around a window of submits that ends with the wait for the window's last tickets."""
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # as bench.py

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RATE_HZ, N_LANES, SECONDS, DEPTH = 16000, 256, 10, 4
SPEEDS = (1.5, 2.0, 3.5)
ORDER = {0: "in sequence", 1: "concurrent", 2: "pipelined"}


def device_input(pipe, xs):
    import torch
    d = torch.zeros(pipe.total_in + 64, dtype=torch.int16, device="cuda")
    d[: pipe.total_in].copy_(torch.from_numpy(pipe.pack(xs)))
    torch.cuda.synchronize()
    return d


def window(submit, pipe, reps):
    """ms per batch of `reps` submits back to back, the clock stopped when the last `depth` tickets have been waited for."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ts = [submit(k) for k in range(reps)]
    for t in ts[-pipe.depth:]:
        pipe.wait(t)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def fixed():
    import bench
    from speedy_amd.batch import Pipeline, Plan
    plan = Plan(RATE_HZ, False)
    L = plan.L
    n = SECONDS * RATE_HZ
    pipe = Pipeline(plan, [n] * N_LANES, 1, 3.5, 1.0, 0.0, depth=DEPTH, device_out=True)
    d_in = device_input(pipe, bench.make_streams(N_LANES, n, 0))
    ptr = d_in.data_ptr()
    routes = [("spx_pipeline_submit", lambda k: L.spx_pipeline_submit(pipe.h, ptr, 1))]
    if hasattr(L, "spx_pipeline_submit_jobs"):
        routes.append(("spx_pipeline_submit_jobs, creation table", lambda k: L.spx_pipeline_submit_jobs(pipe.h, pipe.jobs, ptr, 1)))
    times = {name: [] for name, _ in routes}
    for name, submit in routes:
        window(submit, pipe, 40)   # warm-up: code objects, the launch mode's trial, the buffer sets
    for _ in range(5):             # the routes in turns
        for name, submit in routes:
            times[name].append(window(submit, pipe, 100))
    for name, _ in routes:
        t = times[name]
        print("fixed %-42s ms per batch, 5 windows of 100: %s  min %.4f median %.4f  -> %.1f Gsamples/s  (%s, walk form %d)"
              % (name + ":", " ".join("%.4f" % v for v in t), min(t), statistics.median(t), n * N_LANES / statistics.median(t) / 1e6,
                 ORDER[L.spx_debug_last_call_concurrent()], L.spx_debug_last_walk_form()))
    pipe.close()
    plan.close()


def ragged_tables(rng, batches, lo, hi, n_lanes=N_LANES):
    return [([int(v) for v in rng.integers(lo, hi + 1, n_lanes)], [SPEEDS[int(v)] for v in rng.integers(0, 3, n_lanes)]) for _ in range(batches)]


def ragged():
    import ctypes as C
    import bench
    import torch
    from speedy_amd.batch import Pipeline, Plan
    plan = Plan(RATE_HZ, False)
    L = plan.L
    lane = SECONDS * RATE_HZ
    batches = 100
    tabs = ragged_tables(np.random.default_rng(2024), batches, 2 * RATE_HZ, lane)
    frames = [sum(t[0]) for t in tabs]
    pipe = Pipeline(plan, [lane] * N_LANES, 1, 3.5, 1.0, 0.0, depth=DEPTH, device_out=True)
    d_in = device_input(pipe, bench.make_streams(N_LANES, lane, 0))   # lane i of every batch reads the front of stream i
    ptr = d_in.data_ptr()
    jobs = [pipe.table(lens, speed=speeds) for lens, speeds in tabs]
    assert all(L.spx_pipeline_jobs_fit(pipe.h, j) == 0 for j in jobs)
    orders = []

    def submit(k):
        t = L.spx_pipeline_submit_jobs(pipe.h, jobs[k], ptr, 1)
        orders.append(L.spx_debug_last_call_concurrent())
        return t

    def report(what, ms, n_batches, note=""):
        fr = sum(frames[:n_batches]) / n_batches
        print("ragged %-58s ms per batch %s  median %.4f  -> %.1f Gsamples/s%s"
              % (what + ":", " ".join("%.4f" % v for v in ms), statistics.median(ms), fr / statistics.median(ms) / 1e6, note))

    window(submit, pipe, batches)
    del orders[:]
    ms = [window(submit, pipe, batches) for _ in range(3)]
    report("spx_pipeline_submit_jobs, one pipeline", ms, batches,
           "  launch order of the %d calls: %s" % (len(orders), ", ".join("%s x %d" % (ORDER[o], orders.count(o)) for o in sorted(set(orders)))))
    # the last batch's counts, to compare the routes
    t = L.spx_pipeline_submit_jobs(pipe.h, jobs[-1], ptr, 1)
    _, offsets, counts_ptr = pipe.wait(t)
    want = torch.empty(N_LANES, dtype=torch.int64)
    L.spx_copy_to_host(want.data_ptr(), counts_ptr, N_LANES * 8, None)
    L.spx_stream_synchronize(None)
    # the same batches through spx_batch_run_overlapped: three buffer sets of the caller's, each sized for the longest lanes
    cap = plan.out_capacity(lane, 3.5, 1.0)
    step = (cap + 31) // 32 * 32
    for j in jobs:
        for i in range(N_LANES):
            j[i].out_off, j[i].out_cap = i * step, cap
    wsb = L.spx_batch_workspace_bytes(plan.h, pipe.jobs, N_LANES)
    assert all(L.spx_batch_workspace_bytes(plan.h, j, N_LANES) <= wsb for j in jobs)
    sets = [(torch.zeros(N_LANES * step + 64, dtype=torch.int16, device="cuda"), torch.zeros(N_LANES, dtype=torch.int64, device="cuda"),
             torch.zeros(wsb, dtype=torch.uint8, device="cuda")) for _ in range(3)]
    hs = torch.cuda.current_stream().cuda_stream
    orders2 = []

    def overlapped(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(reps):
            o, c, w = sets[k % 3]
            rc = L.spx_batch_run_overlapped(plan.h, jobs[k], N_LANES, ptr, o.data_ptr(), c.data_ptr(), w.data_ptr(), wsb, None, hs)
            assert rc == 0, L.spx_last_error()
            orders2.append(L.spx_debug_last_call_concurrent())
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps

    overlapped(batches)
    del orders2[:]
    ms = [overlapped(batches) for _ in range(3)]
    report("spx_batch_run_overlapped, three caller-owned buffer sets", ms, batches,
           "  launch order: %s" % ", ".join("%s x %d" % (ORDER[o], orders2.count(o)) for o in sorted(set(orders2))))
    got = sets[(batches - 1) % 3][1].cpu()
    print("ragged: the last batch's counts by both routes are %s" % ("equal" if torch.equal(got, want) else "DIFFERENT"))
    pipe.close()
    del sets
    # a pipeline per shape: created, one batch, waited for, destroyed
    some = 20

    def per_shape():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for lens, speeds in tabs[:some]:
            q = Pipeline(plan, lens, 1, speeds, 1.0, 0.0, depth=2, device_out=True)
            q.wait(L.spx_pipeline_submit(q.h, ptr, 1))   # (the lanes lie densely here and read other samples: the time is what counts)
            q.close()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / some

    per_shape()
    report("a pipeline created per shape (depth 2), %d batches" % some, [per_shape() for _ in range(3)], some)
    plan.close()


def modes(rate, ch):
    import torch
    from speedy_amd.batch import Pipeline, Plan
    plan = Plan(rate, False)
    L = plan.L
    lane = 4 * rate
    tabs = ragged_tables(np.random.default_rng(7), 8, 2 * rate, lane)
    pipe = Pipeline(plan, [lane] * N_LANES, ch, 3.5, 1.0, 0.0, depth=3, device_out=True)
    d = torch.zeros(pipe.total_in + 64, dtype=torch.int16, device="cuda")
    d.random_(-3000, 3000)
    torch.cuda.synchronize()
    seen = []
    for rep in range(3):
        for lens, speeds in tabs:
            t = pipe.submit_jobs(d, lens, speed=speeds)
            seen.append(L.spx_debug_last_call_concurrent())
    pipe.wait(t)
    torch.cuda.synchronize()
    print("modes rate %d channels %d, 256 lanes of 2 .. 4 s, 24 ragged submits (8 tables x 3): spx_debug_last_call_concurrent = %s" % (rate, ch, seen))
    # ... and a batch whose speed class differs: one slow-down lane behind speed-up batches (the lane must have been created for it)
    slow = Pipeline(plan, [lane] * N_LANES, ch, [0.8] + [3.5] * (N_LANES - 1), 1.0, 0.0, depth=3, device_out=True)
    seen = []
    for k in range(6):
        lens, speeds = tabs[k]
        speeds = list(speeds)
        if k % 3 == 2:
            speeds[0] = 0.8
        t = slow.submit_jobs(d, lens, speed=speeds)
        seen.append((speeds[0] < 1, L.spx_debug_last_call_concurrent(), L.spx_debug_last_walk_form()))
    slow.wait(t)
    torch.cuda.synchronize()
    print("modes rate %d channels %d: (a lane at speed 0.8?, launch order, walk form) per submit = %s" % (rate, ch, seen))
    pipe.close()
    slow.close()
    plan.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode not in ("fixed", "ragged", "modes"):
        sys.exit(__doc__)
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    print("library: %s  GPU_MAX_HW_QUEUES=%s" % (os.environ.get("SPEEDY_HIP_LIB") or "speedy_amd/lib/libspeedy_hip.so", os.environ["GPU_MAX_HW_QUEUES"]))
    if mode == "modes":
        modes(int(sys.argv[2]), int(sys.argv[3]))
    else:
        (fixed if mode == "fixed" else ragged)()
