"""Times behind profiles/pipeline_rate.txt: the rate pipeline (spx_pipeline_create_rate) beside the only route a caller with playback
rates had before it, and its all-ones batches beside the ordinary pipeline.  BASELINE configs[3]'s shape: 256 lanes x 10 s, 16 kHz
mono, 3.5x nonlinear, bench.py's own streams, rate 1.25 on every lane, depth 4.

  python tools/pipeline_rate_time.py            the four routes, three windows each, the routes in turns
  python tools/pipeline_rate_time.py --trace    twenty rate batches through the pipeline and nothing else: the run to put under
                                                rocprofv3 --kernel-trace --stats for the kernel split (the gather included)

  (a) rate pipeline, pinned host memory to pinned host memory, rate 1.25 (spx_pipeline_submit_jobs_rate / spx_pipeline_wait)
  (b) what a caller had without it: call by call -- their own host-to-device copy, spx_batch_run_rate, spx_batch_pack_outputs, a copy
      of the offsets and counts and a host wait to learn the produced size, then the copy out of exactly that size and a second wait
  (c) rate pipeline, batches of ones (spx_pipeline_submit_jobs: the overlapped order)
  (d) the ordinary pipeline (spx_pipeline_create) on the same table: the yardstick of (c), same process
Every figure is a host clock around a window of batches behind warm-up batches; the window ends with the wait for its last tickets
and a device synchronise.  A pipeline is created for its window and destroyed behind it, so that no other pipeline's streams share
the process's hardware queues with it.  The kernel split of a rate batch comes from the library's timing hooks (spx_set_timing) on
spx_batch_run_rate calls of the same table: analysis, tension, general walk and rate kernel; the gather is not behind the hooks."""
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # as bench.py

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RATE_HZ, N_LANES, SECONDS, DEPTH, PLAYBACK = 16000, 256, 10, 4, 1.25
WARM, BATCHES, WINDOWS = 10, 60, 3


def window(submit, wait, depth, reps):
    """ms per batch of `reps` submits back to back, the clock stopped when the last `depth` tickets have been waited for."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ts = [submit() for _ in range(reps)]
    for t in ts[-depth:]:
        wait(t)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main(trace_only):
    import ctypes as C
    import bench
    import torch
    from speedy_amd.batch import Batch, Pipeline, Plan
    assert torch.cuda.is_available(), "needs an MI355X"
    n = SECONDS * RATE_HZ
    xs = bench.make_streams(N_LANES, n, 0)
    plan = Plan(RATE_HZ, False)
    L = plan.L
    lens = [n] * N_LANES
    rates = np.full(N_LANES, PLAYBACK, np.float32)
    rates_p = rates.ctypes.data_as(C.POINTER(C.c_float))
    state = {}

    def pipe_route(kind):
        """A pipeline of its own, alive for one window, and (submit, wait).  kind: 'rate' (a), 'ones' (c), 'plain' (d).
        (c)'s lanes are sized for rate 1 -- the same output layout as (d)'s; the workspace still reserves every lane's staging."""
        pipe = Pipeline(plan, lens, 1, 3.5, 1.0, 0.0, depth=DEPTH, rate={"rate": PLAYBACK, "ones": 1.0, "plain": None}[kind])
        if "x" not in state:
            state["x"] = torch.from_numpy(pipe.pack(xs)).pin_memory()
            torch.cuda.synchronize()
        ptr = state["x"].data_ptr()
        jobs = pipe.table(lens)
        o, f, c = C.c_void_p(), C.c_void_p(), C.c_void_p()

        def submit():
            if kind == "rate":
                t = L.spx_pipeline_submit_jobs_rate(pipe.h, jobs, rates_p, ptr, 0)
            else:
                t = L.spx_pipeline_submit_jobs(pipe.h, jobs, ptr, 0)
            assert t >= 0, L.spx_last_error()
            return t

        def wait(t):
            assert L.spx_pipeline_wait(pipe.h, t, C.byref(o), C.byref(f), C.byref(c)) == 0, L.spx_last_error()

        return pipe, submit, wait

    if trace_only:
        pipe, submit, wait = pipe_route("rate")
        window(submit, wait, DEPTH, 20)
        pipe.close()
        plan.close()
        return

    # (b) the batch call with the caller's own copies, packing and waits
    rb = Batch(plan, lens, 1, 3.5, 1.0, 0.0, rate=rates)
    h_in = torch.from_numpy(np.concatenate(xs)).pin_memory()
    h_out = torch.empty(rb.d_out.numel(), dtype=torch.int16).pin_memory()
    h_offs = torch.empty(N_LANES + 1, dtype=torch.int64).pin_memory()
    h_cnt = torch.empty(N_LANES, dtype=torch.int64).pin_memory()

    def call_by_call():
        rb.d_in[: rb.total_in].copy_(h_in, non_blocking=True)
        rb.run()
        packed, offsets = rb.pack_outputs()
        h_offs.copy_(offsets, non_blocking=True)
        h_cnt.copy_(rb.d_nout, non_blocking=True)
        torch.cuda.synchronize()                     # the produced size is known on the device only
        total = int(h_offs[N_LANES])
        h_out[:total].copy_(packed[:total], non_blocking=True)
        torch.cuda.synchronize()
        return 0

    # ---- results first: the two routes deliver the same frames ----
    pa, sub_a, _ = pipe_route("rate")
    out, offs, cnt = pa.wait(sub_a())
    call_by_call()
    assert np.array_equal(h_cnt.numpy(), cnt) and (cnt > 0).all()
    for i in range(N_LANES):
        lo, k, lo2 = int(offs[i]), int(cnt[i]), int(h_offs[i])
        assert np.array_equal(out[lo:lo + k], h_out.numpy()[lo2:lo2 + k]), "lane %d" % i
    print("batch: %d lanes x %d frames = %.1f MB of int16 in, %d frames = %.1f MB out at rate %g (checked: pipeline = spx_batch_run_rate, "
          "same counts and bytes)" % (N_LANES, n, pa.total_in * 2 / 1e6, int(cnt.sum()), int(cnt.sum()) * 2 / 1e6, PLAYBACK))
    pa.close()

    routes = [("(a) rate pipeline, rate %g, pinned host to pinned host" % PLAYBACK, "rate"),
              ("(b) spx_batch_run_rate call by call: own copy in, pack, two copies out, two waits", None),
              ("(c) rate pipeline, batches of ones", "ones"),
              ("(d) ordinary pipeline, same table", "plain")]
    times = {name: [] for name, _ in routes}
    for _ in range(WINDOWS):
        for name, kind in routes:
            if kind is None:
                window(call_by_call, lambda t: None, 1, WARM)
                times[name].append(window(call_by_call, lambda t: None, 1, BATCHES))
                continue
            pipe, submit, wait = pipe_route(kind)
            window(submit, wait, DEPTH, WARM)
            times[name].append(window(submit, wait, DEPTH, BATCHES))
            pipe.close()
    for name, _ in routes:
        t = times[name]
        print("%-90s ms per batch, %d windows of %d: %s  median %.4f" % (name + ":", WINDOWS, BATCHES, " ".join("%.4f" % v for v in t), statistics.median(t)))

    # ---- the kernel split of one rate batch: the library's timing hooks on the batch call ----
    for _ in range(3):
        rb.run()
    torch.cuda.synchronize()
    L.spx_set_timing(1)
    for _ in range(20):
        rb.run()
    torch.cuda.synchronize()
    a, w, k = C.c_double(), C.c_double(), C.c_int()
    L.spx_timing_collect(C.byref(a), C.byref(w), C.byref(k))
    L.spx_set_timing(0)
    print("kernel split of a rate batch (timing hooks, %d spx_batch_run_rate calls, ms per call): analysis %.4f  tension %.4f  general walk %.4f  rate %.4f"
          % (k.value, a.value / k.value, L.spx_timing_last_tension_ms() / k.value, w.value / k.value, L.spx_timing_last_rate_ms() / k.value))
    plan.close()


if __name__ == "__main__":
    print("library: %s  GPU_MAX_HW_QUEUES=%s" % (os.environ.get("SPEEDY_HIP_LIB") or "speedy_amd/lib/libspeedy_hip.so", os.environ["GPU_MAX_HW_QUEUES"]))
    main("--trace" in sys.argv[1:])
