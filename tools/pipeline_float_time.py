"""Times behind profiles/pipeline_float.txt: the pipeline object on float samples (SPX_PIPELINE_FLOAT) beside the int16 pipeline
and beside what a caller with float audio had before it.  BASELINE configs[3]'s shape: 256 lanes x 10 s, 16 kHz mono, 3.5x nonlinear,
bench.py's own streams (as floats: x / 32768), depth 4.

  python tools/pipeline_float_time.py

  (a) float pipeline, pinned host memory to pinned host memory (spx_pipeline_submit_float / spx_pipeline_wait_float)
  (b) float pipeline, device input and SPX_PIPELINE_DEVICE_OUT
  (c) the int16 pipeline, host to host and resident (device input, SPX_PIPELINE_DEVICE_OUT): the yardstick, same process
  (d) what a caller has without it: spx_batch_run_float call by call -- their own host-to-device copy of the floats, the call, their
      own device-to-host copy of the output buffer (its capacity: the counts are known on the device only) and a wait per batch
  and the host-to-device copy of the float input alone: the link floor of (a).
Every figure is a host clock around a window of 100 batches behind 20 warm-up batches; the window ends with the wait for its last
tickets and a device synchronise.  Three windows per route, the routes in turns; a pipeline is created for its window and destroyed
behind it, so that no other pipeline's streams share the process's hardware queues with it (GPU_MAX_HW_QUEUES, INTEGRATION.md
"Hardware queues": the figure depends on it, and the line printed first says what the process ran with)."""
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # as bench.py

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RATE_HZ, N_LANES, SECONDS, DEPTH = 16000, 256, 10, 4
WARM, BATCHES, WINDOWS = 20, 100, 3


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


def main():
    import ctypes as C
    import bench
    import torch
    from speedy_amd.batch import FloatBatch, Pipeline, Plan
    assert torch.cuda.is_available(), "needs an MI355X"
    n = SECONDS * RATE_HZ
    xs = bench.make_streams(N_LANES, n, 0)
    plan = Plan(RATE_HZ, False)
    L = plan.L
    lens = [n] * N_LANES
    floats = [np.asarray(x, np.float32) / np.float32(32768.0) for x in xs]
    inputs = {}

    def pipe_route(float_samples, resident):
        """A pipeline of its own (alive for one window: the streams of several pipelines would share the process's hardware queues
        with one another), its input -- made once per kind -- and (submit, wait)."""
        pipe = Pipeline(plan, lens, 1, 3.5, 1.0, 0.0, depth=DEPTH, device_out=resident, float_samples=float_samples)
        if (float_samples, resident) not in inputs:
            packed = pipe.pack(floats if float_samples else xs)
            if resident:
                x = torch.zeros(pipe.total_in + (0 if float_samples else 64), dtype=torch.float32 if float_samples else torch.int16, device="cuda")
                x[: pipe.total_in].copy_(torch.from_numpy(packed))
            else:
                x = torch.from_numpy(packed).pin_memory()
            torch.cuda.synchronize()
            inputs[(float_samples, resident)] = x
        x = inputs[(float_samples, resident)]
        sub = L.spx_pipeline_submit_float if float_samples else L.spx_pipeline_submit
        wt = L.spx_pipeline_wait_float if float_samples else L.spx_pipeline_wait
        ptr, dev = x.data_ptr(), 1 if resident else 0
        o, f, c = C.c_void_p(), C.c_void_p(), C.c_void_p()

        def submit():
            t = sub(pipe.h, ptr, dev)
            assert t >= 0, L.spx_last_error()
            return t

        def wait(t):
            assert wt(pipe.h, t, C.byref(o), C.byref(f), C.byref(c)) == 0, L.spx_last_error()

        return pipe, submit, wait

    # (d) the plain float call with the caller's own copies and a wait per batch
    fb = FloatBatch(plan, lens, 1, 3.5, 1.0, 0.0)
    h_in = torch.from_numpy(np.concatenate(floats)).pin_memory()
    h_out = torch.empty(fb.d_out.numel(), dtype=torch.float32).pin_memory()
    h_cnt = torch.empty(N_LANES, dtype=torch.int64).pin_memory()
    d_in = torch.empty(fb.total_in, dtype=torch.float32, device="cuda")
    fb.set_input(d_in)

    def call_by_call():
        d_in.copy_(h_in, non_blocking=True)
        fb.run()
        h_out.copy_(fb.d_out, non_blocking=True)
        h_cnt.copy_(fb.d_nout, non_blocking=True)
        torch.cuda.synchronize()
        return 0

    routes = [("(a) float pipeline, pinned host to pinned host", (True, False)),
              ("(b) float pipeline, device in, device out", (True, True)),
              ("(c) int16 pipeline, pinned host to pinned host", (False, False)),
              ("(c) int16 pipeline, device in, device out", (False, True)),
              ("(d) spx_batch_run_float call by call, own copies (in %.0f MB, out %.0f MB: the capacity) and a wait"
               % (h_in.numel() * 4 / 1e6, h_out.numel() * 4 / 1e6), None)]

    # ---- results first: the float pipeline's output is the int16 pipeline's / 32767 and the plain float call's ----
    fa, sub_f, _ = pipe_route(True, False)
    ia, sub_i, _ = pipe_route(False, False)
    tf, ti = sub_f(), sub_i()
    of, offs_f, cnt_f = fa.wait(tf)
    oi, offs_i, cnt_i = ia.wait(ti)
    assert np.array_equal(offs_f, offs_i) and np.array_equal(cnt_f, cnt_i) and (cnt_f > 0).all()
    total = int(offs_f[N_LANES])
    want = oi[:total].astype(np.float32) / np.float32(32767)
    for i in range(N_LANES):
        lo, k = int(offs_f[i]), int(cnt_f[i])
        assert np.array_equal(of[lo:lo + k].view(np.uint32), want[lo:lo + k].view(np.uint32)), "lane %d" % i
    call_by_call()
    assert np.array_equal(h_cnt.numpy(), cnt_f)
    for i in (0, N_LANES // 2, N_LANES - 1):
        lo, k = int(offs_f[i]), int(cnt_f[i])
        assert np.array_equal(of[lo:lo + k].view(np.uint32), h_out.numpy()[fb.out_offs[i]:fb.out_offs[i] + k].view(np.uint32)), "lane %d" % i
    print("batch: %d lanes x %d frames = %d input values (%.1f MB as float, %.1f MB as int16), %d output values "
          "(checked: float pipeline = int16 pipeline / 32767 = spx_batch_run_float, same offsets and counts)"
          % (N_LANES, n, fa.total_in, fa.total_in * 4 / 1e6, fa.total_in * 2 / 1e6, int(cnt_f.sum())))
    fa.close()
    ia.close()

    # ---- the windows: the routes in turns, each behind its own warm-up ----
    times = {name: [] for name, _ in routes}
    for _ in range(WINDOWS):
        for name, kind in routes:
            if kind is None:
                window(call_by_call, lambda t: None, 1, WARM)
                times[name].append(window(call_by_call, lambda t: None, 1, BATCHES))
                continue
            pipe, submit, wait = pipe_route(*kind)
            window(submit, wait, DEPTH, WARM)
            times[name].append(window(submit, wait, DEPTH, BATCHES))
            pipe.close()
    for name, _ in routes:
        t = times[name]
        print("%-110s ms per batch, %d windows of %d: %s  median %.4f" % (name + ":", WINDOWS, BATCHES, " ".join("%.4f" % v for v in t), statistics.median(t)))

    # ---- the link floor: the float input's host-to-device copy alone ----
    marks = []
    for k in range(WARM + 40):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        d_in.copy_(h_in, non_blocking=True)
        b.record()
        marks.append((a, b))
    torch.cuda.synchronize()
    tc = [a.elapsed_time(b) for a, b in marks[WARM:]]
    print("host-to-device copy of the float input alone (%.1f MB pinned, HIP events, 40 copies): min %.4f median %.4f max %.4f ms -> %.1f GB/s"
          % (h_in.numel() * 4 / 1e6, min(tc), statistics.median(tc), max(tc), h_in.numel() * 4 / statistics.median(tc) / 1e6))
    plan.close()


if __name__ == "__main__":
    print("library: %s  GPU_MAX_HW_QUEUES=%s" % (os.environ.get("SPEEDY_HIP_LIB") or "speedy_amd/lib/libspeedy_hip.so", os.environ["GPU_MAX_HW_QUEUES"]))
    main()
