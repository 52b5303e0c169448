"""Times behind profiles/twopass.txt: 256 streams x 10 s, 16 kHz mono, every stream to 10 / 3.5 s (LENGTH mode at 3.5x), nonlinear,
bench.py's own inputs, input resident in device memory.

  python tools/twopass_bench.py [--out profiles/twopass.txt] [--rounds 3] [--reps 30]

Three things, alternating, `rounds` times, each `reps` times back to back after 5 (HIP events on the stream around every repetition):
  (a) spx_batch_run_twopass: both passes and the speed between them in one call;
  (b) the loop a caller writes without it, on the same build: spx_batch_run of the probe table, the counts to the host (a
      synchronising device-to-host copy), the formula on the host, spx_batch_run of the final table;
  (c) one spx_batch_run at 3.5x, for scale.
Then the library's own per-kernel events (spx_set_timing) for each of the three, summed over the calls one repetition makes, and a
byte comparison of (a)'s and (b)'s outputs."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RATE_HZ, FACTOR, N_STREAMS, SECONDS = 16000, 3.5, 256, 10


def timed(fn, reps, warm=5):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    for a, z in ev:
        a.record()
        fn()
        z.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(z) for a, z in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "twopass.txt"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    import bench
    from speedy_amd.batch import Batch, Plan, TwoPassBatch
    n = SECONDS * RATE_HZ
    xs = bench.make_streams(N_STREAMS, n, 0)
    plan = Plan(RATE_HZ, False)
    L = plan.L
    target = SECONDS / FACTOR
    want = np.float64(np.float32(n) / np.float32(RATE_HZ)) / np.float64(target)

    tp = TwoPassBatch(plan, [n] * N_STREAMS, 1, 1.0, 1.0, 0.0, seconds=target)
    tp.upload(xs)
    probe = Batch(plan, [n] * N_STREAMS, 1, np.float32(want), 1.0, 0.0)
    probe.upload(xs)
    final = Batch(plan, [n] * N_STREAMS, 1, np.float32(want), 1.0, 0.0)
    final.d_in = probe.d_in
    plain = Batch(plan, [n] * N_STREAMS, 1, FACTOR, 1.0, 0.0)
    plain.d_in = probe.d_in

    def loop():
        probe.run()
        n_probe = probe.d_nout.cpu().numpy()   # waits for the probe pass: the GPU is idle from here ...
        got = np.float64(n) / n_probe.astype(np.float64)
        speeds = (want * (want / got)).astype(np.float32)
        for i in range(N_STREAMS):
            final.jobs[i].speed = float(speeds[i])
        final.run()                            # ... to here

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("Two passes in one call (spx_batch_run_twopass) against the loop a caller writes today")
    say("=====================================================================================")
    say("%d streams x %d s, %d Hz mono, LENGTH mode to %.4f s (want %.6f), nonlinear 1, feedback 0; bench.make_streams(%d, %d, 0)."
        % (N_STREAMS, SECONDS, RATE_HZ, target, want, N_STREAMS, n))
    say("HIP events on the stream around every repetition, %d repetitions back to back after 5, %d rounds alternating; ms." % (args.reps, args.rounds))
    say("GPU_MAX_HW_QUEUES=%s" % os.environ.get("GPU_MAX_HW_QUEUES", "(library default)"))
    say()
    what = [("(a) spx_batch_run_twopass", tp.run), ("(b) run, counts to host, formula, run", loop), ("(c) one spx_batch_run at 3.5x", plain.run)]
    for r in range(args.rounds):
        for name, fn in what:
            t = timed(fn, args.reps)
            say("round %d  %-40s min %.3f  median %.3f  max %.3f" % (r + 1, name, min(t), statistics.median(t), max(t)))
    say("(a) reused the first pass's analysis: %s; walk form of its second pass %d" % (bool(L.spx_debug_last_twopass() & 1), L.spx_debug_last_walk_form()))
    say()
    # (a) and (b) computed the same thing
    tp.run()
    loop()
    torch.cuda.synchronize()
    same = bool((tp.d_nout == final.d_nout).all()) and bool((tp.d_probe == probe.d_nout).all())
    nout = tp.d_nout.cpu().numpy()
    a_out, b_out = tp.d_out.cpu().numpy(), final.d_out.cpu().numpy()
    for i in range(N_STREAMS):
        same = same and np.array_equal(a_out[tp.out_offs[i]:tp.out_offs[i] + nout[i]], b_out[final.out_offs[i]:final.out_offs[i] + nout[i]])
    n_probe = tp.d_probe.cpu().numpy()
    say("(a) and (b): counts, probe counts and produced frames byte-equal: %s" % same)
    say("lengths: target %d frames; probe pass mean %.0f (off by %.0f on average), final pass mean %.0f (off by %.0f on average)"
        % (round(target * RATE_HZ), n_probe.mean(), np.abs(n_probe - target * RATE_HZ).mean(), nout.mean(), np.abs(nout - target * RATE_HZ).mean()))
    say()
    say("The library's own events per kernel (spx_set_timing), summed over the calls of one repetition, medians of 20 after 5; ms:")
    L.spx_set_timing(1)
    for name, fn in what:
        ka, kw, kt, calls = [], [], [], 0
        for i in range(25):
            fn()
            a, w, c = C.c_double(0), C.c_double(0), C.c_int(0)
            assert L.spx_timing_collect(C.byref(a), C.byref(w), C.byref(c)) == 0
            calls = c.value
            if i >= 5:
                ka.append(a.value); kw.append(w.value); kt.append(L.spx_timing_last_tension_ms())
        say("  %-40s %d timed call(s): analysis %.3f  tension %.3f  walk %.3f" % (name, calls, statistics.median(ka), statistics.median(kt), statistics.median(kw)))
    L.spx_set_timing(0)
    say("(kernels of a call that runs them side by side overlap: their times do not add up to the call's)")
    plan.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
