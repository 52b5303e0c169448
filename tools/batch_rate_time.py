"""Times behind profiles/batch_rate.txt: 256 streams x 10 s, 16 kHz mono, 3.5x nonlinear (BASELINE configs[3]'s shape, bench.py's
own inputs) at playback rate 1.25.

  python tools/batch_rate_time.py handles   the route a library without spx_batch_run_rate has: 256 handles of the streaming API,
                                            set_rate, write all / flush all / read all on one thread, coalescing on and off
                                            (SPEEDY_HIP_LIB selects the build: the parent commit's for the record)
  python tools/batch_rate_time.py batch     spx_batch_run_rate on the same streams, device-resident input: the whole call (events
                                            on the stream), the rate kernel alone (the library's timing events around it: median
                                            of the launches) and spx_batch_run without a rate (speed-up kernels) beside it
Every mode prints one line per figure; outputs are checked against each other (CRC-32 per stream) where both exist."""
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RATE_HZ, SPEED, NL, PLAYBACK, N_STREAMS, SECONDS = 16000, 3.5, 1.0, 1.25, 256, 10


def streams():
    import bench
    return bench.make_streams(N_STREAMS, SECONDS * RATE_HZ, 0)


def crc_line(outs):
    return "%08x" % zlib.crc32(b"".join(np.ascontiguousarray(o, "<i2").tobytes() for o in outs))


def handles(xs):
    import torch
    from speedy_amd.sonic2 import SonicStream
    torch.cuda.synchronize()
    for coalesce in (True, False):
        times, crc = [], None
        for rep in range(4):   # the first repetition warms up (code objects, pools, buffers)
            hs = [SonicStream(RATE_HZ, 1, False, coalesce) for _ in xs]
            for s in hs:
                s.set_speed(SPEED)
                s.set_rate(PLAYBACK)
                s.enable_nonlinear(NL)
                s.set_feedback(0.0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s, x in zip(hs, xs):
                assert s.write_short(x) == 1
            for s in hs:
                assert s.flush() == 1
            outs = []
            for s in hs:
                got = []
                while True:
                    g = s.read_short(1 << 17)
                    if g.size == 0:
                        break
                    got.append(g)
                outs.append(np.concatenate(got))
            dt = (time.perf_counter() - t0) * 1e3
            if rep:
                times.append(dt)
            crc = crc_line(outs)
            for s in hs:
                s.close()
        print("handles coalesce=%d: write all / flush all / read all, ms per batch %s -> min %.2f median %.2f  frames out %d crc %s"
              % (coalesce, ["%.2f" % t for t in times], min(times), statistics.median(times), sum(o.size for o in outs), crc))


def batch(xs):
    import torch
    from speedy_amd.batch import Batch, Plan
    plan = Plan(RATE_HZ, False)
    L = plan.L
    n = SECONDS * RATE_HZ

    def timed(b, reps=30, warm=5):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for _ in range(warm):
            b.run()
        torch.cuda.synchronize()
        for a, z in ev:
            a.record()
            b.run()
            z.record()
        torch.cuda.synchronize()
        return [a.elapsed_time(z) for a, z in ev]

    r = Batch(plan, [n] * len(xs), 1, SPEED, NL, 0.0, rate=PLAYBACK)
    r.upload(xs)
    t = timed(r)
    outs = r.results()
    nout = r.d_nout.cpu().numpy()
    print("spx_batch_run_rate (rate %.2f): ms per call, events on the stream, 30 calls back to back after 5: min %.3f median %.3f max %.3f  "
          "frames out %d crc %s" % (PLAYBACK, min(t), statistics.median(t), max(t), sum(o.size for o in outs), crc_line(outs)))
    # a host clock around one call that ends in a synchronise (what the handle route's figure is)
    ht = []
    for _ in range(10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.run()
        torch.cuda.synchronize()
        ht.append((time.perf_counter() - t0) * 1e3)
    print("spx_batch_run_rate: host clock around call + synchronise, ms: min %.3f median %.3f" % (min(ht), statistics.median(ht)))
    # the kernels of the call one by one: the library's events around each launch
    L.spx_set_timing(1)
    ka, kw, kt, kr = [], [], [], []
    import ctypes as C
    for i in range(25):
        r.run()
        a, w, c = C.c_double(0), C.c_double(0), C.c_int(0)
        assert L.spx_timing_collect(C.byref(a), C.byref(w), C.byref(c)) == 0 and c.value == 1
        if i >= 5:
            ka.append(a.value); kw.append(w.value); kt.append(L.spx_timing_last_tension_ms()); kr.append(L.spx_timing_last_rate_ms())
    L.spx_set_timing(0)
    fin = int(nout.sum())
    # bytes the rate kernel needs: every TSM frame it resamples read once, every final frame written once (int16 mono);
    # final = ceil((tsm - 1) * new / old) with old / new = 16000 / 12800: the TSM frames are final * 1.25 + 1
    tsm_frames = int(sum(int(k) * 16000 // 12800 + 1 for k in nout))
    by = 2 * (tsm_frames + fin)
    med = statistics.median(kr)
    print("rate kernel alone (20 launches after 5): ms min %.4f median %.4f max %.4f; about %d bytes read + %d written = %.1f MB -> %.0f GB/s, "
          "%.1f %% of 8 TB/s" % (min(kr), med, max(kr), 2 * tsm_frames, 2 * fin, by / 1e6, by / med / 1e6, by / med / 1e6 / 8000 * 100))
    print("rate call's kernels, median ms: analysis %.3f tension %.3f walk (general kernel) %.3f rate %.4f"
          % (statistics.median(ka), statistics.median(kt), statistics.median(kw), med))
    p = Batch(plan, [n] * len(xs), 1, SPEED, NL, 0.0)
    p.upload(xs)
    t = timed(p)
    print("spx_batch_run, no rate (speed-up kernels): ms per call: min %.3f median %.3f max %.3f" % (min(t), statistics.median(t), max(t)))
    L.spx_set_timing(1)
    ka, kw, kt = [], [], []
    for i in range(25):
        p.run()
        a, w, c = C.c_double(0), C.c_double(0), C.c_int(0)
        assert L.spx_timing_collect(C.byref(a), C.byref(w), C.byref(c)) == 0
        if i >= 5:
            ka.append(a.value); kw.append(w.value); kt.append(L.spx_timing_last_tension_ms())
    L.spx_set_timing(0)
    print("spx_batch_run's kernels, median ms: analysis %.3f tension %.3f walk (speed-up kernel) %.3f"
          % (statistics.median(ka), statistics.median(kt), statistics.median(kw)))
    plan.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode not in ("handles", "batch"):
        sys.exit(__doc__)
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    print("library: %s" % (os.environ.get("SPEEDY_HIP_LIB") or "speedy_amd/lib/libspeedy_hip.so"))
    (handles if mode == "handles" else batch)(streams())
