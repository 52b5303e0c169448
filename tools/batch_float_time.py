"""Times behind profiles/batch_float.txt: 256 streams x 10 s, 16 kHz mono, 3.5x nonlinear (BASELINE configs[3]'s shape, bench.py's
own inputs), as floats in device memory.

  python tools/batch_float_time.py

  1. spx_batch_run_float and spx_batch_run on the same samples (the floats are the int16 inputs / 32768: on a nonlinear job their
     int16 images are those inputs), by turns in one process, HIP events around every call: one warm-up, one timed window.
  2. Each conversion kernel alone (spx_float_to_short over the batch's input values, spx_short_to_float over as many values as the
     batch produced): bytes read + written / time, beside a device-to-device copy that reads + writes the same number of bytes,
     by turns in the same window.
Outputs are checked: the float call's output is the int16 call's / 32767, value for value."""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RATE_HZ, SPEED, NL, N_STREAMS, SECONDS = 16000, 3.5, 1.0, 256, 10
WARM, CALLS = 5, 40


def _stats(t):
    return "min %.4f median %.4f max %.4f" % (min(t), statistics.median(t), max(t))


def main():
    import torch
    import bench
    from speedy_amd.batch import Batch, FloatBatch, Plan
    assert torch.cuda.is_available(), "needs an MI355X"
    n = SECONDS * RATE_HZ
    xs = bench.make_streams(N_STREAMS, n, 0)
    plan = Plan(RATE_HZ, False)
    L = plan.L
    hs = torch.cuda.current_stream().cuda_stream
    fb = FloatBatch(plan, [n] * len(xs), 1, SPEED, NL, 0.0)
    fb.upload([np.asarray(x, np.float32) / np.float32(32768.0) for x in xs])
    ib = Batch(plan, [n] * len(xs), 1, SPEED, NL, 0.0)
    ib.upload(xs)

    def ev():
        return torch.cuda.Event(enable_timing=True)

    # ---- 1. the two calls by turns ----
    for _ in range(WARM):
        fb.run()
        ib.run()
    torch.cuda.synchronize()
    marks = []
    for _ in range(CALLS):
        a, b, c = ev(), ev(), ev()
        a.record()
        fb.run()
        b.record()
        ib.run()
        c.record()
        marks.append((a, b, c))
    torch.cuda.synchronize()
    tf = [a.elapsed_time(b) for a, b, c in marks]
    ti = [b.elapsed_time(c) for a, b, c in marks]
    nout = ib.d_nout.cpu().numpy()
    assert (nout > 0).all() and np.array_equal(nout, fb.d_nout.cpu().numpy())
    want = ib.d_out.cpu().numpy().astype(np.float32) / np.float32(32767)
    got = fb.d_out.cpu().numpy()
    for i in range(len(xs)):
        lo, k = ib.out_offs[i], int(nout[i])
        assert np.array_equal(got[lo:lo + k].view(np.uint32), want[lo:lo + k].view(np.uint32)), "stream %d" % i
    vin, vout = fb.total_in, int(nout.sum())
    print("batch: %d streams x %d frames, %d input values, %d output values (checked: float out = int16 out / 32767)"
          % (len(xs), n, vin, vout))
    print("spx_batch_run_float, ms per call, %d calls by turns with spx_batch_run after %d warm-up: %s" % (CALLS, WARM, _stats(tf)))
    print("spx_batch_run (int16), ms per call, same window:                                        %s" % _stats(ti))
    mf, mi = statistics.median(tf), statistics.median(ti)
    print("difference of the medians: %.4f ms = %.1f %% of the int16 call" % (mf - mi, (mf - mi) / mi * 100))

    # ---- 2. the conversion kernels alone, each beside a copy of the same bytes ----
    for name, vals, rd, wr in (("spx_float_to_short (32768.0 scale)", vin, 4, 2), ("spx_float_to_short (32767.0f scale)", vin, 4, 2),
                               ("spx_short_to_float", vout, 2, 4)):
        by = vals * (rd + wr)
        src = torch.zeros(vals * rd, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(vals * wr, dtype=torch.uint8, device="cuda")
        if rd == 4:
            src.view(torch.float32).copy_(fb.d_in[:vals])
        else:
            src.view(torch.int16).copy_(torch.randint(-32768, 32768, (vals,), dtype=torch.int16, device="cuda"))
        ca = torch.zeros(by // 2, dtype=torch.uint8, device="cuda")   # the copy reads by / 2 bytes and writes by / 2
        cb = torch.zeros(by // 2, dtype=torch.uint8, device="cuda")

        def conv():
            if rd == 4:
                rc = L.spx_float_to_short(src.data_ptr(), dst.data_ptr(), vals, 1 if "32768" in name else 0, hs)
            else:
                rc = L.spx_short_to_float(src.data_ptr(), dst.data_ptr(), vals, hs)
            assert rc == 0, L.spx_last_error()

        def copy():
            cb.copy_(ca)   # (torch's device-to-device copy on the current stream)

        for _ in range(WARM):
            conv()
            copy()
        torch.cuda.synchronize()
        marks = []
        for _ in range(CALLS):
            a, b, c = ev(), ev(), ev()
            a.record()
            conv()
            b.record()
            copy()
            c.record()
            marks.append((a, b, c))
        torch.cuda.synchronize()
        tk = [a.elapsed_time(b) for a, b, c in marks]
        tc = [b.elapsed_time(c) for a, b, c in marks]
        mk, mc = statistics.median(tk), statistics.median(tc)
        print("%s: %d values, %.1f MB read + %.1f MB written = %.1f MB" % (name, vals, vals * rd / 1e6, vals * wr / 1e6, by / 1e6))
        print("  kernel ms: %s -> %.0f GB/s" % (_stats(tk), by / mk / 1e6))
        print("  device-to-device copy of %.1f MB (reads + writes the same %.1f MB), ms: %s -> %.0f GB/s" % (by / 2e6, by / 1e6, _stats(tc), by / mc / 1e6))
        print("  kernel rate / copy rate: %.2f" % (mc / mk))
        del src, dst, ca, cb
    plan.close()


if __name__ == "__main__":
    print("library: %s" % (os.environ.get("SPEEDY_HIP_LIB") or "speedy_amd/lib/libspeedy_hip.so"))
    main()
