"""Times spx_batch_dtw on the GPU box -> the figures of profiles/dtw.txt.
  python tools/dtw_time.py [--pairs 256] [--rows-a 1000] [--rows-b 286] [--dim 120] [--calls 10] [--warmup 3]
      the library's own timing events (spx_set_timing, spx_timing_last_dtw_ms / _tail_ms) per call: forward kernel, tail, both;
      cells per second.  SPEEDY_HIP_LIB selects another build (a -DSPX_DTW_PHASES=1 / =2 variant: the forward kernel's phases alone).
  python tools/dtw_time.py --host 1 [...]
      the definition (tests/dtw_ref.py, scalar local costs) on the first N of the same pairs on the host, for scale."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_rows(n, rows, dim, seed):
    """Spectrogram-like rows: non-negative, a few thousand in size, float32."""
    rng = np.random.default_rng(seed)
    return np.abs(rng.standard_normal((n * rows, dim)) * 1000.0).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--rows-a", type=int, default=1000)
    ap.add_argument("--rows-b", type=int, default=286)
    ap.add_argument("--dim", type=int, default=120)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host", type=int, default=0)
    a = ap.parse_args()
    A = make_rows(a.pairs, a.rows_a, a.dim, 1)
    B = make_rows(a.pairs, a.rows_b, a.dim, 2)
    cells = a.pairs * a.rows_a * a.rows_b
    if a.host:
        import dtw_ref
        t0 = time.perf_counter()
        for i in range(a.host):
            r = dtw_ref.dtw(A[i * a.rows_a:(i + 1) * a.rows_a], B[i * a.rows_b:(i + 1) * a.rows_b], 10)
        dt = time.perf_counter() - t0
        print("host definition: %d pair(s) of %d x %d, dim %d: %.1f s (%.1f us per cell); last cost %r n_path %d"
              % (a.host, a.rows_a, a.rows_b, a.dim, dt, 1e6 * dt / (a.host * a.rows_a * a.rows_b), float(r["cost"]), r["n_path"]))
        return
    import torch
    from speedy_amd import DtwBatch
    from speedy_amd.batch import Plan
    plan = Plan(16000)
    L = plan.L
    d = DtwBatch(plan, [a.rows_a] * a.pairs, [a.rows_b] * a.pairs, a.dim)
    d_a, d_b = torch.from_numpy(A.ravel()).cuda(), torch.from_numpy(B.ravel()).cuda()
    for _ in range(a.warmup):
        d.run(d_a, d_b)
    torch.cuda.synchronize()
    L.spx_set_timing(1)
    both, tail = [], []
    for _ in range(a.calls):
        d.run(d_a, d_b)
        torch.cuda.synchronize()
        L.spx_timing_collect(None, None, None)
        both.append(L.spx_timing_last_dtw_ms())
        tail.append(L.spx_timing_last_dtw_tail_ms())
    L.spx_set_timing(0)
    both, tail = np.array(both), np.array(tail)
    fwd = both - tail
    res = d.results()
    print("lib %s" % (os.environ.get("SPEEDY_HIP_LIB") or "speedy_amd/lib/libspeedy_hip.so"))
    print("%d pairs of %d x %d rows, dim %d: %d cells; workspace %.1f MB; grid %r" % (a.pairs, a.rows_a, a.rows_b, a.dim, cells,
                                                                                     d.d_ws.numel() / 1e6, d.grid()))
    for name, v in (("forward", fwd), ("tail", tail), ("both", both)):
        print("  %-8s min %.3f  median %.3f  max %.3f ms" % (name, v.min(), np.median(v), v.max()))
    print("  %.1f G cells/s, %.2f T (subtract, multiply, add) per second in the local costs"
          % (cells / np.median(both) / 1e6, 3 * cells * a.dim / np.median(fwd) / 1e9))
    print("  n_path min %d max %d; cost[0] %r" % (res["n_path"].min(), res["n_path"].max(), float(res["cost"][0])))


if __name__ == "__main__":
    main()
