"""Times behind profiles/edit_rows.txt: 256 streams x 10 s, 16 kHz mono (bench.py's own inputs), 3.5x nonlinear and 0.5x linear,
row tracks at hop 160 (100 Hz): int32 labels (dim 1), float32 features of dim 80 and dim 768.

  python tools/edit_rows_time.py

One process per speed setting would double the set-up; both run here, one after the other.  spx_batch_run_edits once, spx_edit_index
once, then, by HIP events on the stream around each call, two rounds interleaved over
  fused    spx_edit_warp_rows NEAREST, spx_edit_warp_rows BLEND (float rows), spx_edit_unwarp_rows
  by hand  what a caller has without them: spx_edit_lookup on the rows' anchor frames (j * 160 + 80, made beforehand), a torch
           integer divide by the hop plus the stream's first row, a clamp, and index_select over the packed track.  It writes no
           rows of zeros and blends nothing: every shortcut is in its favour.
Bytes: the rows written, read once and written once (a blended row reads two rows; not counted).  The share is of 8.0 TB/s, the
HBM3E peak; about 6.3 TB/s is what a plain copy reaches."""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RATE_HZ, N_STREAMS, SECONDS, HOP, PHASE = 16000, 256, 10, 160, 80
PEAK = 8.0e12


def timed(fn, reps=30, warm=5):
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


def line(what, t, nbytes):
    med = statistics.median(t)
    print("%-66s ms min %.4f median %.4f max %.4f   %7.1f MB  %6.0f GB/s  %4.1f %% of 8 TB/s"
          % (what, min(t), med, max(t), nbytes / 1e6, nbytes / med / 1e6, 100.0 * nbytes / (med * 1e-3) / PEAK), flush=True)


def setting(xs, speed, nl):
    import torch
    from speedy_amd._lib import EditRowsTrack
    from speedy_amd.batch import Batch, Plan
    plan = Plan(RATE_HZ, False)
    L = plan.L
    n_in = SECONDS * RATE_HZ
    e = Batch(plan, [n_in] * len(xs), 1, speed, nl, 0.0, edits=True)
    e.upload(xs)
    e.run()
    torch.cuda.synchronize()
    nout, nops = e.d_nout.cpu().numpy(), e.d_nops.cpu().numpy()
    assert (nout > 0).all() and (nops > 0).all()
    print("==== speed %.1f nonlinear %.0f: records per stream median %d, output frames per stream median %d"
          % (speed, nl, int(np.median(nops)), int(np.median(nout))), flush=True)
    hs = torch.cuda.current_stream().cuda_stream
    dev = e.device
    d_index = torch.zeros(e.op_offs[-1], dtype=torch.int32, device=dev)
    assert L.spx_edit_index(plan.h, e.jobs, e.n, e.d_ops.data_ptr(), e._ops_cap_ptr(), e.d_nops.data_ptr(), d_index.data_ptr(), hs) == 0
    limit = n_in // plan.B * plan.B if nl else n_in
    rows_in = -(-n_in // HOP)                                  # rows of a track on the input's timeline
    rows_out = [L.spx_edit_rows(int(v), HOP, PHASE) for v in nout]
    rows_back = L.spx_edit_rows(limit, HOP, PHASE)
    cap_out = max(L.spx_edit_rows(int(c), HOP, PHASE) for c in e.out_caps)
    calls = []
    for name, dtype, dim in (("int32 dim 1", torch.int32, 1), ("float32 dim 80", torch.float32, 80), ("float32 dim 768", torch.float32, 768)):
        for unwarp in (False, True):
            src_rows = cap_out if unwarp else rows_in           # per stream, packed
            dst_rows = rows_back if unwarp else cap_out
            count = [rows_back] * e.n if unwarp else rows_out
            y = (torch.randn(e.n * src_rows, dim, device=dev) * 100).to(dtype)
            out = torch.zeros(e.n * dst_rows, dim, dtype=dtype, device=dev)
            d_count = torch.zeros(e.n, dtype=torch.int64, device=dev)
            tr = (EditRowsTrack * e.n)()
            for i in range(e.n):
                tr[i].in_off, tr[i].out_off, tr[i].n_rows, tr[i].out_cap = i * src_rows * dim, i * dst_rows * dim, src_rows, dst_rows
            nbytes = 2 * sum(count) * dim * 4
            # by hand: the anchors (made beforehand), one lookup, divide, clamp, gather
            offs = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
            q = torch.from_numpy(np.concatenate([np.arange(c, dtype=np.int64) * HOP + PHASE for c in count])).to(dev)
            first = torch.from_numpy(np.repeat(np.arange(e.n, dtype=np.int64) * src_rows, count)).to(dev)
            d_off = torch.from_numpy(offs).to(dev)
            r = torch.zeros_like(q)
            last = e.n * src_rows - 1

            def hand(q=q, r=r, d_off=d_off, first=first, y=y, unwarp=unwarp, last=last):
                assert L.spx_edit_lookup(plan.h, e.jobs, e.n, e.d_ops.data_ptr(), e._ops_cap_ptr(), e.d_nops.data_ptr(), e.d_nout.data_ptr(),
                                         d_index.data_ptr(), d_off.data_ptr(), q.data_ptr(), r.data_ptr(), None, 0 if unwarp else 1, hs) == 0
                idx = (torch.div(r, HOP, rounding_mode="floor") + first).clamp_(0, last)
                return y.index_select(0, idx)

            modes = [0] if unwarp or dtype != torch.float32 else [0, 1]
            for mode in modes:
                def fused(tr=tr, y=y, out=out, d_count=d_count, dim=dim, unwarp=unwarp, mode=mode):
                    if unwarp:
                        rc = L.spx_edit_unwarp_rows(plan.h, e.jobs, e.n, e.d_ops.data_ptr(), e._ops_cap_ptr(), e.d_nops.data_ptr(),
                                                    e.d_nout.data_ptr(), d_index.data_ptr(), tr, HOP, PHASE, dim, dim, dim, 4, y.data_ptr(),
                                                    out.data_ptr(), d_count.data_ptr(), hs)
                    else:
                        rc = L.spx_edit_warp_rows(plan.h, e.jobs, e.n, e.d_ops.data_ptr(), e._ops_cap_ptr(), e.d_nops.data_ptr(),
                                                  e.d_nout.data_ptr(), tr, HOP, PHASE, dim, dim, dim, 4, mode, y.data_ptr(), out.data_ptr(),
                                                  d_count.data_ptr(), hs)
                    assert rc == 0, L.spx_last_error()

                fused()
                torch.cuda.synchronize()
                assert d_count.cpu().numpy().tolist() == list(count)
                what = "%-16s %s" % (name, "unwarp" if unwarp else ("warp BLEND" if mode else "warp NEAREST"))
                calls.append(("fused    " + what + " (grid %d)" % L.spx_debug_last_rows_grid(None), fused, nbytes))
            calls.append(("by hand  %-16s %s" % (name, "unwarp" if unwarp else "warp NEAREST"), hand, nbytes))
    for rnd in (1, 2):   # interleaved: the spread between the rounds is the run-to-run spread of this process
        for what, fn, nbytes in calls:
            line("round %d  %s" % (rnd, what), timed(fn), nbytes)
    plan.close()


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    import bench
    xs = bench.make_streams(N_STREAMS, SECONDS * RATE_HZ, 0)
    setting(xs, 3.5, 1.0)
    setting(xs, 0.5, 0.0)
