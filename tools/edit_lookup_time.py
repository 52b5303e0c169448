"""Times behind profiles/edit_lookup.txt: 256 streams x 10 s, 16 kHz mono, 3.5x nonlinear (bench.py's own inputs).

  python tools/edit_lookup_time.py lookup   this build (SPEEDY_HIP_LIB selects another), one process: spx_batch_run_edits and
                                            spx_batch_run_map once each on the same table, then, by HIP events on the stream, two
                                            rounds interleaved: spx_edit_index; spx_edit_lookup and spx_map_lookup with 1 000 and
                                            with 100 000 queries per stream, forward and inverse (uniform random positions over the
                                            stream, the same for both calls)
  python tools/edit_lookup_time.py ab NAME [NAME ...]
                                            `lookup` in a fresh process per build, twice, alternating: shipped, then
                                            speedy_amd/lib/ab/libspeedy_hip_<NAME>.so for every NAME"""
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RATE_HZ, SPEED, NL, N_STREAMS, SECONDS = 16000, 3.5, 1.0, 256, 10


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


def line(what, t):
    print("%-78s ms min %.4f median %.4f max %.4f" % (what, min(t), statistics.median(t), max(t)), flush=True)


def lookup():
    import bench
    import torch
    from speedy_amd.batch import Batch, Plan
    xs = bench.make_streams(N_STREAMS, SECONDS * RATE_HZ, 0)
    plan = Plan(RATE_HZ, False)
    L = plan.L
    n = SECONDS * RATE_HZ
    args = ([n] * len(xs), 1, SPEED, NL, 0.0)
    m, e = Batch(plan, *args, time_map=True), Batch(plan, *args, edits=True)
    for b in (m, e):
        b.upload(xs)
        b.run()
    torch.cuda.synchronize()
    nout, nops = e.d_nout.cpu().numpy(), e.d_nops.cpu().numpy()
    assert (nout == m.d_nout.cpu().numpy()).all() and (nops > 0).all()
    print("records per stream min %d median %d max %d; output frames per stream median %d" % (nops.min(), int(np.median(nops)), nops.max(),
                                                                                           int(np.median(nout))))
    hs = torch.cuda.current_stream().cuda_stream
    d_index = torch.zeros(e.op_offs[-1], dtype=torch.int32, device=e.device)

    def index():
        assert L.spx_edit_index(plan.h, e.jobs, e.n, e.d_ops.data_ptr(), e._ops_cap_ptr(), e.d_nops.data_ptr(), d_index.data_ptr(), hs) == 0

    index()
    calls = []
    rng = np.random.default_rng(7)
    for per in (1000, 100000):
        offs = torch.from_numpy(np.arange(e.n + 1, dtype=np.int64) * per).to(e.device)
        for inverse in (0, 1):
            hi = nout if inverse else np.full(e.n, n)
            q = torch.from_numpy(np.concatenate([rng.integers(0, h + 1, per) for h in hi]).astype(np.int64)).to(e.device)
            r, r2 = torch.zeros_like(q), torch.zeros_like(q)
            rec = torch.zeros(q.numel(), dtype=torch.int32, device=e.device)

            def exact(q=q, r=r, rec=rec, offs=offs, inverse=inverse):
                assert L.spx_edit_lookup(plan.h, e.jobs, e.n, e.d_ops.data_ptr(), e._ops_cap_ptr(), e.d_nops.data_ptr(), e.d_nout.data_ptr(),
                                         d_index.data_ptr(), offs.data_ptr(), q.data_ptr(), r.data_ptr(), rec.data_ptr(), inverse, hs) == 0

            def by_map(q=q, r2=r2, offs=offs, inverse=inverse):
                assert L.spx_map_lookup(plan.h, m.jobs, m.n, m.d_map.data_ptr(), offs.data_ptr(), q.data_ptr(), r2.data_ptr(), inverse, hs) == 0

            tag = "%6d queries per stream, %s" % (per, "inverse" if inverse else "forward")
            calls += [("spx_edit_lookup  " + tag + " (grid %d x %d)", exact, L.spx_debug_last_edit_lookup_grid),
                      ("spx_map_lookup   " + tag + " (grid %d x %d)", by_map, L.spx_debug_last_lookup_grid)]
    for r in (1, 2):   # interleaved: the spread between the rounds is the run-to-run spread of this process
        line("round %d  spx_edit_index   %d records in %d streams" % (r, int(nops.sum()), e.n), timed(index))
        for what, fn, grid in calls:
            t = timed(fn)
            line("round %d  " % r + what % (grid(None), e.n), t)
    plan.close()


def ab(names):
    for v in (["shipped"] + names) * 2:          # every build twice, alternating
        env = dict(os.environ)
        env.pop("SPEEDY_HIP_LIB", None)
        if v != "shipped":
            env["SPEEDY_HIP_LIB"] = os.path.join(ROOT, "speedy_amd", "lib", "ab", "libspeedy_hip_%s.so" % v)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "lookup"], env=env, capture_output=True, text=True, timeout=300)
        if out.returncode != 0:
            sys.exit("%s: exit %d\n%s" % (v, out.returncode, out.stderr[-2000:]))
        print("---- %s\n%s" % (v, out.stdout.strip()), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode not in ("lookup", "ab"):
        sys.exit(__doc__)
    if mode == "ab":
        ab(sys.argv[2:])
        sys.exit(0)
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    lookup()
