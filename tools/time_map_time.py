"""Times behind profiles/time_map.txt: 256 streams x 10 s, 16 kHz mono, 3.5x nonlinear (BASELINE configs[3]'s shape, bench.py's own
inputs).

  python tools/time_map_time.py run      spx_batch_run, ms per call (HIP events on the stream) -- one line; SPEEDY_HIP_LIB selects
                                         the build, so a script can interleave builds (this one, the parent commit's, the parent
                                         commit's again for the spread): python tools/time_map_time.py ab NAME ...
  python tools/time_map_time.py ab parent parent2
                                         `run` in a fresh process per build, two rounds interleaved: shipped, then
                                         speedy_amd/lib/ab/libspeedy_hip_<NAME>.so for every NAME (tools/build_variant.sh's place)
  python tools/time_map_time.py map      this build: spx_batch_run_map on the same table (and spx_batch_run beside it, same
                                         process), its kernels one by one, and spx_map_lookup for 256 x 1000 queries, both
                                         directions; the outputs of the two calls are compared byte for byte

Times behind profiles/time_map_rate.txt: the same table, every playback rate 1.25.
  python tools/time_map_time.py rate     spx_batch_run_rate, ms per call -- one line; SPEEDY_HIP_LIB selects the build
  python tools/time_map_time.py ab-rate parent parent2
                                         `rate` in a fresh process per build, two rounds interleaved, as `ab` does for `run`
  python tools/time_map_time.py ratemap  this build: spx_batch_run_rate and spx_batch_run_rate_map in one process, the outputs
                                         compared byte for byte, and the map call's kernels one by one -- the rows conversion
                                         kernel (spx_timing_last_map_rows_ms) alone among them"""
import ctypes as C
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RATE_HZ, SPEED, NL, N_STREAMS, SECONDS = 16000, 3.5, 1.0, 256, 10


def streams():
    import bench
    return bench.make_streams(N_STREAMS, SECONDS * RATE_HZ, 0)


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
    print("%s: ms min %.3f median %.3f max %.3f" % (what, min(t), statistics.median(t), max(t)))


def run(xs):
    from speedy_amd.batch import Batch, Plan
    plan = Plan(RATE_HZ, False)
    n = SECONDS * RATE_HZ
    p = Batch(plan, [n] * len(xs), 1, SPEED, NL, 0.0)
    p.upload(xs)
    line("spx_batch_run, 30 calls back to back after 5", timed(p.run))
    plan.close()


RATE = 1.25


def run_rate(xs):
    from speedy_amd.batch import Batch, Plan
    plan = Plan(RATE_HZ, False)
    n = SECONDS * RATE_HZ
    p = Batch(plan, [n] * len(xs), 1, SPEED, NL, 0.0, rate=RATE)
    p.upload(xs)
    line("spx_batch_run_rate at %g, 30 calls back to back after 5" % RATE, timed(p.run))
    plan.close()


def with_rate_map(xs):
    import torch
    from speedy_amd.batch import Batch, Plan
    plan = Plan(RATE_HZ, False)
    L = plan.L
    n = SECONDS * RATE_HZ
    p = Batch(plan, [n] * len(xs), 1, SPEED, NL, 0.0, rate=RATE)
    p.upload(xs)
    m = Batch(plan, [n] * len(xs), 1, SPEED, NL, 0.0, rate=RATE, time_map=True)
    m.upload(xs)
    for r in (1, 2):   # interleaved: the spread between the rounds is the run-to-run spread of this process
        line("round %d  spx_batch_run_rate at %g" % (r, RATE), timed(p.run))
        line("round %d  spx_batch_run_rate_map at %g" % (r, RATE), timed(m.run))
    torch.cuda.synchronize()
    same = bool((m.d_nout == p.d_nout).all()) and bool((m.d_out == p.d_out).all())
    rows = m.d_map.cpu().numpy()
    print("out and n_out of the two calls byte-equal: %s; map rows %d (%.2f MB); last rows equal n_out: %s"
          % (same, rows.size, rows.size * 8 / 1e6, bool((rows[np.asarray(m.map_offs[1:]) - 1] == m.d_nout.cpu().numpy()).all())))
    L.spx_set_timing(1)
    ka, kw, kt, kr, km = [], [], [], [], []
    for i in range(25):
        m.run()
        a, w, c = C.c_double(0), C.c_double(0), C.c_int(0)
        assert L.spx_timing_collect(C.byref(a), C.byref(w), C.byref(c)) == 0 and c.value == 1
        if i >= 5:
            ka.append(a.value); kw.append(w.value); kt.append(L.spx_timing_last_tension_ms())
            kr.append(L.spx_timing_last_rate_ms()); km.append(L.spx_timing_last_map_rows_ms())
    L.spx_set_timing(0)
    print("rate map call's kernels, median ms: analysis %.3f tension %.3f walk (general kernel, map instantiation) %.3f rate %.3f"
          % (statistics.median(ka), statistics.median(kt), statistics.median(kw), statistics.median(kr)))
    line("rows conversion kernel alone (HIP events around its launch, %d rows)" % rows.size, km)
    plan.close()


def ab(names, mode="run"):
    for r in (1, 2):
        for v in ["shipped"] + names:
            env = dict(os.environ)
            env.pop("SPEEDY_HIP_LIB", None)
            if v != "shipped":
                env["SPEEDY_HIP_LIB"] = os.path.join(ROOT, "speedy_amd", "lib", "ab", "libspeedy_hip_%s.so" % v)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), mode], env=env, capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                sys.exit("round %d, %s: exit %d\n%s" % (r, v, out.returncode, out.stderr[-2000:]))
            print("round %d  %-8s %s" % (r, v, out.stdout.strip().splitlines()[-1]), flush=True)


def with_map(xs):
    import torch
    from speedy_amd.batch import Batch, Plan
    plan = Plan(RATE_HZ, False)
    L = plan.L
    n = SECONDS * RATE_HZ
    p = Batch(plan, [n] * len(xs), 1, SPEED, NL, 0.0)
    p.upload(xs)
    line("spx_batch_run (speed-up kernels)", timed(p.run))
    m = Batch(plan, [n] * len(xs), 1, SPEED, NL, 0.0, time_map=True)
    m.upload(xs)
    line("spx_batch_run_map (general walk kernel, kernels in sequence)", timed(m.run))
    torch.cuda.synchronize()
    same = bool((m.d_nout == p.d_nout).all()) and bool((m.d_out == p.d_out).all())
    print("out and n_out of the two calls byte-equal: %s; map rows %d (%.2f MB)" % (same, m.d_map.numel(), m.d_map.numel() * 8 / 1e6))
    L.spx_set_timing(1)
    ka, kw, kt = [], [], []
    for i in range(25):
        m.run()
        a, w, c = C.c_double(0), C.c_double(0), C.c_int(0)
        assert L.spx_timing_collect(C.byref(a), C.byref(w), C.byref(c)) == 0 and c.value == 1
        if i >= 5:
            ka.append(a.value); kw.append(w.value); kt.append(L.spx_timing_last_tension_ms())
    L.spx_set_timing(0)
    print("map call's kernels, median ms: analysis %.3f tension %.3f walk (general kernel, map instantiation) %.3f"
          % (statistics.median(ka), statistics.median(kt), statistics.median(kw)))
    # 256 x 1000 queries, spread over each stream's domain
    nq = 1000
    hs = torch.cuda.current_stream().cuda_stream
    nout = m.d_nout.cpu().numpy()
    d_off = torch.arange(0, (len(xs) + 1) * nq, nq, dtype=torch.int64, device=m.device)
    d_r = torch.zeros(len(xs) * nq, dtype=torch.int64, device=m.device)
    for inverse, top in ((0, np.full(len(xs), n)), (1, nout)):
        q = np.concatenate([np.linspace(0, int(t), nq).astype(np.int64) for t in top])
        d_q = torch.from_numpy(q).to(m.device)

        def look():
            rc = L.spx_map_lookup(plan.h, m.jobs, m.n, m.d_map.data_ptr(), d_off.data_ptr(), d_q.data_ptr(), d_r.data_ptr(), inverse, hs)
            assert rc == 0, L.spx_last_error()

        line("spx_map_lookup %s, 256 x 1000 queries" % ("inverse" if inverse else "forward"), timed(look))
    plan.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode not in ("run", "ab", "map", "rate", "ab-rate", "ratemap"):
        sys.exit(__doc__)
    if mode in ("ab", "ab-rate"):
        ab(sys.argv[2:], "run" if mode == "ab" else "rate")
        sys.exit(0)
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    {"run": run, "map": with_map, "rate": run_rate, "ratemap": with_rate_map}[mode](streams())
