"""Times behind profiles/edit_list.txt: 256 streams x 10 s, 16 kHz mono, 3.5x nonlinear (bench.py's own inputs).

  python tools/edit_list_time.py run     spx_batch_run, ms per call (HIP events on the stream) -- one line; SPEEDY_HIP_LIB selects
                                         the build
  python tools/edit_list_time.py map     spx_batch_run_map, the same way
  python tools/edit_list_time.py ab parent parent2
                                         `run` and `map` in a fresh process per build, two rounds interleaved: shipped, then
                                         speedy_amd/lib/ab/libspeedy_hip_<NAME>.so for every NAME (tools/build_variant.sh's place)
  python tools/edit_list_time.py edits   this build, one process: spx_batch_run, spx_batch_run_map and spx_batch_run_edits in two
                                         interleaved rounds, the outputs compared byte for byte; the edits call's kernels one by one;
                                         spx_edit_replay on a mono and on a 3-channel track beside a device-to-device copy of the
                                         bytes it writes (as many read, as many written), and the fraction of the copy's rate"""
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
    print("%s: ms min %.3f median %.3f max %.3f" % (what, min(t), statistics.median(t), max(t)), flush=True)


def one(xs, time_map):
    from speedy_amd.batch import Batch, Plan
    plan = Plan(RATE_HZ, False)
    p = Batch(plan, [SECONDS * RATE_HZ] * len(xs), 1, SPEED, NL, 0.0, time_map=time_map)
    p.upload(xs)
    line("spx_batch_run_map" if time_map else "spx_batch_run", timed(p.run))
    plan.close()


def ab(names):
    for r in (1, 2):
        for mode in ("run", "map"):
            for v in ["shipped"] + names:
                env = dict(os.environ)
                env.pop("SPEEDY_HIP_LIB", None)
                if v != "shipped":
                    env["SPEEDY_HIP_LIB"] = os.path.join(ROOT, "speedy_amd", "lib", "ab", "libspeedy_hip_%s.so" % v)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), mode], env=env, capture_output=True, text=True, timeout=300)
                if out.returncode != 0:
                    sys.exit("round %d, %s %s: exit %d\n%s" % (r, mode, v, out.returncode, out.stderr[-2000:]))
                print("round %d  %-8s %s" % (r, v, out.stdout.strip().splitlines()[-1]), flush=True)


def edits(xs):
    import torch
    from speedy_amd._lib import EditTrack
    from speedy_amd.batch import Batch, Plan
    plan = Plan(RATE_HZ, False)
    L = plan.L
    n = SECONDS * RATE_HZ
    args = ([n] * len(xs), 1, SPEED, NL, 0.0)
    p, m, e = Batch(plan, *args), Batch(plan, *args, time_map=True), Batch(plan, *args, edits=True)
    for b in (p, m, e):
        b.upload(xs)
    for r in (1, 2):   # interleaved: the spread between the rounds is the run-to-run spread of this process
        line("round %d  spx_batch_run (speed-up kernels)" % r, timed(p.run))
        line("round %d  spx_batch_run_map (general walk kernel)" % r, timed(m.run))
        line("round %d  spx_batch_run_edits (general walk kernel, recording)" % r, timed(e.run))
    torch.cuda.synchronize()
    same = bool((e.d_nout == p.d_nout).all()) and bool((e.d_out == p.d_out).all())
    nops, nout = e.d_nops.cpu().numpy(), e.d_nout.cpu().numpy()
    print("out and n_out of the edits call and the plain call byte-equal: %s; records per stream min %d median %d max %d of a capacity of %d "
          "(%.2f MB stored, %.1f MB reserved); frames per record %.1f" % (same, nops.min(), int(np.median(nops)), nops.max(), int(e.ops_caps[0]),
                                                                        nops.sum() * 16 / 1e6, e.ops_caps.sum() * 16 / 1e6, nout.sum() / nops.sum()))
    L.spx_set_timing(1)
    ka, kw, kt = [], [], []
    for i in range(25):
        e.run()
        a, w, c = C.c_double(0), C.c_double(0), C.c_int(0)
        assert L.spx_timing_collect(C.byref(a), C.byref(w), C.byref(c)) == 0 and c.value == 1
        if i >= 5:
            ka.append(a.value); kw.append(w.value); kt.append(L.spx_timing_last_tension_ms())
    L.spx_set_timing(0)
    print("edits call's kernels, median ms: analysis %.3f tension %.3f walk (general kernel, recording instantiation) %.3f"
          % (statistics.median(ka), statistics.median(kt), statistics.median(kw)))
    hs = torch.cuda.current_stream().cuda_stream
    for ch in (1, 3):
        tr = (EditTrack * e.n)()
        in_off = out_off = 0
        for i in range(e.n):
            tr[i].in_off, tr[i].out_off, tr[i].channels = in_off, out_off, ch
            in_off += n * ch
            out_off += int(e.out_caps[i]) * ch
        d_y = torch.randint(-32768, 32767, (in_off,), dtype=torch.int16, device=e.device)
        d_yout = torch.zeros(out_off, dtype=torch.int16, device=e.device)

        def replay():
            rc = L.spx_edit_replay(plan.h, e.jobs, e.n, e.d_ops.data_ptr(), e._ops_cap_ptr(), e.d_nops.data_ptr(), e.d_nout.data_ptr(),
                                   tr, d_y.data_ptr(), d_yout.data_ptr(), hs)
            assert rc == 0, L.spx_last_error()

        values = int(nout.sum()) * ch
        src, dst = torch.zeros(values, dtype=torch.int16, device=e.device), torch.zeros(values, dtype=torch.int16, device=e.device)
        tr_ms, cp_ms = [], []
        for r in (1, 2):
            t = timed(replay)
            line("round %d  spx_edit_replay, %d channel%s (%.1f MB written, grid %d x %d)" % (
                r, ch, "" if ch == 1 else "s", values * 2 / 1e6, L.spx_debug_last_replay_grid(None), e.n), t)
            tr_ms.append(statistics.median(t))
            t = timed(lambda: dst.copy_(src))
            line("round %d  device-to-device copy of %.1f MB (as many read)" % (r, values * 2 / 1e6), t)
            cp_ms.append(statistics.median(t))
        print("%d channel%s: replay %.1f GB/s written, copy %.1f GB/s written: %.0f %% of the copy's rate" % (
            ch, "" if ch == 1 else "s", values * 2 / min(tr_ms) / 1e6, values * 2 / min(cp_ms) / 1e6, 100.0 * min(cp_ms) / min(tr_ms)))
    # replaying the lists on the jobs' own input gives the jobs' output
    tr = (EditTrack * e.n)()
    for i in range(e.n):
        tr[i].in_off, tr[i].out_off, tr[i].channels = int(e.in_offs[i]), int(e.out_offs[i]), 1
    d_back = torch.zeros_like(e.d_out)
    assert L.spx_edit_replay(plan.h, e.jobs, e.n, e.d_ops.data_ptr(), e._ops_cap_ptr(), e.d_nops.data_ptr(), e.d_nout.data_ptr(), tr,
                             e.d_in.data_ptr(), d_back.data_ptr(), hs) == 0
    torch.cuda.synchronize()
    out, back = e.d_out.cpu().numpy(), d_back.cpu().numpy()
    print("replay on the jobs' own input equals out: %s" % all(
        np.array_equal(out[e.out_offs[i]:e.out_offs[i] + int(nout[i])], back[e.out_offs[i]:e.out_offs[i] + int(nout[i])]) for i in range(e.n)))
    plan.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode not in ("run", "map", "ab", "edits"):
        sys.exit(__doc__)
    if mode == "ab":
        ab(sys.argv[2:])
        sys.exit(0)
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    if mode == "edits":
        edits(streams())
    else:
        one(streams(), mode == "map")
