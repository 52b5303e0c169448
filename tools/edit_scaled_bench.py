"""Times behind profiles/edit_scaled.txt: deciding at 16 kHz, rendering the master (spx_edit_replay_scaled).

Workload: 256 streams x 10 s, 16 kHz mono, 3.5x nonlinear (bench.py's own inputs), the edit list recorded once.

  python tools/edit_scaled_bench.py [--out FILE]
        the driver: every GPU step below in a process of its own under `timeout`, one after the other, and none after one that
        fails; what they print is appended to FILE (default profiles/edit_scaled.txt) under a line "run of <time>"
  python tools/edit_scaled_bench.py replay
        1  spx_edit_replay, int16 mono                 the unchanged kernel: the reference point
        2  spx_edit_replay_scaled at 1 / 1, int16 mono
        3  spx_edit_replay_scaled at 3 / 1, int16 stereo
        4  spx_edit_replay_scaled at 3 / 1, float stereo
        5  a device-to-device copy of as many bytes as (4) reads and writes: the roof
     call after call, in two interleaved rounds; ms per call and GB/s (bytes read plus bytes written, counted from the records)
  python tools/edit_scaled_bench.py master
        6  ONE spx_batch_run of 256 x 10 s as a 48 kHz stereo job (bench.py's inputs for that rate) against one spx_batch_run_edits
           at 16 kHz plus (4): what deciding on the key and rendering the master costs beside walking the master itself

  python tools/edit_scaled_bench.py ab NAME...
        `replay` in a fresh process per build under `timeout`, two rounds interleaved: the shipped library, then
        speedy_amd/lib/ab/libspeedy_hip_<NAME>.so for every NAME (tools/build_variant.sh's place), selected through SPEEDY_HIP_LIB as
        tools/edit_list_time.py ab does; rows (1) to (4) of each, and nothing more after a process that fails

The timing is tools/edit_list_time.py's (30 calls back to back after 5, HIP events on the stream)."""
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
from edit_list_time import N_STREAMS, NL, RATE_HZ, SECONDS, SPEED, line, streams, timed  # noqa: E402

STEP_TIMEOUT_S = {"replay": 240, "master": 300}


def recorded(plan, xs):
    """The workload's Batch(edits=True) after one run: the list every replay below applies."""
    import torch
    from speedy_amd.batch import Batch
    e = Batch(plan, [SECONDS * RATE_HZ] * len(xs), 1, SPEED, NL, 0.0, edits=True)
    e.upload(xs)
    e.run()
    torch.cuda.synchronize()
    assert int(e.d_nops.min()) > 0 and int(e.d_nout.min()) > 0
    return e


def traffic(e, p, q, ch):
    """(values read, values written) of a replay at p / q on tracks of ch channels, from the records: a copy reads one value per
    value it writes, a cross-fade two."""
    nout, nops = e.d_nout.cpu().numpy(), e.d_nops.cpu().numpy()
    ops = e.d_ops.cpu().numpy().astype(np.int64)
    read = written = 0
    for i in range(e.n):
        o = ops[e.op_offs[i]:e.op_offs[i] + int(nops[i])]
        N = int(nout[i]) * p // q
        at, end = o[:, 0] * p // q, (o[:, 0] + o[:, 3]) * p // q
        frames = np.clip(np.minimum(end, N) - at, 0, None)
        read += int((frames * np.where(o[:, 2] >= 0, 2, 1)).sum()) * ch
        written += N * ch
    return read, written


class Render:
    """One spx_edit_replay_scaled call over the recorded lists: tracks of `ch` channels at p / q, random samples."""

    def __init__(self, e, p, q, ch, flt):
        import torch
        from speedy_amd._lib import EditMaster
        self.e, self.p, self.q, self.ch, self.flt = e, p, q, ch, flt
        self.tr = (EditMaster * e.n)()
        in_off = out_off = 0
        n = SECONDS * RATE_HZ * p // q
        for i in range(e.n):
            t = self.tr[i]
            t.in_off, t.out_off, t.n_in, t.out_cap, t.channels = in_off, out_off, n, int(e.out_caps[i]) * p // q, ch
            in_off += n * ch
            out_off += t.out_cap * ch
        if flt:
            self.d_y = torch.rand(in_off, dtype=torch.float32, device=e.device) * 2 - 1
        else:
            self.d_y = torch.randint(-32768, 32767, (in_off,), dtype=torch.int16, device=e.device)
        self.d_yout = torch.zeros(out_off, dtype=self.d_y.dtype, device=e.device)
        self.d_count = torch.zeros(e.n, dtype=torch.int64, device=e.device)
        self.hs = torch.cuda.current_stream().cuda_stream
        self.size = 4 if flt else 2
        r, w = traffic(e, p, q, ch)
        self.bytes = (r + w) * self.size

    def __call__(self):
        e, L = self.e, self.e.plan.L
        rc = L.spx_edit_replay_scaled(e.plan.h, e.jobs, e.n, e.d_ops.data_ptr(), e._ops_cap_ptr(), e.d_nops.data_ptr(), e.d_nout.data_ptr(),
                                      self.tr, self.p, self.q, 1 if self.flt else 0, self.d_y.data_ptr(), self.d_yout.data_ptr(),
                                      self.d_count.data_ptr(), self.hs)
        assert rc == 0, L.spx_last_error()

    def name(self):
        return "spx_edit_replay_scaled %d / %d, %s %s" % (self.p, self.q, "float" if self.flt else "int16", "stereo" if self.ch == 2 else "mono")


def report(k, what, t, nbytes):
    ms = statistics.median(t)
    line("(%d) %s [%.1f MB moved, %.1f GB/s at the median]" % (k, what, nbytes / 1e6, nbytes / ms / 1e6), t)
    return ms


def replay_step():
    import torch
    from speedy_amd._lib import EditTrack
    from speedy_amd.batch import Plan
    plan = Plan(RATE_HZ, False)
    L = plan.L
    e = recorded(plan, streams())
    n = SECONDS * RATE_HZ
    old = (EditTrack * e.n)()
    in_off = out_off = 0
    for i in range(e.n):
        old[i].in_off, old[i].out_off, old[i].channels = in_off, out_off, 1
        in_off += n
        out_off += int(e.out_caps[i])
    d_y = torch.randint(-32768, 32767, (in_off,), dtype=torch.int16, device=e.device)
    d_yout = torch.zeros(out_off, dtype=torch.int16, device=e.device)
    hs = torch.cuda.current_stream().cuda_stream

    def unchanged():
        rc = L.spx_edit_replay(plan.h, e.jobs, e.n, e.d_ops.data_ptr(), e._ops_cap_ptr(), e.d_nops.data_ptr(), e.d_nout.data_ptr(), old,
                               d_y.data_ptr(), d_yout.data_ptr(), hs)
        assert rc == 0, L.spx_last_error()

    r1, w1 = traffic(e, 1, 1, 1)
    new = [Render(e, 1, 1, 1, False), Render(e, 3, 1, 2, False), Render(e, 3, 1, 2, True)]
    half = new[2].bytes // 2
    src, dst = torch.zeros(half, dtype=torch.uint8, device=e.device), torch.zeros(half, dtype=torch.uint8, device=e.device)
    # the new call at 1 / 1 on the same track and offsets is the unchanged kernel's output, byte for byte
    new[0].d_y = d_y
    unchanged()
    new[0]()
    torch.cuda.synchronize()
    print("1 / 1 int16 output equals spx_edit_replay's: %s; grids %d and %d blocks per stream" % (
        bool((new[0].d_yout == d_yout).all()), L.spx_debug_last_replay_grid(None), L.spx_debug_last_scaled_grid(None)))
    ms = {}
    for r in (1, 2):   # interleaved: the spread between the rounds is the run-to-run spread of this process
        print("round %d" % r)
        ms.setdefault(1, []).append(report(1, "spx_edit_replay, int16 mono", timed(unchanged), (r1 + w1) * 2))
        for k, f in zip((2, 3, 4), new):
            ms.setdefault(k, []).append(report(k, f.name(), timed(f), f.bytes))
        ms.setdefault(5, []).append(report(5, "device-to-device copy of %.1f MB" % (half / 1e6), timed(lambda: dst.copy_(src)), 2 * half))
    print("medians of the two rounds, ms: " + "; ".join("(%d) %.4f %.4f" % (k, v[0], v[1]) for k, v in sorted(ms.items())))
    print("(4) against the roof (5): %.0f %% of the copy's rate" % (100.0 * min(ms[5]) / min(ms[4])))
    plan.close()


def master_step():
    import torch
    from speedy_amd.batch import Batch, Plan
    from speedy_amd.synth import speech_like
    plan = Plan(RATE_HZ, False)
    e = recorded(plan, streams())
    render = Render(e, 3, 1, 2, True)
    rate, ch = 3 * RATE_HZ, 2
    n = SECONDS * rate
    big_plan = Plan(rate, False)
    base = [speech_like(n, rate, seed=7000 + i, channels=ch) for i in range(8)]          # bench.py's other_rate_leg inputs
    big = Batch(big_plan, [n] * N_STREAMS, ch, SPEED, NL, 0.0)
    big.upload([base[i % 8] for i in range(N_STREAMS)])
    big.run()
    torch.cuda.synchronize()
    n_out = int(big.d_nout.sum())
    k_out = int(e.d_nout.sum())
    for r in (1, 2):
        print("round %d" % r)
        walk = report(6, "spx_batch_run, 48 kHz stereo int16", timed(big.run), 2 * ch * (n * N_STREAMS + n_out))
        key = report(6, "spx_batch_run_edits, 16 kHz mono key", timed(e.run), 2 * (SECONDS * RATE_HZ * N_STREAMS + k_out))
        rend = report(6, render.name(), timed(render), render.bytes)
        print("(6) walking the master %.3f ms; deciding on the key and rendering the master %.3f + %.3f = %.3f ms: %.2f times" % (
            walk, key, rend, key + rend, walk / (key + rend)))
    big_plan.close()
    plan.close()


def ab(names):
    for r in (1, 2):
        for v in ["shipped"] + names:
            env = dict(os.environ)
            env.pop("SPEEDY_HIP_LIB", None)
            if v != "shipped":
                env["SPEEDY_HIP_LIB"] = os.path.join(ROOT, "speedy_amd", "lib", "ab", "libspeedy_hip_%s.so" % v)
            out = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S["replay"]), sys.executable, os.path.abspath(__file__), "replay"],
                                 env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if out.returncode != 0:
                sys.exit("pass %d, %s: exit status %d, nothing more is started\n%s" % (r, v, out.returncode, out.stdout[-2000:]))
            for l in out.stdout.splitlines():
                if l.startswith(("1 / 1", "(1)", "(2)", "(3)", "(4)", "medians")):
                    print("pass %d  %-8s %s" % (r, v, l), flush=True)


def driver(out_path):
    with open(out_path, "a") as f:
        f.write("run of %s\n" % time.strftime("%Y-%m-%d %H:%M:%S"))
        for step in ("replay", "master"):
            f.write("-- step `%s`\n" % step)
            f.flush()
            r = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S[step]), sys.executable, os.path.abspath(__file__), step],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            f.write(r.stdout)
            f.flush()
            sys.stdout.write(r.stdout)
            if r.returncode != 0:
                f.write("step `%s` ended with exit status %d: nothing more is started\n" % (step, r.returncode))
                sys.exit(r.returncode)
        f.write("\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] in ("replay", "master"):
        import torch
        assert torch.cuda.is_available(), "needs an MI355X"
        replay_step() if args[0] == "replay" else master_step()
    elif len(args) >= 2 and args[0] == "ab":
        ab(args[1:])
    elif not args or (len(args) == 2 and args[0] == "--out"):
        driver(args[1] if args else os.path.join(ROOT, "profiles", "edit_scaled.txt"))
    else:
        sys.exit(__doc__)
