"""Helpers of tests/test_gpu_dirty_memory.py and tests/test_gpu_dirty_owned.py: device memory that is NOT zero when a call gets it.

A scenario is run clean -- buffers as speedy_amd/batch.py allocates them, zeros everywhere -- and again with every buffer the call
may write (workspace, out, n_out, taps, map, edit records, counts) holding a dirt pattern, the input surrounded by noise, and guard
bytes around every buffer.  snap() collects every result as arrays, differences() compares two snapshots byte for byte (so NaN
equals NaN and -0.0 differs from 0.0), guards_intact() says which guard was written.

Patterns (PATTERNS, cheapest first): bytes 0x7F (huge finite floats, huge positive integers), bytes 0xFF (NaN as floats, -1 as
integers), seeded random bytes, and "leftover": the workspace as a call with another table on the same plan left it (the other
buffers: random bytes)."""
import contextlib

import numpy as np
import torch

PATTERNS = ("7f", "ff", "random", "leftover")
GUARD_BYTE = 0x5a          # int16 0x5a5a, the suite's canary
GAPS = (1, 7, 33)          # values between consecutive streams in `in` and between consecutive regions in `out`
PAD_OF = {"7f": "7fff", "ff": "8000", "random": "random", "leftover": "random"}   # what the 64 values behind the last stream hold
FRONT = 64                 # dirty values in front of `in`: a load aligned downward stays inside the allocation


def fill(t, pattern, seed=0):
    """Every byte of a contiguous CUDA tensor."""
    u8 = t.reshape(-1).view(torch.uint8)
    if pattern == "ff":
        u8.fill_(0xFF)
    elif pattern == "7f":
        u8.fill_(0x7F)
    elif pattern == "guard":
        u8.fill_(GUARD_BYTE)
    else:
        rng = np.random.default_rng(seed)
        u8.copy_(torch.from_numpy(rng.integers(0, 256, u8.numel(), dtype=np.uint8)))
    return t


@contextlib.contextmanager
def dirty_allocations(pattern, seed=1000):
    """Inside: every CUDA tensor that torch.zeros / torch.zeros_like hands out holds the pattern instead -- the buffers Batch, DtwBatch
    and their methods (replay, lookup, locate ...) allocate for a call's outputs.  "clean": nothing changes."""
    if pattern == "clean":
        yield
        return
    real_zeros, real_like = torch.zeros, torch.zeros_like
    count = [0]

    def dirt(t):
        if t.is_cuda and t.numel():
            count[0] += 1
            fill(t, pattern, seed + count[0])
        return t

    torch.zeros = lambda *a, **kw: dirt(real_zeros(*a, **kw))
    torch.zeros_like = lambda *a, **kw: dirt(real_like(*a, **kw))
    try:
        yield
    finally:
        torch.zeros, torch.zeros_like = real_zeros, real_like


def _with_guard(t, pattern, seed, front=0, back=16):
    """A dirty tensor of t's shape inside a larger allocation whose other elements hold guard bytes: (view, full, lo, hi in elements
    of the first axis)."""
    n = t.shape[0]
    full = torch.empty((front + n + back,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    fill(full, "guard")
    view = full[front:front + n]
    if n:
        fill(view, pattern, seed)
    return view, full, front, front + n


OUTPUTS = ("d_nout", "t_tension", "t_speed", "t_features", "t_spec", "t_norm", "d_map", "d_ops", "d_nops", "d_probe", "d_speeds")


def ws_bytes(b):
    """The workspace the call b.run() makes asks for with the job table as it stands (the float calls' depends on the offsets)."""
    import speedy_amd.batch as B
    if isinstance(b, B.FloatBatch):
        need = b.plan.L.spx_batch_workspace_bytes_float(b.plan.h, b.jobs, b._rates_ptr(), b.n)
    elif isinstance(b, B.MixedBatch):
        need = b.L.spx_batch_workspace_bytes_mixed(b.hplans, len(b.plans), b.jobs, b.plan_index, b.n)
    else:
        need = b._workspace_bytes()
    assert need > 0
    return int(need)


def place(b, gaps=None, base=0):
    """Lay in and out out again (house()); returns the workspace bytes the call then needs."""
    in_off = out_off = 0
    regions = []
    for i in range(b.n):
        j = b.jobs[i]
        g = gaps[i % len(gaps)] if (gaps and i > 0) else 0
        in_off += g
        out_off += g
        j.in_off, j.out_off = in_off, out_off
        b.in_offs[i], b.out_offs[i] = in_off, out_off
        in_off += int(j.n_in) * int(j.channels)
        regions.append((out_off, out_off + int(j.out_cap) * int(j.channels)))
        out_off += int(j.out_cap) * int(j.channels)
    b._placed = (in_off, out_off, regions, base)
    return ws_bytes(b)


def house(b, pattern, seed=7, gaps=None, base=0, ws=None):
    """Every buffer of a prepared Batch / FloatBatch / TwoPassBatch / MixedBatch moves into a dirty allocation with guards:
    in and out are laid out again -- gaps[i % len(gaps)] values in front of stream i > 0 in `in` and of region i > 0 in `out` (the job
    table's in_off / out_off), both base pointers `base` values into their allocations, FRONT + base dirty values in front of `in`,
    64 behind the last stream.  Input gaps, front and pad are filled by load(); output gaps and the 64 values behind the last region
    hold guard bytes.  ws: a uint8 tensor to take as the workspace as it is (the leftover pattern).  Records what guards_intact()
    needs in b._guards."""
    dev = b.d_out.device
    need = place(b, gaps, base)
    in_off, out_off, regions, base = b._placed
    b.total_in = in_off
    b._in_full = torch.empty(FRONT + base + max(1, in_off) + 64, dtype=b.d_in.dtype, device=dev)
    b.d_in = b._in_full[FRONT + base:]
    out_full = torch.empty(base + max(1, out_off) + 64, dtype=b.d_out.dtype, device=dev)
    fill(out_full, "guard")
    b.d_out = out_full[base:]
    for k, (lo, hi) in enumerate(regions):
        if hi > lo:
            fill(b.d_out[lo:hi], pattern, seed + 100 + k)
    b._guards = {"out": (out_full, [(base + lo, base + hi) for lo, hi in regions])}
    k = 0
    for name in OUTPUTS:
        t = getattr(b, name, None)
        if not isinstance(t, torch.Tensor):
            continue
        k += 1
        view, full, lo, hi = _with_guard(t, pattern, seed + 200 + k)
        setattr(b, name, view)
        b._guards[name] = (full, [(lo, hi)])
    if getattr(b, "taps", None) is not None:
        b.taps.tension, b.taps.speed, b.taps.features = b.t_tension.data_ptr(), b.t_speed.data_ptr(), b.t_features.data_ptr()
        if getattr(b, "t_spec", None) is not None:
            b.taps.spectrogram, b.taps.normalized = b.t_spec.data_ptr(), b.t_norm.data_ptr()
    if ws is None:
        like = torch.empty(need, dtype=torch.uint8, device=dev)
        view, full, lo, hi = _with_guard(like, pattern, seed + 300, front=256, back=256)   # (256: spx_batch_run_float's alignment rule)
        b.d_ws = view
        b._guards["ws"] = (full, [(lo, hi)])
    else:
        assert ws.numel() >= need and ws.data_ptr() % 256 == 0
        b.d_ws = ws[:need]
    return b


def load(b, streams, pad="random", seed=11):
    """The streams to where the job table says, random bytes (full-scale noise; as floats: NaN and infinities among them) everywhere
    else in the allocation, and the 64 values behind the last stream as `pad` says: 0x7FFF, 0x8000 or random."""
    full = getattr(b, "_in_full", None)
    front = 0 if full is None else b.d_in.data_ptr() - full.data_ptr()
    full = b.d_in if full is None else full
    dt = np.float32 if full.dtype == torch.float32 else np.int16
    front //= np.dtype(dt).itemsize
    rng = np.random.default_rng(seed)
    host = np.frombuffer(rng.integers(0, 256, full.numel() * np.dtype(dt).itemsize, dtype=np.uint8).tobytes(), dt).copy()
    end = 0
    for i, x in enumerate(streams):
        x = np.ascontiguousarray(x, dt).ravel()
        assert x.size == int(b.jobs[i].n_in) * int(b.jobs[i].channels)
        o = front + int(b.jobs[i].in_off)
        host[o:o + x.size] = x
        end = max(end, o + x.size)
    if dt == np.int16 and pad != "random":
        host[end:end + 64] = {"7fff": 0x7FFF, "8000": -0x8000}[pad]
    full.copy_(torch.from_numpy(host))


def guards_intact(b):
    """[] or [(buffer, first written byte offset in its allocation)]: everything outside the regions the call owns is as house() left it."""
    torch.cuda.synchronize()
    bad = []
    for name, (full, regions) in getattr(b, "_guards", {}).items():
        row = full[0].numel() * full.element_size() if full.dim() > 1 else full.element_size()
        host = full.cpu().numpy().reshape(-1).view(np.uint8)
        mask = np.ones(host.size, bool)
        for lo, hi in regions:
            mask[lo * row:hi * row] = False
        w = np.nonzero(mask & (host != GUARD_BYTE))[0]
        if w.size:
            bad.append((name, int(w[0])))
    return bad


def snap(b, steps=False, prefix=""):
    """Every result of the last call on b as {name: numpy array}: n_out, out[:n_out] per stream, the taps' rows per stream, map rows,
    ops[:n_ops] and n_ops, n_probe and speeds, spx_batch_read_steps."""
    torch.cuda.synchronize()
    r = {}
    nout = b.d_nout.cpu().numpy().copy()
    r["n_out"] = nout
    out = b.d_out.cpu().numpy()
    for i in range(b.n):
        c, o = int(b.jobs[i].channels), int(b.jobs[i].out_off)
        r["out[%d]" % i] = out[o:o + max(0, int(nout[i])) * c].copy()
    if getattr(b, "taps", None) is not None:
        for i in range(b.n):
            for k, v in b.tap_arrays(i).items():
                r["%s[%d]" % (k, i)] = v.copy()
    if getattr(b, "with_map", False):
        for i in range(b.n):
            r["map[%d]" % i] = b.time_map(i)
    if getattr(b, "with_edits", False):
        cnt = b.op_counts()
        r["n_ops"] = cnt
        for i in range(b.n):
            r["ops[%d]" % i] = b.d_ops[b.op_offs[i]:b.op_offs[i] + max(0, int(cnt[i]))].cpu().numpy().copy()
    if isinstance(getattr(b, "d_probe", None), torch.Tensor):
        r["n_probe"], r["speeds"] = b.probe_counts(), b.final_speeds()
    if steps:
        r["steps"] = b.step_counts()
    return {prefix + k: v for k, v in r.items()}


def differences(clean, dirty):
    """[(result, first differing element or "size a != b", the dirty run's value, the clean run's)] -- byte for byte."""
    bad = []
    assert set(clean) == set(dirty), sorted(set(clean) ^ set(dirty))
    for k in sorted(clean):
        a, d = np.ascontiguousarray(clean[k]), np.ascontiguousarray(dirty[k])
        if a.shape != d.shape or a.dtype != d.dtype:
            bad.append((k, "shape %s %s != %s %s" % (d.shape, d.dtype, a.shape, a.dtype), None, None))
            continue
        if a.tobytes() != d.tobytes():
            fa, fd = a.reshape(-1), d.reshape(-1)
            ua, ud = fa.view(np.uint8).reshape(fa.size, -1), fd.view(np.uint8).reshape(fd.size, -1)
            at = int(np.nonzero((ua != ud).any(axis=1))[0][0])
            bad.append((k, at, fd[at].item() if fd.dtype.names is None else fd[at], fa[at].item() if fa.dtype.names is None else fa[at]))
    return bad
