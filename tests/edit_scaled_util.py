"""Helpers of tests/test_edit_scaled_definition.py and tests/test_gpu_edit_scaled.py: companion tracks (full-scale int16, floats with
denormals and zeros of both signs) and the guarded buffer layout of one spx_edit_replay_scaled call -- the track generator and the
canary layout of tests/test_gpu_edit_list.py, restated for two sample formats and a track table with lengths of its own."""
import numpy as np

import edit_scaled_ref as SC

CANARY16 = 0x5a5a
CANARY32 = 0x5a5a5a5a          # as a float: about 1.5e16, finite, nothing a cross-fade of values in -1 .. 1 produces
COUNT_CANARY = -99
OP_CANARY = -1234567


def full_scale(n_values, seed):
    """Random int16 over the whole range, both ends planted."""
    y = np.random.default_rng(seed).integers(-32768, 32768, max(n_values, 2)).astype(np.int16)
    y[0::97] = -32768
    y[1::89] = 32767
    return y[:n_values]


def float_track(n_values, seed):
    """Random float32 over -1 .. 1 with both ends planted, a few denormals of both signs and a zero of each sign."""
    rng = np.random.default_rng(seed)
    y = rng.uniform(-1.0, 1.0, max(n_values, 8)).astype(np.float32)
    y[0::97] = -1.0
    y[1::89] = 1.0
    y[2::53] = np.float32(1e-41)
    y[3::59] = np.float32(-3e-42)
    y[4::61] = np.float32(0.0)
    y[5::67] = np.float32(-0.0)
    return y[:n_values]


def track(fmt, n_values, seed):
    return float_track(n_values, seed) if fmt == "float" else full_scale(n_values, seed)


def as_bits(a, fmt):
    """What two results are compared as: int64 for int16 samples, the 32 bits of each value for floats."""
    return SC.bits(a).astype(np.int64) if fmt == "float" else np.asarray(a, np.int64)


class Scaled:
    """One spx_edit_replay_scaled call over a Batch(edits=True) -- after its run, or with a planted list -- with a track table of its
    own: in_off / out_off chosen by the test (odd residues modulo 8: never a multiple of 4 elements), guard values around every
    output region and in n_out_y."""

    def __init__(self, b, chans, p, q, fmt, tracks, in_res=(1, 3, 7), out_res=(7, 1, 3), n_in=None, out_caps=None):
        import torch
        from speedy_amd._lib import EditMaster
        self.b, self.p, self.q, self.fmt = b, p, q, fmt
        self.chans = [int(c) for c in chans]
        self.np_dtype = np.float32 if fmt == "float" else np.int16
        self.tracks = [np.ascontiguousarray(y, self.np_dtype) for y in tracks]
        self.tr = (EditMaster * b.n)()
        in_off = out_off = 0
        for i in range(b.n):
            c = self.chans[i]
            in_off += 1 + (in_res[i % len(in_res)] - (in_off + 1)) % 8
            out_off += 1 + (out_res[i % len(out_res)] - (out_off + 1)) % 8
            assert in_off % 2 == 1 and out_off % 2 == 1
            t = self.tr[i]
            t.in_off, t.out_off, t.channels, t.reserved = in_off, out_off, c, 0
            t.n_in = self.tracks[i].size // c if n_in is None else int(n_in[i])
            t.out_cap = SC.S(int(b.out_caps[i]), p, q) if out_caps is None else int(out_caps[i])
            in_off += self.tracks[i].size
            out_off += t.out_cap * c
        host = np.full(in_off + 8, 12345, self.np_dtype)        # (what lies between the tracks is not zero)
        for i, y in enumerate(self.tracks):
            host[self.tr[i].in_off:self.tr[i].in_off + y.size] = y
        self.d_y = torch.from_numpy(host).to(b.device)
        self.size_out = out_off + 8
        self.d_yout = self._canaries()
        self.d_count = torch.full((b.n,), COUNT_CANARY, dtype=torch.int64, device=b.device)

    def _canaries(self):
        import torch
        if self.fmt == "float":
            return torch.from_numpy(np.full(self.size_out, CANARY32, np.uint32).view(np.float32)).to(self.b.device)
        return torch.full((self.size_out,), CANARY16, dtype=torch.int16, device=self.b.device)

    def fmt_code(self):
        return 1 if self.fmt == "float" else 0

    def call(self, **kw):
        import torch
        b, L = self.b, self.b.plan.L
        a = dict(jobs=b.jobs, ops=b.d_ops.data_ptr(), caps=b._ops_cap_ptr(), nops=b.d_nops.data_ptr(), nout=b.d_nout.data_ptr(),
                 tracks=self.tr, p=self.p, q=self.q, fmt=self.fmt_code(), y=self.d_y.data_ptr(), yout=self.d_yout.data_ptr(),
                 count=self.d_count.data_ptr())
        a.update(kw)
        rc = L.spx_edit_replay_scaled(b.plan.h, a["jobs"], b.n, a["ops"], a["caps"], a["nops"], a["nout"], a["tracks"], a["p"], a["q"],
                                      a["fmt"], a["y"], a["yout"], a["count"], torch.cuda.current_stream().cuda_stream)
        msg = L.spx_last_error().decode() if rc != 0 else ""
        torch.cuda.synchronize()
        return rc, msg

    def out(self):
        import torch
        torch.cuda.synchronize()
        return self.d_yout.cpu().numpy().copy()

    def counts(self):
        import torch
        torch.cuda.synchronize()
        return self.d_count.cpu().numpy().copy()

    def untouched(self):
        """No output value and no count was written."""
        out = as_bits(self.out(), self.fmt)
        return bool((out == (CANARY32 if self.fmt == "float" else CANARY16)).all()) and bool((self.counts() == COUNT_CANARY).all())

    def check(self, want):
        """want[i]: the expected values of stream i, flat (None: nothing may be written there); everything else is a guard value."""
        out = as_bits(self.out(), self.fmt)
        canary = CANARY32 if self.fmt == "float" else CANARY16
        mask = np.zeros(out.size, bool)
        for i in range(self.b.n):
            if want[i] is None:
                continue
            w = as_bits(want[i], self.fmt)
            o = int(self.tr[i].out_off)
            got = out[o:o + w.size]
            assert np.array_equal(got, w), "stream %d (%d channels, out_off %d, %s %d/%d): first difference at value %d of %d" % (
                i, self.chans[i], o, self.fmt, self.p, self.q, int(np.nonzero(got != w)[0][0]), w.size)
            mask[o:o + w.size] = True
        assert (out[~mask] == canary).all(), "values written outside the streams' output: %s" % np.nonzero(out[~mask] != canary)[0][:8]
