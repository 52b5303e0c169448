"""Batch dynamic time warping on the GPU (spx_batch_dtw, include/speedy_hip.h "BATCH DTW"): for every pair of float sequences
the accumulated cost, the warp path, its slope and the mean and deviation of its local slopes -- the reference's perceptual check
(sonic_test.cc:639-724) for a whole batch, on rows that are already in device memory."""
import ctypes as C

import numpy as np
import torch

from ._lib import DtwJob

RESULT_DTYPE = np.dtype([("cost", np.float32), ("slope", np.float32), ("local_mean", np.float32), ("local_std", np.float32),
                         ("n_path", np.int32), ("n_local", np.int32)])   # spx_dtw_result, 24 bytes


class DtwBatch:
    """A prepared batch of pairs: pair i aligns lengths_a[i] rows of `a` with lengths_b[i] rows of `b` on the first `dim` values of
    each row.  Rows of a sequence are ld_a / ld_b floats apart (default: dim, packed rows) and the sequences follow one another
    in job order -- the layout of the `spectrogram` tap of a Batch (ld = plan.N), which can be handed to run() where it lies.
    offsets_a / offsets_b (in floats) place the sequences elsewhere.  run(a, b) enqueues the call on device tensors, results() is
    a structured numpy array (RESULT_DTYPE), path(i) the pair's warp path as an (n_path, 2) int32 array of (a index, b index)."""

    def __init__(self, plan, lengths_a, lengths_b, dim, ld_a=None, ld_b=None, half_width=10, device="cuda", offsets_a=None,
                 offsets_b=None):
        if not torch.cuda.is_available():
            raise RuntimeError("speedy_amd needs a HIP device; there is no CPU path")
        if len(lengths_a) != len(lengths_b):
            raise ValueError("lengths_a and lengths_b differ in length")
        self.plan = plan
        self.n = n = len(lengths_a)
        self.dim = int(dim)
        self.ld_a = self.dim if ld_a is None else int(ld_a)
        self.ld_b = self.dim if ld_b is None else int(ld_b)
        self.half_width = int(half_width)
        self.lengths_a = [int(v) for v in lengths_a]
        self.lengths_b = [int(v) for v in lengths_b]
        self.jobs = (DtwJob * max(1, n))()
        self.path_offs = []
        a_off = b_off = p_off = 0
        for i in range(n):
            j = self.jobs[i]
            j.a_off = a_off if offsets_a is None else int(offsets_a[i])
            j.b_off = b_off if offsets_b is None else int(offsets_b[i])
            j.path_off, j.n_a, j.n_b = p_off, self.lengths_a[i], self.lengths_b[i]
            self.path_offs.append(p_off)
            a_off += self.lengths_a[i] * self.ld_a
            b_off += self.lengths_b[i] * self.ld_b
            p_off += max(0, self.lengths_a[i] + self.lengths_b[i] - 1)
        self.values_a, self.values_b = a_off, b_off
        dev = torch.device(device)
        self.device = dev
        ws = plan.L.spx_dtw_workspace_bytes(self.jobs, n, self.dim)
        if ws == 0:
            raise RuntimeError("spx_dtw_workspace_bytes: " + plan.L.spx_last_error().decode())
        self.d_ws = torch.zeros(ws, dtype=torch.uint8, device=dev)
        self.d_results = torch.zeros(n * RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_path = torch.zeros(max(1, p_off) * 2, dtype=torch.int32, device=dev)

    def run(self, a, b, stream=None):
        """Enqueue spx_batch_dtw on `stream` (torch stream or None) for the float32 device tensors a and b."""
        for t in (a, b):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError("run: contiguous float32 CUDA tensors")
        hs = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        rc = self.plan.L.spx_batch_dtw(self.plan.h, self.jobs, self.n, self.dim, self.ld_a, self.ld_b, self.half_width, a.data_ptr(),
                                       b.data_ptr(), self.d_results.data_ptr(), self.d_path.data_ptr(), self.d_ws.data_ptr(),
                                       self.d_ws.numel(), hs)
        if rc != 0:
            raise RuntimeError("spx_batch_dtw: " + self.plan.L.spx_last_error().decode())

    def results(self):
        torch.cuda.synchronize(self.device)
        return self.d_results.cpu().numpy().view(RESULT_DTYPE).copy()

    def path(self, i):
        n_path = int(self.results()["n_path"][i])
        p0 = self.path_offs[i]
        return self.d_path[2 * p0:2 * (p0 + n_path)].cpu().numpy().reshape(n_path, 2)

    def grid(self):
        """(workgroups per launch, launches) of the last spx_batch_dtw of the process."""
        launches = C.c_int(0)
        gx = self.plan.L.spx_debug_last_dtw_grid(C.byref(launches))
        return gx, launches.value
