"""Batch engine: N independent streams, device-resident, one spx_batch_run call (include/speedy_hip.h) -- or, with a playback
rate per stream (sonicSetRate before the first write), one spx_batch_run_rate call.

Host-side mirror of what the reference's caller loop does per stream (speedy_wave.cc:154-242): create,
setSpeed, enableNonlinear, setFeedback, write everything, flush, drain."""
import ctypes as C

import numpy as np
import torch

from ._lib import EditMaster, EditRowsTrack, EditTrack, StreamJob, Taps, lib


class Plan:
    def __init__(self, sample_rate, match_matlab=False):
        self.L = lib()
        if not torch.cuda.is_available():
            raise RuntimeError("speedy_amd needs a HIP device; there is no CPU path")
        self.h = self.L.spx_plan_create(int(sample_rate), int(bool(match_matlab)))
        if not self.h:
            raise RuntimeError("spx_plan_create: " + self.L.spx_last_error().decode())
        self.sample_rate = sample_rate
        self.B = self.L.spx_plan_frame_step(self.h)
        self.W = self.L.spx_plan_window_size(self.h)
        self.N = self.L.spx_plan_fft_size(self.h)
        self.F = self.L.spx_plan_future(self.h)
        self.max_required = self.L.spx_plan_max_required(self.h)

    def frames(self, n_in):
        return self.L.spx_plan_frames(self.h, int(n_in))

    def out_capacity(self, n_in, speed, nonlinear=1.0, rate=None):
        if rate is None:
            return self.L.spx_plan_out_capacity_for(self.h, int(n_in), float(speed), float(nonlinear))
        cap = self.L.spx_plan_out_capacity_rate(self.h, int(n_in), float(speed), float(nonlinear), float(rate))
        if cap < 0:
            raise RuntimeError("spx_plan_out_capacity_rate: " + self.L.spx_last_error().decode())
        return cap

    def close(self):
        if self.h:
            self.L.spx_plan_destroy(self.h)
            self.h = None


class Batch:
    """A prepared batch: inputs packed into one HBM buffer, outputs and workspace allocated once.
    rate: a playback rate (sonicSetRate) for every stream or one per stream -- run() is then spx_batch_run_rate and the
    outputs are the final frames behind the rate stage; None: spx_batch_run, call for call as before.
    time_map: run() is spx_batch_run_map -- the same outputs, counts and taps, and a time map beside them: time_map(i) returns
    stream i's rows (the output frames produced when each 10 ms ring buffer of input is handed to the time-scale stage, then the
    final count), lookup(i, positions) converts input frames to output frames (inverse=True: the other way) on the GPU.  With
    rate= as well, run() is spx_batch_run_rate_map and the rows, like the outputs, count final frames.  The plain call only: no
    run_ahead.
    edits: run() is spx_batch_run_edits -- the same outputs, counts and taps, and the jobs' edit lists beside them: edits(i) returns
    stream i's records (out_at, a, b, n), replay(tracks, channels) applies the lists to companion tracks of the same lengths on the
    GPU (spx_edit_replay), replay_scaled(tracks, channels, ratio) to masters at a higher sample rate, int16 or float32
    (spx_edit_replay_scaled).  The capacities are spx_plan_edit_ops' (ops_caps: one value or one per stream instead); not together
    with rate or time_map.  The plain call only.  locate(i, positions) and locate_all(positions) convert positions through the lists
    to the sample (spx_edit_lookup), where lookup answers to 10 ms.  warp_rows(tracks, hop) brings label or feature rows on the
    input's timeline onto the output's and unwarp_rows(tracks, hop) brings rows on the output's timeline back (spx_edit_warp_rows,
    spx_edit_unwarp_rows)."""

    d_index = None          # the running maximum spx_edit_index writes, beside d_ops: made at the first forward locate
    _index_built = False    # ... and valid until the next run()

    def __init__(self, plan, lengths, channels, speed, nonlinear=1.0, feedback=0.0, device="cuda", taps=False,
                 spectrogram_taps=False, rate=None, time_map=False, edits=False, ops_caps=None):
        if edits and (rate is not None or time_map):
            raise ValueError("edits=True goes with neither rate nor time_map (spx_batch_run_edits is the plain call's)")
        if (time_map or edits) and not torch.cuda.is_available():
            raise RuntimeError("speedy_amd needs a HIP device; there is no CPU path")
        self.plan = plan
        n = len(lengths)
        self.n = n
        self.with_map = bool(time_map)
        self.with_edits = bool(edits)
        self.rates = None
        if rate is not None:
            if not torch.cuda.is_available():
                raise RuntimeError("speedy_amd needs a HIP device; there is no CPU path")
            self.rates = np.ascontiguousarray(np.broadcast_to(np.asarray(rate, np.float32), (n,)))
        ch = np.broadcast_to(np.asarray(channels, np.int32), (n,)).copy()
        sp = np.broadcast_to(np.asarray(speed, np.float32), (n,)).copy()
        nlv = np.broadcast_to(np.asarray(nonlinear, np.float32), (n,)).copy()
        fb = np.broadcast_to(np.asarray(feedback, np.float32), (n,)).copy()
        self.lengths = np.asarray(lengths, np.int64)
        self.channels = ch
        self.jobs = (StreamJob * n)()
        in_off = out_off = 0
        self.in_offs, self.out_offs, self.out_caps, self.frame_offs, self.frames = [], [], [], [], []
        fo = 0
        for i in range(n):
            cap = self._capacity(i, int(self.lengths[i]), float(sp[i]), float(nlv[i]))
            j = self.jobs[i]
            j.in_off, j.n_in, j.out_off, j.out_cap = in_off, int(self.lengths[i]), out_off, cap
            j.channels, j.speed, j.nonlinear, j.feedback = int(ch[i]), float(sp[i]), float(nlv[i]), float(fb[i])
            self.in_offs.append(in_off)
            self.out_offs.append(out_off)
            self.out_caps.append(cap)
            T = plan.frames(int(self.lengths[i])) if nlv[i] != 0 else 0
            self.frame_offs.append(fo)
            self.frames.append(T)
            fo += T
            in_off += int(self.lengths[i]) * int(ch[i])
            out_off += cap * int(ch[i])
        self.total_in, self.total_out, self.total_frames = in_off, out_off, fo
        dev = torch.device(device)
        self.device = dev
        self.d_in = torch.zeros(max(1, in_off) + 64, dtype=torch.int16, device=dev)
        self.d_out = torch.zeros(max(1, out_off), dtype=torch.int16, device=dev)
        self.d_nout = torch.zeros(n, dtype=torch.int64, device=dev)
        self.d_ws = torch.zeros(self._workspace_bytes(), dtype=torch.uint8, device=dev)
        if self.with_map:
            self._alloc_map(nlv)
        if self.with_edits:
            self._alloc_edits(sp, nlv, ops_caps)
        self.taps = None
        if taps:
            T1 = max(1, fo)
            self.t_tension = torch.zeros(T1, dtype=torch.float32, device=dev)
            self.t_speed = torch.zeros(T1, dtype=torch.float32, device=dev)
            self.t_features = torch.zeros(T1 * 15, dtype=torch.float32, device=dev)
            self.taps = Taps(self.t_tension.data_ptr(), self.t_speed.data_ptr(), self.t_features.data_ptr(), None,
                             None)
            if spectrogram_taps:
                self.t_spec = torch.zeros(T1 * plan.N, dtype=torch.float32, device=dev)
                self.t_norm = torch.zeros(T1 * plan.W, dtype=torch.float32, device=dev)
                self.taps.spectrogram = self.t_spec.data_ptr()
                self.taps.normalized = self.t_norm.data_ptr()

    def _alloc_map(self, nonlinear):
        """The time map's device buffer: stream i's rows are d_map[map_offs[i] : map_offs[i + 1]] (spx_plan_map_rows per job, in job order)."""
        plan = self.plan
        self.map_offs = [0]
        for i in range(self.n):
            self.map_offs.append(self.map_offs[-1] + plan.L.spx_plan_map_rows(plan.h, int(self.lengths[i]), float(nonlinear[i])))
        self.d_map = torch.zeros(self.map_offs[-1], dtype=torch.int64, device=self.device)

    def _alloc_edits(self, speed, nonlinear, ops_caps):
        """The edit list's device buffers: stream i's records are d_ops[op_offs[i] : op_offs[i] + n_ops[i]] (rows of four int32)."""
        plan = self.plan
        if ops_caps is None:
            caps = [plan.L.spx_plan_edit_ops(plan.h, int(self.lengths[i]), float(speed[i]), float(nonlinear[i])) for i in range(self.n)]
            if min(caps) < 0:
                raise RuntimeError("spx_plan_edit_ops: " + plan.L.spx_last_error().decode())
        else:
            caps = [int(v) for v in np.broadcast_to(np.asarray(ops_caps, np.int64), (self.n,))]
        self.ops_caps = np.ascontiguousarray(caps, np.int64)
        self.op_offs = [0] + [int(v) for v in np.cumsum(self.ops_caps)]
        self.d_ops = torch.zeros((max(1, self.op_offs[-1]), 4), dtype=torch.int32, device=self.device)
        self.d_nops = torch.zeros(self.n, dtype=torch.int64, device=self.device)

    def _ops_cap_ptr(self):
        return self.ops_caps.ctypes.data_as(C.POINTER(C.c_int64))

    def _capacity(self, i, n_in, speed, nonlinear):
        """Output capacity of stream i in frames (a subclass with another capacity rule overrides this)."""
        return self.plan.out_capacity(n_in, speed, nonlinear, None if self.rates is None else float(self.rates[i]))

    def _workspace_bytes(self):
        """Device workspace of the call run() makes."""
        plan = self.plan
        if self.rates is None:
            return plan.L.spx_batch_workspace_bytes(plan.h, self.jobs, self.n)
        wsb = plan.L.spx_batch_workspace_bytes_rate(plan.h, self.jobs, self._rates_ptr(), self.n)
        if wsb == 0:
            raise RuntimeError("spx_batch_workspace_bytes_rate: " + plan.L.spx_last_error().decode())
        return wsb

    def upload(self, streams):
        """streams: list of int16 numpy arrays (interleaved).  Packs and copies them to HBM."""
        host = np.zeros(self.d_in.numel(), np.int16)
        for i, x in enumerate(streams):
            x = np.ascontiguousarray(x, np.int16).ravel()
            assert x.size == int(self.lengths[i]) * int(self.channels[i])
            host[self.in_offs[i]:self.in_offs[i] + x.size] = x
        self.d_in.copy_(torch.from_numpy(host))

    def _rates_ptr(self):
        return self.rates.ctypes.data_as(C.POINTER(C.c_float))

    def run(self, stream=None):
        """Enqueue the whole hot path (analysis + walk, and the rate stage of a batch with rates) on `stream` (torch stream or None)."""
        hs = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        if self.rates is not None and self.with_map:
            rc = self.plan.L.spx_batch_run_rate_map(self.plan.h, self.jobs, self._rates_ptr(), self.n, self.d_in.data_ptr(),
                                                    self.d_out.data_ptr(), self.d_nout.data_ptr(), self.d_map.data_ptr(),
                                                    self.d_ws.data_ptr(), self.d_ws.numel(),
                                                    C.byref(self.taps) if self.taps is not None else None, hs)
            if rc != 0:
                raise RuntimeError("spx_batch_run_rate_map: " + self.plan.L.spx_last_error().decode())
            return
        if self.rates is not None:
            rc = self.plan.L.spx_batch_run_rate(self.plan.h, self.jobs, self._rates_ptr(), self.n, self.d_in.data_ptr(),
                                                self.d_out.data_ptr(), self.d_nout.data_ptr(), self.d_ws.data_ptr(),
                                                self.d_ws.numel(), C.byref(self.taps) if self.taps is not None else None, hs)
            if rc != 0:
                raise RuntimeError("spx_batch_run_rate: " + self.plan.L.spx_last_error().decode())
            return
        if self.with_map:
            rc = self.plan.L.spx_batch_run_map(self.plan.h, self.jobs, self.n, self.d_in.data_ptr(), self.d_out.data_ptr(),
                                               self.d_nout.data_ptr(), self.d_map.data_ptr(), self.d_ws.data_ptr(), self.d_ws.numel(),
                                               C.byref(self.taps) if self.taps is not None else None, hs)
            if rc != 0:
                raise RuntimeError("spx_batch_run_map: " + self.plan.L.spx_last_error().decode())
            return
        if self.with_edits:
            rc = self.plan.L.spx_batch_run_edits(self.plan.h, self.jobs, self.n, self.d_in.data_ptr(), self.d_out.data_ptr(),
                                                 self.d_nout.data_ptr(), self.d_ops.data_ptr(), self._ops_cap_ptr(),
                                                 self.d_nops.data_ptr(), self.d_ws.data_ptr(), self.d_ws.numel(),
                                                 C.byref(self.taps) if self.taps is not None else None, hs)
            self._index_built = False
            if rc != 0:
                raise RuntimeError("spx_batch_run_edits: " + self.plan.L.spx_last_error().decode())
            return
        rc = self.plan.L.spx_batch_run(self.plan.h, self.jobs, self.n, self.d_in.data_ptr(), self.d_out.data_ptr(),
                                       self.d_nout.data_ptr(), self.d_ws.data_ptr(), self.d_ws.numel(),
                                       C.byref(self.taps) if self.taps is not None else None, hs)
        if rc != 0:
            raise RuntimeError("spx_batch_run: " + self.plan.L.spx_last_error().decode())

    def run_ahead(self, stream=None, in_ready=None, overlap=False):
        """spx_batch_run_ahead: like run(), software-pipelined with the previous call on the same stream (the caller alternates
        two Batch objects).  in_ready: a recorded torch.cuda.Event behind whatever completes the input (None: the input is
        resident when the call is made).  overlap: spx_batch_run_overlapped -- the walk kernels of consecutive calls overlap
        too; nothing enqueued between two calls may touch the later call's buffers (include/speedy_hip.h)."""
        if self.rates is not None:
            raise RuntimeError("a batch with rates runs through the plain call only (spx_batch_run_rate)")
        if self.with_map:
            raise RuntimeError("a batch with a time map runs through the plain call only (spx_batch_run_map)")
        if self.with_edits:
            raise RuntimeError("a batch with an edit list runs through the plain call only (spx_batch_run_edits)")
        hs = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        if overlap:
            assert in_ready is None
            rc = self.plan.L.spx_batch_run_overlapped(self.plan.h, self.jobs, self.n, self.d_in.data_ptr(), self.d_out.data_ptr(),
                                                      self.d_nout.data_ptr(), self.d_ws.data_ptr(), self.d_ws.numel(),
                                                      C.byref(self.taps) if self.taps is not None else None, hs)
            if rc != 0:
                raise RuntimeError("spx_batch_run_overlapped: " + self.plan.L.spx_last_error().decode())
            return
        rc = self.plan.L.spx_batch_run_ahead_when(self.plan.h, self.jobs, self.n, self.d_in.data_ptr(), self.d_out.data_ptr(),
                                                  self.d_nout.data_ptr(), self.d_ws.data_ptr(), self.d_ws.numel(),
                                                  C.byref(self.taps) if self.taps is not None else None, hs,
                                                  in_ready.cuda_event if in_ready is not None else None)
        if rc != 0:
            raise RuntimeError("spx_batch_run_ahead: " + self.plan.L.spx_last_error().decode())

    def step_counts(self):
        """Pitch searches per stream of the last run (the length of each stream's dependent chain); synchronises."""
        steps = (C.c_int32 * self.n)()
        rc = self.plan.L.spx_batch_read_steps(self.plan.h, self.jobs, self.n, self.d_ws.data_ptr(), steps,
                                              torch.cuda.current_stream(self.device).cuda_stream)
        if rc != 0:
            raise RuntimeError("spx_batch_read_steps: " + self.plan.L.spx_last_error().decode())
        torch.cuda.synchronize(self.device)
        return np.frombuffer(steps, np.int32).copy()

    def results(self):
        """Synchronise and return per-stream int16 outputs (host numpy)."""
        torch.cuda.synchronize(self.device)
        nout = self.d_nout.cpu().numpy()
        lost = nout == np.iinfo(np.int64).min   # SPX_NOUT_LOST_PRODUCER
        if lost.any():
            raise RuntimeError("a producer kernel never delivered its frames to streams %s (device-side poll limit)"
                               % np.nonzero(lost)[0][:8])
        if (nout < 0).any():
            raise RuntimeError("output capacity exceeded for streams %s" % np.nonzero(nout < 0)[0][:8])
        out = self.d_out.cpu().numpy()
        res = []
        for i in range(self.n):
            c = int(self.channels[i])
            res.append(out[self.out_offs[i]:self.out_offs[i] + int(nout[i]) * c].copy())
        return res

    def pack_outputs(self, stream=None):
        """Enqueue the gather of all produced frames into one contiguous device buffer (after run() on the same
        stream).  Returns (packed int16 device tensor, offsets int64[n+1] device tensor); stream i is
        packed[offsets[i]:offsets[i+1]].  One device-to-host copy then moves a whole batch's output."""
        if getattr(self, "d_packed", None) is None:
            self.d_packed = torch.empty_like(self.d_out)
            self.d_offsets = torch.zeros(self.n + 1, dtype=torch.int64, device=self.device)
        hs = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        rc = self.plan.L.spx_batch_pack_outputs(self.jobs, self.n, self.d_out.data_ptr(), self.d_nout.data_ptr(),
                                                self.d_packed.data_ptr(), self.d_offsets.data_ptr(), hs)
        if rc != 0:
            raise RuntimeError("spx_batch_pack_outputs: " + self.plan.L.spx_last_error().decode())
        return self.d_packed, self.d_offsets

    def time_map(self, i):
        """Stream i's time-map rows of the last run (host numpy int64): for a nonlinear stream row k < n_in // B is the number of
        output frames produced when input frames [k B, (k + 1) B) are handed to the time-scale stage, the last row is the final
        count; a linear stream has the final count alone.  On a batch with rates (and on a FloatBatch) the rows count final frames,
        behind the rate stage, as the outputs do."""
        if not self.with_map:
            raise RuntimeError("the batch was made without time_map=True")
        torch.cuda.synchronize(self.device)
        return self.d_map[self.map_offs[i]:self.map_offs[i + 1]].cpu().numpy().copy()

    def lookup_all(self, positions, inverse=False, stream=None):
        """spx_map_lookup over the whole batch: positions[i] = stream i's queries (any int sequence, may be empty).  Input frames to
        output frames, inverse=True: output frames to input frames; exact integer interpolation between the map's nodes
        (include/speedy_hip.h).  Returns a list of int64 numpy arrays."""
        if not self.with_map:
            raise RuntimeError("the batch was made without time_map=True")
        assert len(positions) == self.n
        qs = [np.ascontiguousarray(p, np.int64).ravel() for p in positions]
        offs = np.zeros(self.n + 1, np.int64)
        offs[1:] = np.cumsum([q.size for q in qs])
        total = int(offs[-1])
        d_off = torch.from_numpy(offs).to(self.device)
        d_q = torch.from_numpy(np.concatenate(qs) if total else np.zeros(1, np.int64)).to(self.device)
        d_r = torch.zeros_like(d_q)
        hs = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        rc = self.plan.L.spx_map_lookup(self.plan.h, self.jobs, self.n, self.d_map.data_ptr(), d_off.data_ptr(), d_q.data_ptr(),
                                        d_r.data_ptr(), 1 if inverse else 0, hs)
        if rc != 0:
            raise RuntimeError("spx_map_lookup: " + self.plan.L.spx_last_error().decode())
        torch.cuda.synchronize(self.device)
        res = d_r.cpu().numpy()
        return [res[int(offs[i]):int(offs[i + 1])].copy() for i in range(self.n)]

    def lookup(self, i, positions, inverse=False):
        """Stream i's positions through the time map: input frames to output frames (inverse=True: the other way)."""
        empty = np.zeros(0, np.int64)
        return self.lookup_all([positions if k == i else empty for k in range(self.n)], inverse)[i]

    def op_counts(self):
        """Records per stream of the last run (host numpy int64; minus the count where the capacity was too small); synchronises."""
        if not self.with_edits:
            raise RuntimeError("the batch was made without edits=True")
        torch.cuda.synchronize(self.device)
        return self.d_nops.cpu().numpy().copy()

    def edits(self, i):
        """Stream i's edit list of the last run: an (n_ops, 4) int32 array of (out_at, a, b, n) -- b < 0: n frames copied from input
        frame a to output frame out_at; b >= 0: n frames of cross-fade from the run at a (fading out) to the run at b (fading in)."""
        k = int(self.op_counts()[i])
        if k < 0:
            raise RuntimeError("stream %d has %d records, its capacity holds %d" % (i, -k, int(self.ops_caps[i])))
        return self.d_ops[self.op_offs[i]:self.op_offs[i] + k].cpu().numpy().copy()

    def replay(self, tracks, channels, stream=None):
        """spx_edit_replay over the whole batch: tracks[i] = a companion of stream i (int16, interleaved, the stream's length in
        frames), channels = its channel count (one value or one per stream, any count).  Returns the replayed tracks (host numpy
        int16), trimmed to the streams' output lengths."""
        if not self.with_edits:
            raise RuntimeError("the batch was made without edits=True")
        assert len(tracks) == self.n
        ch = np.broadcast_to(np.asarray(channels, np.int32), (self.n,))
        tr = (EditTrack * self.n)()
        in_off = out_off = 0
        for i in range(self.n):
            tr[i].in_off, tr[i].out_off, tr[i].channels, tr[i].reserved = in_off, out_off, int(ch[i]), 0
            in_off += int(self.lengths[i]) * int(ch[i])
            out_off += int(self.out_caps[i]) * int(ch[i])
        host = np.zeros(max(1, in_off), np.int16)
        for i, y in enumerate(tracks):
            y = np.ascontiguousarray(y, np.int16).ravel()
            assert y.size == int(self.lengths[i]) * int(ch[i])
            host[tr[i].in_off:tr[i].in_off + y.size] = y
        d_y = torch.from_numpy(host).to(self.device)
        d_yout = torch.zeros(max(1, out_off), dtype=torch.int16, device=self.device)
        hs = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        rc = self.plan.L.spx_edit_replay(self.plan.h, self.jobs, self.n, self.d_ops.data_ptr(), self._ops_cap_ptr(),
                                         self.d_nops.data_ptr(), self.d_nout.data_ptr(), tr, d_y.data_ptr(), d_yout.data_ptr(), hs)
        if rc != 0:
            raise RuntimeError("spx_edit_replay: " + self.plan.L.spx_last_error().decode())
        torch.cuda.synchronize(self.device)
        nout = self.d_nout.cpu().numpy()
        out = d_yout.cpu().numpy()
        return [out[tr[i].out_off:tr[i].out_off + max(0, int(nout[i])) * int(ch[i])].copy() for i in range(self.n)]

    def replay_scaled(self, tracks, channels, ratio, stream=None):
        """spx_edit_replay_scaled over the whole batch: tracks[i] = the master of stream i at ratio = (p, q) (or an int) times the
        key's sample rate -- numpy or torch, int16 or float32, one dtype per call, interleaved, any length (size // channels frames
        count); channels = its channel count (one value or one per stream).  The output capacity of stream i is out_caps[i] scaled
        by the ratio.  Returns the rendered masters (host numpy of the tracks' dtype), trimmed to the counts the call wrote."""
        if not self.with_edits:
            raise RuntimeError("the batch was made without edits=True")
        assert len(tracks) == self.n
        p, q = (int(ratio), 1) if isinstance(ratio, (int, np.integer)) else (int(ratio[0]), int(ratio[1]))
        ys = [np.ascontiguousarray(y.detach().cpu().numpy() if torch.is_tensor(y) else y).ravel() for y in tracks]
        kinds = {y.dtype for y in ys}
        if len(kinds) != 1 or next(iter(kinds)) not in (np.dtype(np.int16), np.dtype(np.float32)):
            raise ValueError("the tracks of one call are all int16 or all float32, not %s" % sorted(str(k) for k in kinds))
        dtype = next(iter(kinds))
        fmt = 1 if dtype == np.dtype(np.float32) else 0        # SPX_SAMPLES_FLOAT / SPX_SAMPLES_INT16
        L = self.plan.L
        ch = np.broadcast_to(np.asarray(channels, np.int32), (self.n,))
        tr = (EditMaster * self.n)()
        in_off = out_off = 0
        for i in range(self.n):
            cap = L.spx_edit_scale(int(self.out_caps[i]), p, q)
            if cap < 0:
                raise RuntimeError("spx_edit_scale refuses the ratio %d / %d" % (p, q))
            t = tr[i]
            t.in_off, t.out_off, t.channels, t.reserved = in_off, out_off, int(ch[i]), 0
            t.n_in, t.out_cap = ys[i].size // max(1, int(ch[i])), cap
            in_off += ys[i].size
            out_off += cap * int(ch[i])
        host = np.zeros(max(1, in_off), dtype)
        for i, y in enumerate(ys):
            host[tr[i].in_off:tr[i].in_off + y.size] = y
        d_y = torch.from_numpy(host).to(self.device)
        d_yout = torch.zeros(max(1, out_off), dtype=d_y.dtype, device=self.device)
        d_count = torch.zeros(self.n, dtype=torch.int64, device=self.device)
        hs = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        rc = L.spx_edit_replay_scaled(self.plan.h, self.jobs, self.n, self.d_ops.data_ptr(), self._ops_cap_ptr(), self.d_nops.data_ptr(),
                                      self.d_nout.data_ptr(), tr, p, q, fmt, d_y.data_ptr(), d_yout.data_ptr(), d_count.data_ptr(), hs)
        if rc != 0:
            raise RuntimeError("spx_edit_replay_scaled: " + L.spx_last_error().decode())
        torch.cuda.synchronize(self.device)
        count = d_count.cpu().numpy()
        if (count < 0).any():
            raise RuntimeError("output capacity exceeded for streams %s" % np.nonzero(count < 0)[0][:8])
        out = d_yout.cpu().numpy()
        return [out[tr[i].out_off:tr[i].out_off + int(count[i]) * int(ch[i])].copy() for i in range(self.n)]

    def locate_all(self, positions, inverse=False, records=False, stream=None):
        """spx_edit_lookup over the whole batch, to the sample: positions[i] = stream i's queries (any int sequence, may be empty).
        Input frames to the output frame each is first heard at; inverse=True: output frames to the input frame each plays
        (include/speedy_hip.h "POSITION LOOKUP").  Returns a list of int64 numpy arrays; records=True: (that list, a list of int32
        arrays with the index of each answer's record in edits(i), -1 where there is none).  The index a forward lookup searches
        (spx_edit_index) is built at the first one after a run()."""
        if not self.with_edits:
            raise ValueError("the batch was made without edits=True")
        assert len(positions) == self.n
        qs = [np.ascontiguousarray(p, np.int64).ravel() for p in positions]
        offs = np.zeros(self.n + 1, np.int64)
        offs[1:] = np.cumsum([q.size for q in qs])
        total = int(offs[-1])
        d_off = torch.from_numpy(offs).to(self.device)
        d_q = torch.from_numpy(np.concatenate(qs) if total else np.zeros(1, np.int64)).to(self.device)
        d_r = torch.zeros_like(d_q)
        d_rec = torch.zeros(d_q.numel(), dtype=torch.int32, device=self.device) if records else None
        L = self.plan.L
        hs = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        if not inverse:
            self._ensure_index(hs)
        rc = L.spx_edit_lookup(self.plan.h, self.jobs, self.n, self.d_ops.data_ptr(), self._ops_cap_ptr(), self.d_nops.data_ptr(),
                               self.d_nout.data_ptr(), None if inverse else self.d_index.data_ptr(), d_off.data_ptr(), d_q.data_ptr(),
                               d_r.data_ptr(), d_rec.data_ptr() if records else None, 1 if inverse else 0, hs)
        if rc != 0:
            raise RuntimeError("spx_edit_lookup: " + L.spx_last_error().decode())
        torch.cuda.synchronize(self.device)
        res = d_r.cpu().numpy()
        ans = [res[int(offs[i]):int(offs[i + 1])].copy() for i in range(self.n)]
        if not records:
            return ans
        rec = d_rec.cpu().numpy()
        return ans, [rec[int(offs[i]):int(offs[i + 1])].copy() for i in range(self.n)]

    def locate(self, i, positions, inverse=False, records=False):
        """Stream i's positions through its edit list: input frames to output frames (inverse=True: the other way); records=True:
        (answers, record indices)."""
        if not self.with_edits:
            raise ValueError("the batch was made without edits=True")
        empty = np.zeros(0, np.int64)
        got = self.locate_all([positions if k == i else empty for k in range(self.n)], inverse, records)
        return (got[0][i], got[1][i]) if records else got[i]

    def _ensure_index(self, hs):
        """The index of the last run's lists (spx_edit_index), built once per run()."""
        L = self.plan.L
        if self._index_built:
            return
        if self.d_index is None:
            self.d_index = torch.zeros(max(1, self.op_offs[-1]), dtype=torch.int32, device=self.device)
        rc = L.spx_edit_index(self.plan.h, self.jobs, self.n, self.d_ops.data_ptr(), self._ops_cap_ptr(), self.d_nops.data_ptr(),
                              self.d_index.data_ptr(), hs)
        if rc != 0:
            raise RuntimeError("spx_edit_index: " + L.spx_last_error().decode())
        self._index_built = True

    def _rows(self, tracks, hop, phase, blend, unwarp, stream):
        if not self.with_edits:
            raise ValueError("the batch was made without edits=True")
        assert len(tracks) == self.n
        hop = int(hop)
        phase = hop // 2 if phase is None else int(phase)
        ys = [np.ascontiguousarray(y.detach().cpu().numpy() if torch.is_tensor(y) else y) for y in tracks]
        ys = [y.reshape(-1, 1) if y.ndim == 1 else y for y in ys]
        kinds, dims = {y.dtype for y in ys}, {y.shape[1] for y in ys}
        if len(kinds) != 1 or len(dims) != 1 or any(y.ndim != 2 for y in ys):
            raise ValueError("the tracks of one call are (rows, dim) arrays of one dtype and one dim")
        dtype, dim = next(iter(kinds)), int(next(iter(dims)))
        if dtype.itemsize not in (1, 2, 4, 8) or dtype.kind not in "iufb":
            raise ValueError("elements of 1, 2, 4 or 8 bytes, not %s" % dtype)
        if blend and dtype != np.dtype(np.float32):
            raise ValueError("blend=True takes float32 rows, not %s" % dtype)
        L = self.plan.L
        tr = (EditRowsTrack * self.n)()
        in_off = out_off = 0
        for i in range(self.n):
            frames = self._row_limit(i) if unwarp else int(self.out_caps[i])
            cap = L.spx_edit_rows(max(0, frames), hop, phase)
            if cap < 0:
                raise ValueError("spx_edit_rows refuses hop %d, phase %d" % (hop, phase))
            tr[i].in_off, tr[i].out_off, tr[i].n_rows, tr[i].out_cap = in_off, out_off, ys[i].shape[0], cap
            in_off += ys[i].size
            out_off += cap * dim
        bits = np.dtype("u%d" % dtype.itemsize)                  # the rows as bytes: torch has no uint16 / uint64 arithmetic to need
        host = np.zeros(max(1, in_off), bits)
        for i, y in enumerate(ys):
            host[tr[i].in_off:tr[i].in_off + y.size] = y.view(bits).ravel()
        d_y = torch.from_numpy(host.view(np.uint8)).to(self.device)
        d_yout = torch.zeros(max(1, out_off) * dtype.itemsize, dtype=torch.uint8, device=self.device)
        d_count = torch.zeros(self.n, dtype=torch.int64, device=self.device)
        hs = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        if unwarp:
            self._ensure_index(hs)
            rc = L.spx_edit_unwarp_rows(self.plan.h, self.jobs, self.n, self.d_ops.data_ptr(), self._ops_cap_ptr(), self.d_nops.data_ptr(),
                                        self.d_nout.data_ptr(), self.d_index.data_ptr(), tr, hop, phase, dim, dim, dim, dtype.itemsize,
                                        d_y.data_ptr(), d_yout.data_ptr(), d_count.data_ptr(), hs)
        else:
            rc = L.spx_edit_warp_rows(self.plan.h, self.jobs, self.n, self.d_ops.data_ptr(), self._ops_cap_ptr(), self.d_nops.data_ptr(),
                                      self.d_nout.data_ptr(), tr, hop, phase, dim, dim, dim, dtype.itemsize, 1 if blend else 0,
                                      d_y.data_ptr(), d_yout.data_ptr(), d_count.data_ptr(), hs)
        if rc != 0:
            raise RuntimeError("%s: %s" % ("spx_edit_unwarp_rows" if unwarp else "spx_edit_warp_rows", L.spx_last_error().decode()))
        torch.cuda.synchronize(self.device)
        count = d_count.cpu().numpy()
        if (count < 0).any():
            raise RuntimeError("output capacity exceeded for streams %s" % np.nonzero(count < 0)[0][:8])
        out = d_yout.cpu().numpy().view(dtype)
        return [out[tr[i].out_off:tr[i].out_off + int(count[i]) * dim].reshape(-1, dim).copy() for i in range(self.n)]

    def _row_limit(self, i):
        """L of stream i: n_in for a linear job, (n_in // B) * B for a nonlinear one."""
        n_in = int(self.lengths[i])
        return n_in // self.plan.B * self.plan.B if self.jobs[i].nonlinear != 0.0 else n_in

    def warp_rows(self, tracks, hop, phase=None, blend=False, stream=None):
        """spx_edit_warp_rows over the whole batch: tracks[i] = a (rows, dim) numpy array or torch tensor on stream i's INPUT
        timeline, one row per `hop` key frames (labels, flags, features; one dtype of 1, 2, 4 or 8 bytes and one dim per call; a
        1-D array counts as dim 1), brought onto the OUTPUT timeline.  phase: the frame of a row that stands for it, hop // 2 by
        default.  blend=True (float32): a row inside a cross-fade is the cross-fade of its two source rows.  Returns host numpy
        arrays of spx_edit_rows(n_out) rows each."""
        return self._rows(tracks, hop, phase, blend, False, stream)

    def unwarp_rows(self, tracks, hop, phase=None, stream=None):
        """spx_edit_unwarp_rows over the whole batch: tracks[i] on stream i's OUTPUT timeline (what a model computed on the sped-up
        audio) brought back onto the INPUT timeline: spx_edit_rows(L) rows each, nearest row, zeros where nothing at or behind a
        row survives.  The index is built at the first use after a run(), as locate_all builds it."""
        return self._rows(tracks, hop, phase, False, True, stream)

    def tap_arrays(self, i):
        """tension/speed/features rows of stream i (host numpy)."""
        torch.cuda.synchronize(self.device)
        fo, T = self.frame_offs[i], self.frames[i]
        K = max(0, T - self.plan.F + 1)
        r = dict(tension=self.t_tension[fo:fo + K].cpu().numpy(), speed=self.t_speed[fo:fo + K].cpu().numpy(),
                 features=self.t_features[fo * 15:(fo + K) * 15].cpu().numpy().reshape(K, 15))
        if getattr(self, "t_spec", None) is not None:
            N, W = self.plan.N, self.plan.W
            r["spectrogram"] = self.t_spec[fo * N:(fo + T) * N].cpu().numpy().reshape(T, N)
            r["normalized"] = self.t_norm[fo * W:(fo + K) * W].cpu().numpy().reshape(K, W)
        return r


class TwoPassBatch(Batch):
    """Two passes in one call (spx_batch_run_twopass): every stream is probed with a fully nonlinear pass, and the final pass runs
    at a speed the GPU works out from the probe's count -- nothing comes back to the host in between.
    seconds: None or 0 for a stream = MATCH mode, the final pass runs the job (its `nonlinear`, normally 0: the linear control) at
    the speed the nonlinear probe at `speed` achieved (speedy_wave --match_nonlinear); a value > 0 = LENGTH mode, the stream is
    brought to that many seconds (speedy_wave --length) and `speed` is ignored.  One value or one per stream.
    out_caps: output capacities in frames instead of spx_plan_out_capacity_twopass's.
    results() as Batch's; probe_counts() and final_speeds() return what the call measured and decided.  The plain call only."""

    def __init__(self, plan, lengths, channels, speed, nonlinear=1.0, feedback=0.0, device="cuda", taps=False,
                 spectrogram_taps=False, seconds=None, out_caps=None):
        if not torch.cuda.is_available():
            raise RuntimeError("speedy_amd needs a HIP device; there is no CPU path")
        n = len(lengths)
        sec = np.zeros(n, np.float64) if seconds is None else np.broadcast_to(np.asarray(seconds, np.float64), (n,))
        self.seconds = np.ascontiguousarray(sec, np.float64)
        sp = np.broadcast_to(np.asarray(speed, np.float32), (n,))
        # the speed each probe runs at, with the call's own types: (double)((float)T / (float)rate) / seconds, or the job's speed
        self.want = np.array([np.float64(np.float32(int(lengths[i])) / np.float32(plan.sample_rate)) / self.seconds[i]
                              if self.seconds[i] > 0 else np.float64(sp[i]) for i in range(n)], np.float64)
        self._out_caps = None if out_caps is None else np.broadcast_to(np.asarray(out_caps, np.int64), (n,))
        # (the table's speed: what MATCH mode reads; LENGTH mode ignores it)
        super().__init__(plan, lengths, channels, self.want.astype(np.float32), nonlinear, feedback, device, taps, spectrogram_taps)
        self.d_probe = torch.zeros(n, dtype=torch.int64, device=self.device)
        self.d_speeds = torch.zeros(n, dtype=torch.float32, device=self.device)

    def _seconds_ptr(self):
        return self.seconds.ctypes.data_as(C.POINTER(C.c_double))

    def _capacity(self, i, n_in, speed, nonlinear):
        if self._out_caps is not None:
            return int(self._out_caps[i])
        cap = self.plan.L.spx_plan_out_capacity_twopass(self.plan.h, n_in, float(self.want[i]), nonlinear)
        if cap < 0:
            raise RuntimeError("spx_plan_out_capacity_twopass: " + self.plan.L.spx_last_error().decode())
        return cap

    def _workspace_bytes(self):
        wsb = self.plan.L.spx_batch_workspace_bytes_twopass(self.plan.h, self.jobs, self._seconds_ptr(), self.n)
        if wsb == 0:
            raise RuntimeError("spx_batch_workspace_bytes_twopass: " + self.plan.L.spx_last_error().decode())
        return wsb

    def run(self, stream=None):
        """Enqueue both passes and the retarget kernel between them on `stream` (torch stream or None)."""
        hs = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        rc = self.plan.L.spx_batch_run_twopass(self.plan.h, self.jobs, self._seconds_ptr(), self.n, self.d_in.data_ptr(),
                                               self.d_out.data_ptr(), self.d_nout.data_ptr(), self.d_probe.data_ptr(),
                                               self.d_speeds.data_ptr(), self.d_ws.data_ptr(), self.d_ws.numel(),
                                               C.byref(self.taps) if self.taps is not None else None, hs)
        if rc != 0:
            raise RuntimeError("spx_batch_run_twopass: " + self.plan.L.spx_last_error().decode())

    def run_ahead(self, stream=None, in_ready=None, overlap=False):
        raise RuntimeError("a two-pass batch runs through the plain call only (spx_batch_run_twopass)")

    def probe_counts(self):
        """Frames the probe pass produced per stream (host numpy int64; <= 0: nothing to measure); synchronises."""
        torch.cuda.synchronize(self.device)
        return self.d_probe.cpu().numpy().copy()

    def final_speeds(self):
        """The speed the final pass ran at per stream (host numpy float32); synchronises."""
        torch.cuda.synchronize(self.device)
        return self.d_speeds.cpu().numpy().copy()


class FloatBatch(Batch):
    """Batch on FLOAT samples in (-1, 1) (spx_batch_run_float: sonicWriteFloatToStream / sonicReadFloatFromStream for audio that is
    already in device memory).  d_in / d_out are torch.float32 tensors packed like Batch's -- the same job table, offsets in
    float values -- and the int16 work in between is Batch's, bit for bit: the input is scaled per job as the reference scales it
    (nonlinear != 0: x * 32768.0 in double, else x * 32767.0f) and truncated, every output value is an int16 / 32767.0f.
    rate: as Batch has it.  time_map: run() is spx_batch_run_float_map -- time_map(i), lookup_all and lookup as Batch has them, the
    rows in final frames.  The plain call only: no run_ahead, no pack_outputs."""

    def __init__(self, plan, lengths, channels, speed, nonlinear=1.0, feedback=0.0, device="cuda", taps=False,
                 spectrogram_taps=False, rate=None, time_map=False):
        if not torch.cuda.is_available():
            raise RuntimeError("speedy_amd needs a HIP device; there is no CPU path")
        self.plan = plan
        n = len(lengths)
        self.n = n
        self.with_map = bool(time_map)
        self.rates = None
        if rate is not None:
            self.rates = np.ascontiguousarray(np.broadcast_to(np.asarray(rate, np.float32), (n,)))
        ch = np.broadcast_to(np.asarray(channels, np.int32), (n,)).copy()
        sp = np.broadcast_to(np.asarray(speed, np.float32), (n,)).copy()
        nlv = np.broadcast_to(np.asarray(nonlinear, np.float32), (n,)).copy()
        fb = np.broadcast_to(np.asarray(feedback, np.float32), (n,)).copy()
        self.lengths = np.asarray(lengths, np.int64)
        self.channels = ch
        self.jobs = (StreamJob * n)()
        in_off = out_off = fo = 0
        self.in_offs, self.out_offs, self.out_caps, self.frame_offs, self.frames = [], [], [], [], []
        for i in range(n):
            cap = plan.out_capacity(int(self.lengths[i]), float(sp[i]), float(nlv[i]),
                                    None if self.rates is None else float(self.rates[i]))
            j = self.jobs[i]
            j.in_off, j.n_in, j.out_off, j.out_cap = in_off, int(self.lengths[i]), out_off, cap
            j.channels, j.speed, j.nonlinear, j.feedback = int(ch[i]), float(sp[i]), float(nlv[i]), float(fb[i])
            self.in_offs.append(in_off)
            self.out_offs.append(out_off)
            self.out_caps.append(cap)
            T = plan.frames(int(self.lengths[i])) if nlv[i] != 0 else 0
            self.frame_offs.append(fo)
            self.frames.append(T)
            fo += T
            in_off += int(self.lengths[i]) * int(ch[i])
            out_off += cap * int(ch[i])
        self.total_in, self.total_out, self.total_frames = in_off, out_off, fo
        dev = torch.device(device)
        self.device = dev
        self.d_in = torch.zeros(max(1, in_off), dtype=torch.float32, device=dev)   # (no padding: the conversion reads the jobs' values only)
        self.d_out = torch.zeros(max(1, out_off), dtype=torch.float32, device=dev)
        self.d_nout = torch.zeros(n, dtype=torch.int64, device=dev)
        wsb = plan.L.spx_batch_workspace_bytes_float(plan.h, self.jobs, self._rates_ptr(), n)
        if wsb == 0:
            raise RuntimeError("spx_batch_workspace_bytes_float: " + plan.L.spx_last_error().decode())
        self.d_ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
        if self.with_map:
            self._alloc_map(nlv)
        self.taps = None
        if taps:
            T1 = max(1, fo)
            self.t_tension = torch.zeros(T1, dtype=torch.float32, device=dev)
            self.t_speed = torch.zeros(T1, dtype=torch.float32, device=dev)
            self.t_features = torch.zeros(T1 * 15, dtype=torch.float32, device=dev)
            self.taps = Taps(self.t_tension.data_ptr(), self.t_speed.data_ptr(), self.t_features.data_ptr(), None, None)
            if spectrogram_taps:
                self.t_spec = torch.zeros(T1 * plan.N, dtype=torch.float32, device=dev)
                self.t_norm = torch.zeros(T1 * plan.W, dtype=torch.float32, device=dev)
                self.taps.spectrogram = self.t_spec.data_ptr()
                self.taps.normalized = self.t_norm.data_ptr()

    def _rates_ptr(self):
        return None if self.rates is None else self.rates.ctypes.data_as(C.POINTER(C.c_float))

    def upload(self, streams):
        """streams: list of float32 numpy arrays (interleaved).  Packs and copies them to HBM."""
        host = np.zeros(self.d_in.numel(), np.float32)
        for i, x in enumerate(streams):
            x = np.ascontiguousarray(x, np.float32).ravel()
            assert x.size == int(self.lengths[i]) * int(self.channels[i])
            host[self.in_offs[i]:self.in_offs[i] + x.size] = x
        self.d_in.copy_(torch.from_numpy(host))

    def set_input(self, tensor):
        """A float32 CUDA tensor that is already packed (stream i at in_offs[i]) becomes the input: no copy, no padding needed."""
        if not (isinstance(tensor, torch.Tensor) and tensor.is_cuda and tensor.dtype == torch.float32 and tensor.is_contiguous()):
            raise ValueError("set_input: a contiguous float32 CUDA tensor")
        if tensor.device != self.d_in.device or tensor.numel() < self.total_in:
            raise ValueError("set_input: the tensor is on another device or shorter than the batch's %d values" % self.total_in)
        self.d_in = tensor

    def run(self, stream=None):
        """Enqueue input conversion, the int16 call and output conversion on `stream` (torch stream or None)."""
        hs = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        if self.with_map:
            rc = self.plan.L.spx_batch_run_float_map(self.plan.h, self.jobs, self._rates_ptr(), self.n, self.d_in.data_ptr(),
                                                     self.d_out.data_ptr(), self.d_nout.data_ptr(), self.d_map.data_ptr(),
                                                     self.d_ws.data_ptr(), self.d_ws.numel(),
                                                     C.byref(self.taps) if self.taps is not None else None, hs)
            if rc != 0:
                raise RuntimeError("spx_batch_run_float_map: " + self.plan.L.spx_last_error().decode())
            return
        rc = self.plan.L.spx_batch_run_float(self.plan.h, self.jobs, self._rates_ptr(), self.n, self.d_in.data_ptr(),
                                             self.d_out.data_ptr(), self.d_nout.data_ptr(), self.d_ws.data_ptr(),
                                             self.d_ws.numel(), C.byref(self.taps) if self.taps is not None else None, hs)
        if rc != 0:
            raise RuntimeError("spx_batch_run_float: " + self.plan.L.spx_last_error().decode())

    def run_ahead(self, stream=None, in_ready=None, overlap=False):
        raise RuntimeError("a float batch runs through the plain call only (spx_batch_run_float)")

    def pack_outputs(self, stream=None):
        raise RuntimeError("spx_batch_pack_outputs packs int16 outputs; a float batch has none")

    def results(self):
        """Synchronise and return per-stream float32 outputs (host numpy)."""
        torch.cuda.synchronize(self.device)
        nout = self.d_nout.cpu().numpy()
        lost = nout == np.iinfo(np.int64).min   # SPX_NOUT_LOST_PRODUCER
        if lost.any():
            raise RuntimeError("a producer kernel never delivered its frames to streams %s (device-side poll limit)"
                               % np.nonzero(lost)[0][:8])
        if (nout < 0).any():
            raise RuntimeError("output capacity exceeded for streams %s" % np.nonzero(nout < 0)[0][:8])
        return [self.d_out[self.out_offs[i]:self.out_offs[i] + int(nout[i]) * int(self.channels[i])].cpu().numpy().copy()
                for i in range(self.n)]


class MixedBatch:
    """Streams of DIFFERENT sample rates in one call (spx_batch_run_mixed): stream i is served by plans[plan_index[i]].
    Inputs and outputs are packed like Batch's; results() returns the outputs in the order the streams were given."""

    def __init__(self, plans, plan_index, lengths, channels, speed, nonlinear=1.0, feedback=0.0, device="cuda", taps=False):
        n = len(lengths)
        self.plans, self.n = list(plans), n
        self.L = plans[0].L
        self.pidx = [int(v) for v in plan_index]
        self.plan_index = (C.c_int * n)(*self.pidx)
        self.hplans = (C.c_void_p * len(plans))(*[p.h for p in plans])
        ch = np.broadcast_to(np.asarray(channels, np.int32), (n,)).copy()
        sp = np.broadcast_to(np.asarray(speed, np.float32), (n,)).copy()
        nlv = np.broadcast_to(np.asarray(nonlinear, np.float32), (n,)).copy()
        fb = np.broadcast_to(np.asarray(feedback, np.float32), (n,)).copy()
        self.lengths, self.channels = np.asarray(lengths, np.int64), ch
        self.jobs = (StreamJob * n)()
        in_off = out_off = 0
        self.in_offs, self.out_offs, self.frames = [], [], []
        for i in range(n):
            pl = plans[self.pidx[i]]
            cap = pl.out_capacity(int(self.lengths[i]), float(sp[i]), float(nlv[i]))
            j = self.jobs[i]
            j.in_off, j.n_in, j.out_off, j.out_cap = in_off, int(self.lengths[i]), out_off, cap
            j.channels, j.speed, j.nonlinear, j.feedback = int(ch[i]), float(sp[i]), float(nlv[i]), float(fb[i])
            self.in_offs.append(in_off)
            self.out_offs.append(out_off)
            self.frames.append(pl.frames(int(self.lengths[i])) if nlv[i] != 0 else 0)
            in_off += int(self.lengths[i]) * int(ch[i])
            out_off += cap * int(ch[i])
        dev = torch.device(device)
        self.device = dev
        self.total_frames_in = int(self.lengths.sum())
        self.d_in = torch.zeros(max(1, in_off) + 64, dtype=torch.int16, device=dev)
        self.d_out = torch.zeros(max(1, out_off), dtype=torch.int16, device=dev)
        self.d_nout = torch.zeros(n, dtype=torch.int64, device=dev)
        wsb = self.L.spx_batch_workspace_bytes_mixed(self.hplans, len(plans), self.jobs, self.plan_index, n)
        if wsb == 0:
            raise RuntimeError("spx_batch_workspace_bytes_mixed: " + self.L.spx_last_error().decode())
        self.d_ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
        self.taps = None
        if taps:
            # tap rows: streams grouped by plan index, job order inside a group (include/speedy_hip.h)
            self.tap_off = [0] * n
            rows = 0
            for g in range(len(plans)):
                for i in range(n):
                    if self.pidx[i] == g:
                        self.tap_off[i] = rows
                        rows += self.frames[i]
            T1 = max(1, rows)
            self.t_tension = torch.zeros(T1, dtype=torch.float32, device=dev)
            self.t_speed = torch.zeros(T1, dtype=torch.float32, device=dev)
            self.t_features = torch.zeros(T1 * 15, dtype=torch.float32, device=dev)
            self.taps = Taps(self.t_tension.data_ptr(), self.t_speed.data_ptr(), self.t_features.data_ptr(), None, None)

    def upload(self, streams):
        host = np.zeros(self.d_in.numel(), np.int16)
        for i, x in enumerate(streams):
            x = np.ascontiguousarray(x, np.int16).ravel()
            assert x.size == int(self.lengths[i]) * int(self.channels[i])
            host[self.in_offs[i]:self.in_offs[i] + x.size] = x
        self.d_in.copy_(torch.from_numpy(host))

    def run(self, stream=None):
        hs = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        rc = self.L.spx_batch_run_mixed_taps(self.hplans, len(self.plans), self.jobs, self.plan_index, self.n,
                                             self.d_in.data_ptr(), self.d_out.data_ptr(), self.d_nout.data_ptr(),
                                             self.d_ws.data_ptr(), self.d_ws.numel(),
                                             C.byref(self.taps) if self.taps is not None else None, hs)
        if rc != 0:
            raise RuntimeError("spx_batch_run_mixed: " + self.L.spx_last_error().decode())

    def run_ahead(self, stream=None):
        """spx_batch_run_mixed_ahead: like run() (no taps), software-pipelined with the previous call on the same stream (the
        caller alternates two MixedBatch objects over the same plans; inputs are resident when the call is made)."""
        assert self.taps is None
        hs = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        rc = self.L.spx_batch_run_mixed_ahead(self.hplans, len(self.plans), self.jobs, self.plan_index, self.n,
                                              self.d_in.data_ptr(), self.d_out.data_ptr(), self.d_nout.data_ptr(),
                                              self.d_ws.data_ptr(), self.d_ws.numel(), hs)
        if rc != 0:
            raise RuntimeError("spx_batch_run_mixed_ahead: " + self.L.spx_last_error().decode())

    def step_counts(self):
        steps = (C.c_int32 * self.n)()
        torch.cuda.synchronize(self.device)
        rc = self.L.spx_batch_read_steps_mixed(self.hplans, len(self.plans), self.jobs, self.plan_index, self.n,
                                               self.d_ws.data_ptr(), steps, torch.cuda.current_stream(self.device).cuda_stream)
        if rc != 0:
            raise RuntimeError("spx_batch_read_steps_mixed: " + self.L.spx_last_error().decode())
        return np.frombuffer(steps, np.int32).copy()

    def counts(self):
        """Synchronise; produced frames per stream (raises on overflow / a lost producer)."""
        torch.cuda.synchronize(self.device)
        nout = self.d_nout.cpu().numpy()
        if (nout < 0).any():
            raise RuntimeError("output capacity exceeded / lost producer for streams %s" % np.nonzero(nout < 0)[0][:8])
        return nout

    def results(self):
        nout = self.counts()
        out = self.d_out.cpu().numpy()
        return [out[self.out_offs[i]:self.out_offs[i] + int(nout[i]) * int(self.channels[i])].copy() for i in range(self.n)]

    def crcs(self):
        """CRC-32 of every stream's output bytes (what tools/check_scale.py and bench.py compare)."""
        import zlib
        nout = self.counts()
        out = self.d_out.cpu().numpy()
        return [zlib.crc32(out[self.out_offs[i]:self.out_offs[i] + int(nout[i]) * int(self.channels[i])].tobytes())
                for i in range(self.n)]

    def tap_arrays(self, i):
        torch.cuda.synchronize(self.device)
        fo, T = self.tap_off[i], self.frames[i]
        K = max(0, T - self.plans[self.pidx[i]].F + 1)
        return dict(tension=self.t_tension[fo:fo + K].cpu().numpy(), speed=self.t_speed[fo:fo + K].cpu().numpy(),
                    features=self.t_features[fo * 15:(fo + K) * 15].cpu().numpy().reshape(K, 15))


class Pipeline:
    """spx_pipeline (include/speedy_hip.h): batch after batch, host memory to host memory -- the library owns the device buffer
    sets, the pinned output buffers, its streams and events, and overlaps copies in, kernels and copies out of up to `depth`
    batches.  The caller loop of the reference (speedy_wave.cc:154-242: write a chunk, read what is ready) for a caller whose unit
    is a batch of streams.

        pipe = Pipeline(plan, lengths, channels, speed)
        t = pipe.submit(x)            # x: packed int16 input of one batch (numpy / pinned torch tensor; device tensor: device=True)
        outs = pipe.results(t)        # list of per-stream int16 arrays (copies); pipe.wait(t) returns the raw views

    The table given here is the pipeline's CAPACITY and the shape submit() runs; submit_jobs() hands over a batch with its own
    lengths, speeds, nonlinear factors and feedback strengths per lane (spx_pipeline_submit_jobs): lane i takes any job that fits
    what lane i was created with -- for speed >= 1 the capacity is n_in + slack whatever the speed, so lanes created with the
    longest length and nonlinear = 1 take every shorter job at any speed >= 1, linear or nonlinear; a slow-down lane is created
    with the smallest speed it will see.  A length of 0 is an empty lane (a batch with fewer streams than lanes).

        t = pipe.submit_jobs(pipe.pack(xs, lens), lens, speed=speeds)

    plans / plan_index: a batch that mixes sample rates (spx_pipeline_create_mixed); a lane's plan and channel count are fixed.

    float_samples: a pipeline on FLOAT samples in (-1, 1) (SPX_PIPELINE_FLOAT): pack, host_input, submit, submit_jobs, wait and
    results work on float32 -- numpy arrays, pinned torch tensors, CUDA tensors -- with both conversions on the GPU, by FloatBatch's
    rules (the input scale per lane by the nonlinear factor of the batch's job, every output value an int16 / 32767.0f).  A CUDA
    tensor needs numel() >= the batch's extent only: no padding.

    rate: a RATE pipeline (spx_pipeline_create_rate; one plan only): the playback rate (sonicSetRate) every lane is sized for, one
    value or one per lane.  submit() runs the creation table at these rates; table / fits / submit_jobs take rate= for THIS batch
    (None = every rate 1), and a lane takes any rate whose capacity in final frames (Plan.out_capacity(..., rate=)) fits the lane's --
    create a lane with the smallest rate it will see.  Outputs are Batch(..., rate=)'s, byte for byte."""

    def __init__(self, plan, lengths, channels, speed, nonlinear=1.0, feedback=0.0, depth=0, device_out=False, plan_index=None,
                 float_samples=False, rate=None):
        if (float_samples or rate is not None) and not torch.cuda.is_available():
            raise RuntimeError("speedy_amd needs a HIP device; there is no CPU path")
        self.float_samples = bool(float_samples)
        self._np_dt, self._torch_dt, self._c_dt = ((np.float32, torch.float32, C.c_float) if float_samples else
                                                   (np.int16, torch.int16, C.c_int16))
        plans = list(plan) if isinstance(plan, (list, tuple)) else [plan]
        self.plans = plans
        self.L = plans[0].L
        n = len(lengths)
        self.n = n
        ch = np.broadcast_to(np.asarray(channels, np.int32), (n,)).copy()
        sp = np.broadcast_to(np.asarray(speed, np.float32), (n,)).copy()
        nlv = np.broadcast_to(np.asarray(nonlinear, np.float32), (n,)).copy()
        fb = np.broadcast_to(np.asarray(feedback, np.float32), (n,)).copy()
        self.lengths, self.channels = np.asarray(lengths, np.int64), ch
        self.speeds, self.nonlinears, self.feedbacks = sp, nlv, fb   # the creation values: what None means in submit_jobs
        self.jobs = (StreamJob * n)()
        self.in_offs = []
        in_off = 0
        for i in range(n):
            j = self.jobs[i]
            j.in_off, j.n_in, j.out_off, j.out_cap = in_off, int(self.lengths[i]), 0, 0   # (the pipeline lays the outputs out itself)
            j.channels, j.speed, j.nonlinear, j.feedback = int(ch[i]), float(sp[i]), float(nlv[i]), float(fb[i])
            self.in_offs.append(in_off)
            in_off += int(self.lengths[i]) * int(ch[i])
        self.total_in = in_off
        self.device_out = bool(device_out)
        flags = (1 if device_out else 0) | (2 if float_samples else 0)   # SPX_PIPELINE_DEVICE_OUT | SPX_PIPELINE_FLOAT
        self.rates = None
        if rate is not None:
            if plan_index is not None or len(plans) != 1:
                raise ValueError("a rate pipeline has one plan (spx_pipeline_create_rate has no mixed-sample-rate form)")
            self.rates = np.ascontiguousarray(np.broadcast_to(np.asarray(rate, np.float32), (n,)))
            self.h = self.L.spx_pipeline_create_rate(plans[0].h, self.jobs, self.rates.ctypes.data_as(C.POINTER(C.c_float)), n,
                                                     int(depth), flags)
        elif plan_index is None and len(plans) == 1:
            self.h = self.L.spx_pipeline_create(plans[0].h, self.jobs, n, int(depth), flags)
        else:
            self._pidx = (C.c_int * n)(*[int(v) for v in (plan_index if plan_index is not None else [0] * n)])
            self._hplans = (C.c_void_p * len(plans))(*[p.h for p in plans])
            self.h = self.L.spx_pipeline_create_mixed(self._hplans, len(plans), self.jobs, self._pidx, n, int(depth), flags)
        if not self.h:
            raise RuntimeError("spx_pipeline_create: " + self.L.spx_last_error().decode())
        self.depth = self.L.spx_pipeline_depth(self.h)
        assert self.L.spx_pipeline_input_values(self.h) == self.total_in or n == 0
        self._keep = {}   # ticket -> the input object (host memory must stay alive until its copy has been made)

    def pack(self, streams, lengths=None):
        """One batch's input as the pipeline expects it: the streams (int16 numpy arrays, interleaved; float32 on a float pipeline)
        each at its lane's offset.  lengths: this batch's frames per lane (submit_jobs) -- shorter streams start where the lane starts."""
        lengths = self.lengths if lengths is None else lengths
        host = np.zeros(self.total_in, self._np_dt)
        for i, x in enumerate(streams):
            x = np.ascontiguousarray(x, self._np_dt).ravel()
            assert x.size == int(lengths[i]) * int(self.channels[i]) <= int(self.lengths[i]) * int(self.channels[i])
            host[self.in_offs[i]:self.in_offs[i] + x.size] = x
        return host

    def host_input(self):
        """The pinned staging buffer of the NEXT submit as an int16 (float32) numpy view (fill it, then submit(it))."""
        ptr = (self.L.spx_pipeline_host_input_float if self.float_samples else self.L.spx_pipeline_host_input)(self.h)
        if not ptr:
            raise RuntimeError("spx_pipeline_host_input: " + self.L.spx_last_error().decode())
        return np.ctypeslib.as_array((self._c_dt * self.total_in).from_address(ptr))

    def _input_ptr(self, x, extent):
        if isinstance(x, torch.Tensor):
            assert x.dtype == self._torch_dt and x.is_contiguous() and x.numel() >= extent
            # (include/speedy_hip.h: an int16 device input is used in place and must be allocated 64 values past the last stream's end;
            # a float one is read by the conversion, exactly over the jobs' values)
            if not self.float_samples and x.is_cuda and x.numel() < self.total_in + 64:
                raise ValueError("device input: allocate spx_pipeline_input_values() + 64 int16 values (%d), not %d"
                                 % (self.total_in + 64, x.numel()))
            return x, x.data_ptr(), x.is_cuda
        x = np.ascontiguousarray(x, self._np_dt)
        assert x.size >= extent
        return x, x.ctypes.data, False

    def _ticket(self, t, x, call):
        if t < 0:
            raise RuntimeError(call + ": " + self.L.spx_last_error().decode())
        self._keep[t] = x
        self._keep.pop(t - 2 * self.depth, None)
        return t

    def submit(self, x, device=False):
        x, ptr, dev = self._input_ptr(x, self.total_in)
        device = dev if isinstance(x, torch.Tensor) else device
        call = self.L.spx_pipeline_submit_float if self.float_samples else self.L.spx_pipeline_submit
        return self._ticket(call(self.h, ptr, 1 if device else 0), x, "spx_pipeline_submit")

    def _rates(self, rate):
        """This batch's rates as (float32 array kept alive by the caller, pointer), or (None, None)."""
        if rate is None:
            return None, None
        if self.rates is None:
            raise RuntimeError("the pipeline takes no playback rates: create it with rate= (spx_pipeline_create_rate)")
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(rate, np.float32), (self.n,)))
        return r, r.ctypes.data_as(C.POINTER(C.c_float))

    def table(self, lengths, speed=None, nonlinear=None, feedback=None, in_offs=None, rate=None):
        """The job table of one batch (spx_stream_job[n], host): None = the value the lane was created with.  With rate= (a rate
        pipeline): the pair (table, float32 rates) the _rate calls take."""
        if rate is not None:
            return self.table(lengths, speed, nonlinear, feedback, in_offs), self._rates(rate)[0]
        n = self.n
        assert len(lengths) == n
        sp = self.speeds if speed is None else np.broadcast_to(np.asarray(speed, np.float32), (n,))
        nlv = self.nonlinears if nonlinear is None else np.broadcast_to(np.asarray(nonlinear, np.float32), (n,))
        fb = self.feedbacks if feedback is None else np.broadcast_to(np.asarray(feedback, np.float32), (n,))
        offs = self.in_offs if in_offs is None else in_offs
        jobs = (StreamJob * n)()
        for i in range(n):
            j = jobs[i]
            j.in_off, j.n_in, j.out_off, j.out_cap = int(offs[i]), int(lengths[i]), 0, 0   # (the outputs stay where creation put them)
            j.channels, j.speed, j.nonlinear, j.feedback = int(self.channels[i]), float(sp[i]), float(nlv[i]), float(fb[i])
        return jobs

    def fits(self, lengths, speed=None, nonlinear=None, feedback=None, in_offs=None, rate=None):
        """Would submit_jobs accept this batch?  (spx_pipeline_jobs_fit / _fit_rate: enqueues nothing, waits for nothing.)"""
        jobs = self.table(lengths, speed, nonlinear, feedback, in_offs)
        if rate is None:
            return self.L.spx_pipeline_jobs_fit(self.h, jobs) == 0
        _keep, rp = self._rates(rate)
        return self.L.spx_pipeline_jobs_fit_rate(self.h, jobs, rp) == 0

    def submit_jobs(self, x, lengths, speed=None, nonlinear=None, feedback=None, in_offs=None, device=False, rate=None):
        """submit() with THIS batch's lengths, speeds, nonlinear factors, feedback strengths and input offsets per lane (None = the
        creation value) -- and, on a rate pipeline, playback rates (rate=: one value or one per lane; None = every rate 1).
        A host input need only reach this batch's extent: max over lanes of in_off + length * channels.
        RuntimeError with the library's text (the lane and the limit) for a batch that does not fit the pipeline."""
        jobs = self.table(lengths, speed, nonlinear, feedback, in_offs)
        # (at most the pipeline's input: a table that ends behind it is the library's to refuse, not an assertion's)
        extent = min(self.total_in, max(int(j.in_off) + int(j.n_in) * int(j.channels) for j in jobs))
        x, ptr, dev = self._input_ptr(x, extent)
        device = dev if isinstance(x, torch.Tensor) else device
        if rate is not None:
            _keep, rp = self._rates(rate)   # (read before the call returns)
            call = self.L.spx_pipeline_submit_jobs_rate_float if self.float_samples else self.L.spx_pipeline_submit_jobs_rate
            return self._ticket(call(self.h, jobs, rp, ptr, 1 if device else 0), x, "spx_pipeline_submit_jobs_rate")
        call = self.L.spx_pipeline_submit_jobs_float if self.float_samples else self.L.spx_pipeline_submit_jobs
        return self._ticket(call(self.h, jobs, ptr, 1 if device else 0), x, "spx_pipeline_submit_jobs")

    def input_consumed(self, ticket):
        """Blocks until the input handed over with `ticket` may be overwritten (host input: copied in; device input: batch done;
        a float pipeline's input of either kind: converted)."""
        if self.L.spx_pipeline_input_consumed(self.h, int(ticket)) != 0:
            raise RuntimeError("spx_pipeline_input_consumed: " + self.L.spx_last_error().decode())

    def wait(self, ticket):
        """(out, offsets, counts) of a batch: numpy views of the pipeline's pinned host buffers -- device_out: (data pointer of the
        int16 output in device memory, offsets as a numpy array, data pointer of the int64 counts in device memory).  A float
        pipeline: float32 in place of int16, the same offsets and counts."""
        o, f, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        call = self.L.spx_pipeline_wait_float if self.float_samples else self.L.spx_pipeline_wait
        rc = call(self.h, int(ticket), C.byref(o), C.byref(f), C.byref(c))
        if rc != 0:
            raise RuntimeError("spx_pipeline_wait: " + self.L.spx_last_error().decode())
        offsets = np.ctypeslib.as_array((C.c_int64 * (self.n + 1)).from_address(f.value))
        if self.device_out:
            return o.value, offsets, c.value
        counts = np.ctypeslib.as_array((C.c_int64 * self.n).from_address(c.value))
        out = np.ctypeslib.as_array((self._c_dt * max(1, int(offsets[self.n]))).from_address(o.value))
        return out, offsets, counts

    def results(self, ticket):
        """Per-stream int16 (float32) outputs of a batch (copies; raises on overflow / a lost producer)."""
        out, offsets, counts = self.wait(ticket)
        if self.device_out:
            cnt = torch.empty(self.n, dtype=torch.int64)
            self.L.spx_copy_to_host(cnt.data_ptr(), counts, self.n * 8, None)
            self.L.spx_stream_synchronize(None)
            counts = cnt.numpy()
            total = int(offsets[self.n])
            host = torch.empty(total, dtype=self._torch_dt)
            self.L.spx_copy_to_host(host.data_ptr(), out, total * host.element_size(), None)
            self.L.spx_stream_synchronize(None)
            out = host.numpy()
        if (counts < 0).any():
            raise RuntimeError("output capacity exceeded / lost producer for streams %s" % np.nonzero(counts < 0)[0][:8])
        return [out[int(offsets[i]):int(offsets[i]) + int(counts[i]) * int(self.channels[i])].copy() for i in range(self.n)]

    def close(self):
        if self.h:
            self.L.spx_pipeline_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def compress_batch(streams, sample_rate, channels, speed, nonlinear=1.0, feedback=0.0, match_matlab=False,
                   taps=False, spectrogram_taps=False, rate=None):
    """One-call convenience: returns (list of outputs, Batch).  rate: sonicSetRate, one value or one per stream."""
    plan = Plan(sample_rate, match_matlab)
    ch = np.broadcast_to(np.asarray(channels, np.int32), (len(streams),))
    lengths = [np.asarray(x).size // int(c) for x, c in zip(streams, ch)]
    b = Batch(plan, lengths, channels, speed, nonlinear, feedback, taps=taps, spectrogram_taps=spectrogram_taps, rate=rate)
    b.upload(streams)
    b.run()
    return b.results(), b


def compress_batch_float(streams, sample_rate, channels, speed, nonlinear=1.0, feedback=0.0, match_matlab=False,
                         taps=False, spectrogram_taps=False, rate=None):
    """compress_batch on float32 streams in (-1, 1): returns (list of float32 outputs, FloatBatch)."""
    plan = Plan(sample_rate, match_matlab)
    ch = np.broadcast_to(np.asarray(channels, np.int32), (len(streams),))
    lengths = [np.asarray(x).size // int(c) for x, c in zip(streams, ch)]
    b = FloatBatch(plan, lengths, channels, speed, nonlinear, feedback, taps=taps, spectrogram_taps=spectrogram_taps, rate=rate)
    b.upload(streams)
    b.run()
    return b.results(), b


def compress_batch_to_length(streams, sample_rate, channels, seconds, nonlinear=1.0, feedback=0.0, match_matlab=False,
                             taps=False, spectrogram_taps=False):
    """Every stream to `seconds` of audio (one value or one per stream), two passes in one call: returns (list of outputs,
    TwoPassBatch).  The lengths land as near the target as speedy_wave --length brings them: one correction step."""
    plan = Plan(sample_rate, match_matlab)
    ch = np.broadcast_to(np.asarray(channels, np.int32), (len(streams),))
    lengths = [np.asarray(x).size // int(c) for x, c in zip(streams, ch)]
    b = TwoPassBatch(plan, lengths, channels, 1.0, nonlinear, feedback, taps=taps, spectrogram_taps=spectrogram_taps, seconds=seconds)
    b.upload(streams)
    b.run()
    return b.results(), b
