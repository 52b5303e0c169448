// Two passes, one call (include/speedy_hip.h: spx_batch_run_twopass): the two-pass drivers of the reference's CLI
// (speedy_wave.cc:424-462, here tools/speedy_wave_hip.cpp:179-191) for a whole batch, without a host wait in between.
//   pass 1  a plain spx_batch_run of the PROBE table -- every job at (float)want, fully nonlinear -- with the counts in n_probe;
//   pass 2  the job table as given, at speeds the HOST never sees: spx_retarget_kernel (below), launched right behind the second
//           pass's staging kernel, reads n_probe, evaluates spx_twopass.h's formula and patches the speed into every staged
//           SpxStreamDev record (run_impl, SpxCallOpts::retarget: kernels in sequence on the caller's stream, any-speed walk forms).
// The analysis does not depend on the speed: where every final job is nonlinear the two tables have the same workspace layout, and
// pass 2 runs without an analysis launch on the SpxFrameRec records pass 1 left behind (spx_debug_last_twopass bit 0).
// The device code here is a code object of its own (last in the Makefile's SRC): the hot object stays what it was.
#include "spx_engine.h"
#include "spx_twopass.h"

static_assert(sizeof(SpxRetargetJob) == 24 && sizeof(SpxRetargetJob) % sizeof(int) == 0, "the staging kernel copies 32-bit words");

// One thread per stream: the second-pass speed from the probe's count, to the caller's `speeds` and into all `copies` records of the
// stream (a call cut into time chunks has one record per chunk and stream, chunk-major).  Plain vector stores.
__global__ void __launch_bounds__(256)
spx_retarget_kernel(const SpxRetargetJob* __restrict__ tab, int n, int copies, const int64_t* __restrict__ n_probe,
                    float* __restrict__ speeds, SpxStreamDev* __restrict__ streams) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const SpxRetargetJob J = tab[i];
  const float v = spx_twopass_speed(J.want, J.length_mode, J.n_in, n_probe[i]);
  speeds[i] = v;
  for (int c = 0; c < copies; c++) streams[(size_t)c * n + i].speed = v;
}
void spx_launch_retarget(const void* d_table, int n, int copies, const int64_t* n_probe, float* speeds, SpxStreamDev* streams, hipStream_t st) {
  hipLaunchKernelGGL(spx_retarget_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, static_cast<const SpxRetargetJob*>(d_table), n,
                     copies, n_probe, speeds, streams);
}

static std::atomic<int> g_last_twopass{0};

// What a two-pass call is made of, from its arguments: `want` per stream, the probe table, the final table with its placeholder
// speeds, the retarget records.  0, or -1 with spx_last_error: every rule of the call that needs no workspace, in the header's order.
struct TwoPassTables {
  std::vector<spx_stream_job> probe, fin;
  std::vector<SpxRetargetJob> rt;
};
static int twopass_tables(spx_plan_t plan, const spx_stream_job* jobs, const double* seconds, int n, TwoPassTables& TT) {
  if (!plan || !jobs || n <= 0) return fail(-1, "spx_batch: bad arguments");
  TT.probe.assign(jobs, jobs + n);
  TT.fin.assign(jobs, jobs + n);
  TT.rt.resize((size_t)n);
  memset(TT.rt.data(), 0, sizeof(SpxRetargetJob) * (size_t)n);
  for (int i = 0; i < n; i++) {
    const double sec = seconds ? seconds[i] : 0.0;
    if (!(sec >= 0.0) || !std::isfinite(sec)) return fail(-1, "spx_batch_run_twopass: seconds must be finite and >= 0 (0 = match mode)");
    const bool length_mode = sec > 0.0;
    // (the driver's types: total frames and the sample rate as floats, their quotient widened, a double division)
    const double want = length_mode ? (double)((float)jobs[i].n_in / (float)plan->dev.rate) / sec : (double)jobs[i].speed;
    const float wf = (float)want;
    if (!(wf > 0.0f) || !std::isfinite(wf)) return fail(-1, "spx_batch_run_twopass: the probe speed must be finite and > 0");
    TT.probe[i].speed = wf; TT.probe[i].nonlinear = 1.0f;
    TT.fin[i].speed = wf;   // a placeholder: the device writes the speed (it decides nothing on the host)
    TT.rt[i].want = want; TT.rt[i].n_in = jobs[i].n_in; TT.rt[i].length_mode = length_mode ? 1 : 0;
  }
  if (spx_check_jobs(plan, TT.probe.data(), n)) return -1;
  if (spx_check_jobs(plan, TT.fin.data(), n, false, false, true)) return -1;
  // Every speed the device can compute stays below SPX_FAST_MAX_SPEED, the range the any-speed walk forms serve: with a count
  // 1 <= n_probe <= out_cap (a larger one comes back negative) match mode gives T / n_probe and length mode want^2 n_probe / T, and
  // a probe at speed want emits about T / want frames.  want^2 (out_cap + 1) bounds both with room to spare.
  for (int i = 0; i < n; i++)
    if (!(TT.rt[i].want * TT.rt[i].want * ((double)jobs[i].out_cap + 1.0) < (double)SPX_FAST_MAX_SPEED))
      return fail(-1, "spx_batch_run_twopass: probe speed and capacity too large (want * want * (out_cap + 1) >= 1e18)");
  return 0;
}
// workspace: the probe table's plain workspace | SpxRetargetJob[n]
static size_t twopass_workspace(spx_plan_t plan, const TwoPassTables& TT, int n, size_t* off_table) {
  SpxCarve ws(spx_batch_workspace_bytes(plan, TT.probe.data(), n));
  *off_table = ws.take(sizeof(SpxRetargetJob) * (size_t)n);
  return ws.o;
}

extern "C" {

size_t spx_batch_workspace_bytes_twopass(spx_plan_t plan, const spx_stream_job* jobs, const double* seconds, int n_streams) {
  TwoPassTables TT;
  if (twopass_tables(plan, jobs, seconds, n_streams, TT)) return 0;
  size_t off = 0;
  return twopass_workspace(plan, TT, n_streams, &off);
}

int64_t spx_plan_out_capacity_twopass(spx_plan_t plan, int64_t n_in, double want, float nonlinear) {
  if (!plan) { fail(-1, "spx_plan_out_capacity_twopass: bad arguments"); return -1; }
  const float wf = (float)want;
  const SpxJobFault f = spx_check_job(spx_job_limits(plan), {0, n_in, 0, 0, 1, wf, nonlinear, 0.0f});
  if (f != SPX_JOB_OK) return fail(-1, std::string("spx_batch: ") + spx_job_fault_text(f));
  return std::max(spx_internal_out_bound(plan->dev, n_in, wf, true), spx_internal_out_bound(plan->dev, n_in, wf, nonlinear != 0.0f));
}

int spx_batch_run_twopass(spx_plan_t plan, const spx_stream_job* jobs, const double* seconds, int n, const int16_t* in, int16_t* out,
                          int64_t* n_out, int64_t* n_probe, float* speeds, void* ws, size_t ws_bytes, const spx_taps* taps, void* hs) {
  // everything that can be refused, before anything is enqueued
  TwoPassTables TT;
  if (twopass_tables(plan, jobs, seconds, n, TT)) return -1;
  if (!n_probe || !speeds) return fail(-1, "spx_batch_run_twopass: n_probe or speeds is NULL");
  if (!in || !out || !n_out) return fail(-1, "spx_batch_run_twopass: bad arguments");
  size_t off_table = 0;
  const size_t need = twopass_workspace(plan, TT, n, &off_table);
  if (!ws || ws_bytes < need) return fail(-1, "spx_batch_run_twopass: workspace too small (spx_batch_workspace_bytes_twopass)");
  // Reuse of the first pass's analysis: every final job nonlinear, so that both tables count the same frames per stream -- the
  // two layouts are then the same (asserted here, not assumed: a layout rule that comes to depend on more falls back)
  bool reuse = true;
  for (int i = 0; i < n; i++) reuse = reuse && jobs[i].nonlinear != 0.0f;
  if (reuse) {
    const Layout A = layout_for(plan->dev, TT.probe.data(), n), B = layout_for(plan->dev, TT.fin.data(), n);
    reuse = A.total == B.total && A.total_frames == B.total_frames && A.off_streams == B.off_streams && A.off_states == B.off_states &&
            A.off_rec == B.off_rec && A.off_scratch == B.off_scratch;
  }
  // pass 1: a plain call on the probe table (with the caller's taps only where pass 2 will not write the spectrum rows itself)
  int rc = spx_batch_run(plan, TT.probe.data(), n, in, out, n_probe, ws, ws_bytes, reuse ? taps : nullptr, hs);
  if (rc) return rc;
  // pass 2: the final table, its speeds from the device
  SpxRetargetCall RT;
  RT.table.resize(sizeof(SpxRetargetJob) / sizeof(int) * (size_t)n);
  memcpy(RT.table.data(), TT.rt.data(), sizeof(SpxRetargetJob) * (size_t)n);
  RT.d_table = static_cast<unsigned char*>(ws) + off_table;
  RT.n_probe = n_probe;
  RT.speeds = speeds;
  SpxCallOpts o;
  o.retarget = &RT;
  o.do_a = !reuse;
  rc = run_impl({plan, TT.fin.data(), n, in, out, n_out, ws, ws_bytes, taps, hs}, o);
  if (rc) return rc;
  g_last_twopass.store(reuse ? 1 : 0, std::memory_order_relaxed);
  return 0;
}

int spx_debug_last_twopass(void) { return g_last_twopass.load(std::memory_order_relaxed); }

}  // extern "C"
