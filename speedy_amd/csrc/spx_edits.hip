// Edit list of a batch call (include/speedy_hip.h "EDIT LIST": spx_plan_edit_ops, spx_batch_run_edits, spx_edit_replay): the exact
// list of copy and cross-fade operations a job performed, and its replay on any other track of the same length.
//
// The records come from the general walk kernel's recording instantiation (spx_walk.hip, spx_walk_edits_kernel: record_op, one
// 16-byte store per emit_copy / emit_overlap_add).  spx_batch_run_edits is spx_batch_run with SpxCallOpts::edits set (run_impl: the
// whole batch on the general kernel, kernels in sequence on the caller's stream, as a map call).
//
// The replay is spx_edit_replay.h's kernel and host routine with the identity scale on int16 tracks: the body
// spx_edit_replay_scaled (spx_edit_scaled.hip) runs with a ratio, with everything of a master compiled out.
#include "spx_edit_replay.h"

static std::atomic<int> g_last_replay_gx{0}, g_last_replay_launches{0};   // spx_debug_last_replay_grid

// Records a job can need (spx_plan_edit_ops), from the loop of tsm_process (spx_walk.hip) for a job none of whose steps fails.
// The time-scale stage is handed In = L + 2 maxRequired frames, the flush's padding included, in `events` process calls (a linear
// job: the write and the flush; a nonlinear one: one per complete ring buffer and the flush).  Every pass of the loop is
//   a speed-up step    one cross-fade; consumes period + n >= minPeriod input frames        -> at most In / minPeriod of them
//   a slow-down step   a copy and a cross-fade; emits period + n >= minPeriod output frames -> at most Out / minPeriod of them, Out =
//                      the frames the stage can emit before the flush's cut (spx_plan_out_capacity_for); a step at speed >= 0.5
//                      also consumes n = period >= minPeriod input frames                   -> and at most In / minPeriod
//   a piece of `remaining`   one copy; a piece is maxRequired frames of input unless it is the last of its step's
//                                                                                           -> at most steps + In / maxRequired
// and a process call at unity is one copy of everything pending                             -> at most `events`.
// Slow-down steps are counted unless the job can have none: speed > 1 and 0 <= nonlinear <= 1, the class whose time-scale stage
// never sees a speed below 1 (speed_class).
static int64_t edit_ops_bound(const SpxPlanDev& d, int64_t n_in, float speed, float nonlinear) {
  const bool nl = nonlinear != 0.0f;
  const int64_t events = (nl ? n_in / d.B : 1) + 1;
  const int64_t In = (nl ? n_in / d.B * d.B : n_in) + 2 * (int64_t)d.maxRequired;
  const bool up_only = speed > 1.0f && nonlinear >= 0.0f && nonlinear <= 1.0f;
  const bool down_only = !nl && speed < 1.0f;
  const int64_t up = down_only ? 0 : In / d.minPeriod + 1;
  int64_t down = 0;
  if (!up_only) {
    down = spx_internal_out_bound(d, n_in, speed, nl) / d.minPeriod + 1;
    if (!nl && speed >= 0.5f && down > In / d.minPeriod + 1) down = In / d.minPeriod + 1;
  }
  return up + 2 * down + (up + down) + In / d.maxRequired + 1 + events;
}

extern "C" {

int spx_debug_last_replay_grid(int* launches) {
  if (launches) *launches = g_last_replay_launches.load(std::memory_order_relaxed);
  return g_last_replay_gx.load(std::memory_order_relaxed);
}

int64_t spx_plan_edit_ops(spx_plan_t plan, int64_t n_in, float speed, float nonlinear) {
  if (!plan) { fail(-1, "spx_batch: bad arguments"); return -1; }
  spx_stream_job j;
  memset(&j, 0, sizeof(j));
  j.n_in = n_in; j.channels = 1; j.speed = speed; j.nonlinear = nonlinear;
  const SpxJobFault f = spx_check_job(spx_job_limits(plan), j);
  if (f != SPX_JOB_OK) { fail(-1, std::string("spx_batch: ") + spx_job_fault_text(f)); return -1; }
  return edit_ops_bound(plan->dev, n_in, speed, nonlinear);
}

int spx_batch_run_edits(spx_plan_t plan, const spx_stream_job* jobs, int n, const int16_t* in, int16_t* out, int64_t* n_out,
                        spx_edit_op* ops, const int64_t* ops_cap, int64_t* n_ops, void* ws, size_t ws_bytes, const spx_taps* taps,
                        void* hs) {
  // what spx_batch_run refuses, with its messages, before anything else is looked at
  if (spx_check_jobs(plan, jobs, n, true)) return -1;
  if (!ops || !ops_cap || !n_ops) return fail(-1, "spx_batch_run_edits: ops, ops_cap or n_ops is NULL");
  if (reinterpret_cast<uintptr_t>(ops) & 15) return fail(-1, "spx_batch_run_edits: ops is not aligned to 16 bytes");
  if (!in || !out || !n_out) return fail(-1, "spx_batch_run_edits: bad arguments");
  int64_t total = 0;
  for (int i = 0; i < n; i++) {
    if (ops_cap[i] < 0) return fail(-1, "spx_batch_run_edits: a negative capacity");
    if (ops_cap[i] > 0x7fffffff || (total += ops_cap[i]) > 0x7fffffff)
      return fail(-1, "spx_batch_run_edits: more than 2^31 - 1 records of capacity in one call");
  }
  const SpxEditsCall e = {ops, ops_cap, n_ops, total};
  SpxCallOpts o;
  o.edits = &e;
  return run_impl({plan, jobs, n, in, out, n_out, ws, ws_bytes, taps, hs}, o);
}

int spx_edit_replay(spx_plan_t plan, const spx_stream_job* jobs, int n, const spx_edit_op* ops, const int64_t* ops_cap,
                    const int64_t* n_ops, const int64_t* n_out, const spx_edit_track* tracks, const int16_t* y_in, int16_t* y_out,
                    void* hs) {
  if (spx_check_jobs(plan, jobs, n, true)) return -1;
  if (!ops || !ops_cap || !n_ops || !n_out || !tracks || !y_in || !y_out) return fail(-1, "spx_edit_replay: a NULL pointer");
  if ((reinterpret_cast<uintptr_t>(ops) & 15) || (reinterpret_cast<uintptr_t>(y_out) & 1) || (reinterpret_cast<uintptr_t>(y_in) & 1))
    return fail(-1, "spx_edit_replay: ops is not aligned to 16 bytes, or a track buffer not to 2");
  return edit_replay_run(
      "spx_edit_replay", plan, jobs, n, ops_cap, hs, g_last_replay_gx, g_last_replay_launches,
      [&](int i) { return SpxEditTrackDesc{tracks[i].in_off, tracks[i].out_off, 0, 0, tracks[i].channels}; },
      [](int, int64_t key_frames, int64_t) { return key_frames; },
      [&](dim3 grid, const SpxEditStream* tab, int s0, hipStream_t st) {
        hipLaunchKernelGGL((spx_edit_replay_kernel<EditInt16, EditIdentity>), grid, dim3(SPX_EDIT_THREADS), 0, st, tab, s0,
                           reinterpret_cast<const int4*>(ops), n_ops, n_out, 1, 1, y_in, y_out, static_cast<int64_t*>(nullptr));
      });
}

}  // extern "C"
