// Host-only build of the launch-mode decision (spx_mode.h) for tests/test_mode_table.py, of the job rules (spx_jobs.h) for
// tests/test_job_rules.py, of the two-pass call's speed formula (spx_twopass.h) for tests/test_twopass_abi.py and of the frame-rate
// feature chain (spx_frame_math.h) for tests/test_frame_math.py: plain g++ (-ffp-contract=off: no fused multiply-add), no HIP.  The mode query and its answer are flat arrays of 64-bit integers so that the Python
// side mirrors them by NAME (the two name lists below are exported).
#include <string.h>

#include "spx_frame_math.h"
#include "spx_jobs.h"
#include "spx_mode.h"
#include "spx_twopass.h"

#define SPX_Q_FIELDS(X)                                                                                                         \
  X(n) X(max_channels) X(do_a) X(do_w) X(has_frames) X(forced) X(force_concurrent) X(force_ahead) X(force_total_streams)        \
  X(ahead_req) X(overlap_req) X(cu_count) X(lds_per_cu) X(walk_lds) X(walk_waves) X(walk_vgprs) X(walk_fast) X(walk_nwc)        \
  X(lean_lds) X(lean_waves) X(lean_vgprs) X(lean_fast) X(lean_nwc) X(lean_valid) X(tension_lds) X(tension_vgprs)                \
  X(tile_default) X(tile_big) X(tile_small) X(an_lds_default) X(an_lds_small) X(an_vgprs_default) X(an_vgprs_small)             \
  X(concurrent_enabled) X(chunks_set) X(chunks) X(trial_state_key) X(trial_calls) X(trial_choice) X(two_workspaces)            \
  X(guard_busy) X(trial_times_ready) X(us_seq) X(us_con) X(trial_key) X(device_ours)
#define SPX_A_FIELDS(X)                                                                                                         \
  X(lean_walk) X(launch_lean) X(tile_frames) X(co_resident) X(doubtful) X(trial_slot) X(want_concurrent) X(concurrent)          \
  X(ahead) X(seq_ahead) X(ahead_forced) X(walk2) X(nch) X(exclusive_cu) X(asked_device) X(next_key) X(next_calls) X(next_choice)

enum {
#define X(f) Q_##f,
  SPX_Q_FIELDS(X)
#undef X
  Q_COUNT
};
enum {
#define X(f) A_##f,
  SPX_A_FIELDS(X)
#undef X
  A_COUNT
};

static bool ours_cb(void* ctx) { return *static_cast<long long*>(ctx) != 0; }

extern "C" {
const char* spx_mode_table_query_fields(void) {
  return
#define X(f) #f " "
      SPX_Q_FIELDS(X)
#undef X
      ;
}
const char* spx_mode_table_answer_fields(void) {
  return
#define X(f) #f " "
      SPX_A_FIELDS(X)
#undef X
      ;
}
int spx_mode_table_eval(const long long* q, int nq, long long* a, int na) {
  if (nq != Q_COUNT || na != A_COUNT) return -1;
  SpxModeShape S;
  SpxModeResources R;
  SpxModeEnv E;
  SpxModeRuntime T;
  memset(&S, 0, sizeof(S)); memset(&R, 0, sizeof(R)); memset(&E, 0, sizeof(E)); memset(&T, 0, sizeof(T));
  S.n = (int)q[Q_n]; S.max_channels = (int)q[Q_max_channels]; S.do_a = q[Q_do_a]; S.do_w = q[Q_do_w]; S.has_frames = q[Q_has_frames];
  S.forced = q[Q_forced]; S.force_concurrent = q[Q_force_concurrent]; S.force_ahead = q[Q_force_ahead];
  S.force_total_streams = (int)q[Q_force_total_streams]; S.ahead_req = q[Q_ahead_req]; S.overlap_req = q[Q_overlap_req];
  R.cu_count = (int)q[Q_cu_count]; R.lds_per_cu = (size_t)q[Q_lds_per_cu];
  R.walk = {(size_t)q[Q_walk_lds], (int)q[Q_walk_waves], (int)q[Q_walk_vgprs], q[Q_walk_fast] != 0, (int)q[Q_walk_nwc]};
  R.walk_lean = {(size_t)q[Q_lean_lds], (int)q[Q_lean_waves], (int)q[Q_lean_vgprs], q[Q_lean_fast] != 0, (int)q[Q_lean_nwc]};
  R.lean_valid = q[Q_lean_valid];
  R.tension_lds = (size_t)q[Q_tension_lds]; R.tension_vgprs = (int)q[Q_tension_vgprs];
  R.tile_default = (int)q[Q_tile_default]; R.tile_big = (int)q[Q_tile_big]; R.tile_small = (int)q[Q_tile_small];
  R.an_lds_default = (size_t)q[Q_an_lds_default]; R.an_lds_small = (size_t)q[Q_an_lds_small];
  R.an_vgprs_default = (int)q[Q_an_vgprs_default]; R.an_vgprs_small = (int)q[Q_an_vgprs_small];
  E.concurrent_enabled = q[Q_concurrent_enabled]; E.chunks_set = q[Q_chunks_set]; E.chunks = (int)q[Q_chunks];
  const SpxModeTrial trial = {q[Q_trial_state_key], (int)q[Q_trial_calls], (int)q[Q_trial_choice]};
  T.two_workspaces = q[Q_two_workspaces]; T.guard_busy = q[Q_guard_busy]; T.trial_times_ready = q[Q_trial_times_ready];
  T.ms_seq = (float)q[Q_us_seq] / 1000.0f; T.ms_con = (float)q[Q_us_con] / 1000.0f; T.trial_key = q[Q_trial_key];
  long long ours = q[Q_device_ours];
  T.device_ours = ours_cb; T.device_ctx = &ours;
  const SpxMode M = spx_choose_mode(S, R, E, T, trial);
  a[A_lean_walk] = M.lean_walk; a[A_launch_lean] = M.launch_lean; a[A_tile_frames] = M.tile_frames; a[A_co_resident] = M.co_resident;
  a[A_doubtful] = M.doubtful; a[A_trial_slot] = M.trial_slot; a[A_want_concurrent] = M.want_concurrent; a[A_concurrent] = M.concurrent;
  a[A_ahead] = M.ahead; a[A_seq_ahead] = M.seq_ahead; a[A_ahead_forced] = M.ahead_forced; a[A_walk2] = M.walk2; a[A_nch] = M.nch;
  a[A_exclusive_cu] = M.exclusive_cu; a[A_asked_device] = M.asked_device; a[A_next_key] = M.trial_next.key;
  a[A_next_calls] = M.trial_next.calls; a[A_next_choice] = M.trial_next.choice;
  return 0;
}
// a mixed-rate call: groups[g] = {n, walk_lds, walk_waves, walk_vgprs, any_nonlinear, an_lds, an_vgprs}; out = {concurrent, ahead, chain_analyses, asked_device}
// (spx_choose_mixed_mode's inputs as they are now; the earlier spx_mode_table_eval_mixed also took the removed A/B switches, and a
// caller of that signature now finds no symbol instead of passing an integer where out4 is expected)
int spx_mode_table_mixed_mode(const long long* groups, int n_groups, int n_total, int cu_count, long long lds_per_cu, long long tension_lds,
                              int tension_vgprs, int concurrent_enabled, int ahead_req, int guard_busy, int device_ours, long long* out4) {
  SpxModeGroup G[8];
  if (n_groups < 0 || n_groups > 8) return -1;
  for (int g = 0; g < n_groups; g++) {
    const long long* p = groups + 7 * g;
    G[g].n = (int)p[0];
    G[g].walk = {(size_t)p[1], (int)p[2], (int)p[3], true, 4};
    G[g].any_nonlinear = p[4] != 0;
    G[g].an_lds = (size_t)p[5];
    G[g].an_vgprs = (int)p[6];
  }
  SpxModeEnv E;
  memset(&E, 0, sizeof(E));
  E.concurrent_enabled = concurrent_enabled; E.chunks = 1;
  SpxModeRuntime T;
  memset(&T, 0, sizeof(T));
  long long ours = device_ours;
  T.guard_busy = guard_busy; T.device_ours = ours_cb; T.device_ctx = &ours;
  const SpxMixedMode M = spx_choose_mixed_mode(G, n_groups, n_total, cu_count, (size_t)lds_per_cu, (size_t)tension_lds, tension_vgprs, E,
                                               ahead_req != 0, T);
  out4[0] = M.concurrent; out4[1] = M.ahead; out4[2] = M.chain_analyses; out4[3] = M.asked_device;
  return 0;
}
// spx_mixed_walk2 for a decided mixed mode {concurrent, ahead}
int spx_mode_table_mixed_walk2(int concurrent, int ahead, int detached, int taps) {
  SpxMixedMode M = {concurrent != 0, ahead != 0, false, false};
  return spx_mixed_walk2(M, detached != 0, taps != 0) ? 1 : 0;
}
// spx_check_job for one job of a plan with window W, frame step B; the SpxJobFault code, and the rule's text for a code
int spx_mode_table_check_job(int W, int B, int analysis_fits, int channels, long long n_in, long long in_off, long long out_off,
                             long long out_cap, float speed, float nonlinear, float feedback) {
  const spx_stream_job j = {in_off, n_in, out_off, out_cap, channels, speed, nonlinear, feedback};
  return spx_check_job({W, B, analysis_fits != 0}, j);
}
const char* spx_mode_table_job_fault_text(int code) {
  return code < SPX_JOB_OK || code > SPX_JOB_TOO_LONG ? "" : spx_job_fault_text(static_cast<SpxJobFault>(code));
}
// spx_twopass_speed: the second-pass speed the retarget kernel writes for one stream (the same text, compiled for the host)
float spx_mode_table_twopass_speed(double want, int length_mode, long long n_in, long long n_probe) {
  return spx_twopass_speed(want, length_mode, n_in, n_probe);
}

// spx_frame_math.h stage by stage over n rows: out[i] = stage(inputs[i]), the text the kernels compile
void spx_frame_math_lowpass(int n, float one_minus_alpha, float alpha, const float* x, const float* y, float* out) {
  for (int i = 0; i < n; i++) out[i] = spx_fm_lowpass(one_minus_alpha, alpha, x[i], y[i]);
}
void spx_frame_math_local_energy(int n, const float* e, const float* l, float* out) {
  for (int i = 0; i < n; i++) out[i] = spx_fm_local_energy(e[i], l[i]);
}
void spx_frame_math_compress(int n, const float* local, float* out) {
  for (int i = 0; i < n; i++) out[i] = spx_fm_compress(local[i]);
}
// one tapered maximum over taps c[0 .. n) with weights taper[0 .. n), and the half-sum of two
float spx_frame_math_tapered_max(int n, const float* c, const float* taper) {
  float m = 0.0f;
  for (int i = 0; i < n; i++) {
    const float v = spx_fm_hysteresis_tap(c[i], taper[i]);
    if (v > m) m = v;
  }
  return m;
}
float spx_frame_math_hysteresis(float past_max, float future_max) { return spx_fm_hysteresis(past_max, future_max); }
// the low gate of tension frames k0 .. k0 + n, as the kernels write it
void spx_frame_math_low(int n, const float* e, int k0, int first_k, float* out) {
  for (int i = 0; i < n; i++) out[i] = (spx_fm_low_energy(e[i]) || k0 + i == first_k) ? 1.0f : 0.0f;
}
float spx_frame_math_low_threshold(void) { return SPX_FM_LOW_THRESHOLD; }
void spx_frame_math_start_values(float* lp_lpf) { lp_lpf[0] = SPX_FM_ENERGY_LP0; lp_lpf[1] = SPX_FM_DIFFERENCE_LP0; }
void spx_frame_math_weighted(int n, const float* lsd, const float* hyst, float* out) {
  for (int i = 0; i < n; i++) out[i] = spx_fm_weighted(lsd[i], hyst[i]);
}
void spx_frame_math_relative(int n, const float* ewld, const float* l, float* out) {
  for (int i = 0; i < n; i++) out[i] = spx_fm_relative(ewld[i], l[i]);
}
void spx_frame_math_clamp(int n, const float* rel, float* out) {
  for (int i = 0; i < n; i++) out[i] = spx_fm_clamp(rel[i]);
}
void spx_frame_math_tension(int n, const float* hyst, const float* sc, float* out) {
  for (int i = 0; i < n; i++) out[i] = spx_fm_tension(hyst[i], sc[i]);
}
// the speed stage over n tensions in sequence, durations[2] = {cur_dur, des_dur} carried in and out: the statements of
// spx_speed_kernel and of the kernels' closed-loop pass, then the blend
void spx_frame_math_speed(int n, const float* tension, float Rg, float nl, float fb, float* durations, float* out) {
  float cur_dur = durations[0], des_dur = durations[1];
  for (int i = 0; i < n; i++) {
    float req = spx_fm_raw_speed(Rg, tension[i]);
    if (fb > 0) req = spx_fm_feedback(req, fb, cur_dur, des_dur);
    cur_dur = spx_fm_advance(cur_dur, req);
    des_dur = spx_fm_advance(des_dur, Rg);
    out[i] = spx_fm_blend(req, nl, Rg);
  }
  durations[0] = cur_dur; durations[1] = des_dur;
}
}
