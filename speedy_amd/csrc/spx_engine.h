// Host side of the batch engine, shared by its translation units (round 6: spx_engine.hip was 1 800 lines):
//   spx_plan.hip    plan tables (DFT spec twiddles, window, Rader), sizes and capacities
//   spx_engine.hip  one batch call: workspace layout, staging, the library's streams, the plan's ring of earlier calls,
//                   run_impl (decide with spx_mode.h, then launch), sub-batches, the rate call
//   spx_mixed.hip   one call over several plans (BASELINE configs[4])
//   spx_map.hip     the call with a time map, and the lookup
//   spx_twopass.hip the two-pass call (a probe pass, then the final pass at a speed worked out on the device), its retarget kernel
//   spx_dtw.hip     batch dynamic time warping (spx_batch_dtw): its two kernels and the call
//   spx_convert.hip the call on float samples: two conversions around the int16 call
//   spx_pipeline.hip the pipeline object: it includes this header for the entries it calls (spx_internal_run*, spx_conv_*)
//   spx_diag.hip    kernel names, resource queries, timing collection, output packing, small copies
// What they share is declared HERE, once: the pinned staging slot and its protocol (SpxStage, SpxStagePair), the workspace carver
// (SpxCarve), a call's arguments and options (SpxCall, SpxCallOpts), the device guard's scope (SpxGuardScope), mode_runtime (of
// spx_choose_mode's inputs; mode_shape is spx_engine.hip's own) and taps_advance.
// Nothing here is part of the C-ABI (include/speedy_hip.h).
#pragma once
#include <algorithm>
#include <math.h>
#include <cmath>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/speedy_hip.h"
#include "spx_internal.h"
#include "spx_jobs.h"
#include "spx_mode.h"

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif


// the calling thread's last error (spx_last_error)
extern thread_local std::string g_spx_err;
static inline int fail(int code, const std::string& msg) {
  g_spx_err = msg;
  return code;
}
#define HIPCHK(expr)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return fail(-2, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// roctx ranges around the host side of a batch call (rocprofv3 --marker-trace shows them next to the kernels).  The
// tracer library is looked up at run time: the product has no link-time dependency on it and works without it.
#include <dlfcn.h>
struct SpxRoctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  SpxRoctx() {
    // rocprofv3 follows the rocprofiler-sdk flavour of the API; the roctracer one (libroctx64) is the fallback
    void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_LAZY | RTLD_LOCAL);
    if (!h) h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_LAZY | RTLD_LOCAL);
    if (!h) h = dlopen("libroctx64.so", RTLD_LAZY | RTLD_LOCAL);
    if (!h) h = dlopen("libroctx64.so.4", RTLD_LAZY | RTLD_LOCAL);
    if (h) {
      push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
      pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
      if (!push || !pop) { push = nullptr; pop = nullptr; }
    }
  }
};
struct SpxRange {
  static SpxRoctx& api() { static SpxRoctx a; return a; }
  explicit SpxRange(const char* name) { if (api().push) api().push(name); }
  ~SpxRange() { if (api().pop) api().pop(); }
};

#define SPX_MAX_CHUNKS 16
// The plan's ring of earlier calls (ring_wait below) and the library's walk streams per device (dev_walk_streams): the walk kernels
// of consecutive pipelined calls take turns on up to SPX_MAX_WALK_STREAMS streams, and the ring remembers twice as many calls.
#define SPX_MAX_WALK_STREAMS 4
#define SPX_RING (2 * SPX_MAX_WALK_STREAMS)
// Pinned staging slot for the small host tables of a call (job tables, tile order): the async copies read it after the
// call has returned, so it outlives the call (plan-owned, or a thread's own) and is reused only once its copies have retired.
// The protocol, in this order: acquire, fill p, enqueue the reader, release on the reader's stream.  Under the owner's mutex.
struct SpxStage {
  void* p = nullptr;
  size_t cap = 0;
  hipEvent_t done = nullptr;
  int acquire(size_t bytes);      // a host wait for whatever last read the slot (or the event's creation), then room for `bytes`
  int release(hipStream_t on);    // `done` recorded behind the reader
  void destroy();
};
// Two slots taking turns: the reader of the slot a call takes was enqueued two calls ago, so acquire rarely has to wait.
struct SpxStagePair {
  SpxStage slot[2];
  int next = 0;
  SpxStage& take() { SpxStage& s = slot[next]; next ^= 1; return s; }
  void destroy() { for (auto& s : slot) s.destroy(); }
};
// Workspace carving: consecutive parts, each on a 256-byte boundary (the base is rounded up too).
struct SpxCarve {
  size_t o;
  explicit SpxCarve(size_t base = 0) : o((base + 255) & ~(size_t)255) {}
  size_t take(size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; }
};
struct spx_plan {
  SpxPlanDev dev;
  int device = 0;           // the HIP device the tables live on; calls must be made with it current
  int cu_count = 1;
  size_t lds_per_cu = 65536;
  std::mutex mu;            // one launch sequence at a time per plan: side streams, events and staging are plan-owned
  SpxStagePair stage;
  // Mode trial for batch shapes where the register file admits only ONE analysis wave per SIMD beside the consumers:
  // whether the concurrent mode pays then depends on how long the walk is (16 kHz stereo: 3.4 ms concurrent, 3.8 in
  // sequence; 22.05 kHz mono: 3.0-4.6 against 2.3-3.2), so the second call of a shape runs concurrently and the third in
  // sequence, both bracketed by events on the caller's stream, and later calls take the faster.  Results do not depend on it.
  struct Trial {
    SpxModeTrial state = {-1, 0, -1};   // key, calls, choice (-1 undecided, 0 sequential, 1 concurrent): spx_mode.h
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // [mode][begin / end]
  } trial;
  std::map<long long, SpxModeResources> res_cache;   // mode_resources: per batch shape
  // an overlapped call of more streams than CUs, split into overlapping sub-batches (run_split): how the call that last used a
  // workspace was split (spx_batch_read_steps must find the states)
  std::map<const void*, int> split_of;
  void* tables = nullptr;  // one device allocation behind dev.tw/tw2/window/taper*
  // time-chunk pipelining of one batch call: the analysis of chunk c+1 runs on `side` while the walk of chunk c
  // runs on the caller's stream
  hipStream_t side = nullptr;
  hipStream_t side2 = nullptr;   // concurrent mode: the tension kernel's stream
  hipEvent_t ev_tension = nullptr;
  hipEvent_t ev_chunk[SPX_MAX_CHUNKS] = {};
  // spx_batch_run_ahead: the walk kernels of the plan's previous FOUR calls (ring_wait / ring_record below), the started-counter
  // of the last one
  hipEvent_t ev_walk[SPX_RING] = {};   // slot = call number mod SPX_RING
  bool ev_walk_valid[SPX_RING] = {};
  void* ring_ws[SPX_RING] = {};         // the workspace and the caller's stream of the call in the slot
  hipStream_t ring_st[SPX_RING] = {};
  int ahead_calls = 0;
  hipEvent_t ev_call[2] = {nullptr, nullptr};   // the caller's stream as it stood when the last two pipelined calls were made
  const void* ahead_last_out = nullptr;
  const void* ahead_last_nout = nullptr;
  bool ev_call_valid[2] = {false, false};
  hipStream_t ev_call_st[2] = {nullptr, nullptr};   // ... and which stream each note was taken on (a detached call leaves none)
  std::vector<std::pair<const int*, int>> mixed_started;   // the same for the groups of the last mixed call (lead plan)
  const int* ahead_started = nullptr;
  int ahead_n = 0;
  // spx_batch_run_mixed: this plan's group runs on `mix`; the first plan of a call also lends the fork event and a staging slot
  hipStream_t mix = nullptr;
  hipEvent_t ev_join = nullptr, ev_fork = nullptr, ev_an = nullptr;
  std::mutex mix_mu;
  SpxStagePair mix_stage;        // (two, taking turns: a pipelined mixed call's upload sits behind the batch's H2D copy, and waiting
                                 //  for the one slot's event made the host wait for that copy -- ADVICE r5)
};

// ---- process-wide state (spx_engine.hip) ----
struct EvPair { hipEvent_t a, b; int kind; };  // kind 0 = analysis launch, 1 = walk launch, 2 = tension launch, 3 = rate launch (spx_batch_run_rate), 4 = the map's rows conversion (spx_batch_run_rate_map), 5 / 6 = the forward / tail kernel of spx_batch_dtw
extern std::atomic<bool> g_timing;
extern std::atomic<int> g_last_concurrent;   // spx_debug_last_call_concurrent (2 = pipelined with the previous call)
extern std::atomic<int> g_concurrent;        // spx_set_concurrent
extern std::atomic<int> g_tension_form;      // spx_set_tension_form
extern std::atomic<int> g_last_tension_form; // spx_debug_last_tension_form (run_impl alone sets it)
extern std::atomic<int> g_last_call_chunks;  // spx_debug_last_call_chunks (run_impl alone sets it)
extern std::atomic<bool> g_chunks_set;       // the caller chose a chunk count (spx_set_pipeline_chunks)
extern std::atomic<int> g_chunks;
extern std::mutex g_tmu;
extern std::vector<EvPair> g_ev_pending;
extern std::vector<hipEvent_t> g_ev_free;
extern int g_calls_pending;
struct SpxDevGuard {
  std::mutex mu;
  hipEvent_t last = nullptr;
  hipStream_t last_stream = nullptr;
  bool valid = false;
};
extern SpxDevGuard g_guard[64];
// A call's hold on its device's guard (run_impl, mixed_impl).  A call that wants the concurrent mode enters: the guard is locked
// and the last concurrent call's event queried.  idle_start: that call (if any) has drained.  Still in flight on ANOTHER stream:
// `redecide` runs with the guard locked, then the guard is unlocked (the call takes the sequential order).  Otherwise the guard
// stays locked until the scope ends, by which time a concurrent call has left its own event behind (leave_event).
struct SpxGuardScope {
  SpxDevGuard& guard;
  std::unique_lock<std::mutex> lock;
  bool idle_start = false;
  explicit SpxGuardScope(int device) : guard(g_guard[(device >= 0 && device < 64) ? device : 0]), lock(guard.mu, std::defer_lock) {}
  template <class Redecide>
  void enter(hipStream_t st, Redecide&& redecide) {
    lock.lock();
    const hipError_t q = guard.valid ? hipEventQuery(guard.last) : hipSuccess;
    (void)hipGetLastError();  // hipErrorNotReady is not an error of this call
    idle_start = (q == hipSuccess);
    if (guard.valid && guard.last_stream != st && q == hipErrorNotReady) {
      redecide();
      lock.unlock();
    }
  }
  int leave_event(hipStream_t st);   // this call's completion, for the next concurrent-mode call on the device (guard still locked)
};

// frame j is sent to the analysis once sample j*B + W has been written (soniclib.c:440-444)
static inline int64_t frames_for(const SpxPlanDev& d, int64_t n_in) {
  if (n_in < d.W + 1) return 0;
  return (n_in - d.W - 1) / d.B + 1;
}
// rows of a job's time map (spx_plan_map_rows): one per complete ring buffer and the final count; a linear job has the count alone
static inline int64_t spx_map_rows(const SpxPlanDev& d, int64_t n_in, bool nonlinear) { return nonlinear ? n_in / d.B + 1 : 1; }
spx_plan* shared_plan_full(int sample_rate, int match_matlab);   // spx_plan.hip: one plan per (device, rate, hysteresis mode), cached

// ---- spx_engine.hip ----
struct Layout {
  size_t off_streams, off_states, off_rec, off_scratch, off_order, off_flags, off_ready, total;
  int64_t max_tiles;
  int64_t total_frames;
};
Layout layout_for(const SpxPlanDev& d, const spx_stream_job* jobs, int n);
int dev_side_streams(int dev, hipStream_t* side, hipStream_t* side2);
int walk_stream_count();
int dev_walk_streams(int dev, hipStream_t* w, int n);
int ring_note(spx_plan* plan, hipStream_t st);
int ring_wait(spx_plan* plan, hipStream_t sa, const void* ws, hipStream_t st, bool* waited_prev);
bool ring_previous_in_flight(spx_plan* plan);
int ring_record(spx_plan* plan, hipStream_t on, void* ws, hipStream_t st, const void* out, const void* n_out, bool detached = false);
SpxModeEnv mode_env();
bool device_ours_cb(void* ctx);
struct SpxSpeedClass { int maxC; bool speedup_only, any_speed; };
SpxSpeedClass speed_class(const spx_stream_job* jobs, int n);
SpxModeWalk mode_walk(const SpxPlanDev& d, const SpxWalkAsk& ask);
void spx_launch_gate(const int* started, int n_walk, unsigned max_spins, hipStream_t st);   // the idle-start / previous-call gate kernel
// `force`: the call is one group of a mixed-rate batch (spx_batch_run_mixed): the launch mode was decided for all groups
// together, and the device guard is held by the caller.
//   ahead_sa: the group of a pipelined mixed call -- its producers go to this stream at once (spx_batch_run_mixed_ahead orders it);
//   started_out: where the group's walk workgroups count themselves in (for the next call's gate)
//   total_streams: of all groups of the mixed call; after_analysis: recorded behind the group's analysis launch (or null)
struct SpxForce { int concurrent; bool idle_start; int total_streams; hipEvent_t after_analysis; hipStream_t ahead_sa; const int** started_out;
                  bool no_exclusive;   // the walk workgroups do NOT ask for a CU of their own and take the 4096-frame window (a mixed call whose walk
                                       // kernels overlap the previous call's: two calls' walk workgroups and an analysis workgroup on a CU)
};
// A call with a playback rate per stream (spx_batch_run_rate): jobs with rate != 1 go through the GENERAL walk kernel without the
// flush truncation (SPX_F_NO_TRUNC) into a TSM buffer inside the workspace, and a batched rate kernel (spx_rate_batch.hip) behind
// the walk kernel writes the caller's buffer.  Kernels in sequence on the caller's stream.
struct SpxRateCall {
  std::vector<int64_t> walk_out_off, walk_out_cap;   // per job: where the walk kernel writes (int16 values from `out`; may be negative)
  std::vector<unsigned char> no_trunc;               // per job: rate != 1
  std::vector<int> table;                            // the SpxRateJob records, as the staging kernel copies them (32-bit words)
  SpxRateJob* d_table = nullptr;                     // DEVICE (workspace): the records, ...
  int64_t* d_tsm_n = nullptr;                        // ... the walk kernel's counts
  const int16_t* tsm_base = nullptr;                 // the base SpxRateJob::tsm_off counts from
  int max_blocks = 1;
};
// spx_map.hip: the rows of a rate call with a time map (spx_batch_run_rate_map), from speed-stage frames to final frames in place,
// behind the rate kernel.  jobs: DEVICE, the call's SpxRateJob records; streams: DEVICE, the SpxStreamDev records of the call's last
// time chunk; n_out: DEVICE, the final counts; max_rows: the longest stream's row count.
void spx_launch_map_rate_rows(const SpxRateJob* jobs, const SpxStreamDev* streams, int n_streams, int B, int64_t max_rows,
                              const int64_t* n_out, int64_t* map, hipStream_t hs);
// The second pass of a two-pass call (spx_batch_run_twopass, spx_twopass.hip): the speeds of the job table are not known on the host
// -- a retarget kernel behind the staging kernel works them out from the first pass's counts (spx_twopass.h) and patches them into
// the staged SpxStreamDev records.  Kernels in sequence on the caller's stream; the speed in the host table is a placeholder that
// decides nothing.
struct SpxRetargetCall {
  std::vector<int> table;                // the SpxRetargetJob records, as the staging kernel copies them (32-bit words)
  void* d_table = nullptr;               // DEVICE (workspace): where they go
  const int64_t* n_probe = nullptr;      // DEVICE [n]: the first pass's counts
  float* speeds = nullptr;               // DEVICE [n]: the second-pass speeds, for the caller
};
// spx_twopass.hip: one thread per stream; `copies` = the time chunks the call was cut into (streams holds copies * n records)
void spx_launch_retarget(const void* d_table, int n, int copies, const int64_t* n_probe, float* speeds, SpxStreamDev* streams, hipStream_t st);
// What every batch call is given (the arguments of spx_batch_run, in its order): the extern "C" entries fill one.
struct SpxCall {
  spx_plan_t plan;
  const spx_stream_job* jobs;
  int n;
  const int16_t* in;
  int16_t* out;
  int64_t* n_out;
  void* ws;
  size_t ws_bytes;
  const spx_taps* taps;
  void* hs;
};
struct SpxCallOpts {
  bool do_a = true, do_w = true;   // the analysis / the walk half of the call (spx_batch_analyze, spx_batch_walk: one of them)
  const SpxForce* force = nullptr;
  const SpxRateCall* rate = nullptr;   // spx_batch_run_rate with at least one rate != 1
  // spx_batch_run_map: DEVICE, the call's time map (spx_map_rows per job, in job order).  Handled like a rate call: the whole batch on
  // the GENERAL walk kernel (its map instantiation; neither speed-up form writes a map), kernels in sequence on the caller's stream
  int64_t* map = nullptr;
  // spx_batch_run_edits: the call's edit list.  Handled as a map call is -- the general walk kernel (its recording instantiation),
  // kernels in sequence on the caller's stream -- and refused together with rate, map or retarget
  const SpxEditsCall* edits = nullptr;
  // spx_batch_run_twopass's second pass: the speeds come from the device.  Handled like a rate call and a map call -- kernels in
  // sequence on the caller's stream -- but on the walk kernels' any-speed forms (the speed class is "any speed", whatever the
  // placeholder in the host table says); with do_a = false the pass reuses the frame records the first pass left in the workspace
  const SpxRetargetCall* retarget = nullptr;
  bool ahead_req = false;     // spx_batch_run_ahead: pipelined with the plan's previous call where the shape allows
  bool overlap_req = false;    // spx_batch_run_overlapped: ... and its walk kernel beside the previous call's
  void* in_ready = nullptr;    // hipEvent_t: the producers wait for it (the caller's "input is there")
  bool split_part = false;     // one of the sub-batches run_split cut the call into (spx_batch_read_steps finds their state records by it)
  bool sub = false;            // a sub-batch of a plain call the engine has split (run_split): its `out` is the whole call's, never
                               // "the previous call's output buffer handed over again"
  // The pipeline object's calls (spx_pipeline.hip): done_event (a hipEvent_t) is recorded behind everything the call enqueued --
  // and with `detached`, a call whose walk kernel goes to one of the library's walk streams does not touch hip_stream AT ALL
  // (no note, no wait for the walk kernel: the event is recorded on the walk stream).  A caller stream that carries nothing but
  // waits for walk kernels is a hardware queue whose head is a blocked barrier packet for 2 ms of every 2; depending on where
  // that queue happens to land among the process's queues, the kernels of the side stream were dispatched 50 us late after each
  // such packet (profiles/r05/r5e_trace_*.txt, r5f_queue_probe.txt: 1.14 against 1.03 ms per batch).
  void* done_event = nullptr;
  bool detached = false;
};
int run_impl(const SpxCall& c, const SpxCallOpts& opt = SpxCallOpts());
SpxModeRuntime mode_runtime(spx_plan* plan);   // zeroed, with the plan's device behind device_ours
// the taps of a part of a call that begins `rows` frames in, with `spec` / `norm` elements of the two spectrum taps in front of it
spx_taps taps_advance(const spx_taps& t, int64_t rows, int64_t spec, int64_t norm);
// what a call refuses about its job table (spx_jobs.h, then the walk kernel's LDS window), asked before anything is enqueued
SpxJobLimits spx_job_limits(spx_plan_t plan);
int spx_check_jobs(spx_plan_t plan, const spx_stream_job* jobs, int n, bool rate_call = false, bool short_window = false, bool device_speeds = false);
int spx_read_steps(const SpxPlanDev& d, const spx_stream_job* jobs, int n, const void* ws, int32_t* steps, hipStream_t st);

// ---- what the pipeline object (spx_pipeline.hip) calls ----
void spx_internal_set_error(const char* msg);   // spx_plan.hip: other translation units' errors reach spx_last_error
// spx_engine.hip: the call in its plain, pipelined (ahead) or overlapped order, behind in_ready, with done_event behind everything
int spx_internal_run(const SpxCall& c, bool ahead, bool overlap, void* in_ready, void* done_event, bool detached);
// ... and the rate call's side of a rate pipeline (spx_pipeline_create_rate)
int spx_internal_rate_check(spx_plan_t plan, float rate);
size_t spx_internal_rate_workspace_all(spx_plan_t plan, const spx_stream_job* jobs, int n);
int spx_internal_run_rate(const SpxCall& c, const float* rates, void* in_ready, void* done_event);
// spx_mixed.hip
int spx_internal_run_mixed(const spx_plan_t* plans, int n_plans, const spx_stream_job* jobs, const int* plan_index, int n, const int16_t* in,
                           int16_t* out, int64_t* n_out, void* ws, size_t ws_bytes, void* hs, bool ahead, void* in_ready,
                           void* done_event, bool detached);
// spx_convert.hip: the float batch call's conversion table and its two kernels, launched for a buffer set of the pipeline's
size_t spx_conv_table_bytes(int n);
int spx_conv_table_fill(void* pinned, const spx_stream_job* jobs, int n, int* max_in, int* max_out);
void spx_conv_table_upload(const void* pinned, void* d_tab, int n, hipStream_t st);
void spx_conv_launch_in(const void* d_tab, int n, int max_in, const float* in, int16_t* st_in, hipStream_t st);
void spx_conv_launch_out(const void* d_tab, int n, int max_out, const int64_t* n_out, const int16_t* st_out, float* out, hipStream_t st);
