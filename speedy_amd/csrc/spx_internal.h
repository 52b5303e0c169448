// Internal definitions shared by the HIP kernels and the C-ABI host code.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stdlib.h>
#include <type_traits>

// The library reads the documented environment variables only (INTEGRATION.md "Environment"): SPX_NO_POOL, SPX_POOL_*,
// SPX_SHARED_GPU, SPX_LOCK_DIR, SPX_DEBUG_MODE, SPX_DEBUG_TRIAL, SPX_KEEP_HW_QUEUES and GPU_MAX_HW_QUEUES.  Variants are
// compile-time (-DSPX_WALK_PAD=n, -DSPX_STAMPS, SPX_HOT_SCHED: tools/build_variant.sh).

// Speeds the speed-up walk kernel (spx_walk_fast.hip) serves: its division for the step lengths is the IEEE sequence without
// the scaling half, exact for speed - 1 in [2^-60, 2^80) (fast_div).  Anything beyond (a speed of 1e18 turns every step into a
// failed one anyway) runs on the general kernel.
#define SPX_FAST_MAX_SPEED 1.0e18f

#define SPX_MAX_STAGES 16
#define SPX_WAVE 64
#define SPX_BLOCK 256
#define SPX_FEATURE_COUNT 15  // speedy.h:115

// Constant tables and sizes of one plan; passed BY VALUE to every kernel.
struct SpxPlanDev {
  int rate;
  int B;  // frame step   = rate/100              (speedy.c:335-338)
  int W;  // window size  = (int)(1.5*rate/100)   (speedy.c:213)
  int N;  // fft size     = 2*W                   (speedy.c:214)
  int F;  // kTemporalHysteresisFuture            (speedy.h:136-146)
  int Pp; // kTemporalHysteresisPast
  int nstages;
  int radix[SPX_MAX_STAGES];
  int minPeriod, maxPeriod, maxRequired, skip;  // libsonic limits
  int tile_frames;  // frames per analysis tile (spx_analysis_tile_frames)
  int dft_waves;    // waves of an analysis workgroup that transform frames (4; fewer for the windows of the highest sample rates)
  float alpha;            // (float)exp(-1.0/100)             (speedy.c:67,287)
  float one_minus_alpha;  // (1 - alpha) evaluated in float   (speedy.c:74)
  const double* tw;    // [W]  (cos, -sin)(2 pi t / W)
  const double* tw2;   // [W]  (cos, -sin)(2 pi k / 2W)
  const float* window; // [W]  Hamming                         (speedy.c:256-258)
  const float* taperF; // [F+1]  (F-i)/(float)F               (speedy.c:597)
  const float* taperP; // [P+1]  (P-i)/(float)P               (speedy.c:604)
  // Rader's algorithm for a large prime W whose W-1 is smooth (44.1 kHz: W = 661, 660 = 4*3*5*11; DESIGN.md "DFT
  // spec"): the W-point transform as a cyclic convolution of length M = W-1 done with an M-point plan.
  int rader;                     // 0: plain mixed-radix stages
  int nstagesM;
  int radixM[SPX_MAX_STAGES];
  const double* twM;   // [M]  (cos, -sin)(2 pi t / M)
  const double* bfft;  // [M]  M-point transform of b[q] = tw[iperm[q]]
  const int* perm;     // [M]  perm[p]  = g^p  mod W, g the smallest primitive root
  const int* iperm;    // [M]  iperm[q] = g^-q mod W
  const int* qlog;     // [W]  qlog[k] = the q with g^-q = k (k = 1 .. M; entry 0 unused)
  // W = 240 only (else null): what a lane of spx_analysis_kernel<16, 240> takes from tw, tw2 and window, lane-major --
  // entry [c][lane] at 16 bytes each, c as in spx_lane_consts_fill (spx_plan.hip) -- so that the kernel loads a group of constants
  // right where a stage uses it (one address register, immediate offsets) instead of holding all sixty registers across the tile
  const void* lane_consts;
};
// The samples' 2^-15 lives in the window values a lane multiplies by (spx_analysis.hip spx_preemph_win; -DSPX_PREEMPH_V1: the
// literal sequence, scale 1).  A power of two: the float multiplication is exact, on the host as on the device.
#ifdef SPX_PREEMPH_V1
#define SPX_WIN_SCALE 1.0f
#else
#define SPX_WIN_SCALE 0x1p-15f
#endif
// The lane-major table of W = 240: 14 double2 entries (the twiddles of stages 1 - 3, the untangle factors) and one float4 (the
// four window values times SPX_WIN_SCALE) per lane.
#define SPX_LC_W1 0     // [3]  tw[bb j], j = 1..3, bb = lane < 60 ? lane : 0
#define SPX_LC_W2 3     // [3]  tw[4 (bb >> 2) j]
#define SPX_LC_W3 6     // [2][2]  tw[16 p3], tw[32 p3], p3 = (lane + 64 u) >> 4 below 80, else 0
#define SPX_LC_WU 10    // [4]  tw2[k], k = lane + 64 u below 240, else 0
#define SPX_LC_WN 14    // window[2 bb], [2 bb + 1], [2 bb + 120], [2 bb + 121], each times SPX_WIN_SCALE
#define SPX_LC_ENTRIES 15
#define SPX_LC_BYTES (SPX_LC_ENTRIES * 64 * 16)
// fills out[SPX_LC_BYTES] from the plan's host tables (tw, tw2: (cos, -sin) pairs; win: floats) -- copies only, and the one exact
// multiplication of the window values
void spx_lane_consts_fill(const double* tw, const double* tw2, const float* win, unsigned char* out);

// Per-stream job in device memory.  A job covers "everything new since the last call": batch jobs start
// from scratch (SPX_F_INIT) and end the stream (SPX_F_FLUSH) in one go; the streaming API issues a job
// per sonicWrite*/sonicFlush call with the state record carried in device memory between calls.
#define SPX_F_INIT 1   // ignore the stored state, start a fresh stream
#define SPX_F_FLUSH 2  // after the new input: sonicFlushStream (soniclib.c:529-552)
#define SPX_F_TENSION_RANGE 4  // unit-level API: compute exactly the tension frames [tension_skip, tension_to)
#define SPX_F_NO_SPEED 8       // unit-level API: no speed / duration pass (speedyComputeSpeedFromTension is its own call)
#define SPX_F_NO_TRUNC 16      // a rate stage follows (sonicSetRate != 1): the flush does not truncate the TSM output -- the
                               // dependency truncates the FINAL output there -- and leaves `flush_remaining` in the state record
#define SPX_F_SPEED_SET 32     // sonicSetSpeed was called since the last job: it reaches the TSM stage at once, in nonlinear
                               // mode too (soniclib.c:177-182) -- a flush right behind it hands out the ring buffers at that speed
#define SPX_F_KEEP_SPEED 64    // a linear job on a stream that has been nonlinear (soniclib.c:397-399 short-circuits per write): the
                               // TSM stage keeps the speed it was last given instead of taking the global one
#define SPX_F_HANDED_IN 128    // ... and on such a stream the ring-buffer counts come with the job (handed_in, ring_bufs): its TSM input is a
                               // sequence of its own, n_in describes that one
struct SpxStreamDev {
  int64_t in_off, n_in, out_off, out_cap;  // n_in = input frames present so far (from the stream start)
  int64_t frame_off;    // index of this stream's analysis frame 0 in the per-frame arrays
  int32_t n_frames;     // analysis frames available with n_in samples
  int32_t frame_begin;  // analysis frames already done by earlier jobs
  int32_t channels;
  int32_t flags;
  float speed, nonlinear, feedback;
  int32_t first_tile;   // index of this job's first analysis tile
  // Streams that are written again after sonicFlushStream (soniclib.c:529-552 leaves the stream usable):
  int64_t tsm_shift;     // frames of flush padding the TSM stage has seen so far: TSM position = input frame + tsm_shift
  int32_t tension_skip;  // tension frames below this index that were not computed before the last flush never are:
                         // the shim's read index jumps to its write index there (soniclib.c:538-550)
  // The unit-level API of include/speedy.h (reference speedy.h:61-133) adds frames and asks for tensions one call at
  // a time, with its own time base:
  int32_t unit_time0;    // 0: frame j is added at time j + 1 (the shim, soniclib.c:288-296); 1: at time j (speedyAddData(.., j))
  int32_t tension_to;    // SPX_F_TENSION_RANGE: compute tension frames [tension_skip, tension_to)
  int32_t handed_in;     // SPX_F_HANDED_IN: ring buffers handed to the TSM stage before this job ...
  int32_t ring_bufs;     // ... and complete ring buffers that exist (n_in is the TSM input's length there, not the ring's)
  int32_t map_row;       // spx_batch_run_map: index of this stream's row 0 in the call's time map (read by spx_walk_map_kernel only);
                         // spx_batch_run_edits: index of this stream's record 0 in the call's edit list (spx_walk_edits_kernel)
};

// TSM-stage state (libsonic's stream struct) in absolute stream coordinates.
struct SpxWalkState {
  int64_t base;    // absolute index of the first sample still buffered in the TSM stage
  int64_t out_n;   // frames produced since the stream start
  int64_t avail;   // frames handed to the TSM stage so far
  int remaining;   // remainingInputToCopy
  int prevPeriod, prevMinDiff;
  int overflow;
  int prevPeriod_toggle;  // which of the two LDS lag-sum buffers the next pitch step uses (walk kernel internal)
  int steps;       // pitch searches (findPitchPeriod calls) since the stream started: the length of its chain of dependent
                   // steps (diagnostic -- bench.py's latency roofline divides the walk kernel's time by it)
};
// Everything a stream carries from one job to the next.
struct SpxStreamState {
  SpxWalkState w;
  float lp;        // energy low-pass state          (speedy.c:166,288)
  float lpf;       // difference low-pass state      (speedy.c:167,291)
  float cur_dur;   // speedy.c:170
  float des_dur;   // speedy.c:171
  float curSpeed;  // speed currently set in the TSM stage
  int handed;      // ring buffers handed to the TSM stage so far (readBufferFrameIndex, soniclib.c:73)
  int flush_remaining;  // frames the TSM stage held when its last flush began (the rate stage's expected length needs it)
  int flush_out_mark;   // ... and the frames it had produced by then (events of the same job before the flush included)
  int tension_first;    // time index of the first tension frame ever computed (-1: none yet): that call alone is "skipped"
                        // (skip_frame_count starts at 1, speedy.c:293,691) -- frame 0 unless a flush came before it
  int pad2_;
};

// Rate stage (sonicSetRate != 1: the dependency's adjustRate, oracle/orc_sonic.c adjust_rate): the TSM stage's output
// is the input sequence, one sample always stays behind as the next call's left neighbour.
#define SPX_RATE_MAX_CHANNELS 16
struct SpxRateState {
  int64_t tsm_seen;   // TSM output frames already taken
  int64_t final_n;    // frames of final output produced so far
  int32_t old_pos, new_pos;  // oldRatePosition / newRatePosition
  int32_t has_left;   // a sample is waiting in the pitch buffer
  int32_t overflow;
  int16_t left[SPX_RATE_MAX_CHANNELS];
};
// One workgroup: takes TSM output frames [tsm_seen, |*tsm_n|) from `tsm` and appends to `fin` -- resampled at new_rate /
// old_rate (already reduced to 14 bits), or copied when `bypass`.  `flush`: sonicIntFlushStream's truncation to the
// expected length and emptying of the pitch buffer.
void spx_launch_rate(SpxRateState* rs, const SpxStreamState* st, const int64_t* tsm_n, const int16_t* tsm, int16_t* fin,
                     int64_t fin_cap, int channels, int old_rate, int new_rate, float rate, int bypass, int flush,
                     hipStream_t hs);

// Rate stage of a batch call (spx_batch_run_rate, spx_rate_batch.hip): every stream is one whole life cycle, so nothing is
// carried -- one record per stream, written by the host, and a grid over (output block, stream).
struct SpxRateJob {
  int64_t tsm_off;    // the stream's TSM output (the walk kernel's, flush not truncated): first value, in int16 values from tsm_base
  int64_t tsm_cap;    // ... and its capacity in frames
  int64_t fin_off;    // the caller's out_off / out_cap: the final frames
  int64_t fin_cap;
  int32_t channels;
  int32_t old_rate, new_rate;   // sample rate and (int)(sample rate / rate), both halved until they fit 14 bits
  int32_t bypass;     // rate == 1: the walk kernel wrote the caller's buffer itself, only the count is handed on
  float rate;
  int32_t n_blocks;   // blocks that cover the most this stream can emit (known on the host); the grid's surplus blocks leave at once
  int64_t pad_;
};
int spx_rate_batch_blocks(int64_t frames, int channels);
// tsm_n: DEVICE, the walk kernel's counts (negative = the TSM buffer overflowed, SPX_NOUT_LOST_PRODUCER passes through);
// n_out: DEVICE, the final counts (negative = fin_cap was too small).  Nothing is written past fin_off + fin_cap * channels.
void spx_launch_rate_batch(const SpxRateJob* jobs, int n_streams, int max_blocks, const SpxStreamState* states, const int64_t* tsm_n,
                           const int16_t* tsm_base, int16_t* fin_base, int64_t* n_out, hipStream_t hs);

// Per-analysis-frame record written by the analysis kernel and consumed by the walk kernel.
struct SpxFrameRec {
  float energy;  // sum_{i=1}^{N/2-1} s[i]^2, float, index order  (speedy.c:513-516 == :633-640)
  float lsd;     // local spectral difference with cur = this frame, last = previous (speedy.c:711-719)
};

// Scratch per analysis frame used by the walk kernel's frame-rate passes.
struct SpxTapsDev {
  float* tension;
  float* speed;
  float* features;
  float* spectrogram;
  float* normalized;
};

// mono: as for spx_analysis_lds_bytes -- true only if NO stream of the launch has more than one channel
void spx_launch_analysis(const SpxPlanDev& P, const SpxStreamDev* streams, int n_streams, int n_tiles,
                         const int16_t* in, SpxFrameRec* rec, SpxTapsDev taps, const int* tile_order, int* tile_flags,
                         bool mono, hipStream_t st);
// The same kernel fed with explicit float frames (unit-level API): frame j = frames[j*W .. j*W + W), pre-emphasis state
// carried from the previous frame's last sample (speedy.c:416-425); preemph = false: the frame is windowed as it is
// (speedySpectrogram, speedy.c:438-473).
void spx_launch_analysis_frames(const SpxPlanDev& P, const SpxStreamDev* streams, int n_tiles, const float* frames,
                                bool preemph, SpxFrameRec* rec, SpxTapsDev taps, hipStream_t st);
// Frame-rate stage: energy / hysteresis / difference filters -> tension -> speed per tension frame (scratch[4k+3]) and
// the tension, speed and feature taps.  tile_flags / speed_ready: the concurrent-mode hand-off (nullptr = sequential).
// form: which kernel -- SPX_TENSION_POLL spx_tension_kernel (four passes, polls tile flags where given: the concurrent mode's
// consumer, and the kernel of the streaming and unit-level call sites), SPX_TENSION_SEQ spx_tension_seq_kernel (one pass over LDS,
// the three recurrences side by side; launches without tile flags only -- asked for with flags, the polling kernel runs).  Both
// write the same bits to the same places.  Returns the form launched.
#define SPX_TENSION_POLL 0
#define SPX_TENSION_SEQ 1
int spx_launch_tension(const SpxPlanDev& P, const SpxStreamDev* streams, int n_streams, SpxStreamState* states,
                       const SpxFrameRec* rec, float* scratch, SpxTapsDev taps, const int* tile_flags, int* speed_ready,
                       hipStream_t st, int form = SPX_TENSION_POLL);
// spx_tension_seq.hip: the launch itself (called by spx_launch_tension alone) and whether the kernel's rings hold the plan's
// hysteresis reach (F, Pp at most one block: every plan's are 8 and 12)
void spx_launch_tension_seq(const SpxPlanDev& P, const SpxStreamDev* streams, int n_streams, SpxStreamState* states,
                            const SpxFrameRec* rec, float* scratch, SpxTapsDev taps, int* speed_ready, hipStream_t st);
bool spx_tension_seq_serves(const SpxPlanDev& P);
// An instantiation of a kernel template as its family's selector picked it (spx_analysis_select, spx_walk_select,
// spx_walk_fast_select -- each the ONE place its template-ids are written): the launch, the register query and the kernel's
// name (spx_batch_kernel_names) all come from the same pick.
struct SpxKernelChoice {
  const char* name;  // the template's name, as a profiler prints it in front of the template values
  const void* fn;    // host function pointer: hipLaunchKernel, spx_kernel_vgprs
  int block;       // threads per workgroup
  int n_targs;     // template values in use ...
  int targs[5];    // ... in the template's order
};
// The argument lists of the three kernel templates (every instantiation of a template has its template's one signature): each
// selector asserts its list against its kernel, and a launch through SpxLaunch<list> is type-checked against the list -- a
// parameter added to a kernel stops the build at the selector, and then at every launch, as a direct launch would.
using SpxAnalysisArgs = void(SpxPlanDev, const SpxStreamDev*, int, const int16_t*, SpxFrameRec*, SpxTapsDev, const int*, int*, const float*, int);
using SpxWalkArgs = void(SpxPlanDev, const SpxStreamDev*, const int16_t*, int16_t*, int64_t*, SpxStreamState*, const float*, int, const int*);
using SpxWalkMapArgs = void(SpxPlanDev, const SpxStreamDev*, const int16_t*, int16_t*, int64_t*, SpxStreamState*, const float*, int, const int*, int64_t*);
using SpxWalkEditsArgs = void(SpxPlanDev, const SpxStreamDev*, const int16_t*, int16_t*, int64_t*, SpxStreamState*, const float*, int, const int*, int4*, int64_t*, int);
using SpxWalkFastArgs =void(SpxPlanDev, const SpxStreamDev*, const int16_t*, int16_t*, int64_t*, SpxStreamState*, const float*, const int*, int);
template <typename F> struct SpxLaunch;
template <typename... P> struct SpxLaunch<void(P...)> {
  static void go(const SpxKernelChoice& k, int grid, size_t lds, hipStream_t st, P... p) {
    void* args[] = {&p...};
    // (a launch error surfaces at the callers' hipGetLastError or at their synchronisation, as with a direct launch)
    (void)hipLaunchKernel(k.fn, dim3(grid), dim3(k.block), args, lds, st);
  }
};
// What a caller asks of the walk stage: the batch's shape and the flags that pick the kernel's form.  Call sites name the
// fields they set.
struct SpxWalkAsk {
  int n_streams = 0;
  int max_channels = 1;
  // every job has speed > 1 and 0 <= nonlinear <= 1 (and a streamed job has never had another setting), so the time-scale
  // stage only ever sees speeds >= 1: selects the walk kernel specialised for that
  bool speedup_only = false;
  // (round 5; the batch engine) the jobs do NOT all speed up, but every speed the time-scale stage can be given is a valid one
  // below SPX_FAST_MAX_SPEED -- the speed-up kernel's instantiations that also run libsonic's insertPitchPeriod serve the batch
  // (spx_walk_fast.hip, MC + 2) instead of the general kernel
  bool any_speed = false;
  // the streams bring a few pitch steps each (coalesced sonic2.h writes): latency form whatever their number
  bool short_jobs = false;
  // no output waves (and the usual window) although the streams have a CU each -- the search waves do the output work: one walk
  // wave per SIMD instead of two, which is what lets two analysis waves of 168 registers sit beside it (22.05 kHz)
  bool lean = false;
  // the 4 + 4 form with the usual 4096-frame window where it would take the long one (36.9 instead of 69.7 KB of LDS per stream:
  // two calls' walk workgroups AND an analysis workgroup on a CU -- a mixed call whose walk kernels overlap the previous call's)
  bool short_window = false;
};
// What spx_batch_run_edits hands down (SpxCallOpts::edits): the caller's edit list.  ops: DEVICE, 16-byte records, stream i's from
// the sum of ops_cap[0 .. i) on; ops_cap: HOST; n_ops: DEVICE, the counts; total: the sum of all capacities (below 2^31).
struct SpxEditsCall {
  void* ops;
  const int64_t* ops_cap;
  int64_t* n_ops;
  int64_t total;
};
// lds_min: the caller wants the workgroups ONE to a CU (it asks for more than half a CU's LDS, spx_engine.hip); 0 otherwise
// map: DEVICE, the call's time map (spx_batch_run_map: the general kernel's map instantiation, SpxStreamDev::map_row), or null
// edits: the call's edit list (spx_batch_run_edits: the general kernel's recording instantiation), or null
void spx_launch_walk(const SpxPlanDev& P, const SpxWalkAsk& ask, const SpxStreamDev* streams, const int16_t* in, int16_t* out,
                     int64_t* n_out, SpxStreamState* states, const float* scratch, const int* speed_ready, size_t lds_min,
                     hipStream_t st, int64_t* map = nullptr, const SpxEditsCall* edits = nullptr);
// mono: every stream of the launch has one channel (the 16 kHz 16-frame instantiation then reads its samples from global memory and
// asks for no staged span)
size_t spx_analysis_lds_bytes(const SpxPlanDev& P, bool mono);
int spx_analysis_ct_window(const SpxPlanDev& P);
// The DFT of the spec run on the host (same operation order as the kernel): used to build the Rader tables.
void spx_host_dft(int n, const int* radix, int nstages, const double* tw, const double* in, double* out);
size_t spx_walk_lds_bytes(const SpxPlanDev& P, int max_channels, bool speedup_only);
// What spx_launch_walk will do for a batch (kernel instantiation, waves and LDS per stream).
struct SpxWalkConfig {
  int mode;          // 0 general, 1 mono speed-up, 2 multi-channel speed-up
  bool fast_kernel;  // mode 1 on spx_walk_fast_kernel
  int nw;            // waves per stream of spx_walk_kernel
  int nwm, nwc, wcap;  // spx_walk_fast_kernel: search waves, output waves, window frames
  int waves;         // waves per stream of the kernel that will run
  size_t lds;        // its LDS bytes per stream
  bool slow;         // the fast kernel's instantiation that also serves speeds below 1
  SpxKernelChoice kernel;  // the instantiation itself
};
SpxWalkConfig spx_walk_config(const SpxPlanDev& P, const SpxWalkAsk& ask);
SpxKernelChoice spx_walk_select(int nw, int mode);   // spx_walk.hip: the general kernel, waves per stream and mode
SpxKernelChoice spx_walk_map_select(int nw);         // ... and its instantiation that writes a time map (mode 0)
SpxKernelChoice spx_walk_edits_select(int nw);       // ... and the one that records an edit list (mode 0)
// spx_walk_fast.hip
size_t spx_walk_fast_lds_bytes(const SpxPlanDev& P, int wcap);
bool spx_walk_fast_supports(const SpxPlanDev& P, int nwm);
SpxKernelChoice spx_walk_fast_select(const SpxPlanDev& P, int nwm, int nwc, int wcap, int max_channels, bool slow);
SpxKernelChoice spx_analysis_select(int tile_frames, int ct_window);   // spx_analysis.hip; ct_window 0: the plan-driven instantiation
// n_out value of a stream whose producer kernel never delivered (concurrent mode poll limit): not an overflow
#define SPX_NOUT_LOST_PRODUCER INT64_MIN
size_t spx_tension_lds_bytes();
// VGPRs per lane the hardware allocates to a wave of the kernel that would be launched (hipFuncGetAttributes, rounded up
// to the allocation granule of 8): the engine's co-residency rule needs them
// (helper: allocated VGPRs of a kernel, cached per function -- the query is not free and the engine asks on every call)
int spx_kernel_vgprs(const void* fn, int* scratch_bytes = nullptr);   // spx_engine.hip (one cache, behind a mutex)
int spx_tension_vgprs();
int spx_analysis_vgprs(const SpxPlanDev& P, int* scratch_bytes = nullptr);
int spx_walk_vgprs(const SpxPlanDev& P, const SpxWalkAsk& ask, int* scratch_bytes);
// speedyComputeSpeedFromTension (speedy.c:768-788) on the stream's state record: *speed_out = requested speed, the
// duration sums of the record advance.
void spx_launch_speed_from_tension(SpxStreamState* state, float tension, float Rg, float feedback, float* speed_out,
                                   hipStream_t st);
int spx_analysis_tile_frames();
int spx_analysis_small_tile_frames();
int spx_analysis_tiny_tile_frames();
int spx_analysis_prefers_small_tile(const SpxPlanDev& P);

// The library's long-lived device allocations (pipeline slots, the pool's workspace and record arrays, the stream and unit APIs'
// state) go through this one helper.  g_spx_alloc_fill (spx_debug_set_alloc_fill, spx_diag.hip): -1 (default) = hipMalloc /
// hipMallocAsync and, where the site always cleared its block (zero), the fill with 0 it made before -- nothing else; 0 .. 255 = the
// new block is filled with that byte before anything else uses it, INSTEAD of the clearing, so that a kernel that relies on fresh
// memory being zero shows (tests/test_gpu_dirty_owned.py).  Read at allocation time only.
// spx_dev_alloc: hipMalloc, the fill on the null stream.  spx_dev_alloc_on: the fill on `st`, the stream whose work uses the block
// first; from_pool: hipMallocAsync on `st` instead of hipMalloc.
extern int g_spx_alloc_fill;
template <typename T>
static inline hipError_t spx_dev_alloc_impl(T** p, size_t bytes, bool zero, bool on_stream, bool from_pool, hipStream_t st) {
  void* q = nullptr;
  const hipError_t e = from_pool ? hipMallocAsync(&q, bytes, st) : hipMalloc(&q, bytes);
  if (e != hipSuccess) return e;
  *p = static_cast<T*>(q);
  const int fill = __atomic_load_n(&g_spx_alloc_fill, __ATOMIC_RELAXED);
  if (fill < 0 && !zero) return hipSuccess;
  const int v = fill < 0 ? 0 : (fill & 255);
  if (on_stream) return hipMemsetAsync(q, v, bytes, st);
  const hipError_t m = hipMemset(q, v, bytes);
  // (a debug fill on the null stream: the library's own streams do not wait for that stream, so the host does)
  return (m == hipSuccess && fill >= 0) ? hipStreamSynchronize(nullptr) : m;
}
template <typename T>
static inline hipError_t spx_dev_alloc(T** p, size_t bytes, bool zero = false) {
  return spx_dev_alloc_impl(p, bytes, zero, false, false, nullptr);
}
template <typename T>
static inline hipError_t spx_dev_alloc_on(T** p, size_t bytes, hipStream_t st, bool zero = false, bool from_pool = true) {
  return spx_dev_alloc_impl(p, bytes, zero, true, from_pool, st);
}

// Shared, cached plan per (sample rate, hysteresis mode); owned by the library for the process lifetime.
struct spx_plan;
int64_t spx_internal_out_bound(const SpxPlanDev& P, int64_t n_in, float speed, bool nonlinear);
const SpxPlanDev* spx_internal_shared_plan(int sample_rate, int match_matlab);
// false above about 61 kHz: the analysis tile does not fit one CU's LDS, the plan serves linear (TSM-only) work
bool spx_internal_analysis_fits(const SpxPlanDev& d);
int64_t spx_internal_frames_for(const SpxPlanDev& d, int64_t n_in);
