// Edit list of a batch call (include/speedy_hip.h "EDIT LIST": spx_plan_edit_ops, spx_batch_run_edits, spx_edit_replay): the exact
// list of copy and cross-fade operations a job performed, and its replay on any other track of the same length.
//
// The records come from the general walk kernel's recording instantiation (spx_walk.hip, spx_walk_edits_kernel: record_op, one
// 16-byte store per emit_copy / emit_overlap_add).  spx_batch_run_edits is spx_batch_run with SpxCallOpts::edits set (run_impl: the
// whole batch on the general kernel, kernels in sequence on the caller's stream, as a map call).
//
// The replay kernel has no dependent chain: a grid over (output block, stream), one workgroup of 256 threads per 4096 output VALUES
// (frame x channel, interleaved as they lie in memory), bound by memory.  A block
//   * finds the records that cover its first and its last frame by a 64-way search over the stream's out_at column (every wave for
//     itself, one probe per lane: two round trips to memory for a list of a thousand records),
//   * stages that slice -- up to 512 records, and the reciprocal of each n for the cross-fade quotient -- in LDS (12 KB); a slice
//     that does not fit (records of a frame or two: speed 200) is read where it lies, through the cache,
//   * gives every lane four consecutive values per pass, four passes: the lane finds the record of its first value by a binary
//     search over the staged slice, walks on from there, and writes its four values in ONE aligned 8-byte store.  Blocks are cut at
//     8-byte boundaries of the output ADDRESS, whatever out_off and the channel count are: only the first and the last group of a
//     stream fall back to 2-byte stores.
// Source runs start at arbitrary int16 offsets and are read with plain 2-byte loads: a wave's 256 values are contiguous per record,
// so every load instruction still touches whole cache lines, and nothing is ever read outside [0, L) of a track (no padding is
// asked of y_in).  The form with aligned 8-byte loads and a funnel shift (-DSPX_EDIT_ALIGNED_LOADS=1) measured 17 to 19 % slower
// (profiles/edit_list.txt): the kernel waits on latencies, not on bytes.
// The cross-fade quotient is xfade_rcp / xfade_quot of spx_walk_common.h, the walk kernels' own.
#include "spx_engine.h"
#include "spx_walk_common.h"

#define SPX_EDIT_THREADS 256
#define SPX_EDIT_VEC 4                                                     // int16 values per lane and store
#define SPX_EDIT_PASSES 4
#define SPX_EDIT_BLOCK (SPX_EDIT_THREADS * SPX_EDIT_VEC * SPX_EDIT_PASSES)   // values per workgroup
#define SPX_EDIT_SLOTS 512                                                 // records a block stages in LDS
#define SPX_EDIT_MAX_CHANNELS 65535

// What the replay kernel knows of a stream (HOST table in pinned memory).
struct SpxEditStream {
  int64_t in_off, out_off;   // the track: first value of its input / output, in int16 values from y_in / y_out
  int64_t op0, op_cap;       // index of the stream's first record in `ops`, and how many records its region holds
  int64_t limit;             // L: source frames at or behind it read as 0
  int64_t out_cap;           // frames the output region holds
  int32_t channels;
  uint32_t inv_channels;     // ceil(2^32 / channels): x / channels == mulhi(x, inv_channels) for x * channels <= 2^32
};

// Where the records of a block come from: the staged slice, or -- it did not fit -- the list itself.
template <bool STAGED>
struct EditOps {
  const int4* lds;
  const double* rcp;
  const int4* __restrict__ glob;
  __device__ __forceinline__ int out_at(int k) const { return STAGED ? lds[k].x : glob[k].x; }
  __device__ __forceinline__ int4 op(int k) const { return STAGED ? lds[k] : glob[k]; }
  __device__ __forceinline__ double inv(int k, int n) const { return STAGED ? rcp[k] : xfade_rcp(n); }
};

// the largest k in [0, nk) with out_at(k) <= f (out_at(0) = 0 <= f)
template <class Ops>
__device__ __forceinline__ int edit_find(const Ops& O, int nk, int f) {
  int lo = 0, hi = nk;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (O.out_at(mid) <= f) lo = mid; else hi = mid;
  }
  return lo;
}

// The records that cover frames fa <= fb of a stream: *ka (*kb) = the largest k in [0, nk) with out_at(k) <= fa (fb).  Every wave
// searches for itself with 64 probes per round trip to memory, both searches in the same round: a list of 1 000 records takes two
// round trips where two binary searches take twenty loads one behind the other -- that chain was most of a block's life
// (profiles/edit_list.txt).  Whatever the records hold, the indices stay inside [0, nk).
__device__ __forceinline__ void edit_find_pair(const int4* __restrict__ g, int nk, int fa, int fb, int* ka, int* kb) {
  const int lane = threadIdx.x & 63;
  const int f[2] = {fa, fb};
  int lo[2] = {0, 0}, hi[2] = {nk, nk};
  while (hi[0] - lo[0] > 1 || hi[1] - lo[1] > 1) {
    int x[2], step[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {                  // both probes in flight before either is looked at
      step[q] = (hi[q] - lo[q] + 63) >> 6;
      const int idx = lo[q] + lane * step[q];
      x[q] = idx < hi[q] ? g[idx].x : 0x7fffffff;
    }
#pragma unroll
    for (int q = 0; q < 2; q++) {
      // out_at rises: the lanes at or below f are a prefix, and lane 0 (out_at(lo) <= f) is among them
      const unsigned long long at_or_below = __builtin_amdgcn_ballot_w64(x[q] <= f[q]);
      const int j = at_or_below ? __builtin_popcountll(at_or_below) - 1 : 0;
      lo[q] = __builtin_amdgcn_readfirstlane(lo[q] + j * step[q]);
      hi[q] = hi[q] < lo[q] + step[q] ? hi[q] : lo[q] + step[q];
    }
  }
  *ka = lo[0];
  *kb = lo[1];
}

// -DSPX_EDIT_ALIGNED_LOADS=1: the other load form, for A/B runs (profiles/edit_list.txt has both).  A group whose four values come
// from ONE record, with every source frame inside [0, L), reads each source run as the one or two aligned 8-byte words that hold it
// and shifts the four values out; the words must lie inside the track too (y_in is read nowhere else), so a track's first and
// last values, like every group that straddles two records, take the 2-byte loads.
#ifndef SPX_EDIT_ALIGNED_LOADS
#define SPX_EDIT_ALIGNED_LOADS 0
#endif
// four values from element s of a track of `len` elements, if the aligned words around them lie inside the track
__device__ __forceinline__ bool edit_load4(const int16_t* __restrict__ y, int64_t s, int64_t len, int out[4]) {
  const uintptr_t addr = reinterpret_cast<uintptr_t>(y + s);
  const unsigned m = (unsigned)(addr >> 1) & 3u;                 // values between the word's start and element s
  if (s - (int64_t)m < 0 || s - (int64_t)m + (m ? 8 : 4) > len) return false;
  const uint2* q = reinterpret_cast<const uint2*>(addr & ~(uintptr_t)7);
  const uint2 w0 = q[0];
  unsigned long long v = (unsigned long long)w0.x | ((unsigned long long)w0.y << 32);
  if (m) {
    const uint2 w1 = q[1];
    const unsigned long long h = (unsigned long long)w1.x | ((unsigned long long)w1.y << 32);
    v = (v >> (16 * m)) | (h << (64 - 16 * m));
  }
  out[0] = (int)(short)(v & 0xffffu); out[1] = (int)(short)((v >> 16) & 0xffffu);
  out[2] = (int)(short)((v >> 32) & 0xffffu); out[3] = (int)(short)(v >> 48);
  return true;
}

// The values [v0, v1) of the block's range, v counted from the 8-byte boundary at or below the stream's first output value (`mis`
// values in front of it), total = n_out * channels.
template <bool STAGED>
__device__ __forceinline__ void edit_block(const EditOps<STAGED>& O, int nk, const SpxEditStream& S, int64_t vbase, int mis, int64_t total,
                                           const int16_t* __restrict__ yin, int16_t* __restrict__ yout) {
  const int C = S.channels;
  const int L = (int)S.limit;
  // frame and channel of the block's first value (64-bit once per block; a lane's values are 32-bit offsets from there)
  const int64_t e_blk = vbase > mis ? vbase - mis : 0;
  const int64_t f_blk = e_blk / C;
  const int c_blk = (int)(e_blk - f_blk * C);
#pragma unroll 1
  for (int pass = 0; pass < SPX_EDIT_PASSES; pass++) {
    const int64_t v = vbase + (int64_t)(pass * SPX_EDIT_THREADS + (int)threadIdx.x) * SPX_EDIT_VEC;
    const int64_t e0 = v - mis;                    // the group's first value in the stream (negative: in front of it)
    if (e0 + SPX_EDIT_VEC <= 0 || e0 >= total) continue;
    const int64_t e_first = e0 < 0 ? 0 : e0;
    const unsigned r = (unsigned)(e_first - e_blk);                      // < SPX_EDIT_BLOCK: r * channels < 2^32
    unsigned df = C == 1 ? r : __umulhi(r, S.inv_channels);
    int c = (int)(r - df * (unsigned)C) + c_blk;
    if (c >= C) { c -= C; df++; }
    int f = (int)(f_blk + df);
    int k = edit_find(O, nk, f);
    int4 op = O.op(k);
    double inv = op.z >= 0 ? O.inv(k, op.w) : 0.0;
    int val[SPX_EDIT_VEC];
    bool ok[SPX_EDIT_VEC];
    bool done = false;
    if (SPX_EDIT_ALIGNED_LOADS && e0 >= 0 && e0 + SPX_EDIT_VEC <= total) {
      while (f >= op.x + op.w && k + 1 < nk) {
        k++;
        op = O.op(k);
        inv = op.z >= 0 ? O.inv(k, op.w) : 0.0;
      }
      int tj[SPX_EDIT_VEC];                          // each value's frame inside the record
      int fj = f, cj = c;
#pragma unroll
      for (int j = 0; j < SPX_EDIT_VEC; j++) {
        tj[j] = fj - op.x;
        if (++cj == C) { cj = 0; fj++; }
      }
      const int t0 = tj[0], t3 = tj[SPX_EDIT_VEC - 1];
      const int64_t len = (int64_t)L * C;
      int av[4], bv[4];
      if (t0 >= 0 && t3 < op.w && op.y + t0 >= 0 && op.y + t3 < L && (op.z < 0 || (op.z + t0 >= 0 && op.z + t3 < L)) &&
          edit_load4(yin, (int64_t)(op.y + t0) * C + c, len, av) && (op.z < 0 || edit_load4(yin, (int64_t)(op.z + t0) * C + c, len, bv))) {
#pragma unroll
        for (int j = 0; j < SPX_EDIT_VEC; j++) {
          ok[j] = true;
          val[j] = op.z < 0 ? av[j] : xfade_quot(av[j] * (op.w - tj[j]) + bv[j] * tj[j], inv);
        }
        done = true;
      }
    }
#pragma unroll
    for (int j = 0; j < SPX_EDIT_VEC; j++) {
      if (done) break;
      const int64_t e = e0 + j;
      ok[j] = e >= 0 && e < total;
      val[j] = 0;
      if (!ok[j]) continue;
      while (f >= op.x + op.w && k + 1 < nk) {     // the next record (n >= 1: at most a frame's worth of steps)
        k++;
        op = O.op(k);
        inv = op.z >= 0 ? O.inv(k, op.w) : 0.0;
      }
      const int t = f - op.x;
      const int fa = op.y + t;
      // (a frame outside [0, L) reads as 0 -- the flush's padding; and no record, whatever it holds, reads outside the track)
      const int a = (unsigned)fa < (unsigned)L ? (int)yin[(int64_t)fa * C + c] : 0;
      if (op.z < 0) {
        val[j] = a;
      } else {
        const int fb = op.z + t;
        const int b = (unsigned)fb < (unsigned)L ? (int)yin[(int64_t)fb * C + c] : 0;
        val[j] = xfade_quot(a * (op.w - t) + b * t, inv);
      }
      if (++c == C) { c = 0; f++; }
    }
    int16_t* dst = yout + e0;
    if (ok[0] && ok[SPX_EDIT_VEC - 1]) {           // the whole group: one aligned 8-byte store
      uint2 w;
      w.x = ((unsigned)val[0] & 0xffffu) | ((unsigned)val[1] << 16);
      w.y = ((unsigned)val[2] & 0xffffu) | ((unsigned)val[3] << 16);
      *reinterpret_cast<uint2*>(dst) = w;
    } else {                                        // the stream's head or tail
#pragma unroll
      for (int j = 0; j < SPX_EDIT_VEC; j++)
        if (ok[j]) dst[j] = (int16_t)val[j];
    }
  }
}

__global__ void __launch_bounds__(SPX_EDIT_THREADS)
spx_edit_replay_kernel(const SpxEditStream* __restrict__ streams, int stream0, const int4* __restrict__ ops,
                       const int64_t* __restrict__ n_ops, const int64_t* __restrict__ n_out, const int16_t* __restrict__ y_in,
                       int16_t* __restrict__ y_out) {
  __shared__ int4 s_ops[SPX_EDIT_SLOTS];
  __shared__ double s_rcp[SPX_EDIT_SLOTS];
  const int s = stream0 + (int)blockIdx.y;
  const SpxEditStream S = streams[s];
  int64_t no = n_out[s];
  const int64_t nk64 = n_ops[s];
  // nothing for a stream without output, or one whose list did not fit (and never more than the region holds or the list has)
  if (no <= 0 || nk64 <= 0 || nk64 > S.op_cap) return;
  if (no > S.out_cap) no = S.out_cap;
  if (no > 0x7fffffff) no = 0x7fffffff;
  const int nk = (int)nk64;
  const int C = S.channels;
  int16_t* __restrict__ yout = y_out + S.out_off;
  const int16_t* __restrict__ yin = y_in + S.in_off;
  const int mis = (int)((reinterpret_cast<uintptr_t>(yout) >> 1) & (SPX_EDIT_VEC - 1));
  const int64_t total = no * C;
  const int64_t vbase = (int64_t)blockIdx.x * SPX_EDIT_BLOCK;
  if (vbase >= total + mis) return;
  int64_t vend = vbase + SPX_EDIT_BLOCK;
  if (vend > total + mis) vend = total + mis;
  const int f_first = (int)((vbase > mis ? vbase - mis : 0) / C);
  const int f_last = (int)((vend - mis - 1) / C);
  const int4* __restrict__ gops = ops + S.op0;
  int k0, k1;
  edit_find_pair(gops, nk, f_first, f_last, &k0, &k1);
  const int kn = k1 - k0 + 1;
  if (kn <= SPX_EDIT_SLOTS) {
    for (int t = threadIdx.x; t < kn; t += SPX_EDIT_THREADS) {
      const int4 op = gops[k0 + t];
      s_ops[t] = op;
      s_rcp[t] = op.z >= 0 ? xfade_rcp(op.w) : 0.0;
    }
    __syncthreads();
    const EditOps<true> O = {s_ops, s_rcp, nullptr};
    edit_block<true>(O, kn, S, vbase, mis, total, yin, yout);
  } else {
    const EditOps<false> O = {nullptr, nullptr, gops + k0};
    edit_block<false>(O, kn, S, vbase, mis, total, yin, yout);
  }
}

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
  const int B = plan->dev.B;
  std::vector<SpxEditStream> tab((size_t)n);
  int64_t row = 0, gx = 1;
  for (int i = 0; i < n; i++) {
    const spx_edit_track& t = tracks[i];
    if (t.channels < 1 || t.channels > SPX_EDIT_MAX_CHANNELS) return fail(-1, "spx_edit_replay: a track's channels are outside 1 .. 65535");
    if (t.in_off < 0 || t.out_off < 0) return fail(-1, "spx_edit_replay: a negative track offset");
    if (ops_cap[i] < 0) return fail(-1, "spx_edit_replay: a negative capacity");
    SpxEditStream& s = tab[i];
    s.in_off = t.in_off; s.out_off = t.out_off;
    s.op0 = row; s.op_cap = ops_cap[i];
    s.limit = jobs[i].nonlinear != 0.0f ? jobs[i].n_in / B * B : jobs[i].n_in;
    s.out_cap = jobs[i].out_cap;
    s.channels = t.channels;
    s.inv_channels = (uint32_t)((0x100000000ull + (uint64_t)t.channels - 1) / (uint64_t)t.channels);
    row += ops_cap[i];
    if (row > 0x7fffffff) return fail(-1, "spx_edit_replay: more than 2^31 - 1 records of capacity in one call");
    const int64_t cap_frames = jobs[i].out_cap > 0x7fffffff ? 0x7fffffff : jobs[i].out_cap;
    const int64_t blocks = (cap_frames * t.channels + (SPX_EDIT_VEC - 1) + SPX_EDIT_BLOCK - 1) / SPX_EDIT_BLOCK;
    if (blocks > gx) gx = blocks;
  }
  if (gx > 0x7fffffff) return fail(-1, "spx_edit_replay: a track of more than 2^43 values");
  hipStream_t st = static_cast<hipStream_t>(hs);
  std::lock_guard<std::mutex> plan_lock(plan->mu);
  // the table: through one of the plan's two pinned staging slots (SpxStage, spx_engine.h), as spx_map_lookup's
  SpxStage& G = plan->stage.take();
  if (G.acquire(sizeof(SpxEditStream) * (size_t)n)) return -2;
  memcpy(G.p, tab.data(), sizeof(SpxEditStream) * (size_t)n);
  g_last_replay_gx.store((int)gx, std::memory_order_relaxed);
  g_last_replay_launches.store((n + 65534) / 65535, std::memory_order_relaxed);
  for (int s0 = 0; s0 < n; s0 += 65535) {   // (the grid's second dimension holds 65 535)
    const int m = n - s0 < 65535 ? n - s0 : 65535;
    hipLaunchKernelGGL(spx_edit_replay_kernel, dim3((unsigned)gx, (unsigned)m), dim3(SPX_EDIT_THREADS), 0, st,
                       static_cast<const SpxEditStream*>(G.p), s0, reinterpret_cast<const int4*>(ops), n_ops, n_out, y_in, y_out);
  }
  if (G.release(st)) return -2;
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
