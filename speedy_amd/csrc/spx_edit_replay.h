// The edit list's replay kernel and its host routine, ONE body for spx_edit_replay (spx_edits.hip) and spx_edit_replay_scaled
// (spx_edit_scaled.hip): include/speedy_hip.h "EDIT LIST" and "EDIT LIST, SCALED".
//
// With S(x) the call's scale -- x itself for the plain call, floor(x p / q) for a master at p / q of the key's rate -- record
// (out_at, a, b, n) covers track frames [S(out_at), S(out_at + n)): n' = S(out_at + n) - S(out_at) >= 1 because p >= q, a' = S(a),
// b' = S(b), and a source frame at or behind L' reads as 0 (L' = L for the plain call, min(S(L), the track's own length) for a
// master).  tests/edit_list_ref.py and tests/edit_scaled_ref.py state the definitions; the kernel is held to them bit for bit.
//
// The kernel has no dependent chain: a grid over (output block, stream), one workgroup of 256 threads per 4096 output VALUES
// (frame x channel, interleaved as they lie in memory), bound by memory.  A block
//   * finds the records that cover its first and its last frame by a 64-way search over the stream's S(out_at) column (every wave
//     for itself, one probe per lane: two round trips to memory for a list of a thousand records; S does not decrease, so the
//     search carries over to a master, with S evaluated per probe in 64-bit),
//   * stages that slice ALREADY SCALED -- up to 512 records (S(out_at), a', b', n') and, for int16, the reciprocal of each n' for
//     the cross-fade quotient -- in LDS (12 KB, 8 for float): the scaling is paid per record and block, and the per-value loop is
//     32-bit; a slice that does not fit (records of a frame or two: speed 200) is read where it lies, through the cache,
//   * gives every lane four consecutive values per pass, four passes: the lane finds the record of its first value by a binary
//     search over the staged slice, walks on from there, and writes its four values in ONE aligned store (8 bytes of int16, 16 of
//     float).  Blocks are cut at store boundaries of the output ADDRESS, whatever out_off and the channel count are: only the
//     first and the last group of a stream fall back to scalar stores,
//   * for a master: thread 0 of block 0 writes the stream's count n_out_y.
// Source runs start at arbitrary sample offsets and are read with plain scalar-sized loads: a wave's 256 values are contiguous per
// record, so every load instruction still touches whole cache lines, and no padding is asked of y_in (aligned 8-byte loads with a
// funnel shift measured 17 to 19 % slower: profiles/edit_list.txt).
//
// Two template parameters and no other switch: the sample format F (EditInt16, EditFloat) and the scale policy P
//   EditIdentity   S(x) = x and nothing of a master compiled in: no n_out_y, no capacity of the track's own, L' = L, no scaling
//                  or saturation anywhere -- spx_edit_replay's instantiation (int16 only)
//   EditMultiply   q == 1 (3 / 1, 2 / 1, 1 / 1): one multiplication, and no division in the kernel's code
//   EditRatio      q > 1: a double division of the exact product and one correction by the remainder
// (five kernels: identity x int16, {multiply, ratio} x {int16, float}).  A policy changes what a position IS, never who computes
// it: the wave search's step and bounds stay uniform over the wave (ballot and readfirstlane depend on it).
//
// Positions are advanced and compared in UNSIGNED arithmetic in every instantiation: the record advance is
// (unsigned)f - (unsigned)out_at >= (unsigned)n, source frames are wrapped unsigned sums compared against L' < 2^31, the int16
// cross-fade numerator is an unsigned product sum.  On a contiguous list -- every list spx_batch_run_edits writes -- these are
// the signed values; on anything else the output is unspecified, as it always was, but nothing is undefined and NO RECORD,
// WHATEVER IT HOLDS, READS OUTSIDE [0, L') OF ITS TRACK OR WRITES OUTSIDE ITS n_out FRAMES, by construction, in both calls.
//
// The int16 cross-fade quotient is xfade_rcp / xfade_quot of spx_walk_common.h, the walk kernels' own (exact for n' <= 65535); the
// float one is three roundings and a correctly rounded division (-ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt, as
// spx_dtw.hip relies on).  Float samples travel as their 32 bits: a copy changes no bit of any value, NaN payloads included.
#pragma once
#include "spx_engine.h"
#include "spx_walk_common.h"

#define SPX_EDIT_THREADS 256
#define SPX_EDIT_VEC 4                                                     // values per lane and store, either sample type
#define SPX_EDIT_PASSES 4
#define SPX_EDIT_BLOCK (SPX_EDIT_THREADS * SPX_EDIT_VEC * SPX_EDIT_PASSES)   // values per workgroup
#define SPX_EDIT_SLOTS 512                                                 // records a block stages in LDS
#define SPX_EDIT_MAX_CHANNELS 65535

// What the kernel knows of a stream (HOST table in pinned memory).  The identity kernel reads neither n_in nor out_cap.
struct SpxEditStream {
  int64_t in_off, out_off;   // the track: first value of its input / output, in elements of the sample type from y_in / y_out
  int64_t op0, op_cap;       // index of the stream's first record in `ops`, and how many records its region holds
  int64_t limit;             // L of the key: n_in for a linear job, (n_in / B) * B for a nonlinear one
  int64_t key_cap;           // jobs[i].out_cap: frames at the key's rate
  int64_t n_in, out_cap;     // a master's own length and output capacity, in frames at its rate
  int32_t channels;
  uint32_t inv_channels;     // ceil(2^32 / channels): x / channels == mulhi(x, inv_channels) for x * channels <= 2^32
};

// The scale policies.  scale(x) = S(x) for |x| <= 2^32, 1 <= q <= p <= 32768: the product is below 2^48 and exact as a double, the
// double quotient is within one of the integer one, and the remainder says which way.
struct EditIdentity {
  static constexpr bool MASTER = false;
  __device__ static __forceinline__ int64_t scale(int64_t x, int, int) { return x; }
};
struct EditMultiply {
  static constexpr bool MASTER = true;
  __device__ static __forceinline__ int64_t scale(int64_t x, int p, int) { return x * p; }
};
struct EditRatio {
  static constexpr bool MASTER = true;
  __device__ static __forceinline__ int64_t scale(int64_t x, int p, int q) {
    const int64_t num = x * p;
    int64_t d = (int64_t)((double)num / (double)q);
    const int64_t r = num - d * q;
    if (r < 0) d--;
    else if (r >= q) d++;
    return d;
  }
};
__device__ __forceinline__ int edit_sat32(int64_t v) {
  return v > 0x7fffffffLL ? 0x7fffffff : (v < -0x7fffffffLL - 1 ? (int)(-0x7fffffffLL - 1) : (int)v);
}
// A position at the track's rate.  Positions of a list spx_batch_run_edits wrote fit int32 (the host refuses the call otherwise);
// those of a planted list saturate, which keeps a frame outside [0, L') outside it.
template <class P>
__device__ __forceinline__ int edit_pos(int x, int p, int q) {
  if constexpr (!P::MASTER) return x;
  else return edit_sat32(P::scale(x, p, q));
}
// A record at the track's rate: (S(out_at), a', b' or -1, n').
template <class P>
__device__ __forceinline__ int4 edit_scaled_op(const int4 op, int p, int q) {
  if constexpr (!P::MASTER) {
    return op;
  } else {
    const int64_t at = P::scale(op.x, p, q);
    const int64_t end = P::scale((int64_t)op.x + op.w, p, q);
    int4 r;
    r.x = edit_sat32(at);
    r.y = edit_pos<P>(op.y, p, q);
    r.z = op.z < 0 ? -1 : edit_pos<P>(op.z, p, q);
    r.w = edit_sat32(end - at);
    return r;
  }
}

// Where the records of a block come from: the staged slice, already scaled, or -- it did not fit -- the list itself, scaled as read.
template <bool STAGED, class P>
struct EditOps {
  const int4* lds;
  const double* rcp;
  const int4* __restrict__ glob;
  int p, q;
  __device__ __forceinline__ int out_at(int k) const { return STAGED ? lds[k].x : edit_pos<P>(glob[k].x, p, q); }
  __device__ __forceinline__ int4 op(int k) const { return STAGED ? lds[k] : edit_scaled_op<P>(glob[k], p, q); }
  __device__ __forceinline__ double inv(int k, int n) const { return STAGED ? rcp[k] : xfade_rcp(n); }
};

// the largest k in [0, nk) with S(out_at(k)) <= f (out_at(0) = 0 <= f)
template <class Ops>
__device__ __forceinline__ int edit_find(const Ops& O, int nk, int f) {
  int lo = 0, hi = nk;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (O.out_at(mid) <= f) lo = mid; else hi = mid;
  }
  return lo;
}

// The records that cover frames fa <= fb of a stream's track: *ka (*kb) = the largest k in [0, nk) with S(out_at(k)) <= fa (fb).
// Every wave searches for itself with 64 probes per round trip to memory, both searches in the same round: a list of 1 000 records
// takes two round trips where two binary searches take twenty loads one behind the other -- that chain was most of a block's life
// (profiles/edit_list.txt).  Whatever the records hold, the indices stay inside [0, nk).
template <class P>
__device__ __forceinline__ void edit_find_pair(const int4* __restrict__ g, int nk, int p, int q, int fa, int fb, int* ka, int* kb) {
  const int lane = threadIdx.x & 63;
  const int f[2] = {fa, fb};
  int lo[2] = {0, 0}, hi[2] = {nk, nk};
  while (hi[0] - lo[0] > 1 || hi[1] - lo[1] > 1) {
    int x[2], step[2];
#pragma unroll
    for (int s = 0; s < 2; s++) {                  // both probes in flight before either is looked at
      step[s] = (hi[s] - lo[s] + 63) >> 6;
      const int idx = lo[s] + lane * step[s];
      x[s] = idx < hi[s] ? g[idx].x : 0x7fffffff;
    }
#pragma unroll
    for (int s = 0; s < 2; s++) {
      // S(out_at) rises: the lanes at or below f are a prefix, and lane 0 (S(out_at(lo)) <= f) is among them; the probe past the
      // end compares as it is
      const int xs = x[s] == 0x7fffffff ? x[s] : edit_pos<P>(x[s], p, q);
      const unsigned long long at_or_below = __builtin_amdgcn_ballot_w64(xs <= f[s]);
      const int j = at_or_below ? __builtin_popcountll(at_or_below) - 1 : 0;
      lo[s] = __builtin_amdgcn_readfirstlane(lo[s] + j * step[s]);
      hi[s] = hi[s] < lo[s] + step[s] ? hi[s] : lo[s] + step[s];
    }
  }
  *ka = lo[0];
  *kb = lo[1];
}

// The two sample types.  T: a sample in memory; V: a value in registers (a float as its 32 bits).
struct EditInt16 {
  typedef int16_t T;
  typedef int V;
  static constexpr bool RCP = true;                   // the quotient takes the reciprocal of n'
  __device__ static __forceinline__ V zero() { return 0; }
  __device__ static __forceinline__ V load(const T* __restrict__ y, int64_t i) { return (int)y[i]; }
  __device__ static __forceinline__ V xfade(V a, V b, int n, int t, double inv) {
    // (|a|, |b| <= 2^15: the numerator fits for every n <= 65535; beyond, it wraps -- unsigned, so that nothing is undefined)
    return xfade_quot((int)((unsigned)a * (unsigned)(n - t) + (unsigned)b * (unsigned)t), inv);
  }
  __device__ static __forceinline__ void store1(T* dst, V v) { *dst = (int16_t)v; }
  __device__ static __forceinline__ void store4(T* dst, const V v[4]) {
    uint2 w;
    w.x = ((unsigned)v[0] & 0xffffu) | ((unsigned)v[1] << 16);
    w.y = ((unsigned)v[2] & 0xffffu) | ((unsigned)v[3] << 16);
    *reinterpret_cast<uint2*>(dst) = w;
  }
};
struct EditFloat {
  typedef float T;
  typedef unsigned V;                                 // the value's 32 bits
  static constexpr bool RCP = false;                  // (an IEEE division)
  __device__ static __forceinline__ V zero() { return 0u; }
  __device__ static __forceinline__ V load(const T* __restrict__ y, int64_t i) { return reinterpret_cast<const unsigned*>(y)[i]; }
  __device__ static __forceinline__ V xfade(V a, V b, int n, int t, double) {
    const float down = __uint_as_float(a) * (float)(n - t);
    const float up = __uint_as_float(b) * (float)t;
    return __float_as_uint((down + up) / (float)n);
  }
  __device__ static __forceinline__ void store1(T* dst, V v) { *reinterpret_cast<unsigned*>(dst) = v; }
  __device__ static __forceinline__ void store4(T* dst, const V v[4]) {
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    u4 w = {v[0], v[1], v[2], v[3]};
    // (the four registers as ONE value: otherwise the optimizer shares the fourth store with the tail's scalar stores and this one
    //  goes out as 12 + 4 bytes)
    asm volatile("" : "+v"(w));
    *reinterpret_cast<u4*>(dst) = w;
  }
};

// The values [vbase, vbase + SPX_EDIT_BLOCK) of the block's range, v counted from the store boundary (8 bytes for int16, 16 for
// float) at or below the stream's first output value (`mis` values in front of it), total = N' * channels, Lp = L'.
template <class F, class Ops>
__device__ __forceinline__ void edit_block(const Ops& O, int nk, const SpxEditStream& S, int Lp, int64_t vbase, int mis,
                                           int64_t total, const typename F::T* __restrict__ yin, typename F::T* __restrict__ yout) {
  typedef typename F::V V;
  const int C = S.channels;
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
    double inv = F::RCP && op.z >= 0 ? O.inv(k, op.w) : 0.0;
    V val[SPX_EDIT_VEC];
    bool ok[SPX_EDIT_VEC];
#pragma unroll
    for (int j = 0; j < SPX_EDIT_VEC; j++) {
      const int64_t e = e0 + j;
      ok[j] = e >= 0 && e < total;
      val[j] = F::zero();
      if (!ok[j]) continue;
      // the next record (n' >= 1: at most a frame's worth of steps); f - S(out_at) as unsigned, so that nothing a record holds overflows
      while ((unsigned)f - (unsigned)op.x >= (unsigned)op.w && k + 1 < nk) {
        k++;
        op = O.op(k);
        inv = F::RCP && op.z >= 0 ? O.inv(k, op.w) : 0.0;
      }
      const int t = (int)((unsigned)f - (unsigned)op.x);
      // (a frame outside [0, L') reads as 0 -- the flush's padding; and no record, whatever it holds, reads outside the track: the
      //  sums wrap as unsigned, and a wrapped one is at or above 2^31 > L'; below L' a frame is an int again, and its index one
      //  32 x 32-bit multiplication)
      const unsigned fa = (unsigned)op.y + (unsigned)t;
      const V a = fa < (unsigned)Lp ? F::load(yin, (int64_t)(int)fa * C + c) : F::zero();
      if (op.z < 0) {
        val[j] = a;
      } else {
        const unsigned fb = (unsigned)op.z + (unsigned)t;
        const V b = fb < (unsigned)Lp ? F::load(yin, (int64_t)(int)fb * C + c) : F::zero();
        val[j] = F::xfade(a, b, op.w, t, inv);
      }
      if (++c == C) { c = 0; f++; }
    }
    typename F::T* dst = yout + e0;
    if (ok[0] && ok[SPX_EDIT_VEC - 1]) {           // the whole group: one aligned store
      F::store4(dst, val);
    } else {                                        // the stream's head or tail
#pragma unroll
      for (int j = 0; j < SPX_EDIT_VEC; j++)
        if (ok[j]) F::store1(dst + j, val[j]);
    }
  }
}

// p, q and n_out_y: a master's (the identity kernel reads none of them).
template <class F, class P>
__global__ void __launch_bounds__(SPX_EDIT_THREADS)
spx_edit_replay_kernel(const SpxEditStream* __restrict__ streams, int stream0, const int4* __restrict__ ops,
                       const int64_t* __restrict__ n_ops, const int64_t* __restrict__ n_out, int p, int q,
                       const typename F::T* __restrict__ y_in, typename F::T* __restrict__ y_out, int64_t* __restrict__ n_out_y) {
  typedef typename F::T T;
  __shared__ int4 s_ops[SPX_EDIT_SLOTS];
  __shared__ double s_rcp[SPX_EDIT_SLOTS];
  const int s = stream0 + (int)blockIdx.y;
  const SpxEditStream S = streams[s];
  int64_t no = n_out[s];
  const int64_t nk64 = n_ops[s];
  const bool reports = P::MASTER && blockIdx.x == 0 && threadIdx.x == 0;
  // nothing for a stream without output, or one whose list did not fit (and never more than the region holds or the list has)
  if (no <= 0 || nk64 <= 0 || nk64 > S.op_cap) {
    if (reports) n_out_y[s] = 0;
    return;
  }
  if (no > S.key_cap) no = S.key_cap;
  if (no > 0x7fffffff) no = 0x7fffffff;
  if (no < 0) no = 0;
  const int64_t Np = P::scale(no, p, q);                    // N' (the host made sure it fits int32)
  if constexpr (P::MASTER) {
    if (Np > S.out_cap) {
      if (reports) n_out_y[s] = -Np;
      return;
    }
    if (reports) n_out_y[s] = Np;
  }
  int64_t Lp64 = P::scale(S.limit, p, q);
  if constexpr (P::MASTER)
    if (Lp64 > S.n_in) Lp64 = S.n_in;
  const int Lp = (int)(Lp64 > 0x7fffffff ? 0x7fffffff : Lp64);
  const int nk = (int)nk64;
  const int C = S.channels;
  T* __restrict__ yout = y_out + S.out_off;
  const T* __restrict__ yin = y_in + S.in_off;
  const int mis = (int)((reinterpret_cast<uintptr_t>(yout) / sizeof(T)) & (SPX_EDIT_VEC - 1));
  const int64_t total = Np * C;
  const int64_t vbase = (int64_t)blockIdx.x * SPX_EDIT_BLOCK;
  if (total == 0 || vbase >= total + mis) return;
  int64_t vend = vbase + SPX_EDIT_BLOCK;
  if (vend > total + mis) vend = total + mis;
  const int f_first = (int)((vbase > mis ? vbase - mis : 0) / C);
  const int f_last = (int)((vend - mis - 1) / C);
  const int4* __restrict__ gops = ops + S.op0;
  int k0, k1;
  edit_find_pair<P>(gops, nk, p, q, f_first, f_last, &k0, &k1);
  const int kn = k1 - k0 + 1;
  if (kn <= SPX_EDIT_SLOTS) {
    for (int t = threadIdx.x; t < kn; t += SPX_EDIT_THREADS) {
      const int4 op = edit_scaled_op<P>(gops[k0 + t], p, q);
      s_ops[t] = op;
      if (F::RCP) s_rcp[t] = op.z >= 0 ? xfade_rcp(op.w) : 0.0;
    }
    __syncthreads();
    const EditOps<true, P> O = {s_ops, s_rcp, nullptr, p, q};
    edit_block<F>(O, kn, S, Lp, vbase, mis, total, yin, yout);
  } else {
    const EditOps<false, P> O = {nullptr, nullptr, gops + k0, p, q};
    edit_block<F>(O, kn, S, Lp, vbase, mis, total, yin, yout);
  }
}

// What an entry point says of stream i's track.  n_in and out_cap are a master's (the plain call leaves them 0).
struct SpxEditTrackDesc {
  int64_t in_off, out_off, n_in, out_cap;
  int32_t channels;
};

// The host side of both calls behind their own argument checks: the per-stream checks (`who` prefixes every refusal), the table,
// the grid's width, the table's trip through one of the plan's two pinned staging slots (SpxStage, spx_engine.h, as
// spx_map_lookup's) and the launches.
//   track(i)                        stream i's SpxEditTrackDesc
//   frames(i, key_frames, limit)    the frames the stream's output region can hold at the track's rate, from the key's
//                                   min(out_cap, 2^31 - 1) and L; negative after a refusal of its own
//   launch(grid, table, s0, st)     the call's kernel on streams [s0, s0 + grid.y)
// last_gx, last_launches: the call's debug counters.
template <class Track, class Frames, class Launch>
static int edit_replay_run(const char* who, spx_plan_t plan, const spx_stream_job* jobs, int n, const int64_t* ops_cap, void* hs,
                           std::atomic<int>& last_gx, std::atomic<int>& last_launches, Track track, Frames frames, Launch launch) {
  const auto refuse = [who](const char* why) { return fail(-1, std::string(who) + ": " + why); };
  const int B = plan->dev.B;
  std::vector<SpxEditStream> tab((size_t)n);
  int64_t row = 0, gx = 1;
  for (int i = 0; i < n; i++) {
    const SpxEditTrackDesc t = track(i);
    if (t.channels < 1 || t.channels > SPX_EDIT_MAX_CHANNELS) return refuse("a track's channels are outside 1 .. 65535");
    if (t.in_off < 0 || t.out_off < 0) return refuse("a negative track offset");
    if (t.n_in < 0 || t.out_cap < 0) return refuse("a negative track length or capacity");
    if (ops_cap[i] < 0) return refuse("a negative capacity");
    SpxEditStream& s = tab[i];
    s.in_off = t.in_off; s.out_off = t.out_off;
    s.op0 = row; s.op_cap = ops_cap[i];
    s.limit = jobs[i].nonlinear != 0.0f ? jobs[i].n_in / B * B : jobs[i].n_in;
    s.key_cap = jobs[i].out_cap;
    s.n_in = t.n_in; s.out_cap = t.out_cap;
    s.channels = t.channels;
    s.inv_channels = (uint32_t)((0x100000000ull + (uint64_t)t.channels - 1) / (uint64_t)t.channels);
    row += ops_cap[i];
    if (row > 0x7fffffff) return refuse("more than 2^31 - 1 records of capacity in one call");
    const int64_t cap_frames = frames(i, jobs[i].out_cap > 0x7fffffff ? (int64_t)0x7fffffff : jobs[i].out_cap, s.limit);
    if (cap_frames < 0) return -1;
    const int64_t blocks = (cap_frames * t.channels + (SPX_EDIT_VEC - 1) + SPX_EDIT_BLOCK - 1) / SPX_EDIT_BLOCK;
    if (blocks > gx) gx = blocks;
  }
  if (gx > 0x7fffffff) return refuse("a track of more than 2^43 values");
  hipStream_t st = static_cast<hipStream_t>(hs);
  std::lock_guard<std::mutex> plan_lock(plan->mu);
  SpxStage& G = plan->stage.take();
  if (G.acquire(sizeof(SpxEditStream) * (size_t)n)) return -2;
  memcpy(G.p, tab.data(), sizeof(SpxEditStream) * (size_t)n);
  last_gx.store((int)gx, std::memory_order_relaxed);
  last_launches.store((n + 65534) / 65535, std::memory_order_relaxed);
  for (int s0 = 0; s0 < n; s0 += 65535) {   // (the grid's second dimension holds 65 535)
    const int m = n - s0 < 65535 ? n - s0 : 65535;
    launch(dim3((unsigned)gx, (unsigned)m), static_cast<const SpxEditStream*>(G.p), s0, st);
  }
  if (G.release(st)) return -2;
  HIPCHK(hipGetLastError());
  return 0;
}
