// Replay of an edit list on tracks at a HIGHER sample rate, int16 or float (include/speedy_hip.h "EDIT LIST, SCALED":
// spx_edit_scale, spx_edit_replay_scaled): speed and pitch are decided on a 16 kHz key, and the 44.1 or 48 kHz master the key was
// made from is cut in the same places.  tests/edit_scaled_ref.py states the definition in Python integers (and np.float32 scalars for
// the float cross-fade); the kernel is held to it bit for bit.
//
// With S(x) = floor(x p / q), p / q the master's rate over the key's, record (out_at, a, b, n) covers master frames
// [S(out_at), S(out_at + n)): n' = S(out_at + n) - S(out_at) >= 1 because p >= q, a' = S(a), b' = S(b), and a source frame at or
// behind L' = min(S(L), the track's own length) reads as 0.
//
// The kernel has spx_edit_replay_kernel's shape (spx_edits.hip, which stays what it is and is the comparison point): a grid over
// (output block, stream), one workgroup of 256 threads per 4096 output VALUES, the block's slice of records staged in LDS with the
// unstaged fallback, four values per lane and pass in ONE aligned store.  What differs:
//   * the block search runs over S(out_at) -- S is non-decreasing, so the 64-way search carries over -- and evaluates S per probe in
//     64-bit;
//   * the slice is staged ALREADY SCALED (S(out_at), a', b', n' and the reciprocal of n'): the scaling is paid per record and block,
//     and the per-value loop stays 32-bit;
//   * the sample type is a template parameter: int16 values go out as one aligned 8-byte store, floats as one aligned 16-byte store,
//     with scalar stores at a stream's head and tail;
//   * thread 0 of block 0 writes the stream's count n_out_y.
// The int16 cross-fade quotient is xfade_rcp / xfade_quot of spx_walk_common.h (exact for n' <= 65535); the float one is three
// roundings and a correctly rounded division (-ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt, as spx_dtw.hip relies on).
// Float samples travel as their 32 bits: a copy changes no bit of any value, NaN payloads included.
#include "spx_engine.h"
#include "spx_walk_common.h"

#define SPX_ESC_THREADS 256
#define SPX_ESC_VEC 4                                                     // values per lane and store, either sample type
#define SPX_ESC_PASSES 4
#define SPX_ESC_BLOCK (SPX_ESC_THREADS * SPX_ESC_VEC * SPX_ESC_PASSES)    // values per workgroup
#define SPX_ESC_SLOTS 512                                                 // records a block stages in LDS
#define SPX_ESC_MAX_CHANNELS 65535
#define SPX_ESC_MAX_P 32768
#define SPX_ESC_MAX_RATIO 32

// What the kernel knows of a stream (HOST table in pinned memory).
struct SpxScaledStream {
  int64_t in_off, out_off;   // the track: first value of its input / output, in elements of the sample type from y_in / y_out
  int64_t op0, op_cap;       // index of the stream's first record in `ops`, and how many records its region holds
  int64_t limit;             // L of the key: n_in for a linear job, (n_in / B) * B for a nonlinear one
  int64_t key_cap;           // jobs[i].out_cap: frames at the key's rate
  int64_t n_in, out_cap;     // the track's own length and output capacity, in frames at the master's rate
  int32_t channels;
  uint32_t inv_channels;     // ceil(2^32 / channels): x / channels == mulhi(x, inv_channels) for x * channels <= 2^32
};

// S(x) = floor(x p / q) for |x| <= 2^32, 1 <= q <= p <= 32768: the product is below 2^48 and exact as a double, the double
// quotient is within one of the integer one, and the remainder says which way.  QONE: q == 1 (3 / 1, 2 / 1, 1 / 1 -- the kernel has
// an instantiation of its own for these: one multiplication, and no division in its code).
template <bool QONE>
__device__ __forceinline__ int64_t esc_scale(int64_t x, int p, int q) {
  const int64_t num = x * p;
  if (QONE) return num;
  int64_t d = (int64_t)((double)num / (double)q);
  const int64_t r = num - d * q;
  if (r < 0) d--;
  else if (r >= q) d++;
  return d;
}
__device__ __forceinline__ int esc_sat32(int64_t v) {
  return v > 0x7fffffffLL ? 0x7fffffff : (v < -0x7fffffffLL - 1 ? (int)(-0x7fffffffLL - 1) : (int)v);
}
// A record at the master's rate: (S(out_at), a', b' or -1, n').  Positions of a list spx_batch_run_edits wrote fit int32 (the host
// refuses the call otherwise); those of a planted list saturate, which keeps a frame outside [0, L') outside it.
template <bool QONE>
__device__ __forceinline__ int4 esc_scaled_op(const int4 op, int p, int q) {
  const int64_t at = esc_scale<QONE>(op.x, p, q);
  const int64_t end = esc_scale<QONE>((int64_t)op.x + op.w, p, q);
  int4 r;
  r.x = esc_sat32(at);
  r.y = esc_sat32(esc_scale<QONE>(op.y, p, q));
  r.z = op.z < 0 ? -1 : esc_sat32(esc_scale<QONE>(op.z, p, q));
  r.w = esc_sat32(end - at);
  return r;
}

// Where the records of a block come from: the staged slice, already scaled, or -- it did not fit -- the list itself, scaled as read.
template <bool STAGED, bool QONE>
struct EscOps {
  const int4* lds;
  const double* rcp;
  const int4* __restrict__ glob;
  int p, q;
  __device__ __forceinline__ int out_at(int k) const { return STAGED ? lds[k].x : esc_sat32(esc_scale<QONE>(glob[k].x, p, q)); }
  __device__ __forceinline__ int4 op(int k) const { return STAGED ? lds[k] : esc_scaled_op<QONE>(glob[k], p, q); }
  __device__ __forceinline__ double inv(int k, int n) const { return STAGED ? rcp[k] : xfade_rcp(n); }
};

// the largest k in [0, nk) with S(out_at(k)) <= f (out_at(0) = 0 <= f)
template <class Ops>
__device__ __forceinline__ int esc_find(const Ops& O, int nk, int f) {
  int lo = 0, hi = nk;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (O.out_at(mid) <= f) lo = mid; else hi = mid;
  }
  return lo;
}

// The records that cover master frames fa <= fb of a stream: *ka (*kb) = the largest k in [0, nk) with S(out_at(k)) <= fa (fb).
// Every wave searches for itself with 64 probes per round trip to memory, both searches in the same round (edit_find_pair of
// spx_edits.hip, with S evaluated per probe).  Whatever the records hold, the indices stay inside [0, nk).
template <bool QONE>
__device__ __forceinline__ void esc_find_pair(const int4* __restrict__ g, int nk, int p, int q, int fa, int fb, int* ka, int* kb) {
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
      // S(out_at) rises: the lanes at or below f are a prefix, and lane 0 (S(out_at(lo)) <= f) is among them
      const int xs = x[s] == 0x7fffffff ? x[s] : esc_sat32(esc_scale<QONE>(x[s], p, q));
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
struct EscInt16 {
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
struct EscFloat {
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

// The values [vbase, vbase + SPX_ESC_BLOCK) of the block's range, v counted from the store boundary (8 bytes for int16, 16 for
// float) at or below the stream's first output value (`mis` values in front of it), total = N' * channels, Lp = L'.
template <class F, class Ops>
__device__ __forceinline__ void esc_block(const Ops& O, int nk, const SpxScaledStream& S, int Lp, int64_t vbase, int mis,
                                          int64_t total, const typename F::T* __restrict__ yin, typename F::T* __restrict__ yout) {
  typedef typename F::V V;
  const int C = S.channels;
  // frame and channel of the block's first value (64-bit once per block; a lane's values are 32-bit offsets from there)
  const int64_t e_blk = vbase > mis ? vbase - mis : 0;
  const int64_t f_blk = e_blk / C;
  const int c_blk = (int)(e_blk - f_blk * C);
#pragma unroll 1
  for (int pass = 0; pass < SPX_ESC_PASSES; pass++) {
    const int64_t v = vbase + (int64_t)(pass * SPX_ESC_THREADS + (int)threadIdx.x) * SPX_ESC_VEC;
    const int64_t e0 = v - mis;                    // the group's first value in the stream (negative: in front of it)
    if (e0 + SPX_ESC_VEC <= 0 || e0 >= total) continue;
    const int64_t e_first = e0 < 0 ? 0 : e0;
    const unsigned r = (unsigned)(e_first - e_blk);                      // < SPX_ESC_BLOCK: r * channels < 2^32
    unsigned df = C == 1 ? r : __umulhi(r, S.inv_channels);
    int c = (int)(r - df * (unsigned)C) + c_blk;
    if (c >= C) { c -= C; df++; }
    int f = (int)(f_blk + df);
    int k = esc_find(O, nk, f);
    int4 op = O.op(k);
    double inv = F::RCP && op.z >= 0 ? O.inv(k, op.w) : 0.0;
    V val[SPX_ESC_VEC];
    bool ok[SPX_ESC_VEC];
#pragma unroll
    for (int j = 0; j < SPX_ESC_VEC; j++) {
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
      // (a frame outside [0, L') reads as 0; and no record, whatever it holds, reads outside the track: the sums wrap as unsigned,
      //  and a wrapped one is at or above 2^31 > L')
      const unsigned fa = (unsigned)op.y + (unsigned)t;
      const V a = fa < (unsigned)Lp ? F::load(yin, (int64_t)fa * C + c) : F::zero();
      if (op.z < 0) {
        val[j] = a;
      } else {
        const unsigned fb = (unsigned)op.z + (unsigned)t;
        const V b = fb < (unsigned)Lp ? F::load(yin, (int64_t)fb * C + c) : F::zero();
        val[j] = F::xfade(a, b, op.w, t, inv);
      }
      if (++c == C) { c = 0; f++; }
    }
    typename F::T* dst = yout + e0;
    if (ok[0] && ok[SPX_ESC_VEC - 1]) {            // the whole group: one aligned store
      F::store4(dst, val);
    } else {                                        // the stream's head or tail
#pragma unroll
      for (int j = 0; j < SPX_ESC_VEC; j++)
        if (ok[j]) F::store1(dst + j, val[j]);
    }
  }
}

template <class F, bool QONE>
__global__ void __launch_bounds__(SPX_ESC_THREADS)
spx_edit_scaled_kernel(const SpxScaledStream* __restrict__ streams, int stream0, const int4* __restrict__ ops,
                       const int64_t* __restrict__ n_ops, const int64_t* __restrict__ n_out, int p, int q,
                       const typename F::T* __restrict__ y_in, typename F::T* __restrict__ y_out, int64_t* __restrict__ n_out_y) {
  typedef typename F::T T;
  __shared__ int4 s_ops[SPX_ESC_SLOTS];
  __shared__ double s_rcp[SPX_ESC_SLOTS];
  const int s = stream0 + (int)blockIdx.y;
  const SpxScaledStream S = streams[s];
  int64_t no = n_out[s];
  const int64_t nk64 = n_ops[s];
  const bool reports = blockIdx.x == 0 && threadIdx.x == 0;
  // nothing for a stream without output, or one whose list did not fit (and never more than the region holds or the list has)
  if (no <= 0 || nk64 <= 0 || nk64 > S.op_cap) {
    if (reports) n_out_y[s] = 0;
    return;
  }
  if (no > S.key_cap) no = S.key_cap;
  if (no > 0x7fffffff) no = 0x7fffffff;
  if (no < 0) no = 0;
  const int64_t Np = esc_scale<QONE>(no, p, q);             // N' (the host made sure it fits int32)
  if (Np > S.out_cap) {
    if (reports) n_out_y[s] = -Np;
    return;
  }
  if (reports) n_out_y[s] = Np;
  int64_t Lp64 = esc_scale<QONE>(S.limit, p, q);
  if (Lp64 > S.n_in) Lp64 = S.n_in;
  const int Lp = (int)(Lp64 > 0x7fffffff ? 0x7fffffff : Lp64);
  const int nk = (int)nk64;
  const int C = S.channels;
  T* __restrict__ yout = y_out + S.out_off;
  const T* __restrict__ yin = y_in + S.in_off;
  const int mis = (int)((reinterpret_cast<uintptr_t>(yout) / sizeof(T)) & (SPX_ESC_VEC - 1));
  const int64_t total = Np * C;
  const int64_t vbase = (int64_t)blockIdx.x * SPX_ESC_BLOCK;
  if (total == 0 || vbase >= total + mis) return;
  int64_t vend = vbase + SPX_ESC_BLOCK;
  if (vend > total + mis) vend = total + mis;
  const int f_first = (int)((vbase > mis ? vbase - mis : 0) / C);
  const int f_last = (int)((vend - mis - 1) / C);
  const int4* __restrict__ gops = ops + S.op0;
  int k0, k1;
  esc_find_pair<QONE>(gops, nk, p, q, f_first, f_last, &k0, &k1);
  const int kn = k1 - k0 + 1;
  if (kn <= SPX_ESC_SLOTS) {
    for (int t = threadIdx.x; t < kn; t += SPX_ESC_THREADS) {
      const int4 op = esc_scaled_op<QONE>(gops[k0 + t], p, q);
      s_ops[t] = op;
      if (F::RCP) s_rcp[t] = op.z >= 0 ? xfade_rcp(op.w) : 0.0;
    }
    __syncthreads();
    const EscOps<true, QONE> O = {s_ops, s_rcp, nullptr, p, q};
    esc_block<F>(O, kn, S, Lp, vbase, mis, total, yin, yout);
  } else {
    const EscOps<false, QONE> O = {nullptr, nullptr, gops + k0, p, q};
    esc_block<F>(O, kn, S, Lp, vbase, mis, total, yin, yout);
  }
}

static std::atomic<int> g_last_scaled_gx{0}, g_last_scaled_launches{0};   // spx_debug_last_scaled_grid

static int64_t esc_gcd(int64_t a, int64_t b) {
  while (b) { const int64_t t = a % b; a = b; b = t; }
  return a;
}
// p / q reduced by its gcd, if the ratio is one the call takes: 1 <= q <= p <= 32 q and p <= 32768 after the reduction
static bool esc_ratio(int32_t p, int32_t q, int* rp, int* rq) {
  if (p < 1 || q < 1) return false;
  const int64_t g = esc_gcd(p, q);
  const int64_t P = p / g, Q = q / g;
  if (P < Q || P > SPX_ESC_MAX_RATIO * Q || P > SPX_ESC_MAX_P) return false;
  *rp = (int)P;
  *rq = (int)Q;
  return true;
}
// S on the host, for 0 <= x < 2^48 (twice per stream and call, in front of the launch: no division where q is 1)
static inline int64_t esc_scale_host(int64_t x, int p, int q) {
  const uint64_t num = (uint64_t)x * (uint64_t)p;
  return (int64_t)(q == 1 ? num : num / (uint64_t)q);
}

extern "C" {

int spx_debug_last_scaled_grid(int* launches) {
  if (launches) *launches = g_last_scaled_launches.load(std::memory_order_relaxed);
  return g_last_scaled_gx.load(std::memory_order_relaxed);
}

int64_t spx_edit_scale(int64_t x, int32_t p, int32_t q) {
  int P, Q;
  if (x < 0 || !esc_ratio(p, q, &P, &Q)) return -1;
  const unsigned __int128 v = (unsigned __int128)(uint64_t)x * (unsigned)P / (unsigned)Q;
  return v > (unsigned __int128)INT64_MAX ? -1 : (int64_t)v;
}

int spx_edit_replay_scaled(spx_plan_t plan, const spx_stream_job* jobs, int n, const spx_edit_op* ops, const int64_t* ops_cap,
                           const int64_t* n_ops, const int64_t* n_out, const spx_edit_master* tracks, int32_t p, int32_t q,
                           int sample_format, const void* y_in, void* y_out, int64_t* n_out_y, void* hs) {
  if (spx_check_jobs(plan, jobs, n, true)) return -1;
  if (!ops || !ops_cap || !n_ops || !n_out || !tracks || !y_in || !y_out || !n_out_y)
    return fail(-1, "spx_edit_replay_scaled: a NULL pointer");
  if (sample_format != SPX_SAMPLES_INT16 && sample_format != SPX_SAMPLES_FLOAT)
    return fail(-1, "spx_edit_replay_scaled: an unknown sample_format");
  const uintptr_t amask = sample_format == SPX_SAMPLES_FLOAT ? 3 : 1;
  if ((reinterpret_cast<uintptr_t>(ops) & 15) || (reinterpret_cast<uintptr_t>(y_out) & amask) || (reinterpret_cast<uintptr_t>(y_in) & amask))
    return fail(-1, "spx_edit_replay_scaled: ops is not aligned to 16 bytes, or a track buffer not to its sample size");
  int P, Q;
  if (!esc_ratio(p, q, &P, &Q))
    return fail(-1, "spx_edit_replay_scaled: the ratio p / q must reduce to 1 <= q <= p <= 32 q with p <= 32768");
  const int B = plan->dev.B;
  std::vector<SpxScaledStream> tab((size_t)n);
  int64_t row = 0, gx = 1;
  for (int i = 0; i < n; i++) {
    const spx_edit_master& t = tracks[i];
    if (t.channels < 1 || t.channels > SPX_ESC_MAX_CHANNELS) return fail(-1, "spx_edit_replay_scaled: a track's channels are outside 1 .. 65535");
    if (t.in_off < 0 || t.out_off < 0) return fail(-1, "spx_edit_replay_scaled: a negative track offset");
    if (t.n_in < 0 || t.out_cap < 0) return fail(-1, "spx_edit_replay_scaled: a negative track length or capacity");
    if (ops_cap[i] < 0) return fail(-1, "spx_edit_replay_scaled: a negative capacity");
    SpxScaledStream& s = tab[i];
    s.in_off = t.in_off; s.out_off = t.out_off;
    s.op0 = row; s.op_cap = ops_cap[i];
    s.limit = jobs[i].nonlinear != 0.0f ? jobs[i].n_in / B * B : jobs[i].n_in;
    s.key_cap = jobs[i].out_cap;
    s.n_in = t.n_in; s.out_cap = t.out_cap;
    s.channels = t.channels;
    s.inv_channels = (uint32_t)((0x100000000ull + (uint64_t)t.channels - 1) / (uint64_t)t.channels);
    row += ops_cap[i];
    if (row > 0x7fffffff) return fail(-1, "spx_edit_replay_scaled: more than 2^31 - 1 records of capacity in one call");
    // master positions fit int32 inside the kernel, as the key's do in spx_edit_replay's
    const int64_t key_frames = jobs[i].out_cap > 0x7fffffff ? 0x7fffffff : (jobs[i].out_cap < 0 ? 0 : jobs[i].out_cap);
    int64_t cap_frames = esc_scale_host(key_frames, P, Q);
    if (cap_frames > 0x7fffffff || esc_scale_host(s.limit, P, Q) > 0x7fffffff)
      return fail(-1, "spx_edit_replay_scaled: a stream's positions at the master's rate do not fit 2^31 - 1");
    if (cap_frames > t.out_cap) cap_frames = t.out_cap;      // (a stream whose N' is above the track's capacity writes nothing)
    const int64_t blocks = (cap_frames * t.channels + (SPX_ESC_VEC - 1) + SPX_ESC_BLOCK - 1) / SPX_ESC_BLOCK;
    if (blocks > gx) gx = blocks;
  }
  if (gx > 0x7fffffff) return fail(-1, "spx_edit_replay_scaled: a track of more than 2^43 values");
  hipStream_t st = static_cast<hipStream_t>(hs);
  std::lock_guard<std::mutex> plan_lock(plan->mu);
  // the table: through one of the plan's two pinned staging slots (SpxStage, spx_engine.h), as spx_edit_replay's
  SpxStage& G = plan->stage.take();
  if (G.acquire(sizeof(SpxScaledStream) * (size_t)n)) return -2;
  memcpy(G.p, tab.data(), sizeof(SpxScaledStream) * (size_t)n);
  g_last_scaled_gx.store((int)gx, std::memory_order_relaxed);
  g_last_scaled_launches.store((n + 65534) / 65535, std::memory_order_relaxed);
  for (int s0 = 0; s0 < n; s0 += 65535) {   // (the grid's second dimension holds 65 535)
    const int m = n - s0 < 65535 ? n - s0 : 65535;
    const dim3 grid((unsigned)gx, (unsigned)m), block(SPX_ESC_THREADS);
    const SpxScaledStream* tab_d = static_cast<const SpxScaledStream*>(G.p);
    const int4* ops4 = reinterpret_cast<const int4*>(ops);
    if (sample_format == SPX_SAMPLES_FLOAT) {
      const float* yi = static_cast<const float*>(y_in);
      float* yo = static_cast<float*>(y_out);
      if (Q == 1) hipLaunchKernelGGL((spx_edit_scaled_kernel<EscFloat, true>), grid, block, 0, st, tab_d, s0, ops4, n_ops, n_out, P, Q, yi, yo, n_out_y);
      else hipLaunchKernelGGL((spx_edit_scaled_kernel<EscFloat, false>), grid, block, 0, st, tab_d, s0, ops4, n_ops, n_out, P, Q, yi, yo, n_out_y);
    } else {
      const int16_t* yi = static_cast<const int16_t*>(y_in);
      int16_t* yo = static_cast<int16_t*>(y_out);
      if (Q == 1) hipLaunchKernelGGL((spx_edit_scaled_kernel<EscInt16, true>), grid, block, 0, st, tab_d, s0, ops4, n_ops, n_out, P, Q, yi, yo, n_out_y);
      else hipLaunchKernelGGL((spx_edit_scaled_kernel<EscInt16, false>), grid, block, 0, st, tab_d, s0, ops4, n_ops, n_out, P, Q, yi, yo, n_out_y);
    }
  }
  if (G.release(st)) return -2;
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
