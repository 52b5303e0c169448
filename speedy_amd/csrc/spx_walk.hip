// Walk kernel for gfx950: one workgroup of NW wavefronts (NW = 1, 2, 4, 8 or 16) per stream.
//
// The sample-rate stage, inherently sequential per stream (each step's position depends on the last period):
//   a10 AMDF pitch search on the decimated then the full-rate signal   (libsonic)
//   a11 skip / insert pitch periods with a linear cross-fade, FIFO bookkeeping, flush padding
//       driven exactly as the shim drives it: one (setSpeed, write frameStep samples) pair per tension
//       frame (soniclib.c:354,369), the un-analysed tail at the last speed (soniclib.c:538-550), then
//       sonicIntFlushStream (soniclib.c:551).
// The speed of every tension frame comes from the tension kernel (spx_tension.hip) through scratch[4k + 3]; in
// concurrent mode that kernel runs beside this one and publishes how many speeds are final (`speed_ready`).
// Two variants: FAST (all streams mono and speeding up, rates below 32 kHz; the bench and the usual case) and the
// general one (any channel count, slow-down, any rate).
//
// How a pitch step maps to the hardware:
//   * the input lives in an LDS sliding window (int16, refilled with coalesced loads every ~25 steps), so a
//     step touches HBM only to store its 2n output bytes; the stores are never waited for (the workgroup
//     barrier used here drains lgkmcnt only);
//   * the search signals are kept in LDS as u16 biased by 32768, twice (once shifted by a sample), so that
//     any lag reads two aligned sample PAIRS per ds_read_b32 and one v_sad_u16 adds two |a-b| terms;
//   * the lags x sample-pairs space is spread over all lanes; partial sums meet in LDS with ds_add_u32;
//   * arg-min / arg-max of diff/lag: float ratios, DPP wave reduction, then an exact integer resolve of
//     the few lanes within 2^-16 of the extremum on the scalar unit (ties -> smallest lag, as a sequential
//     scan would);  every wave does this redundantly, so no broadcast barrier is needed.
// All sample arithmetic is integer; results are bit-exact against oracle/orc_sonic.c.
#include <atomic>
#include <stdlib.h>

#include "spx_internal.h"

#define SPX_CH 1024  // frames per prologue chunk held in LDS
#define SPX_WCH 64   // frames in the first walk chunk when the analysis kernel runs concurrently (multiple of the tile)

#include "spx_walk_common.h"
#include "spx_select.h"

// Diagnostic build only (-DSPX_STAMPS): per-phase shader-cycle sums of workgroup 0, lane 0.  Never in the product.
#ifdef SPX_STAMPS
__device__ unsigned long long g_spx_stamps[32];
#ifndef SPX_STAMP_SEL
#define SPX_STAMP_SEL 0
#endif
// One region per build (SPX_STAMP_SEL): a single accumulator keeps the register pressure of the measured kernel
// close to the product's.  Slot 30 = whole kernel, slot 31 = pitch steps.
#define STAMP_DECL                                         \
  X.stamp_acc = 0; X.stamp_steps = 0;                      \
  X.stamp_last = __builtin_readcyclecounter();             \
  X.stamp_t0 = X.stamp_last;
#define STAMP(i)                                                          \
  do {                                                                    \
    const unsigned long long t_ = __builtin_readcyclecounter();           \
    if ((i) == SPX_STAMP_SEL) X.stamp_acc += t_ - X.stamp_last;           \
    if ((i) == 1) X.stamp_steps++;                                        \
    X.stamp_last = t_;                                                    \
  } while (0)
#define STAMP_FLUSH                                                                              \
  if (threadIdx.x == 0 && blockIdx.x == 0) {                                                     \
    g_spx_stamps[SPX_STAMP_SEL] += X.stamp_acc;                                                  \
    g_spx_stamps[30] += __builtin_readcyclecounter() - X.stamp_t0;                               \
    g_spx_stamps[31] += X.stamp_steps;                                                           \
  }
extern "C" void spx_debug_stamps(unsigned long long* out, int reset) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_spx_stamps), sizeof(unsigned long long) * 32);
  if (reset) {
    unsigned long long z[32] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_spx_stamps), z, sizeof(z));
  }
}
#else
#define STAMP_DECL
#define STAMP(i)
#define STAMP_FLUSH
#endif

struct WalkCtx {
  int* flush_rem;     // SPX_F_NO_TRUNC: where the flush leaves {frames the stage held, frames produced so far} (nullptr: truncate as usual)
  int64_t* map;       // time map (spx_walk_map_kernel): the stream's rows, row k = frames produced when ring buffer k is handed over (nullptr: none)
  int4* ops;          // edit list (spx_walk_edits_kernel): the stream's records, {out_at, a, b, n} each (record_op)
  int ops_cap, n_ops; // ... how many fit there, and how many the stream has had so far (counted on past the capacity, stored below it)
  const int16_t* in;  // stream input (interleaved)
  int16_t* out;       // stream output
  pos_t out_cap;
  pos_t limit;      // absolute frame index from which reads return 0 (end of input / flush padding)
  int C;
  // LDS sliding window over frames [wbase, wbase + wcap)
  unsigned short* monoH;   // mono mix biased by 32768: monoH[k] = mono(wbase + k) + 32768
  unsigned short* monoHB;  // the same shifted by one frame: monoHB[k] = monoH[k + 1]
  short* raw;              // interleaved raw samples, only kept when C > 1 (the cross-fade is per channel)
  pos_t wbase;           // -1 = window invalid
  int wcap;
  unsigned short* dnH;     // biased decimated signal of the current step (and its shifted copy)
  unsigned short* dnHB;
  // FAST kernels: the decimated signal of EVERY window position, built once per refill.  Plane r (r < skip) holds
  // S[m*skip + r], S[i] = mean of window samples i .. i+skip-1, so the decimated signal of a step at window offset o
  // is plane (o % skip) from element o / skip on, contiguous.  plB is the copy shifted by one element.
  unsigned short* pl;
  unsigned short* plB;
  int plStride;            // elements per plane (even)
  int skip, skipM;         // skipM = ceil(2^16 / skip): i / skip == (i * skipM) >> 16 for i < 8192
  unsigned skipM32;        // ceil(2^32 / skip): x / skip == mulhi(x, skipM32) for x < 2^18
  unsigned* diffC;    // per-lag AMDF sums, coarse search
  unsigned* diffR;    // per-lag AMDF sums, refine search
#ifdef SPX_STAMPS
  unsigned long long stamp_last, stamp_acc, stamp_t0;
  unsigned stamp_steps;
#endif
};

__device__ __forceinline__ int global_sample(const WalkCtx& X, pos_t a, int c) {
  return (a < X.limit) ? (int)X.in[(size_t)a * X.C + c] : 0;
}
// sample through the LDS window when it covers frame a, else from HBM
__device__ __forceinline__ int any_sample(const WalkCtx& X, pos_t a, int c) {
  const pos_t o = a - X.wbase;
  if (X.wbase >= 0 && o >= 0 && o < X.wcap) {
    if (X.C == 1) return (int)X.monoH[o] - 32768;
    return (int)X.raw[o * X.C + c];
  }
  return global_sample(X, a, c);
}

// Make the window cover [pos, pos + need).  Uniform across the workgroup.  The biased mono signal and its
// shifted copy are built here, once per refill, so a pitch step never touches HBM for its input.
template <int NW, int FAST>
__device__ __forceinline__ void ensure_window(WalkCtx& X, pos_t pos, int need) {
  constexpr int NT = 64 * NW;
  if (X.wbase >= 0 && pos >= X.wbase && pos + need <= X.wbase + X.wcap) return;
  lds_sync<NW>();  // everyone is done reading the old window
  const pos_t nb = pos & ~7;
  const int C = (FAST == 1) ? 1 : X.C;
  if (C == 1) {
    const int16_t* __restrict__ src = X.in + nb;
    const pos_t room = X.limit - nb;  // frames of real input from nb on
    for (int k0 = threadIdx.x; k0 < X.wcap + 1; k0 += 8 * NT) {
      int v[8];
      const int last = (int)(room < X.wcap + 1 ? room : X.wcap + 1) - 1;  // last index holding real input
      if (last >= 0) {  // uniform
#pragma unroll
        for (int u = 0; u < 8; u++) {  // eight coalesced loads in flight before the first LDS write:
          const int k = k0 + u * NT;   // clamped address, unconditional load, so nothing serialises them
          v[u] = (int)src[k < last ? k : last];
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const int k = k0 + u * NT;
          if (k > last) v[u] = 0;
        }
      } else {  // the whole window lies in the zero padding: no address there may be touched
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = 0;
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int k = k0 + u * NT;
        const unsigned short w = (unsigned short)(v[u] + 32768);
        if (k < X.wcap) X.monoH[k] = w;
        if (k > 0 && k < X.wcap + 1) X.monoHB[k - 1] = w;
      }
    }
  } else {
    for (int k = threadIdx.x; k < X.wcap + 1; k += NT) {
      const pos_t g = nb + k;
      int sum = 0;
      for (int c = 0; c < C; c++) {
        const int v = (g < X.limit) ? (int)X.in[(size_t)g * C + c] : 0;
        if (k < X.wcap) X.raw[(size_t)k * C + c] = (short)v;
        sum += v;
      }
      const unsigned short u = (unsigned short)(sum / C + 32768);
      if (k < X.wcap) X.monoH[k] = u;
      if (k > 0) X.monoHB[k - 1] = u;
    }
  }
  X.wbase = nb;
  lds_sync<NW>();
  if (FAST == 1 || (FAST == 2 && C == 1)) {
    // One thread per decimated index m: it reads the 2*skip-1 window samples m*skip .. m*skip+2*skip-2 once and slides
    // the sum over them, giving element m of every plane.  |sum| < 2^18 and skip <= 7, so the truncating division is
    // exactly mulhi(|sum|, ceil(2^32 / skip)).
    const int skip = X.skip;
    const unsigned M = X.skipM32;
    const int bias = 32768 * skip;
    for (int m = threadIdx.x; (m + 1) * skip <= X.wcap; m += NT) {
      const unsigned short* w = X.monoH + m * skip;
      int sum = 0;
      for (int j = 0; j < skip; j++) sum += (int)w[j];
      for (int r = 0; r < skip; r++) {
        if ((m + 1) * skip + r > X.wcap) break;  // the last element of the higher planes needs samples past the window
        const int v = sum - bias;
        const unsigned mag = (unsigned)(v < 0 ? -v : v);
        const int qm = (int)__umulhi(mag, M);
        const unsigned short u = (unsigned short)((v < 0 ? -qm : qm) + 32768);
        X.pl[r * X.plStride + m] = u;
        if (m > 0) X.plB[r * X.plStride + m - 1] = u;
        sum += (int)w[skip + r] - (int)w[r];
      }
    }
  } else if (FAST == 2) {
    // Several channels: the decimated sample is the sum of skip*C RAW samples divided ONCE by skip*C (the dependency's
    // downSampleInput), not the mean of the per-frame channel means.  |sum| < 2^21, skip*C <= 56: mulhi is still exact.
    const int skip = X.skip, div = skip * C;
    const unsigned M = (unsigned)((0x100000000ull + (unsigned)div - 1) / (unsigned)div);
    for (int m = threadIdx.x; (m + 1) * skip <= X.wcap; m += NT) {
      const short* w = X.raw + (size_t)m * div;
      int sum = 0;
      for (int j = 0; j < div; j++) sum += (int)w[j];
      for (int r = 0; r < skip; r++) {
        if ((m + 1) * skip + r > X.wcap) break;
        const unsigned mag = (unsigned)(sum < 0 ? -sum : sum);
        const int qm = (int)__umulhi(mag, M);
        const unsigned short u = (unsigned short)((sum < 0 ? -qm : qm) + 32768);
        X.pl[r * X.plStride + m] = u;
        if (m > 0) X.plB[r * X.plStride + m - 1] = u;
        // slide by one frame: drop frame r, take frame skip + r (its samples may lie past the window: unused then)
        for (int c = 0; c < C; c++) sum += (int)w[(skip + r) * C + c] - (int)w[r * C + c];
      }
    }
  }
  if (FAST) {
    lds_sync<NW>();
  }
}

// (Sel, select_fold, select_finish -- the running arg-min / arg-max over lags -- live in spx_select.h: the selector check includes them too.)

// One lane per lag, the whole sum in the lane (no cross-lane traffic): used for the coarse search, which every
// wave runs redundantly.  A0/A1: dword views of the signal array and of its copy shifted by one sample; o = offset
// of the search position inside them.
template <bool WANT_MAX, int FAST>
__device__ __forceinline__ void search_lane_per_lag(const unsigned* A0, const unsigned* A1, int o, int minP, int nl,
                                                    Sel& S, unsigned* dlane = nullptr) {
  const int lane = threadIdx.x & 63;
  const unsigned* ap = (o & 1) ? A1 + ((o - 1) >> 1) : A0 + (o >> 1);
  for (int base = 0; base < (FAST ? 1 : nl); base += 64) {  // FAST: at most 64 lags per search
    const bool valid = base + lane < nl;
    const int p = minP + base + lane;
    const int ob = o + p;
    const unsigned* bp = (ob & 1) ? A1 + ((ob - 1) >> 1) : A0 + (ob >> 1);
    const int nfull = valid ? (p >> 1) : 0;
    unsigned d = sad_run(ap, bp, 0, nfull);
    if (valid && (p & 1)) d = __builtin_amdgcn_sad_u16(ap[nfull] & 0xffffu, bp[nfull] & 0xffffu, d);  // term i = p-1
    if (dlane && base == 0) *dlane = d;
    select_fold<WANT_MAX, (FAST != 0)>(S, d, minP + base, valid);
  }
}

// The same search spread over the NW waves of the workgroup: wave w takes the pairs [w*CH, (w+1)*CH) of every lag
// (one lane per lag), the partial sums meet in LDS (ds_add_u32 into `buf`, which is all zero on entry), one
// LDS barrier, then every wave folds the totals itself.  `other` is the buffer the PREVIOUS step used; every wave
// is past reading it once this step's barrier is crossed, so it is cleared here for the next step.
template <int NW, bool WANT_MAX, int FAST>
__device__ __forceinline__ void search_split(const unsigned* A0, const unsigned* A1, int o, int minP, int nl,
                                             unsigned* buf, unsigned* other, Sel& S, WalkCtx& X, int sb, unsigned* dlane = nullptr) {
  (void)X; (void)sb;
  if (NW == 1) {
    search_lane_per_lag<WANT_MAX, FAST>(A0, A1, o, minP, nl, S, dlane);
    return;
  }
  constexpr int NT = 64 * NW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int maxP = minP + nl - 1;
  const int CH = (((maxP >> 1) + NW) / NW + 3) & ~3;
  const unsigned* ap = (o & 1) ? A1 + ((o - 1) >> 1) : A0 + (o >> 1);
  for (int base = 0; base < (FAST ? 1 : nl); base += 64) {  // FAST: at most 64 lags per search
    const bool valid = base + lane < nl;
    const int p = minP + base + lane;
    const int ob = o + p;
    const unsigned* bp = (ob & 1) ? A1 + ((ob - 1) >> 1) : A0 + (ob >> 1);
    const int nfull = valid ? (p >> 1) : 0;
    // Chunk c of the pairs goes to wave c for c < 4 and to wave 11 - c above (8 waves): low chunks are the busy ones
    // (every lag has those pairs), and waves w and w + 4 share a SIMD, so each SIMD gets a busy and a light chunk.
    const int cw = (NW == 8) ? (wave < 4 ? wave : 11 - wave) : wave;
    int j1 = (cw + 1) * CH;
    if (j1 > nfull) j1 = nfull;
    unsigned d = sad_run(ap, bp, cw * CH, j1);
    if (cw == NW - 1 && valid && (p & 1))
      d = __builtin_amdgcn_sad_u16(ap[nfull] & 0xffffu, bp[nfull] & 0xffffu, d);  // the lone term i = p-1
    if (valid) atomicAdd(&buf[base + lane], d);
  }
  STAMP(sb);
  lds_sync<NW>();
  STAMP(sb + 1);
  for (int t = tid; t < 256; t += NT) other[t] = 0;
  for (int base = 0; base < (FAST ? 1 : nl); base += 64) {  // FAST: at most 64 lags per search
    const bool valid = base + lane < nl;
    const unsigned d = valid ? buf[base + lane] : 0u;
    if (dlane && base == 0) *dlane = d;
    select_fold<WANT_MAX, (FAST != 0)>(S, d, minP + base, valid);
  }
}

// findPitchPeriod at absolute position pos (all threads return the same value).
template <int NW, int FAST>
__device__ __forceinline__ int find_pitch_period(const SpxPlanDev& P, WalkCtx& X, WalkState& st, pos_t pos) {
  constexpr int NT = 64 * NW;
  const int tid = threadIdx.x;
  const int C = FAST ? 1 : X.C, skip = P.skip, maxRequired = P.maxRequired;
  STAMP(1);
  ensure_window<NW, FAST>(X, pos, maxRequired + 2 * skip + 2);
  STAMP(2);
  const int o = (int)(pos - X.wbase);
  const bool direct = FAST ? false : (C == 1 && skip == 1);
  // ---- phase B: the decimated, biased search signal of this step (earlier readers are past a barrier) ----
  const int cnt = maxRequired / skip;
  if (!FAST && !direct) {
    const int div = skip * C;
    const double inv = xfade_rcp(div);
    for (int t = tid; t < cnt + 2; t += NT) {
      int sum = 0;
      if (C == 1) {
        const unsigned short* w = X.monoH + o + t * skip;
        for (int j = 0; j < skip; j++) sum += (int)w[j];
        sum -= 32768 * skip;
      } else {
        const short* w = X.raw + (size_t)(o + t * skip) * C;
        for (int j = 0; j < div; j++) sum += w[j];
      }
      // truncating sum / div via the exact double-reciprocal form (xfade_quot: |sum| <= 32768 div)
      const unsigned short u = (unsigned short)(xfade_quot(sum, inv) + 32768);
      X.dnH[t] = u;
      if (t > 0) X.dnHB[t - 1] = u;
    }
  }
  STAMP(3);
  // FAST: nothing was built, and the sum buffers this step adds into were cleared before the previous step's last
  // barrier, so no barrier is needed here
  if (!FAST) lds_sync<NW>();  // decimated signal visible; last step's buffer clearing finished
  STAMP(4);
  // ---- first search ----
  const unsigned* M0 = reinterpret_cast<const unsigned*>(X.monoH);
  const unsigned* M1 = reinterpret_cast<const unsigned*>(X.monoHB);
  const unsigned* D0 = reinterpret_cast<const unsigned*>(X.dnH);
  const unsigned* D1 = reinterpret_cast<const unsigned*>(X.dnHB);
  int oD = 0;  // where the decimated signal of this step starts in D0 / D1
  if (FAST) {
    oD = (o * X.skipM) >> 16;
    const int r = o - oD * skip;
    D0 = reinterpret_cast<const unsigned*>(X.pl + r * X.plStride);
    D1 = reinterpret_cast<const unsigned*>(X.plB + r * X.plStride);
  }
  int period, minDiff, maxDiff;
  const int minC = direct ? P.minPeriod : P.minPeriod / skip;
  const int maxC = direct ? P.maxPeriod : P.maxPeriod / skip;
  const int tg = st.prevPeriod_toggle & 1;
  st.prevPeriod_toggle ^= 1;
  st.steps++;
  Sel S1 = {0u, 0u, 0, 0};
  if (!FAST && (direct || skip == 1)) {  // this search is the final one: it also needs the worst lag
    search_split<NW, true, FAST>(direct ? M0 : D0, direct ? M1 : D1, direct ? o : 0, minC, maxC - minC + 1,
                           X.diffC + 256 * tg, X.diffC + 256 * (1 - tg), S1, X, 5);
    select_finish(S1, &period, &minDiff, &maxDiff);
    STAMP(7);
  } else {
    search_split<NW, false, FAST>(D0, D1, oD, minC, maxC - minC + 1, X.diffC + 256 * tg, X.diffC + 256 * (1 - tg), S1, X, 5);
    STAMP(7);
    period = S1.bestP * skip;
    int lo = period - (skip << 2), hi = period + (skip << 2);
    if (lo < P.minPeriod) lo = P.minPeriod;
    if (hi > P.maxPeriod) hi = P.maxPeriod;
    // ---- refine at full rate ----
    Sel S2 = {0u, 0u, 0, 0};
    if (FAST) {
      // Only "maxDiff > 3*minDiff" is ever asked of the worst lag, and max_p floor(d_p/p) = floor(max_p d_p/p), so
      // the test is "some lag has d_p >= (3*minDiff+1)*p": no arg-max, and only on the steps where the
      // previous-period rule can fire at all.
      unsigned dl = 0;
      search_split<NW, false, FAST>(M0, M1, o, lo, hi - lo + 1, X.diffR + 256 * tg, X.diffR + 256 * (1 - tg), S2, X, 8,
                                    &dl);
      period = uni(S2.bestP);
      minDiff = uni((int)udiv_small(S2.bestD, (unsigned)S2.bestP));
      maxDiff = 0x7fffffff;  // "a clear match" unless shown otherwise
      if (minDiff != 0 && st.prevPeriod != 0 && minDiff * 2 > st.prevMinDiff * 3) {
        const int lane = tid & 63;
        const bool valid = lane < hi - lo + 1;
        const unsigned long long need = (unsigned long long)(3u * (unsigned)minDiff + 1u) * (unsigned)(lo + lane);
        if (__builtin_amdgcn_ballot_w64(valid && (unsigned long long)dl >= need) == 0) maxDiff = 0;  // no lag that bad: keep the old period
      }
    } else {
      search_split<NW, true, FAST>(M0, M1, o, lo, hi - lo + 1, X.diffR + 256 * tg, X.diffR + 256 * (1 - tg), S2, X, 8);
      select_finish(S2, &period, &minDiff, &maxDiff);
    }
    STAMP(10);
  }
  int ret = period;
  if (!(minDiff == 0 || st.prevPeriod == 0) && !(maxDiff > minDiff * 3) && !(minDiff * 2 <= st.prevMinDiff * 3))
    ret = st.prevPeriod;
  st.prevMinDiff = minDiff;
  st.prevPeriod = period;
  return ret;
}

// Append n frames copied from absolute input position a.
template <int NW, int FAST>
__device__ __forceinline__ void emit_copy(const WalkCtx& X, WalkState& st, pos_t a, pos_t n) {
  constexpr int NT = 64 * NW;
  const int C = (FAST == 1) ? 1 : X.C;
  if (st.out_n + n > X.out_cap) st.overflow = 1;
  pos_t nv = X.out_cap - st.out_n;  // frames that still fit
  if (nv > n) nv = n;
  const pos_t o = a - X.wbase;
  int16_t* __restrict__ dst = X.out + (size_t)st.out_n * C;
  if (C == 1 && X.wbase >= 0 && o >= 0 && o + n <= X.wcap) {  // whole run inside the LDS window
    const unsigned short* w = X.monoH + o;
    for (int t = threadIdx.x; t < (int)nv; t += NT) dst[t] = (int16_t)((int)w[t] - 32768);
  } else if (FAST == 2 && X.wbase >= 0 && o >= 0 && o + n <= X.wcap) {  // multi-channel run inside the window
    const short* w = X.raw + (size_t)o * C;
    const int total = (int)nv * C;
    for (int e = threadIdx.x; e < total; e += NT) dst[e] = w[e];
  } else {
    const pos_t total = nv * C;
    for (pos_t e = threadIdx.x; e < total; e += NT) {
      pos_t f = e;
      int c = 0;
      if (C != 1) { f = e / C; c = (int)(e - f * C); }
      dst[e] = (int16_t)any_sample(X, a + f, c);
    }
  }
  st.out_n += n;
}

// Append n frames of cross-fade: out[t] = (down[t]*(n-t) + up[t]*t)/n, integer, truncating toward zero.
// |numerator| <= 32768*n < 2^31; the quotient: xfade_rcp / xfade_quot (spx_walk_common.h).
template <int NW, int FAST>
__device__ __forceinline__ void emit_overlap_add(const WalkCtx& X, pos_t a_down, pos_t a_up, int n,
                                                 pos_t out_at) {
  constexpr int NT = 64 * NW;
  const int C = (FAST == 1) ? 1 : X.C;
  const double inv = xfade_rcp(n);
  pos_t nv64 = X.out_cap - out_at;
  const int nv = nv64 > n ? n : (nv64 < 0 ? 0 : (int)nv64);
  int16_t* __restrict__ dst = X.out + (size_t)out_at * C;
  const pos_t od = a_down - X.wbase, ou = a_up - X.wbase;
  const bool inwin = X.wbase >= 0 && od >= 0 && ou >= 0 && od + n <= X.wcap && ou + n <= X.wcap;
  if (FAST == 1 || (C == 1 && inwin)) {  // FAST: ensure_window(pos, maxRequired + ...) of the search covers both ramps
    const unsigned short* wd = X.monoH + od;
    const unsigned short* wu = X.monoH + ou;
    // FAST: n <= maxPeriod < 512 (rates below 32 kHz), so with eight waves this is one predicated pass, no loop
    for (int t = threadIdx.x; t < nv; t += NT) {
      const int d = (int)wd[t] - 32768, u = (int)wu[t] - 32768;
      dst[t] = (int16_t)xfade_quot(d * (n - t) + u * t, inv);
      if (FAST && NT >= 512) break;
    }
  } else if (FAST == 2) {
    // multi-channel speed-up kernel: both ramps lie in the window; element e = t*C + c of each is contiguous in `raw`
    const short* rd = X.raw + (size_t)od * C;
    const short* ru = X.raw + (size_t)ou * C;
    const int total = nv * C;
    const unsigned invC = (0x10000u + (unsigned)C - 1u) / (unsigned)C;  // e / C for e < 8192, C <= 8
    for (int e = threadIdx.x; e < total; e += NT) {
      const int t = (C == 2) ? (e >> 1) : (int)(((unsigned)e * invC) >> 16);
      const int d = rd[e], u = ru[e];
      dst[e] = (int16_t)xfade_quot(d * (n - t) + u * t, inv);
    }
  } else {
    const int total = nv * C;
    for (int e = threadIdx.x; e < total; e += NT) {
      int t = e, c = 0;
      if (C != 1) { t = e / C; c = e - t * C; }
      const int d = any_sample(X, a_down + t, c), u = any_sample(X, a_up + t, c);
      dst[e] = (int16_t)xfade_quot(d * (n - t) + u * t, inv);
    }
  }
}

// Edit list (spx_walk_edits_kernel; include/speedy_hip.h "EDIT LIST"): one record per emit_copy / emit_overlap_add of n >= 1 frames,
// written where tsm_process calls them -- a copy is {out_at, a, -1, n}, a cross-fade {out_at, a_down, a_up, n}.  Thread 0 writes one
// 16-byte store that nobody waits for; past the stream's capacity the count goes on and nothing is stored.
template <bool EDITS>
__device__ __forceinline__ void record_op(WalkCtx& X, pos_t out_at, pos_t a, pos_t b, pos_t n) {
  if constexpr (EDITS) {
    if (n < 1) return;
    if (X.n_ops < X.ops_cap && threadIdx.x == 0) X.ops[X.n_ops] = make_int4((int)out_at, (int)a, (int)b, (int)n);
    X.n_ops++;
  }
}

// processStreamInput with `avail` frames handed over so far (absolute count).
template <int NW, int FAST, bool EDITS = false>
__device__ __forceinline__ void tsm_process(const SpxPlanDev& P, WalkCtx& X, WalkState& st, float speed, pos_t avail) {
  const int maxRequired = P.maxRequired;
  if ((double)speed > 1.00001 || (double)speed < 0.99999) {
    const pos_t numSamples = avail - st.base;
    if (numSamples < maxRequired) return;
    pos_t position = 0;
    do {
      if (st.remaining > 0) {
        int n = st.remaining;
        if (n > maxRequired) n = maxRequired;
        record_op<EDITS>(X, st.out_n, st.base + position, -1, n);
        emit_copy<NW, FAST>(X, st, st.base + position, n);
        st.remaining -= n;
        position += n;
      } else {
        const pos_t pos = st.base + position;
        const int period = find_pitch_period<NW, FAST>(P, X, st, pos);
        if ((double)speed > 1.0) {
          int n;  // the dependency converts to long; every value here fits an int
          if (speed >= 2.0f) {
            n = uni((int)((float)period / (speed - 1.0f)));
          } else {
            n = period;
            st.remaining = uni((int)((float)period * (2.0f - speed) / (speed - 1.0f)));
          }
          if (st.out_n + n > X.out_cap) st.overflow = 1;
          if (n == 0) return;  // the dependency treats this as failure and leaves the input untouched
          STAMP(11);
          record_op<EDITS>(X, st.out_n, pos, pos + period, n);
          emit_overlap_add<NW, FAST>(X, pos, pos + period, n, st.out_n);
          STAMP(13);
          st.out_n += n;
          position += period + n;
        } else {
          int n;
          if (speed < 0.5f) {
            n = uni((int)((float)period * speed / (1.0f - speed)));
          } else {
            n = period;
            st.remaining = uni((int)((float)period * (2.0f * speed - 1.0f) / (1.0f - speed)));
          }
          record_op<EDITS>(X, st.out_n, pos, -1, period);
          emit_copy<NW, FAST>(X, st, pos, period);
          if (st.out_n + n > X.out_cap) st.overflow = 1;
          if (n == 0) return;   // (a failed step leaves its copy, and its record)
          record_op<EDITS>(X, st.out_n, pos + period, pos, n);
          emit_overlap_add<NW, FAST>(X, pos + period, pos, n, st.out_n);
          st.out_n += n;
          position += n;
        }
      }
    } while (position + maxRequired <= numSamples);
    st.base += position;
  } else {
    record_op<EDITS>(X, st.out_n, st.base, -1, avail - st.base);
    emit_copy<NW, FAST>(X, st, st.base, avail - st.base);
    st.base = avail;
  }
}

// ---- FAST kernels (mono, every job's speed > 1 and 0 <= nonlinear <= 1, so every speed the stage sees is >= 1) ----
// The pitch steps one event can run = the loop of processStreamInput for speed > 1 with `avail` frames handed over.
// The caller guarantees avail - st.base >= maxRequired.  Returns false when a step fails (n == 0): the dependency
// then returns without removing the input it has consumed in this call, so st.base keeps its value.
template <int NW, int FAST>
__device__ __forceinline__ bool fast_steps(const SpxPlanDev& P, WalkCtx& X, WalkState& st, float speed, pos_t avail) {
  const int maxRequired = P.maxRequired;
  const bool ge2 = speed >= 2.0f;
  const float sm1 = speed - 1.0f, twom = 2.0f - speed;
  pos_t pos = st.base;
  do {
    if (st.remaining > 0) {
      int n = st.remaining;
      if (n > maxRequired) n = maxRequired;
      ensure_window<NW, FAST>(X, pos, n);
      emit_copy<NW, FAST>(X, st, pos, n);
      st.remaining -= n;
      pos += n;
    } else {
      const int period = find_pitch_period<NW, FAST>(P, X, st, pos);
      int n;
      if (ge2) {
        n = uni((int)((float)period / sm1));
      } else {
        n = period;
        st.remaining = uni((int)((float)period * twom / sm1));
      }
      if (st.out_n + n > X.out_cap) st.overflow = 1;
      if (n == 0) return false;
      STAMP(11);
      emit_overlap_add<NW, FAST>(X, pos, pos + period, n, st.out_n);
      STAMP(13);
      st.out_n += n;
      pos += period + n;
    }
  } while (pos + maxRequired <= avail);
  st.base = pos;
  return true;
}


// All events of a chunk through ONE call site of the step code (the kernel stays small):
//   ordinary events [ev0, ev1): nonlinear -- event e sets the speed of tension frame e (e < K; later events keep the
//     last speed) and hands over B more frames (soniclib.c:354,369,538-550); linear -- one event handing over
//     everything new at the stream's speed (soniclib.c:397-399);
//   then, if `fin`, sonicIntFlushStream (soniclib.c:551): pad 2*maxRequired zeros, process, truncate.
// Most nonlinear events cannot run a step (a step needs maxRequired frames, an event brings B): those cost a few
// scalar instructions.  The speeds of 64 consecutive events sit in one VGPR (lane = event), so picking one is a
// v_readlane, not a memory access.
template <int NW, int FAST>
__device__ __forceinline__ void fast_events(const SpxPlanDev& P, WalkCtx& X, WalkState& st, const float* scr, pos_t ev0,
                                            pos_t ev1, pos_t K, pos_t& avail, int B, bool linear, pos_t n_in, bool fin,
                                            float& curSpeed) {
  const int lane = threadIdx.x & 63;
  const int maxRequired = P.maxRequired;
  const pos_t Kc = ev1 < K ? ev1 : K;  // tension events of this chunk: [ev0, Kc)
  float tailSpeed = curSpeed;          // what later events run at, and what the stream carries on
  if (Kc > ev0) tailSpeed = unif(scr[4 * (size_t)(Kc - 1) + 3]);
  const bool tailUnity = speed_is_unity(tailSpeed);
  pos_t blk0 = ev0 - 64;
  float spv = 0.0f;
  unsigned long long unityMask = 0;
  const pos_t ev_end = ev1 + (fin ? 1 : 0);
  for (pos_t e = ev0; e < ev_end; e++) {
    float speed = tailSpeed;
    bool unity = tailUnity;
    pos_t expected = 0;
    const bool flush = e >= ev1;
    if (!flush) {
      avail = linear ? n_in : avail + B;
      if (e < K) {
        int i = e - blk0;
        if (i >= 64) {  // next 64 events' speeds into the lanes
          blk0 = e;
          i = 0;
          const pos_t idx = blk0 + lane;
          spv = (idx < K) ? scr[4 * (size_t)idx + 3] : 2.0f;
          unityMask = __builtin_amdgcn_ballot_w64(speed_is_unity(spv));
        }
        unity = (unityMask >> i) & 1;
        if (!unity && avail - st.base < maxRequired) continue;
        speed = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, spv), i));
      }
    } else {
      const pos_t remainingS = avail - st.base;
      expected = st.out_n + uni((int)(((float)remainingS / tailSpeed + 0) / 1.0f + 0.5f));
      if (X.flush_rem) {  // a rate stage follows: it truncates its own output (and needs the count)
        expected = 0x7fffffff;
        if (threadIdx.x == 0) { X.flush_rem[0] = (int)remainingS; X.flush_rem[1] = (int)st.out_n; }
      }
      X.limit = avail;  // everything from here on reads as the flush's zero padding
      lds_sync<NW>();
      X.wbase = -1;     // the window may hold samples past the new limit
      avail += 2 * maxRequired;
    }
    STAMP(0);
    if (unity) {
      emit_copy<NW, FAST>(X, st, st.base, avail - st.base);
      st.base = avail;
    } else if (avail - st.base >= maxRequired) {
      (void)fast_steps<NW, FAST>(P, X, st, speed, avail);
    }
    STAMP(12);
    if (flush) {
      if (st.out_n > expected) st.out_n = expected;
      st.base = avail;  // the dependency empties its input after a flush
      st.remaining = 0;
    }
  }
  curSpeed = tailSpeed;
}

// LDS layout (bytes), shared by host and device
struct WalkLds {
  int off_sA, off_mono, off_monoB, off_raw, off_dn, off_dnB, off_pl, off_plB, plStride, off_diffC, off_diffR,
      off_wait, total, wcap;
};
// fast != 0: the speed-up kernels, which need neither the speed staging array nor the per-step decimated signal.
static __host__ __device__ inline WalkLds walk_lds_layout(const SpxPlanDev& P, int maxC, int fast = 0) {
  WalkLds L;
  const int need = P.maxRequired + 2 * P.skip + 2;
  int wcap = 4096;
  if (wcap < 4 * need) wcap = 4 * need;
  // many channels: a shorter window (every channel of it sits in LDS), but never shorter than one search needs
  while ((size_t)wcap * (maxC > 1 ? maxC + 2 : 2) * 2 > 48 * 1024 && wcap > need + 64) wcap = wcap / 2 > need + 64 ? wcap / 2 : need + 64;
  wcap = (wcap + 7) & ~7;
  L.wcap = wcap;
  int o = 0;
  L.off_sA = o; if (!fast) o += SPX_CH * 4;
  L.off_wait = o; o += 16;
  L.off_mono = o;
  const int mb = ((wcap + 8) * 2 + 15) & ~15;
  o += mb;
  L.off_monoB = o; o += mb;
  L.off_raw = o;
  if (maxC > 1) o += ((wcap + 1) * maxC * 2 + 15) & ~15;
  const int dnb = fast ? 0 : ((P.maxRequired / P.skip + 8) * 2 + 15) & ~15;
  L.off_dn = o; o += dnb;
  L.off_dnB = o; o += dnb;
  // decimated planes of the FAST kernels (allocated always: the layout does not depend on the kernel variant)
  L.plStride = ((wcap / (P.skip > 0 ? P.skip : 1) + 4) + 1) & ~1;
  const int plb = (L.plStride * (P.skip > 0 ? P.skip : 1) * 2 + 15) & ~15;
  L.off_pl = o; o += plb;
  L.off_plB = o; o += plb;
  L.off_diffC = o; o += 2 * 256 * 4;  // double-buffered per-lag sums, first search
  L.off_diffR = o; o += 2 * 256 * 4;  // double-buffered per-lag sums, refine search
  L.total = o;
  return L;
}

// The body of the walk kernels.  MAP (spx_walk_map_kernel, FAST == 0 only): the stream's time-map rows are written as the events
// go by -- everything that belongs to the map sits behind `if constexpr (MAP)`, so spx_walk_kernel's instantiations compile from
// the code they always compiled from.  EDITS (spx_walk_edits_kernel, FAST == 0 only): the stream's edit list, behind `if constexpr
// (EDITS)` in the same way (record_op).  A stream's records start at ops_base[map_row] -- the job record's row field counts records
// in such a call -- and its capacity reaches to the next stream's row (ops_total behind the last).  The running count lives in
// n_ops between the time chunks of a call: reset under SPX_F_INIT, read back otherwise (minus the count once the capacity is passed).
template <int NW, int FAST, bool MAP, bool EDITS = false>
__device__ __forceinline__ void
walk_body(const SpxPlanDev& P, const SpxStreamDev* __restrict__ streams, const int16_t* __restrict__ in_base,
          int16_t* __restrict__ out_base, int64_t* __restrict__ n_out, SpxStreamState* __restrict__ states,
          const float* scratch_base, int maxC, const int* speed_ready, int64_t* __restrict__ map_base,
          int4* __restrict__ ops_base = nullptr, int64_t* __restrict__ n_ops = nullptr, int ops_total = 0) {
  static_assert(!MAP || FAST == 0, "the time map is the general kernel's");
  static_assert(!EDITS || (FAST == 0 && !MAP), "the edit list is the general kernel's, in a call of its own");
  constexpr int NT = 64 * NW;
  // the walk is the latency-critical chain: where the analysis kernel shares a SIMD, these waves issue first
  __builtin_amdgcn_s_setprio(3);
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x;
  const SpxStreamDev S = streams[blockIdx.x];
  const int Ttot = S.n_frames, F = P.F, B = P.B;
  const float Rg = S.speed, nl = S.nonlinear;

  const WalkLds LY = walk_lds_layout(P, maxC, FAST);
  float* sA = reinterpret_cast<float*>(lds + LY.off_sA);  // [SPX_CH]

  // ---- the part of the stream state this stage owns (the tension kernel owns the filter states) ----
  SpxStreamState Z;
  if (S.flags & SPX_F_INIT) {
    Z.w.base = 0; Z.w.out_n = 0; Z.w.avail = 0; Z.w.remaining = 0; Z.w.prevPeriod = 0; Z.w.prevMinDiff = 0;
    Z.w.overflow = 0; Z.w.prevPeriod_toggle = 0; Z.w.steps = 0;
    Z.curSpeed = Rg;    // sonicSetSpeed -> sonicIntSetSpeed, soniclib.c:182
    Z.handed = 0;
  } else {
    Z.w = states[blockIdx.x].w;
    Z.curSpeed = states[blockIdx.x].curSpeed;
    Z.handed = states[blockIdx.x].handed;
    // sonicSetSpeed between writes reaches the TSM stage at once (soniclib.c:182); in nonlinear mode the
    // next tension frame overrides it (soniclib.c:354)
    if ((nl == 0.0f && !(S.flags & SPX_F_KEEP_SPEED)) || (S.flags & SPX_F_SPEED_SET)) Z.curSpeed = Rg;
  }

  const float* scr = scratch_base + (size_t)S.frame_off * 4;  // per frame: ..., speed (written by the tension kernel)
  int* sWait = reinterpret_cast<int*>(lds + LY.off_wait);
  // ---------------------------------- TSM stage context ----------------------------------
  WalkCtx X;
  X.flush_rem = (S.flags & SPX_F_NO_TRUNC) ? &states[blockIdx.x].flush_remaining : nullptr;
  X.map = nullptr;
  if constexpr (MAP) X.map = map_base ? map_base + S.map_row : nullptr;
  if constexpr (EDITS) {
    const int row1 = blockIdx.x + 1 < gridDim.x ? streams[blockIdx.x + 1].map_row : ops_total;
    X.ops = ops_base + S.map_row;
    X.ops_cap = uni(row1 - S.map_row);
    X.n_ops = 0;
    if (!(S.flags & SPX_F_INIT)) {
      const int64_t had = n_ops[blockIdx.x];
      X.n_ops = uni((int)(had < 0 ? -had : had));
    }
  }
  X.in = in_base + S.in_off - S.tsm_shift * S.channels;  // indexed by TSM position (= input frame + flush padding so far)
  X.out = out_base + S.out_off;
  X.out_cap = (pos_t)(S.out_cap > 0x7fffffff ? 0x7fffffff : S.out_cap);
  X.limit = (pos_t)(S.n_in + S.tsm_shift);
  X.C = S.channels;
  X.monoH = reinterpret_cast<unsigned short*>(lds + LY.off_mono);
  X.monoHB = reinterpret_cast<unsigned short*>(lds + LY.off_monoB);
  X.raw = reinterpret_cast<short*>(lds + LY.off_raw);
  X.wbase = -1;
  X.wcap = LY.wcap;
  X.dnH = reinterpret_cast<unsigned short*>(lds + LY.off_dn);
  X.dnHB = reinterpret_cast<unsigned short*>(lds + LY.off_dnB);
  X.pl = reinterpret_cast<unsigned short*>(lds + LY.off_pl);
  X.plB = reinterpret_cast<unsigned short*>(lds + LY.off_plB);
  X.plStride = LY.plStride;
  X.skip = P.skip;
  X.skipM = (65536 + P.skip - 1) / P.skip;
  X.skipM32 = (unsigned)((0x100000000ull + (unsigned)P.skip - 1) / (unsigned)P.skip);
  X.diffC = reinterpret_cast<unsigned*>(lds + LY.off_diffC);
  X.diffR = reinterpret_cast<unsigned*>(lds + LY.off_diffR);
  for (int t = tid; t < 512; t += NT) { X.diffR[t] = 0; X.diffC[t] = 0; }
  __syncthreads();
  STAMP_DECL
  WalkState st;
  st.base = uni((pos_t)Z.w.base); st.out_n = uni((pos_t)Z.w.out_n); st.avail = uni((pos_t)Z.w.avail);
  st.remaining = uni(Z.w.remaining); st.prevPeriod = uni(Z.w.prevPeriod); st.prevMinDiff = uni(Z.w.prevMinDiff);
  st.overflow = uni(Z.w.overflow); st.prevPeriod_toggle = uni(Z.w.prevPeriod_toggle); st.steps = 0;
  float curSpeed = unif(Z.curSpeed);
  pos_t avail = st.avail;
  pos_t handed = (nl != 0.0f) ? ((S.flags & SPX_F_HANDED_IN) ? S.handed_in : Z.handed) : 0;
  const bool do_flush = (S.flags & SPX_F_FLUSH) != 0;
  // The speeds come from the tension kernel.  Sequential launches (speed_ready == nullptr): all of them are there.
  // Concurrent launches: the tension kernel runs beside this one and publishes the number of tension frames whose
  // speeds are final (agent-scope release there; one relaxed poll + agent-scope acquire here, Guideline 16); the walk
  // takes whatever is ready, and only waits when it has caught up -- after the first frames it never does.
  const int K_total = (nl != 0.0f && Ttot >= F) ? Ttot - F + 1 : 0;   // soniclib.c:317
  // concurrent mode: this workgroup has been placed (the engine's idle-start gate counts the arrivals, spx_engine.hip)
  if (speed_ready != nullptr && tid == 0)
    __hip_atomic_fetch_add(const_cast<int*>(speed_ready) + gridDim.x, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (;;) {
    int K = K_total;
    if (speed_ready != nullptr && K_total > 0) {
      if (tid == 0) {
        int got;
        unsigned spins = 0;
        for (;;) {
          got = __hip_atomic_load(&speed_ready[blockIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (got < 0 || got > (int)handed || got >= K_total) break;
          __builtin_amdgcn_s_sleep(32);
          if (++spins > (1u << 22)) { got = -2; break; }  // ~seconds: never hang the GPU on a lost producer
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        *sWait = got;
      }
      __syncthreads();
      K = uni(*sWait);
      __syncthreads();  // sWait may be rewritten by the next round
      if (K < 0) { st.overflow = 2; break; }  // the producer was lost: its own status, not an overflow
      if (K > K_total) K = K_total;
    }
    const bool last = K >= K_total;
    // Events, in the order the shim issues them:
    //   nonlinear: one (setSpeed, write B) per tension frame           soniclib.c:354,369
    //              at flush, the remaining complete ring buffers at the last speed   soniclib.c:538-550
    //   linear:    one write of everything new (soniclib.c:397-399; chunking is irrelevant at constant speed)
    //   at flush:  sonicIntFlushStream (soniclib.c:551): pad 2*maxRequired zeros, process, truncate
    const bool fin = last && do_flush;
    const pos_t ev0 = handed;
    pos_t ev1;  // one past the last ordinary event of this chunk
    if (nl != 0.0f) ev1 = fin ? ((S.flags & SPX_F_HANDED_IN) ? (pos_t)S.ring_bufs : (pos_t)(S.n_in / B)) : K;  // complete ring buffers written: soniclib.c:446-449
    else ev1 = (last && (pos_t)(S.n_in + S.tsm_shift) > avail) ? 1 : 0;
    if (ev1 < ev0) ev1 = ev0;
    const pos_t ev_end = ev1 + (fin ? 1 : 0);
    (void)ev_end;
    if constexpr (FAST != 0) {
      fast_events<NW, FAST>(P, X, st, scr, ev0, ev1, (pos_t)K, avail, B, nl == 0.0f, (pos_t)(S.n_in + S.tsm_shift), fin,
                            curSpeed);
    } else {
      for (pos_t ev = ev0; ev < ev_end; ev++) {
        pos_t expected = 0;
        if (ev < ev1) {
          if (nl != 0.0f) {
            if (ev < K) {
              const int i = (int)((ev - ev0) % SPX_CH);
              if (i == 0) {  // stage the next chunk of speeds in LDS
                __syncthreads();
                const int n = (int)min((pos_t)SPX_CH, (pos_t)K - ev);
                for (int t = tid; t < n; t += NT) sA[t] = scr[4 * (ev + t) + 3];
                __syncthreads();
              }
              curSpeed = unif(sA[i]);
            }
            avail += B;
          } else {
            avail = (pos_t)(S.n_in + S.tsm_shift);
          }
        } else {
          const pos_t remainingS = avail - st.base;
          expected = st.out_n + uni((int)(((float)remainingS / curSpeed + 0) / 1.0f + 0.5f));
          if (X.flush_rem) {  // a rate stage follows: it truncates its own output (and needs the count)
            expected = 0x7fffffff;
            if (threadIdx.x == 0) { X.flush_rem[0] = (int)remainingS; X.flush_rem[1] = (int)st.out_n; }
          }
          X.limit = avail;  // everything from here on reads as the flush's zero padding
          lds_sync<NW>();
          X.wbase = -1;     // the window may hold samples past the new limit
          avail += 2 * P.maxRequired;
        }
        STAMP(0);
        if constexpr (MAP) {
          // ring buffer `ev` is about to be handed over: the frames produced so far are its row (one 8-byte store per 10 ms of
          // input, never waited for; a linear job's one event has no row of its own)
          if (X.map && nl != 0.0f && ev < ev1 && tid == 0) X.map[ev] = (int64_t)st.out_n;
        }
        tsm_process<NW, FAST, EDITS>(P, X, st, curSpeed, avail);
        STAMP(12);
        if (ev >= ev1) {
          if (st.out_n > expected) st.out_n = expected;
          st.base = avail;  // the dependency empties its input after a flush
          st.remaining = 0;
        }
      }
    }
    if (nl != 0.0f) handed = ev1;
    if (last) break;
  }
  STAMP_FLUSH
  if (tid == 0) {
    Z.w.base = st.base; Z.w.out_n = st.out_n; Z.w.avail = avail; Z.w.remaining = st.remaining;
    Z.w.prevPeriod = st.prevPeriod; Z.w.prevMinDiff = st.prevMinDiff; Z.w.overflow = st.overflow;
    Z.w.prevPeriod_toggle = st.prevPeriod_toggle; Z.w.steps += st.steps;   // (Z.w.steps: 0 on a fresh stream, else what earlier jobs ran)
    states[blockIdx.x].w = Z.w;  // field-wise: the tension kernel may be writing its own fields of this record
    states[blockIdx.x].curSpeed = curSpeed;
    if (nl != 0.0f) states[blockIdx.x].handed = (int)handed;
    if (n_out) n_out[blockIdx.x] = st.overflow == 2 ? INT64_MIN : (st.overflow ? -(int64_t)st.out_n : (int64_t)st.out_n);
    if constexpr (MAP) {
      // the last row: the job's final count, behind flush and truncation (a linear job's only row)
      if (X.map && do_flush) X.map[nl != 0.0f ? S.n_in / B : 0] = st.overflow == 2 ? INT64_MIN : (st.overflow ? -(int64_t)st.out_n : (int64_t)st.out_n);
    }
    if constexpr (EDITS) n_ops[blockIdx.x] = X.n_ops > X.ops_cap ? -(int64_t)X.n_ops : (int64_t)X.n_ops;
  }
}

template <int NW, int FAST>
__global__ void __launch_bounds__(64 * NW)
spx_walk_kernel(SpxPlanDev P, const SpxStreamDev* __restrict__ streams, const int16_t* __restrict__ in_base,
                int16_t* __restrict__ out_base, int64_t* __restrict__ n_out, SpxStreamState* __restrict__ states,
                const float* scratch_base, int maxC, const int* speed_ready) {
  walk_body<NW, FAST, false>(P, streams, in_base, out_base, n_out, states, scratch_base, maxC, speed_ready, nullptr);
}
// The general kernel with a time map (spx_batch_run_map): row k of a stream at map_base[streams[i].map_row + k].
template <int NW>
__global__ void __launch_bounds__(64 * NW)
spx_walk_map_kernel(SpxPlanDev P, const SpxStreamDev* __restrict__ streams, const int16_t* __restrict__ in_base,
                    int16_t* __restrict__ out_base, int64_t* __restrict__ n_out, SpxStreamState* __restrict__ states,
                    const float* scratch_base, int maxC, const int* speed_ready, int64_t* __restrict__ map_base) {
  walk_body<NW, 0, true>(P, streams, in_base, out_base, n_out, states, scratch_base, maxC, speed_ready, map_base);
}
// The general kernel with an edit list (spx_batch_run_edits): stream i's records at ops_base[streams[i].map_row ...], counts in n_ops.
template <int NW>
__global__ void __launch_bounds__(64 * NW)
spx_walk_edits_kernel(SpxPlanDev P, const SpxStreamDev* __restrict__ streams, const int16_t* __restrict__ in_base,
                      int16_t* __restrict__ out_base, int64_t* __restrict__ n_out, SpxStreamState* __restrict__ states,
                      const float* scratch_base, int maxC, const int* speed_ready, int4* __restrict__ ops_base,
                      int64_t* __restrict__ n_ops, int ops_total) {
  walk_body<NW, 0, false, true>(P, streams, in_base, out_base, n_out, states, scratch_base, maxC, speed_ready, nullptr, ops_base, n_ops,
                                ops_total);
}

// Which kernel variant a batch gets: 0 general, 1 speed-up mono, 2 speed-up multi-channel.  FAST: all streams speeding
// up (speed > 1, 0 <= nonlinear <= 1: the stage never sees a speed below 1), decimated search, at most 128 lags in the coarse
// search (more than 64: the wide-coarse instantiations, round 5 -- 11.025 kHz has 72) and 121 in the refine search (rates below 64 kHz; spx_walk_fast_supports has the last word per wave count), and
// skip x channels <= 56 (the refill's exact division of the decimated planes).
static int walk_mode(const SpxPlanDev& P, int maxC, bool speedup_only) {
  if (speedup_only && P.skip >= 2 && (P.maxPeriod / P.skip - P.minPeriod / P.skip + 1) <= 128 && (8 * P.skip + 1) <= 121 &&
      P.skip * maxC <= 56 && maxC <= 8)
    return (maxC == 1) ? 1 : 2;
  return 0;
}

// Kernel variant, waves per stream and LDS per stream for a batch, and the instantiation itself (the two selectors' pick): the one
// place the launcher, the register query, the kernel names and the engine's co-residency arithmetic all ask.
SpxWalkConfig spx_walk_config(const SpxPlanDev& P, const SpxWalkAsk& ask) {
  const int n_streams = ask.n_streams, maxC = ask.max_channels < 1 ? 1 : ask.max_channels;
  const bool speedup_only = ask.speedup_only, short_jobs = ask.short_jobs, lean = ask.lean, short_window = ask.short_window;
  SpxWalkConfig c;
  const bool slow = !speedup_only && ask.any_speed;
  c.mode = walk_mode(P, maxC, speedup_only || slow);
  c.fast_kernel = c.mode == 1 || c.mode == 2;  // spx_walk_fast_kernel: mono and (round 2) multi-channel
  // Waves per stream of spx_walk_kernel.  Measured on MI355X, 10 s streams (ms per call; 2 / 4 / 8 waves): 256 streams
  // 3.67 / 3.19 / 2.91 (walk kernel alone), 512: 5.40 / 4.78 / 5.63, 1024: 10.3 / 9.3 / 10.5, 2048: 19.7 / 17.7 / -.
  c.nw = (n_streams <= 256) ? 8 : 4;
  // spx_walk_fast_kernel: search waves + output waves, window frames.  Three regimes (MI355X, 16 kHz mono x 10 s, ms per call;
  // profiles/r03/r03l_tp_variants.txt):
  //   up to two streams per CU: 4 search + 4 output waves, 4096-frame window -- a stream's chain is the run time, the
  //     output work is off it (512 streams: 3.63 against 3.89 without output waves)
  //   beyond: THROUGHPUT form -- 2 search waves, no output waves, 1536-frame window: 15 KB of LDS and two waves per stream,
  //     eight streams per CU at four waves per SIMD; the chains hide each other's latencies and the control flow is
  //     executed twice per stream, not four times (1024 streams: 5.5 against 6.3; 2048: 9.6 against 12.4; 4096: 19.0)
  // (per device: a process may hold plans on several GPUs; the count is cached, the query is not free)
  const int cus = [] {
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return 256; }
    int v = cache[dev].load(std::memory_order_relaxed);
    if (v > 0) return v;
    hipDeviceProp_t prop;
    v = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    (void)hipGetLastError();
    cache[dev].store(v, std::memory_order_relaxed);
    return v;
  }();
  //   (the register file holds five waves of the 4 + 4 form per SIMD, i.e. TWO such workgroups per CU: a third waits for a
  //   slot -- 576 streams 5.8 ms -- so the throughput form starts right above two streams per CU)
  //   short jobs (coalesced sonic2.h writes: a few pitch steps per stream and launch): nothing to amortise a 2-wave step's
  //   longer latency over; 4 search waves, output waves while a stream has a CU to itself (1024 handles x 1000 frames:
  //   511 us per round against 714 in the throughput form)
  const bool throughput = !short_jobs && n_streams > 2 * cus;
  c.nwm = throughput ? 2 : 4;
  c.nwc = throughput ? 0 : ((short_jobs && n_streams > cus) ? 0 : 4);
  c.wcap = throughput ? 1536 : 4096;
  // long jobs with at most two streams per CU on the rate-specialised kernels with output waves: the 8192-frame window (half
  // as many refills; spx_walk_fast.hip, SPEC = 1)
  // (not for the instantiations that serve slow-down: those exist in their plan-driven form only)
  if (!throughput && !short_jobs && c.fast_kernel && (P.rate == 16000 || P.rate == 22050) && !slow) c.wcap = 8192;
  // rates from 24 kHz (the eight-search-wave form): a step needs up to 2 x maxRequired frames of window, so the 4096-frame window
  // is refilled every ~2 700 frames at 44.1 kHz -- 160 times per 10 s stream; twice the window, a third of the refills
  if (!throughput && !short_jobs && c.fast_kernel && P.skip >= 6) c.wcap = 8192;
  if (lean && !throughput) { c.nwc = 0; c.wcap = 4096; }
  if (short_window && !throughput && P.skip < 6 && c.wcap > 4096) c.wcap = 4096;
  const int need = P.maxRequired + 2 * P.skip + 2;
  if (c.wcap < 2 * need) c.wcap = 2 * need;
  c.wcap = (c.wcap + 7) & ~7;
  c.nwc = c.nwc >= 4 ? 4 : 0;          // the library's forms (spx_walk_fast.hip SPX_FAST_FORMS)
  if (c.nwm == 2) c.nwc = 0;
  while (c.fast_kernel && !spx_walk_fast_supports(P, c.nwm)) {  // the coarse triangle must fit the search lanes
    if (c.nwm < 4) c.nwm = 4; else if (c.nwm < 8) c.nwm = 8; else c.fast_kernel = false;
  }
  // without spx_walk_fast_kernel: modes 1 / 2 of spx_walk_kernel hold one lag per lane and the 4096-frame window
  if (!c.fast_kernel && c.mode != 0 && !((8 * P.skip + 1) <= 64 && (P.maxPeriod / P.skip - P.minPeriod / P.skip + 1) <= 64 &&
                                           walk_lds_layout(P, maxC).wcap == 4096)) c.mode = 0;
  c.slow = slow && c.fast_kernel;
  if (c.fast_kernel) {
    c.mode = 1;
    if (c.nwm == 8) c.nwc = 4;           // the eight-search-wave form always has its four output waves
    c.waves = c.nwm + c.nwc;
    c.lds = spx_walk_fast_lds_bytes(P, c.wcap);
  } else {
    c.waves = c.nw;
    c.lds = (size_t)walk_lds_layout(P, maxC, c.mode).total;
  }
  c.kernel = c.fast_kernel ? spx_walk_fast_select(P, c.nwm, c.nwc, c.wcap, maxC, c.slow) : spx_walk_select(c.nw, c.mode);
  return c;
}
// The one place that maps (waves per stream, mode) to an instantiation of the general kernel.
SpxKernelChoice spx_walk_select(int nw, int mode) {
#define WALK_K(NWV, FASTV) SpxKernelChoice{"spx_walk_kernel", reinterpret_cast<const void*>(spx_walk_kernel<NWV, FASTV>), 64 * NWV, 2, {NWV, FASTV}}
  static_assert(std::is_same<decltype(spx_walk_kernel<8, 1>), SpxWalkArgs>::value, "SpxWalkArgs is the kernel's argument list");
  if (nw == 8) return mode == 1 ? WALK_K(8, 1) : mode == 2 ? WALK_K(8, 2) : WALK_K(8, 0);
  return mode == 1 ? WALK_K(4, 1) : mode == 2 ? WALK_K(4, 2) : WALK_K(4, 0);
#undef WALK_K
}
// ... and of the general kernel that writes a time map (mode 0 only: the speed-up forms have none).
SpxKernelChoice spx_walk_map_select(int nw) {
  static_assert(std::is_same<decltype(spx_walk_map_kernel<8>), SpxWalkMapArgs>::value, "SpxWalkMapArgs is the kernel's argument list");
  if (nw == 8) return SpxKernelChoice{"spx_walk_map_kernel", reinterpret_cast<const void*>(spx_walk_map_kernel<8>), 64 * 8, 1, {8}};
  return SpxKernelChoice{"spx_walk_map_kernel", reinterpret_cast<const void*>(spx_walk_map_kernel<4>), 64 * 4, 1, {4}};
}
// ... and of the general kernel that records an edit list (mode 0 only, as the map's).
SpxKernelChoice spx_walk_edits_select(int nw) {
  static_assert(std::is_same<decltype(spx_walk_edits_kernel<8>), SpxWalkEditsArgs>::value, "SpxWalkEditsArgs is the kernel's argument list");
  if (nw == 8) return SpxKernelChoice{"spx_walk_edits_kernel", reinterpret_cast<const void*>(spx_walk_edits_kernel<8>), 64 * 8, 1, {8}};
  return SpxKernelChoice{"spx_walk_edits_kernel", reinterpret_cast<const void*>(spx_walk_edits_kernel<4>), 64 * 4, 1, {4}};
}
int spx_walk_vgprs(const SpxPlanDev& P, const SpxWalkAsk& ask, int* scratch_bytes) {
  return spx_kernel_vgprs(spx_walk_config(P, ask).kernel.fn, scratch_bytes);
}
size_t spx_walk_lds_bytes(const SpxPlanDev& P, int maxC, bool speedup_only) {
  return spx_walk_config(P, {.n_streams = 256, .max_channels = maxC, .speedup_only = speedup_only}).lds;
}

static std::atomic<int> g_last_walk_form{0};
extern "C" int spx_debug_last_walk_form(void) { return g_last_walk_form.load(std::memory_order_relaxed); }

void spx_launch_walk(const SpxPlanDev& P, const SpxWalkAsk& ask, const SpxStreamDev* streams, const int16_t* in, int16_t* out,
                     int64_t* n_out, SpxStreamState* states, const float* scratch, const int* speed_ready, size_t lds_min,
                     hipStream_t st, int64_t* map, const SpxEditsCall* edits) {
  const int n_streams = ask.n_streams;
  if (n_streams <= 0) return;
  const int maxC = ask.max_channels < 1 ? 1 : ask.max_channels;
  const SpxWalkConfig cfg = spx_walk_config(P, ask);
  if (map) {
    // a time map: the general kernel's own instantiation, same waves and LDS.  (run_impl has refused a map call whose shape asks
    // for a speed-up form before it enqueued anything: there is no such kernel, and none is launched in its place.)
    if (cfg.fast_kernel || cfg.mode != 0) return;
    g_last_walk_form.store(0, std::memory_order_relaxed);
    SpxLaunch<SpxWalkMapArgs>::go(spx_walk_map_select(cfg.nw), n_streams, cfg.lds, st, P, streams, in, out, n_out, states, scratch, maxC, speed_ready, map);
    return;
  }
  if (edits) {
    // an edit list: the general kernel's recording instantiation, same waves and LDS (run_impl has refused, before it enqueued
    // anything, a call whose shape asks for a speed-up form)
    if (cfg.fast_kernel || cfg.mode != 0) return;
    g_last_walk_form.store(0, std::memory_order_relaxed);
    SpxLaunch<SpxWalkEditsArgs>::go(spx_walk_edits_select(cfg.nw), n_streams, cfg.lds, st, P, streams, in, out, n_out, states, scratch, maxC, speed_ready,
                                    reinterpret_cast<int4*>(edits->ops), edits->n_ops, (int)edits->total);
    return;
  }
  g_last_walk_form.store(cfg.fast_kernel ? 16 * cfg.nwm + cfg.nwc : 0, std::memory_order_relaxed);
  static const bool dbg_mode = getenv("SPX_DEBUG_MODE") != nullptr;
  if (dbg_mode) fprintf(stderr, "[spx walk] rate %d n %d maxC %d: %s %d + %d waves, window %d frames, %zu B LDS per stream (at least %zu asked)\n", P.rate, n_streams, maxC,
                        cfg.fast_kernel ? "fast kernel" : "general kernel", cfg.fast_kernel ? cfg.nwm : cfg.nw, cfg.fast_kernel ? cfg.nwc : 0, cfg.wcap, cfg.lds, lds_min);
  // lds_min (the fast kernel's callers): walk kernels of several groups launched side by side otherwise land two to a CU here and
  // there, and those chains end the call (spx_engine.hip)
  const size_t lds = cfg.fast_kernel && lds_min > cfg.lds ? lds_min : cfg.lds;
  if (cfg.fast_kernel) SpxLaunch<SpxWalkFastArgs>::go(cfg.kernel, n_streams, lds, st, P, streams, in, out, n_out, states, scratch, speed_ready, cfg.wcap);
  else SpxLaunch<SpxWalkArgs>::go(cfg.kernel, n_streams, lds, st, P, streams, in, out, n_out, states, scratch, maxC, speed_ready);
}
