// Tension kernel for launches WITHOUT tile flags (kernels in sequence, pipelined and overlapped calls, time chunks, sub-batches):
// the chain of spx_tension_kernel (spx_tension.hip) in one pass over LDS.  Both kernels compile the arithmetic of spx_frame_math.h:
// they differ in staging, in the waves that run each chain and in polling, not in the text of an operation.
//
// spx_tension_kernel makes four passes, each through global memory, and runs its three recurrences one after the other on one
// lane.  That layout serves the concurrent mode, where the kernel polls tile flags and must stay inside 48 registers and 4 KB of
// LDS (spx_mode.h).  A launch behind a finished analysis kernel has every frame at hand, so here the stages form a pipeline over
// 64-slot blocks, one block per step and one __syncthreads() per step, nothing else between the waves:
//
//   step s   wave 0   the prefetched records of block s go to LDS, the loads of block s + 1 are issued,
//                     chain 1 (energy low-pass) runs over block s - 1
//            wave 1   chain 2 (difference low-pass, block s - 5); blended speeds to memory (block s - 8)
//            wave 2   chain 3 (duration sums, block s - 7); local energy, sqrt compression (block s - 2)
//            wave 3   hysteresis maxima, gate, emphasis weighting (block s - 4); relative difference, tension, raw speed
//                     (block s - 6)
// (the one-lane-per-frame stages are spread so that no wave carries much more than a chain's worth of cycles per step)
//
// A slot is a time index tau: it holds frame tau - t0 (spx_tension.hip: "frame j is added at time j + t0"), and tension frame k
// lives in slot k.  Every per-slot value sits in a ring of eight blocks, so the LDS does not grow with the stream; a value is
// written to global memory once and never read back by a later stage.  Only a resumed job (frame_begin > 0: a later time chunk of
// a large call) loads the compressed energies of the F + Pp frames before its first one, once, with the records of their block.
// The trip count of the step loop is fixed before it starts: there is no flag, no poll and no sleep in this kernel.
#include "spx_internal.h"
#include "spx_frame_math.h"

#define SPX_TSQ_THREADS 256
#define SPX_TSQ_BLK 64                 // slots per block = lanes of a wave
#define SPX_TSQ_NBLK 8                 // blocks per ring: a block's values are last read eight steps after its load
#define SPX_TSQ_RING (SPX_TSQ_BLK * SPX_TSQ_NBLK)
#define SPX_TSQ_TAPS (SPX_TSQ_BLK + 1)  // F + 1, Pp + 1 <= 65: the hysteresis reaches at most one block ahead and back

// One block of y[i] = a*x[i] + b*y[i-1] over the slots [lo, hi) of the block (uniform bounds), as iir_wave of spx_tension.hip:
// 64 products a*x[i] in parallel, the chain on lane 0 with a v_readlane per element.  Run by one whole wave; returns the last y.
__device__ __forceinline__ float tsq_iir_block(const float* x, float* yo, int lo, int hi, float a, float b, float y) {
  const int lane = threadIdx.x & 63;
  const float ax = spx_fm_lowpass_input(a, (lane >= lo && lane < hi) ? x[lane] : 0.0f);
  if (lo == 0 && hi == SPX_TSQ_BLK) {
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < SPX_TSQ_BLK; j++) {
        const float s = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ax), j));
        y = spx_fm_lowpass_step(s, b, y);
        yo[j] = y;
      }
    }
  } else if (lane == 0) {
#pragma unroll
    for (int j = 0; j < SPX_TSQ_BLK; j++) {
      if (j >= lo && j < hi) {  // uniform
        const float s = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ax), j));
        y = spx_fm_lowpass_step(s, b, y);
        yo[j] = y;
      }
    }
  }
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, y)));
}

// The tapered maxima of the hysteresis (speedy.c:590-610) for tension frame k: slot tau holds frame tau - t0, earlier slots are the
// zero init.  NF, NP: the plan's F and Pp as constants (the two shapes every plan has: the taps' LDS reads then go out together);
// <0, 0>: any F, Pp at run time.  The same products and comparisons in the same order either way.
template <int NF, int NP>
__device__ __forceinline__ void tsq_hyst_max(const float* sC, const float* sTF, const float* sTP, int k, int base, int t0, int F,
                                             int Pp, float& future_max, float& past_max) {
  const int nf = NF ? NF : F, np = NP ? NP : Pp;
#pragma unroll
  for (int i = 0; i <= nf; i++) {
    const int tau = k + i;
    const float c = sC[(tau - base) & (SPX_TSQ_RING - 1)];
    const float v = spx_fm_hysteresis_tap((tau >= t0) ? c : 0.0f, sTF[i]);
    if (v > future_max) future_max = v;
  }
#pragma unroll
  for (int i = 0; i <= np; i++) {
    const int tau = k - i;
    const float c = sC[(tau - base) & (SPX_TSQ_RING - 1)];
    const float v = spx_fm_hysteresis_tap((tau >= t0) ? c : 0.0f, sTP[i]);
    if (v > past_max) past_max = v;
  }
}

__global__ void __launch_bounds__(SPX_TSQ_THREADS)
spx_tension_seq_kernel(SpxPlanDev P, const SpxStreamDev* __restrict__ streams, SpxStreamState* __restrict__ states,
                       const SpxFrameRec* __restrict__ rec_base, float* __restrict__ scratch_base, SpxTapsDev taps,
                       int* speed_ready) {
  constexpr int BLK = SPX_TSQ_BLK, RING = SPX_TSQ_RING;
  // per slot: energy, lsd, low-passed energy, comp, hyst, ewld, low-passed ewld, raw speed, blended speed
  __shared__ float sE[RING], sL[RING], sLP[RING], sC[RING], sH[RING], sW[RING], sLF[RING], sV[RING], sS[RING];
  __shared__ float sTF[SPX_TSQ_TAPS], sTP[SPX_TSQ_TAPS];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const SpxStreamDev S = streams[blockIdx.x];
  const int T = S.n_frames, fa = S.frame_begin, F = P.F, Pp = P.Pp;
  const int t0 = S.unit_time0 ? 0 : 1;
  const float Rg = S.speed, nl = S.nonlinear, fb = S.feedback;
  if (nl == 0.0f) return;  // a linear stream has no frames (uniform per workgroup)

  float lp, lpf, cur_dur, des_dur;
  int first_k;
  if (S.flags & SPX_F_INIT) {
    lp = SPX_FM_ENERGY_LP0;
    lpf = SPX_FM_DIFFERENCE_LP0;
    cur_dur = 0.0f; des_dur = 0.0f;
    first_k = -1;
  } else {
    const SpxStreamState& in = states[blockIdx.x];
    lp = in.lp; lpf = in.lpf; cur_dur = in.cur_dur; des_dur = in.des_dur;
    first_k = in.tension_first;
  }
  const SpxFrameRec* rec = rec_base + S.frame_off;
  float* scr = scratch_base + (size_t)S.frame_off * 4;  // per frame: comp, hyst, tension, speed
  const float lowthr = SPX_FM_LOW_THRESHOLD;
  float* tfeat = taps.features ? taps.features + (size_t)S.frame_off * SPX_FEATURE_COUNT : nullptr;

  // the tension frames of this job, as spx_tension.hip forms them
  int K0 = (fa + t0 >= F) ? fa + t0 - F : 0;
  if (K0 < S.tension_skip) K0 = S.tension_skip;
  int K = (T + t0 >= F) ? T + t0 - F : 0;
  if (S.flags & SPX_F_TENSION_RANGE) {
    K0 = S.tension_skip;
    if (K > S.tension_to) K = S.tension_to;
  }
  if (first_k < 0 && K > K0) first_k = K0;
  const int K4 = (S.flags & SPX_F_NO_SPEED) ? K0 : K;  // the end of the duration / blend stage

  // The slots the pipeline runs over: the new frames' [fa + t0, T + t0) and the tension frames with their reach, [K0 - Pp, K + F).
  // (K + F <= T + t0 always, so every slot at or above t0 holds a frame below T.)
  int lo = 0, hi = 0;
  if (T > fa) { lo = fa + t0; hi = T + t0; }
  if (K > K0) {
    const int l2 = K0 > Pp ? K0 - Pp : 0, h2 = K + F;
    if (hi <= lo) { lo = l2; hi = h2; }
    else { lo = lo < l2 ? lo : l2; hi = hi > h2 ? hi : h2; }
  }
  const int base = lo;
  const int nb = hi > lo ? (hi - lo + BLK - 1) / BLK : 0;

  for (int i = tid; i <= F; i += SPX_TSQ_THREADS) sTF[i] = P.taperF[i];
  for (int i = tid; i <= Pp; i += SPX_TSQ_THREADS) sTP[i] = P.taperP[i];

  // wave 0's prefetch of one block: the record of the slot's frame, and for a frame of an earlier job its compressed energy
  SpxFrameRec pre = {0.0f, 0.0f};
  float pre_c = 0.0f;
  auto prefetch = [&](int b) {
    int j = base + b * BLK + lane - t0;
    j = j < 0 ? 0 : (j >= T ? T - 1 : j);         // nb > 0 implies T >= 1; readers take only slots whose frame is in range
    pre = rec[j];
    if (fa > 0) pre_c = scr[4 * (j < fa ? j : fa - 1) + 0];
  };
  if (wave == 0 && nb > 0) prefetch(0);
  __syncthreads();

  const int steps = nb > 0 ? nb + SPX_TSQ_NBLK : 0;
  for (int s = 0; s < steps; s++) {
    if (wave == 0) {
      if (s < nb) {
        const int r = (s & (SPX_TSQ_NBLK - 1)) * BLK + lane;
        const int j = base + s * BLK + lane - t0;
        sE[r] = pre.energy;
        sL[r] = pre.lsd;
        if (j >= 0 && j < fa) sC[r] = pre_c;
      }
      if (s + 1 < nb) prefetch(s + 1);
      const int b = s - 1;
      if (b >= 0 && b < nb) {
        // ---- chain 1: energy low-pass over the new frames (speedy.c:74) ----
        const int j0 = base + b * BLK - t0, r0 = (b & (SPX_TSQ_NBLK - 1)) * BLK;
        int l1 = fa - j0, h1 = T - j0;
        l1 = l1 < 0 ? 0 : l1; h1 = h1 > BLK ? BLK : h1;
        if (h1 > l1) lp = tsq_iir_block(sE + r0, sLP + r0, l1, h1, P.one_minus_alpha, P.alpha, lp);
      }
    } else if (wave == 3) {
      int b = s - 4;
      if (b >= 0 && b < nb) {
        // ---- hysteresis and emphasis-weighted difference, one lane per tension frame ----
        const int r = (b & (SPX_TSQ_NBLK - 1)) * BLK + lane;
        const int k = base + b * BLK + lane;
        if (k >= K0 && k < K) {
          float future_max = 0.0f, past_max = 0.0f;
          if (F == 12 && Pp == 8) tsq_hyst_max<12, 8>(sC, sTF, sTP, k, base, t0, F, Pp, future_max, past_max);
          else if (F == 8 && Pp == 12) tsq_hyst_max<8, 12>(sC, sTF, sTP, k, base, t0, F, Pp, future_max, past_max);
          else tsq_hyst_max<0, 0>(sC, sTF, sTP, k, base, t0, F, Pp, future_max, past_max);
          const float hyst = spx_fm_hysteresis(past_max, future_max);
          const float e_cur = (k < t0) ? 0.0f : sE[r];                        // slot k holds frame k - t0
          const bool low = spx_fm_low_energy(e_cur) || k == first_k;          // the very first call is skipped
          const float lsd = low ? 0.0f : sL[r];
          const float ewld = low ? 0.0f : spx_fm_weighted(lsd, hyst);
          sH[r] = hyst;
          sW[r] = ewld;
          if (tfeat) {
            float* f = tfeat + (size_t)k * SPX_FEATURE_COUNT;
            f[0] = e_cur; f[4] = hyst; f[5] = low ? 1.0f : 0.0f; f[6] = lsd; f[7] = ewld;
            f[13] = (float)k; f[14] = lowthr;
          }
        }
      }
      b = s - 6;
      if (b >= 0 && b < nb) {
        // ---- relative difference, clamp, tension, raw speed ----
        const int r = (b & (SPX_TSQ_NBLK - 1)) * BLK + lane;
        const int k = base + b * BLK + lane;
        if (k >= K0 && k < K) {
          const float ewld = sW[r], l = sLF[r];
          const float hyst = sH[r];
          const float e_cur = (k < t0) ? 0.0f : sE[r];
          const bool low = spx_fm_low_energy(e_cur) || k == first_k;
          float rel = 0.0f, sc = 0.0f;
          if (!low) {
            rel = spx_fm_relative(ewld, l);
            sc = spx_fm_clamp(rel);
          }
          const float tension = spx_fm_tension(hyst, sc);
          const float v = spx_fm_raw_speed(Rg, tension);
          sV[r] = v;
          scr[4 * k + 1] = hyst;
          scr[4 * k + 2] = tension;
          if (k >= K4) scr[4 * k + 3] = v;   // no duration / blend stage follows (SPX_F_NO_SPEED)
          if (tfeat) {
            float* f = tfeat + (size_t)k * SPX_FEATURE_COUNT;
            f[8] = l; f[9] = rel; f[10] = sc; f[11] = tension;
          }
          if (taps.tension) taps.tension[S.frame_off + k] = tension;
        }
      }
    } else if (wave == 2) {
      int b = s - 7;
      if (b >= 0 && b < nb) {
        // ---- chain 3: duration sums, blend with the global speed ----
        const int k0 = base + b * BLK, r0 = (b & (SPX_TSQ_NBLK - 1)) * BLK;
        int l3 = K0 - k0, h3 = K4 - k0;
        l3 = l3 < 0 ? 0 : l3; h3 = h3 > BLK ? BLK : h3;
        if (h3 > l3) {
          if (!(fb > 0)) {
            // open loop (speedy.c:779 not taken): only the two float sums are sequential
            const float cstep = spx_fm_frame_time(Rg);
            const bool mine = lane >= l3 && lane < h3;
            const float req = mine ? sV[r0 + lane] : 1.0f;
            const float q = spx_fm_frame_time(req);
            if (lane == 0) {
              if (l3 == 0 && h3 == BLK) {
#pragma unroll
                for (int j = 0; j < BLK; j++) {
                  cur_dur += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, q), j));
                  des_dur += cstep;
                }
              } else {
#pragma unroll
                for (int j = 0; j < BLK; j++) {
                  if (j >= l3 && j < h3) {  // uniform
                    cur_dur += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, q), j));
                    des_dur += cstep;
                  }
                }
              }
            }
            if (mine) sS[r0 + lane] = spx_fm_blend(req, nl, Rg);
          } else if (lane == 0) {
            for (int i = l3; i < h3; i++) {
              float req = sV[r0 + i];
              if (fb > 0) req = spx_fm_feedback(req, fb, cur_dur, des_dur);
              cur_dur = spx_fm_advance(cur_dur, req);
              des_dur = spx_fm_advance(des_dur, Rg);
              sS[r0 + i] = spx_fm_blend(req, nl, Rg);
            }
          }
          cur_dur = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, cur_dur)));
          des_dur = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, des_dur)));
        }
      }
      b = s - 2;
      if (b >= 0 && b < nb) {
        // ---- local energy, compression ----
        const int r = (b & (SPX_TSQ_NBLK - 1)) * BLK + lane;
        const int j = base + b * BLK + lane - t0;
        if (j >= fa && j < T) {
          const float e = sE[r], l = sLP[r];
          const float local = spx_fm_local_energy(e, l);
          const float comp = spx_fm_compress(local);
          sC[r] = comp;
          scr[4 * j + 0] = comp;
          const int k = j + t0 - F;  // the tension frame whose callback sees these AddData-time values
          if (tfeat && k >= 0) {
            float* f = tfeat + (size_t)k * SPX_FEATURE_COUNT;
            f[1] = l; f[2] = local; f[3] = comp; f[12] = (float)(j + t0);
          }
        }
      }
    } else {
      int b = s - 5;
      if (b >= 0 && b < nb) {
        // ---- chain 2: difference low-pass over the tension frames ----
        const int k0 = base + b * BLK, r0 = (b & (SPX_TSQ_NBLK - 1)) * BLK;
        int l2 = K0 - k0, h2 = K - k0;
        l2 = l2 < 0 ? 0 : l2; h2 = h2 > BLK ? BLK : h2;
        if (h2 > l2) lpf = tsq_iir_block(sW + r0, sLF + r0, l2, h2, P.one_minus_alpha, P.alpha, lpf);
      }
      b = s - 8;
      if (b >= 0 && b < nb) {
        // ---- the blended speeds leave ----
        const int r = (b & (SPX_TSQ_NBLK - 1)) * BLK + lane;
        const int k = base + b * BLK + lane;
        if (k >= K0 && k < K4) {
          const float v = sS[r];
          scr[4 * k + 3] = v;
          if (taps.speed) taps.speed[S.frame_off + k] = v;
        }
      }
    }
    __syncthreads();
  }

  // every chain's wave leaves its part of the state record
  if (lane == 0) {
    SpxStreamState& o = states[blockIdx.x];
    if (wave == 0) { o.lp = lp; o.tension_first = first_k; }
    else if (wave == 1) o.lpf = lpf;
    else if (wave == 2) { o.cur_dur = cur_dur; o.des_dur = des_dur; }
  }
  if (speed_ready != nullptr) spx_publish_speed_ready(speed_ready, K);   // this job's speeds, taps and state
}

void spx_launch_tension_seq(const SpxPlanDev& P, const SpxStreamDev* streams, int n_streams, SpxStreamState* states,
                            const SpxFrameRec* rec, float* scratch, SpxTapsDev taps, int* speed_ready, hipStream_t st) {
  hipLaunchKernelGGL(spx_tension_seq_kernel, dim3(n_streams), dim3(SPX_TSQ_THREADS), 0, st, P, streams, states, rec, scratch,
                     taps, speed_ready);
}
bool spx_tension_seq_serves(const SpxPlanDev& P) { return P.F < SPX_TSQ_TAPS && P.Pp < SPX_TSQ_TAPS; }
