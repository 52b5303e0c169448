// The lag selectors of the two walk kernels -- which lag wins an AMDF search -- in one header, so that the device check
// (spx_select_check.hip, a code object of its own) runs the very functions the kernels inline.  gfx950 only.
#pragma once
#include "spx_walk_common.h"

// ---- spx_walk_fast.hip: integer keys, one or two lags per lane ----
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
  SPX_WAVE_REDUCE("v_min_u32_dpp", v);
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}


// arg-min over the lanes of diff/lag (first lag wins ties, as the dependency's sequential scan).  Returns the lane.
__device__ __forceinline__ int fast_select(unsigned dsum, double scale, bool valid, bool needResolve, int p0,
                                           unsigned& kmin) {
  const double q = __builtin_fma((double)dsum, scale, 0x1p-12);  // floor(dsum * 65536 / p) + frac; exact (header comment)
  const unsigned key = valid ? (unsigned)q : 0xffffffffu;
  kmin = wave_min_u32(key);
  unsigned long long m = __builtin_amdgcn_ballot_w64(key == kmin);
  int idx = __builtin_ctzll(m);
  m &= m - 1;
  if (needResolve && m) {  // lag products can exceed 2^16: equal keys need not be equal ratios -- exact scan of the ties
    unsigned bd = (unsigned)__builtin_amdgcn_readlane((int)dsum, idx);
    int bp = p0 + idx;
    while (m) {
      const int i = __builtin_ctzll(m);
      m &= m - 1;
      const unsigned di = (unsigned)__builtin_amdgcn_readlane((int)dsum, i);
      const int pi = p0 + i;
      if ((unsigned long long)di * (unsigned)bp < (unsigned long long)bd * (unsigned)pi) { bd = di; bp = pi; idx = i; }
    }
  }
  return idx;
}

// The same over two lags per lane (lags lane and 64 + lane; refine searches of more than 64 lags).  Returns the lag index.
__device__ __forceinline__ int fast_select2(unsigned dsum, unsigned dsum2, double scale, double scale2, bool valid, bool valid2,
                                            bool needResolve, int p0, unsigned& kmin) {
  const double q = __builtin_fma((double)dsum, scale, 0x1p-12), q2 = __builtin_fma((double)dsum2, scale2, 0x1p-12);
  const unsigned key = valid ? (unsigned)q : 0xffffffffu, key2 = valid2 ? (unsigned)q2 : 0xffffffffu;
  kmin = wave_min_u32(key < key2 ? key : key2);
  unsigned long long m = __builtin_amdgcn_ballot_w64(key == kmin), m2 = __builtin_amdgcn_ballot_w64(key2 == kmin);
  int idx = m ? __builtin_ctzll(m) : 64 + __builtin_ctzll(m2);
  if (m) m &= m - 1; else m2 &= m2 - 1;
  if (needResolve && (m | m2)) {  // exact scan of the ties, in lag order
    unsigned bd = idx < 64 ? (unsigned)__builtin_amdgcn_readlane((int)dsum, idx) : (unsigned)__builtin_amdgcn_readlane((int)dsum2, idx - 64);
    int bp = p0 + idx;
    while (m) {
      const int i = __builtin_ctzll(m);
      m &= m - 1;
      const unsigned di = (unsigned)__builtin_amdgcn_readlane((int)dsum, i);
      const int pi = p0 + i;
      if ((unsigned long long)di * (unsigned)bp < (unsigned long long)bd * (unsigned)pi) { bd = di; bp = pi; idx = i; }
    }
    while (m2) {
      const int i = __builtin_ctzll(m2);
      m2 &= m2 - 1;
      const unsigned di = (unsigned)__builtin_amdgcn_readlane((int)dsum2, i);
      const int pi = p0 + 64 + i;
      if ((unsigned long long)di * (unsigned)bp < (unsigned long long)bd * (unsigned)pi) { bd = di; bp = pi; idx = 64 + i; }
    }
  }
  return idx;
}

// ---- spx_walk.hip: float ratios and an exact rescan, 64 lags per fold ----
// Running result of the dependency's sequential arg-min / arg-max scan over lags.
struct Sel {
  unsigned bestD, worstD;
  int bestP, worstP;
};

// Fold the 64 lanes' (d, p) candidates (lane order = ascending lag) into the running result, exactly as a
// sequential scan would: float ratios, DPP wave min/max, then an exact integer resolve on the scalar unit of the
// lanes within 2^-16 of the extremum (strict compare, so the FIRST lag wins ties).  Wave-uniform result.
template <bool WANT_MAX, bool FRESH = false>
__device__ __forceinline__ void select_fold(Sel& S, unsigned d, int p0, bool valid) {
  const int lane = threadIdx.x & 63;
  const float r = (float)d * __builtin_amdgcn_rcpf((float)(p0 + lane));  // within 2^-21 of d/p
  const float rmin = wave_min_f(valid ? r : __builtin_huge_valf());
  unsigned long long mmin = __builtin_amdgcn_ballot_w64(valid && r <= rmin * 1.0000153f);  // 1 + 2^-16
  if (FRESH) {  // S is empty and some lane is valid: the first candidate is taken without a comparison
    const int i = __builtin_ctzll(mmin);
    mmin &= mmin - 1;
    S.bestD = (unsigned)__builtin_amdgcn_readlane((int)d, i);
    S.bestP = p0 + i;
  }
  while (mmin) {
    const int i = __builtin_ctzll(mmin);
    mmin &= mmin - 1;
    const unsigned di = (unsigned)__builtin_amdgcn_readlane((int)d, i);
    const int pi = p0 + i;
    if (S.bestP == 0 || (unsigned long long)di * (unsigned)S.bestP < (unsigned long long)S.bestD * (unsigned)pi) {
      S.bestD = di;
      S.bestP = pi;
    }
  }
  if (WANT_MAX) {
    const float rmax = wave_max_f(valid ? r : 0.0f);
    unsigned long long mmax = __builtin_amdgcn_ballot_w64(valid && r >= rmax * 0.9999847f);
    while (mmax) {
      const int i = __builtin_ctzll(mmax);
      mmax &= mmax - 1;
      const unsigned di = (unsigned)__builtin_amdgcn_readlane((int)d, i);
      const int pi = p0 + i;
      if (S.worstP == 0 ||
          (unsigned long long)di * (unsigned)S.worstP > (unsigned long long)S.worstD * (unsigned)pi) {
        S.worstD = di;
        S.worstP = pi;
      }
    }
  }
}
__device__ __forceinline__ void select_finish(const Sel& S, int* retBest, int* retMin, int* retMax) {
  // the scan's initial (maxDiff = 0, worstPeriod = 255) survives unless some lag has diff > 0
  const unsigned worstD = S.worstD;
  const int worstP = (worstD == 0) ? 255 : S.worstP;
  *retBest = uni(S.bestP);
  *retMin = uni((int)udiv_small(S.bestD, (unsigned)S.bestP));
  *retMax = uni((int)udiv_small(worstD, (unsigned)worstP));
}

