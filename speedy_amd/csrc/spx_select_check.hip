// Device checks of the walk kernels' lag selectors (spx_select.h: fast_select, fast_select2 of the speed-up kernel; select_fold,
// select_finish of the general one) on vectors of sums the host supplies -- the idiom of spx_debug_xfade_check.  A code object of
// its own: nothing is added to the code objects of the walk kernels.  One wave per vector.
#include "spx_select.h"

// the documented precondition of both checks: d <= 65535 * lag in the valid lanes (the keys and udiv_small rely on it)
static bool select_rows_in_range(const unsigned* d, int n_vectors, int width, int p0, int n_lags) {
  for (int v = 0; v < n_vectors; v++)
    for (int i = 0; i < n_lags; i++)
      if ((unsigned long long)d[(size_t)v * width + i] > 65535ull * (unsigned)(p0 + i)) return false;
  return true;
}

// The speed-up kernel's selector: lane = lag index (two: lags lane and 64 + lane).  `scale` is the expression the kernel's table is
// filled from (65536.0 / (double)lag; an invalid lane reads the first lag's entry), needResolve the kernel's (maxP^2 >= 65536).
// A row is 64 words (128 with two lags per lane), ALL of them read: what lies in the invalid lanes must not matter.
__global__ void __launch_bounds__(64) spx_select_check_kernel(const unsigned* __restrict__ d, int n_vectors, int p0, int nl, int maxP,
                                                              int two, int* __restrict__ idx_out, unsigned* __restrict__ kmin_out) {
  const int lane = threadIdx.x;
  const bool needResolve = (long)maxP * maxP >= 65536;
  const bool valid = lane < nl, valid2 = two && lane + 64 < nl;
  const double scale = 65536.0 / (double)(valid ? p0 + lane : p0);
  const double scale2 = two ? 65536.0 / (double)(valid2 ? p0 + 64 + lane : p0) : 0.0;
  const int width = two ? 128 : 64;
  for (int v = blockIdx.x; v < n_vectors; v += gridDim.x) {
    const unsigned* row = d + (size_t)v * width;
    const unsigned dsum = row[lane], dsum2 = two ? row[64 + lane] : 0u;
    unsigned kmin;
    int best;
    if (two) best = fast_select2(dsum, dsum2, scale, scale2, valid, valid2, needResolve, p0, kmin);
    else best = fast_select(dsum, scale, valid, needResolve, p0, kmin);
    if (lane == 0) { idx_out[v] = best; kmin_out[v] = kmin; }
  }
}
extern "C" int spx_debug_select_check(const unsigned* d, int n_vectors, int p0, int n_lags, int max_period, int two_per_lane,
                                      int* lag_index, unsigned* kmin) {
  const int width = two_per_lane ? 128 : 64;
  if (!d || !lag_index || !kmin || n_vectors < 1 || n_vectors > (1 << 22) || p0 < 1 || n_lags < 1 || n_lags > width ||
      p0 + n_lags - 1 > 4096 || max_period < 1 || max_period > 4096) return -1;
  if (!select_rows_in_range(d, n_vectors, width, p0, n_lags)) return -1;
  const size_t nb = sizeof(unsigned) * (size_t)n_vectors * width;
  unsigned* dd = nullptr;
  int* di = nullptr;
  unsigned* dk = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&dd), nb);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&di), sizeof(int) * (size_t)n_vectors);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&dk), sizeof(unsigned) * (size_t)n_vectors);
  if (e == hipSuccess) e = hipMemcpy(dd, d, nb, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(spx_select_check_kernel, dim3(n_vectors < 4096 ? n_vectors : 4096), dim3(64), 0, nullptr, dd, n_vectors, p0,
                       n_lags, max_period, two_per_lane ? 1 : 0, di, dk);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(lag_index, di, sizeof(int) * (size_t)n_vectors, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(kmin, dk, sizeof(unsigned) * (size_t)n_vectors, hipMemcpyDeviceToHost);
  (void)hipFree(dd); (void)hipFree(di); (void)hipFree(dk);
  return e == hipSuccess ? 0 : -1;
}

// The general kernel's selector: a vector of nl lags is folded 64 lags at a time into one running result, as search_split does.
// fresh: the first fold takes its first candidate without a comparison (the FRESH form, what the one-fold searches of the FAST
// modes use); the later folds are always the plain form.  A row is nl rounded up to whole folds, ALL words read.
__global__ void __launch_bounds__(64) spx_select_fold_check_kernel(const unsigned* __restrict__ d, int n_vectors, int p0, int nl,
                                                                   int want_max, int fresh, int* __restrict__ out3) {
  const int lane = threadIdx.x;
  const int width = (nl + 63) & ~63;
  for (int v = blockIdx.x; v < n_vectors; v += gridDim.x) {
    const unsigned* row = d + (size_t)v * width;
    Sel S = {0u, 0u, 0, 0};
    for (int base = 0; base < nl; base += 64) {
      const bool valid = base + lane < nl;
      const unsigned dd = row[base + lane];
      if (want_max) {
        if (fresh && base == 0) select_fold<true, true>(S, dd, p0 + base, valid);
        else select_fold<true, false>(S, dd, p0 + base, valid);
      } else {
        if (fresh && base == 0) select_fold<false, true>(S, dd, p0 + base, valid);
        else select_fold<false, false>(S, dd, p0 + base, valid);
      }
    }
    int best, minDiff, maxDiff;
    select_finish(S, &best, &minDiff, &maxDiff);
    if (lane == 0) { out3[3 * v] = best; out3[3 * v + 1] = minDiff; out3[3 * v + 2] = maxDiff; }
  }
}
extern "C" int spx_debug_select_fold_check(const unsigned* d, int n_vectors, int p0, int n_lags, int want_max, int fresh, int* out3) {
  if (!d || !out3 || n_vectors < 1 || n_vectors > (1 << 22) || p0 < 10 || n_lags < 1 || n_lags > 2048 || p0 + n_lags - 1 > 2048) return -1;
  const int width = (n_lags + 63) & ~63;
  if (!select_rows_in_range(d, n_vectors, width, p0, n_lags)) return -1;
  const size_t nb = sizeof(unsigned) * (size_t)n_vectors * width;
  unsigned* dd = nullptr;
  int* dout = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&dd), nb);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&dout), sizeof(int) * 3 * (size_t)n_vectors);
  if (e == hipSuccess) e = hipMemcpy(dd, d, nb, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(spx_select_fold_check_kernel, dim3(n_vectors < 4096 ? n_vectors : 4096), dim3(64), 0, nullptr, dd, n_vectors, p0,
                       n_lags, want_max ? 1 : 0, fresh ? 1 : 0, dout);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out3, dout, sizeof(int) * 3 * (size_t)n_vectors, hipMemcpyDeviceToHost);
  (void)hipFree(dd); (void)hipFree(dout);
  return e == hipSuccess ? 0 : -1;
}
