// The two-pass batch call's second-pass speed (include/speedy_hip.h: spx_batch_run_twopass) as ONE inline function without HIP: the
// retarget kernel (spx_twopass.hip) and the host-only table library (spx_mode_table.cpp, plain g++; tests/test_twopass_abi.py
// compares it with a numpy definition bit for bit) compile this text.  Types and rounding points are those of the two-pass drivers
// of tools/speedy_wave_hip.cpp:179-191 (speedy_wave.cc:424-461): the achieved speed is frames read / frames produced in double,
// the correction want * (want / got) in double, and the speed reaches the stream as a float (sonicSetSpeed).
// Both builds evaluate / and * as single correctly rounded IEEE operations (-fno-fast-math -ffp-contract=off on the device; there is
// no product-sum here that a host compiler could fuse).
#ifndef SPX_TWOPASS_H_
#define SPX_TWOPASS_H_
#include <stdint.h>

#if defined(__HIPCC__)
#define SPX_TWOPASS_FN __host__ __device__ static inline
#else
#define SPX_TWOPASS_FN static inline
#endif

// want: the speed the probe pass was asked for, as a double (the probe itself ran at (float)want)
// length_mode: 0 = the final pass runs at the achieved speed (--match_nonlinear), else at want * (want / achieved) (--length)
// T: the stream's input frames; n_probe: the probe pass's count (<= 0: nothing to measure -- an empty stream, one too short to
// emit anything, an overflow, a lost producer -- and the final pass runs at the probe's speed)
SPX_TWOPASS_FN float spx_twopass_speed(double want, int length_mode, int64_t T, int64_t n_probe) {
  if (n_probe <= 0) return (float)want;
  const double got = (double)T / (double)n_probe;
  if (!length_mode) return (float)got;
  const double ratio = want / got;
  return (float)(want * ratio);
}

// One record per stream of the retarget table (HOST-built, DEVICE-read): 32-bit words for the staging kernel.
struct SpxRetargetJob {
  double want;
  int64_t n_in;
  int32_t length_mode;
  int32_t pad_;
};

#endif  // SPX_TWOPASS_H_
