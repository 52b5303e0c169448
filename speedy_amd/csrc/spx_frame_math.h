// The frame-rate feature chain (rows a6 - a9 of DESIGN.md: energy low-pass ... tension, speed, duration feedback, blend) as ONE
// text without HIP: one inline function per statement of the reference, with that statement's line in speedy.c / soniclib.c.
// spx_tension_kernel and spx_speed_kernel (spx_tension.hip), spx_tension_seq_kernel (spx_tension_seq.hip), the hk_* kernels of the
// unit-level API (speedy_api.hip), the analysis kernel's low-energy threshold (spx_analysis.hip) and the host-only table library
// (spx_mode_table.cpp, plain g++ with -ffp-contract=off; tests/test_frame_math.py holds it to the oracle's taps bit for bit) compile
// this text; none restates it.
//
// Every rounding point is load-bearing: which products are float and which double, each cast, and no fused multiply-add.
//
// BY VALUE: arguments and results are passed by value, never through a reference or a pointer.  Inlined by-value functions
// leave the kernels' ISA what the written-out expressions gave (profiles/frame_math.txt); a `float&` out-parameter on the
// compression alone moved spx_tension_kernel's spill register and took it from 48 to 49 VGPRs, one over its budget.
#ifndef SPX_FRAME_MATH_H_
#define SPX_FRAME_MATH_H_
#include <math.h>

#if defined(__HIPCC__)   // (__forceinline__ is the HIP runtime header's: a .hip file includes this one behind spx_internal.h)
#define SPX_FM_FN __host__ __device__ __forceinline__
#else
#define SPX_FM_FN static inline
#endif

#define SPX_FM_ENERGY_LP0 2.14204f                                   // speedy.c:263,288  start of the energy low-pass
#define SPX_FM_DIFFERENCE_LP0 123.837f                               // speedy.c:264,291  start of the difference low-pass
#define SPX_FM_RELATIVE_OFFSET (0.01 * (double)123.979f)             // speedy.c:726      a double
#define SPX_FM_CLAMP (4 * 0.971975f)                                 // speedy.c:728      a float product
#define SPX_FM_LOW_THRESHOLD ((float)(0.04 * (double)1.41421f))      // speedy.c:682      a double product stored as float
#define SPX_FM_FRAME_DURATION ((float)(1.0 / 100.0))                 // speedy.c:783
#define SPX_FM_A 0.5f                                                // speedy.c:754      a, b, M_E, M_S of the tension
#define SPX_FM_B 0.25f
#define SPX_FM_M_E 0.7f
#define SPX_FM_M_S 1.0f

// speedy.c:74  y = one_minus_alpha * x + alpha * y: float product, float product, float sum.  In two halves, because the kernels
// form the input products of 64 frames at once and run only the step in sequence.
SPX_FM_FN float spx_fm_lowpass_input(float one_minus_alpha, float x) { return one_minus_alpha * x; }
SPX_FM_FN float spx_fm_lowpass_step(float input, float alpha, float y) { return input + alpha * y; }
SPX_FM_FN float spx_fm_lowpass(float one_minus_alpha, float alpha, float x, float y) {
  return spx_fm_lowpass_step(spx_fm_lowpass_input(one_minus_alpha, x), alpha, y);
}

// speedy.c:519  local energy: the frame's energy over its low-pass
SPX_FM_FN float spx_fm_local_energy(float e, float l) { return e / l; }
// speedy.c:520  compression: the double sqrt of min(local, 2)
SPX_FM_FN float spx_fm_compress(float local) { return (float)__builtin_sqrt(local > 2 ? 2.0 : (double)local); }

// speedy.c:594-608  one tap of a tapered maximum: the compressed energy under its weight.  The caller keeps the running maximum,
// `if (v > max) max = v`, an exact operation.  (NOT SHARED: returned from a function here, the maximum changed the code of
// spx_tension_seq_kernel's hysteresis stage -- same registers, 22 instructions fewer, a kernel nobody has timed.)
SPX_FM_FN float spx_fm_hysteresis_tap(float c, float taper) { return c * taper; }
// speedy.c:609
SPX_FM_FN float spx_fm_hysteresis(float past_max, float future_max) { return (float)((double)(past_max + future_max) / 2.0); }

// speedy.c:682-692  the low-energy gate.  A frame is low if this holds OR it is the first tension call ever, which is skipped whatever
// its energy (speedy.c:293,691); each caller writes `spx_fm_low_energy(e) || k == first_k` itself, the unit-level API with its own
// notion of "first".  (NOT SHARED: with the `||` inside a function -- operands either way round, `|`, or the test passed as a bool --
// one s_or_b64 and one s_and_b64 of spx_tension_kernel swap their operands or two compares change their encoding.)
SPX_FM_FN bool spx_fm_low_energy(float e) { return e <= SPX_FM_LOW_THRESHOLD; }

// speedy.c:720  emphasis-weighted local difference
SPX_FM_FN float spx_fm_weighted(float lsd, float hyst) { return lsd * hyst; }
// speedy.c:725-726  relative difference: a double quotient stored as float
SPX_FM_FN float spx_fm_relative(float ewld, float l) { return (float)((double)ewld / ((double)l + SPX_FM_RELATIVE_OFFSET)); }
// speedy.c:727-728
SPX_FM_FN float spx_fm_clamp(float rel) { return (float)fmin((double)rel, (double)SPX_FM_CLAMP); }

// speedy.c:761
SPX_FM_FN float spx_fm_tension(float hyst, float sc) { return SPX_FM_A * (hyst - SPX_FM_M_E) + SPX_FM_B * (sc - SPX_FM_M_S); }

// speedy.c:773-776  speed from tension, before the feedback
SPX_FM_FN float spx_fm_raw_speed(float Rg, float tension) {
  if ((double)Rg > 1.0) return (float)fmax(1.0, (double)(Rg + (1 - Rg) * tension));   // speedy.c:774
  return (float)fmax(0.01, fmin(1.0, (double)(Rg - (1 - Rg) * tension)));             // speedy.c:776
}
// speedy.c:780-781  the requested speed under duration feedback (the caller asks fb > 0, speedy.c:779)
SPX_FM_FN float spx_fm_feedback(float req, float fb, float cur_dur, float des_dur) {
  const float excess = cur_dur - des_dur;
  return (float)((double)req + fmax(0.01, (double)(fb * excess)));
}
// speedy.c:784-785  both duration sums advance by one frame's time at a speed: the current one at the requested speed, the
// desired one at the global speed
SPX_FM_FN float spx_fm_frame_time(float speed) { return SPX_FM_FRAME_DURATION / speed; }
SPX_FM_FN float spx_fm_advance(float dur, float speed) { return dur + spx_fm_frame_time(speed); }
// soniclib.c:344-345  blend with the global speed
SPX_FM_FN float spx_fm_blend(float req, float nl, float Rg) { return req * nl + Rg * (1 - nl); }

#if defined(__HIPCC__)
// ---- device only: what the two tension kernels share beyond scalar arithmetic ----------------------------------------------------
// A part is here only where both kernels' ISA stayed what their own copies gave (profiles/frame_math.txt).

// Publish `count` tension frames of this workgroup's stream as final: every store of the workgroup (speeds, taps, state) is complete
// and visible device-wide before the count moves.  Called by the whole workgroup.
__device__ __forceinline__ void spx_publish_speed_ready(int* speed_ready, int count) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(&speed_ready[blockIdx.x], count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// NOT SHARED, each kernel keeps its own text, because one text moved the ISA:
//   the K0 / K / first_k range of a job   as a function returning {K0, K}: one s_cselect_b32 moves and one s_or_b64 swaps its operands in
//                                         spx_tension_kernel, one s_cselect_b32 moves in spx_tension_seq_kernel; as two functions, more
//   the state record's start / load       as a function returning the five values: spx_tension_kernel is laid out anew (5 671 diff lines)
//   the lane-0 IIR block                  iir_wave on tsq_iir_block's body with a lower bound of 0 (lane from threadIdx.x or passed in):
//                                         spx_tension_kernel's chain gains a v_mov_b32 and an s_nop per block and its labels move
//   the open-loop duration-sum chain      as a function over the slots [lo, hi) of a block returning {cur_dur, des_dur}: both kernels
//                                         are laid out anew (4 770 and 1 791 diff lines); both take their quotients from spx_fm_frame_time
#endif  // __HIPCC__

#endif  // SPX_FRAME_MATH_H_
