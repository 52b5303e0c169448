// Rate stage of a BATCH call (spx_batch_run_rate: sonicSetRate before the first write, sonic2.h:70): the dependency's adjustRate
// (oracle/orc_sonic.c adjust_rate) over a grid of (output block, stream).  spx_rate.hip has the closed form of the sequential
// two-position walk: output k is emitted at t = floor(k*old/new) as (ratio*in[t] + (new - ratio)*in[t+1]) / new with
// ratio = (t+1)*new - k*old.  A batch job is one whole life cycle -- rate set before the first write, one flush at the end -- so
// the streaming kernel's carried state (old_pos, new_pos, left[], has_left) is zero at the start and every output frame of every
// stream stands alone.  With rem = k*old - t*new (0 <= rem < new) the sample is ((new - rem)*in[t] + rem*in[t+1]) / new, and one
// step of k adds old to k*old: t += old / new, rem += old % new, one carry.
// PARITY UNPINNED like the whole TSM stage (DESIGN.md "Oracle"): bit-exact against the oracle's restatement.
//
// Work split: a thread owns 8 consecutive int16 VALUES of the stream's interleaved output, cut so that full groups start on a
// 16-byte boundary of the caller's buffer whatever out_off is (one 16-byte store per thread; the edges of a stream go value by
// value); a block of 256 threads owns 2048 values.  Per block one 64-bit division fixes (t, rem) of its first frame, a thread
// reaches its own first frame with 32-bit arithmetic (at most 2056 frames further: rem + j*old < 2^26) and then steps.  The inputs
// of neighbouring values are neighbours or the same value, so the 2-byte loads of a wave fall into a few cache lines.
// The arithmetic is the oracle's: int32, |(new - rem)*l + rem*r| <= new * 32768 <= 2^29, a plain truncating division.
#include "spx_internal.h"

#define SPX_RB_THREADS 256
#define SPX_RB_VALUES 8   // per thread: one 16-byte store

typedef short spx_short8 __attribute__((ext_vector_type(8)));

__global__ void __launch_bounds__(SPX_RB_THREADS)
spx_rate_batch_kernel(const SpxRateJob* __restrict__ jobs, int stream0, const SpxStreamState* __restrict__ states,
                      const int64_t* __restrict__ tsm_n, const int16_t* __restrict__ tsm_base, int16_t* __restrict__ fin_base,
                      int64_t* __restrict__ n_out) {
  const int s = stream0 + (int)blockIdx.y;
  const SpxRateJob J = jobs[s];
  const int tid = threadIdx.x;
  if ((int64_t)blockIdx.x >= J.n_blocks) return;   // (the grid is as wide as the call's longest stream)
  int64_t tn = tsm_n[s];
  if (J.bypass || tn == SPX_NOUT_LOST_PRODUCER) {
    // a job with rate 1 ran as spx_batch_run runs it: the walk kernel wrote the caller's buffer and truncated at the flush
    if (blockIdx.x == 0 && tid == 0) n_out[s] = tn;
    return;
  }
  bool over = false;
  if (tn < 0) { tn = -tn; over = true; }                 // the TSM buffer overflowed (its capacity is the plan's bound: never)
  if (tn > J.tsm_cap) { tn = J.tsm_cap; over = true; }
  const int oldR = J.old_rate, newR = J.new_rate, C = J.channels;
  // frames the rate stage emits for M input frames: the k with floor(k*old/new) <= M - 2
  const int64_t M = tn;
  const int64_t nOut = M >= 2 ? ((M - 1) * (int64_t)newR + oldR - 1) / oldR : 0;
  // sonicIntFlushStream: expected = numOutputSamples + (int)((remaining/speed + numPitchSamples)/rate + 0.5f), taken before the padded
  // input is processed; the FINAL output is cut back to it (spx_rate.hip, the flush branch, with nothing carried in)
  const SpxStreamState* st = states + s;
  const float speed = st->curSpeed;
  int64_t mark = st->flush_out_mark;
  if (mark < 0) mark = 0;
  if (mark > tn) mark = tn;
  const int64_t outA = mark >= 2 ? ((mark - 1) * (int64_t)newR + oldR - 1) / oldR : 0;
  const int64_t leftA = mark >= 1 ? 1 : 0;
  const int64_t expected = outA + (int)(((float)st->flush_remaining / speed + (float)leftA) / J.rate + 0.5f);
  int64_t fin_n = nOut < expected ? nOut : expected;
  if (fin_n < 0) fin_n = 0;
  int64_t wr_n = fin_n;
  if (wr_n > J.fin_cap) { wr_n = J.fin_cap; over = true; }
  if (blockIdx.x == 0 && tid == 0) n_out[s] = over ? -fin_n : fin_n;

  // ---- this block's values: [e_blk, ...) of the stream's wr_n * C, groups of 8 aligned to the caller's buffer ----
  const int64_t E = wr_n * C;
  const int a = (int)((reinterpret_cast<uintptr_t>(fin_base) / sizeof(int16_t) + (uint64_t)J.fin_off) & (SPX_RB_VALUES - 1));
  const int64_t blk_lo = (int64_t)blockIdx.x * (SPX_RB_THREADS * SPX_RB_VALUES) - a;
  const int64_t e_blk = blk_lo > 0 ? blk_lo : 0;
  if (e_blk >= E) return;
  const int64_t k_blk = e_blk / C;                       // the block's one 64-bit division pair
  const int c_blk = (int)(e_blk - k_blk * C);
  const int64_t t_blk = (k_blk * oldR) / newR;
  const int rem_blk = (int)(k_blk * oldR - t_blk * newR);
  const int step_t = oldR / newR, step_rem = oldR % newR;

  const int64_t g_lo = blk_lo + (int64_t)tid * SPX_RB_VALUES;
  const int64_t e_lo = g_lo > 0 ? g_lo : 0;
  const int64_t e_hi = (g_lo + SPX_RB_VALUES < E) ? g_lo + SPX_RB_VALUES : E;
  if (e_lo >= e_hi) return;
  const unsigned de = (unsigned)(e_lo - e_blk) + (unsigned)c_blk;   // < 2048 + 8 + C
  const unsigned j = de / (unsigned)C;                               // frames past the block's first
  int c = (int)(de - j * (unsigned)C);
  const unsigned x = (unsigned)rem_blk + j * (unsigned)oldR;         // < 2^14 + 2056 * 2^14
  const unsigned dt = x / (unsigned)newR;
  int rem = (int)(x - dt * (unsigned)newR);
  int64_t t = t_blk + dt;
  const int16_t* __restrict__ in = tsm_base + J.tsm_off;
  int16_t* __restrict__ out = fin_base + J.fin_off;
  const int n = (int)(e_hi - e_lo);
  short v[SPX_RB_VALUES];
#pragma unroll
  for (int i = 0; i < SPX_RB_VALUES; i++) {
    if (i < n) {
      const int l = (int)in[t * C + c];
      const int r = (int)in[(t + 1) * C + c];
      v[i] = (short)(((newR - rem) * l + rem * r) / newR);
      if (++c == C) {
        c = 0;
        t += step_t;
        rem += step_rem;
        if (rem >= newR) { rem -= newR; t++; }
      }
    } else {
      v[i] = 0;
    }
  }
  if (n == SPX_RB_VALUES) {   // a full group: e_lo = g_lo, on a 16-byte boundary by the choice of `a`
    spx_short8 w;
#pragma unroll
    for (int i = 0; i < SPX_RB_VALUES; i++) w[i] = v[i];
    *reinterpret_cast<spx_short8*>(out + e_lo) = w;
  } else {
#pragma unroll
    for (int i = 0; i < SPX_RB_VALUES; i++)
      if (i < n) out[e_lo + i] = v[i];
  }
}

// Blocks that cover `frames` output frames of `channels` values each, wherever the stream starts in the caller's buffer.
int spx_rate_batch_blocks(int64_t frames, int channels) {
  const int64_t per = SPX_RB_THREADS * SPX_RB_VALUES;
  const int64_t b = (frames * channels + (SPX_RB_VALUES - 1) + per - 1) / per;
  return (int)(b < 1 ? 1 : (b > 0x7fffffff ? 0x7fffffff : b));
}

void spx_launch_rate_batch(const SpxRateJob* jobs, int n_streams, int max_blocks, const SpxStreamState* states, const int64_t* tsm_n,
                           const int16_t* tsm_base, int16_t* fin_base, int64_t* n_out, hipStream_t hs) {
  if (max_blocks < 1) max_blocks = 1;
  for (int s0 = 0; s0 < n_streams; s0 += 65535) {   // (the grid's second dimension holds 65 535)
    const int m = n_streams - s0 < 65535 ? n_streams - s0 : 65535;
    hipLaunchKernelGGL(spx_rate_batch_kernel, dim3((unsigned)max_blocks, (unsigned)m), dim3(SPX_RB_THREADS), 0, hs, jobs, s0, states,
                       tsm_n, tsm_base, fin_base, n_out);
  }
}
