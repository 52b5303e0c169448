// Replay of an edit list on tracks at a HIGHER sample rate, int16 or float (include/speedy_hip.h "EDIT LIST, SCALED":
// spx_edit_scale, spx_edit_replay_scaled): speed and pitch are decided on a 16 kHz key, and the 44.1 or 48 kHz master the key was
// made from is cut in the same places.  tests/edit_scaled_ref.py states the definition in Python integers (and np.float32 scalars for
// the float cross-fade); the kernel is held to it bit for bit.
//
// The kernel and the host routine are spx_edit_replay.h's, the ones spx_edit_replay (spx_edits.hip) runs with the identity scale:
// here S(x) = floor(x p / q), p / q the master's rate over the key's, in an instantiation for q == 1 (one multiplication, no
// division) and one for q > 1, each for int16 and for float samples.  This file keeps what is the scaled call's own: the rule for
// p / q, the sample format, and the refusal of positions that do not fit int32 at the master's rate.
#include "spx_edit_replay.h"

#define SPX_ESC_MAX_P 32768
#define SPX_ESC_MAX_RATIO 32

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
  const int4* ops4 = reinterpret_cast<const int4*>(ops);
  return edit_replay_run(
      "spx_edit_replay_scaled", plan, jobs, n, ops_cap, hs, g_last_scaled_gx, g_last_scaled_launches,
      [&](int i) { return SpxEditTrackDesc{tracks[i].in_off, tracks[i].out_off, tracks[i].n_in, tracks[i].out_cap, tracks[i].channels}; },
      [&](int i, int64_t key_frames, int64_t limit) -> int64_t {
        // master positions fit int32 inside the kernel, as the key's do in spx_edit_replay's
        const int64_t cap_frames = esc_scale_host(key_frames, P, Q);
        if (cap_frames > 0x7fffffff || esc_scale_host(limit, P, Q) > 0x7fffffff)
          return fail(-1, "spx_edit_replay_scaled: a stream's positions at the master's rate do not fit 2^31 - 1");
        return cap_frames > tracks[i].out_cap ? tracks[i].out_cap : cap_frames;   // (a stream whose N' is above the track's capacity writes nothing)
      },
      [&](dim3 grid, const SpxEditStream* tab, int s0, hipStream_t st) {
        const dim3 block(SPX_EDIT_THREADS);
        if (sample_format == SPX_SAMPLES_FLOAT) {
          const float* yi = static_cast<const float*>(y_in);
          float* yo = static_cast<float*>(y_out);
          if (Q == 1) hipLaunchKernelGGL((spx_edit_replay_kernel<EditFloat, EditMultiply>), grid, block, 0, st, tab, s0, ops4, n_ops, n_out, P, Q, yi, yo, n_out_y);
          else hipLaunchKernelGGL((spx_edit_replay_kernel<EditFloat, EditRatio>), grid, block, 0, st, tab, s0, ops4, n_ops, n_out, P, Q, yi, yo, n_out_y);
        } else {
          const int16_t* yi = static_cast<const int16_t*>(y_in);
          int16_t* yo = static_cast<int16_t*>(y_out);
          if (Q == 1) hipLaunchKernelGGL((spx_edit_replay_kernel<EditInt16, EditMultiply>), grid, block, 0, st, tab, s0, ops4, n_ops, n_out, P, Q, yi, yo, n_out_y);
          else hipLaunchKernelGGL((spx_edit_replay_kernel<EditInt16, EditRatio>), grid, block, 0, st, tab, s0, ops4, n_ops, n_out, P, Q, yi, yo, n_out_y);
        }
      });
}

}  // extern "C"
