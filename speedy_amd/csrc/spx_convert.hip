// FLOAT samples for the batch call (spx_batch_run_float: sonicWriteFloatToStream / sonicReadFloatFromStream, sonic2.h:64-68, for
// audio that is already in device memory): two streaming kernels around the int16 call, and the host layer that lays the
// workspace out and enqueues them.  The engine (run_impl) is not involved: the float call converts the jobs' samples into an int16
// staging inside its workspace, runs spx_batch_run_rate (or spx_batch_run) on the stagings with the SAME job table -- in_off /
// out_off count values, and a float value sits where its int16 image sits -- and converts what that call produced.
//
// The reference has TWO input scales (oracle/orc_sonic2.c:147 = soniclib.c:496, oracle/orc_sonic.c:320) and one output scale
// (oracle/orc_sonic.c:341):
//   nonlinear != 0   (short)(x * 32768.0)    the product in double
//   nonlinear == 0   (short)(x * 32767.0f)   the product in float (the file is built with -ffp-contract=off: a plain multiply)
//   output           v / 32767.0f            the IEEE division (-fhip-fp32-correctly-rounded-divide-sqrt)
// The C cast is undefined outside the short range and the GPU's convert instructions saturate, so the conversion is DEFINED here
// as what the streaming API's host loop does on x86: truncate toward zero to a 32-bit integer and keep the low 16 bits (full
// scale 1.0f on a nonlinear job gives -32768); a product that is NaN or of magnitude >= 2^31 gives 0.
//
// Work split, both kernels: a grid over (block, stream) as spx_rate_batch_kernel has; a thread owns 8 consecutive values of the
// stream's interleaved samples, cut so that full groups start on a boundary of the DESTINATION whatever the offsets are (16 bytes
// of int16, 32 bytes of float: the stores are always 16-byte stores); the loads are 16-byte loads where the source group happens
// to lie on a 16-byte boundary and scalar loads where it does not (a float base is only 4-byte aligned and in_off is arbitrary);
// the ragged head and tail of a stream go value by value.  A block of 256 threads owns 2048 values.
#include "spx_engine.h"

#define SPX_CV_THREADS 256
#define SPX_CV_VALUES 8

typedef short spx_cv_short8 __attribute__((ext_vector_type(8)));
typedef float spx_cv_float4 __attribute__((ext_vector_type(4)));

// One stream of a conversion launch (48 bytes, written by the host).
struct SpxConvJob {
  int64_t in_off;     // first input value (float in the caller's `in`, int16 in the input staging)
  int64_t in_vals;    // n_in * channels
  int64_t out_off;    // first output value (int16 in the output staging, float in the caller's `out`)
  int64_t out_cap;    // capacity in frames
  int32_t channels;
  int32_t nonlinear;  // the input scale: != 0 the 32768.0 double product, 0 the 32767.0f float product
  int32_t in_blocks, out_blocks;   // blocks that cover in_vals / out_cap * channels wherever the stream starts; the grid's surplus blocks leave at once
};
static_assert(sizeof(SpxConvJob) == 48 && sizeof(SpxConvJob) % sizeof(unsigned) == 0, "the table kernel copies 32-bit words");

// Truncation toward zero to 32 bits, low 16 bits; NaN and |p| >= 2^31 give 0 (the explicit test keeps the cast in its defined range).
__device__ __forceinline__ short spx_cv_low16(int i) { return (short)(unsigned short)((unsigned)i & 0xffffu); }
__device__ __forceinline__ short spx_cv_short_nl(float x) {
  const double p = (double)x * 32768.0;
  if (!(fabs(p) < 2147483648.0)) return 0;
  return spx_cv_low16((int)p);
}
__device__ __forceinline__ short spx_cv_short_lin(float x) {
  const float p = x * 32767.0f;
  if (!(fabsf(p) < 2147483648.0f)) return 0;
  return spx_cv_low16((int)p);
}

// jobs == nullptr: ONE stream, described by `one` (spx_float_to_short / spx_short_to_float on contiguous values).
__global__ void __launch_bounds__(SPX_CV_THREADS)
spx_float_to_short_kernel(const SpxConvJob* __restrict__ jobs, SpxConvJob one, int stream0, const float* __restrict__ src_base,
                          int16_t* __restrict__ dst_base) {
  const SpxConvJob J = jobs ? jobs[stream0 + (int)blockIdx.y] : one;
  if ((int)blockIdx.x >= J.in_blocks) return;
  const int64_t E = J.in_vals;
  const float* __restrict__ src = src_base + J.in_off;
  int16_t* __restrict__ dst = dst_base + J.in_off;
  const int a = (int)((reinterpret_cast<uintptr_t>(dst) / sizeof(int16_t)) & (SPX_CV_VALUES - 1));
  const int64_t g_lo = (int64_t)blockIdx.x * (SPX_CV_THREADS * SPX_CV_VALUES) - a + (int64_t)threadIdx.x * SPX_CV_VALUES;
  const int64_t e_lo = g_lo > 0 ? g_lo : 0;
  const int64_t e_hi = g_lo + SPX_CV_VALUES < E ? g_lo + SPX_CV_VALUES : E;
  if (e_lo >= e_hi) return;
  const bool nl = J.nonlinear != 0;
  if (e_hi - e_lo == SPX_CV_VALUES) {   // a full group: dst + e_lo lies on a 16-byte boundary by the choice of `a`
    float x[SPX_CV_VALUES];
    if ((reinterpret_cast<uintptr_t>(src + e_lo) & 15) == 0) {
      const spx_cv_float4 p = *reinterpret_cast<const spx_cv_float4*>(src + e_lo);
      const spx_cv_float4 q = *reinterpret_cast<const spx_cv_float4*>(src + e_lo + 4);
#pragma unroll
      for (int i = 0; i < 4; i++) { x[i] = p[i]; x[4 + i] = q[i]; }
    } else {
#pragma unroll
      for (int i = 0; i < SPX_CV_VALUES; i++) x[i] = src[e_lo + i];
    }
    spx_cv_short8 w;
    if (nl) {
#pragma unroll
      for (int i = 0; i < SPX_CV_VALUES; i++) w[i] = spx_cv_short_nl(x[i]);
    } else {
#pragma unroll
      for (int i = 0; i < SPX_CV_VALUES; i++) w[i] = spx_cv_short_lin(x[i]);
    }
    *reinterpret_cast<spx_cv_short8*>(dst + e_lo) = w;
  } else {
    for (int64_t e = e_lo; e < e_hi; e++) dst[e] = nl ? spx_cv_short_nl(src[e]) : spx_cv_short_lin(src[e]);
  }
}

// n_out == nullptr: the count is `one.out_cap` frames (spx_short_to_float).  Otherwise the stream's count is read HERE, on the
// device -- the grid was sized on the host from the capacities, no synchronisation is added: min(|n_out[s]|, out_cap) frames are
// converted (a negative count reports an output that was cut at out_cap), a stream whose producer never delivered writes nothing.
__global__ void __launch_bounds__(SPX_CV_THREADS)
spx_short_to_float_kernel(const SpxConvJob* __restrict__ jobs, SpxConvJob one, int stream0, const int64_t* __restrict__ n_out,
                          const int16_t* __restrict__ src_base, float* __restrict__ dst_base) {
  const int s = stream0 + (int)blockIdx.y;
  const SpxConvJob J = jobs ? jobs[s] : one;
  if ((int)blockIdx.x >= J.out_blocks) return;
  int64_t frames = J.out_cap;
  if (n_out) {
    int64_t k = n_out[s];
    if (k == SPX_NOUT_LOST_PRODUCER) return;
    if (k < 0) k = -k;
    if (k < frames) frames = k;
  }
  const int64_t E = frames * J.channels;
  const int16_t* __restrict__ src = src_base + J.out_off;
  float* __restrict__ dst = dst_base + J.out_off;
  const int a = (int)((reinterpret_cast<uintptr_t>(dst) / sizeof(float)) & (SPX_CV_VALUES - 1));
  const int64_t g_lo = (int64_t)blockIdx.x * (SPX_CV_THREADS * SPX_CV_VALUES) - a + (int64_t)threadIdx.x * SPX_CV_VALUES;
  const int64_t e_lo = g_lo > 0 ? g_lo : 0;
  const int64_t e_hi = g_lo + SPX_CV_VALUES < E ? g_lo + SPX_CV_VALUES : E;
  if (e_lo >= e_hi) return;
  if (e_hi - e_lo == SPX_CV_VALUES) {   // a full group: dst + e_lo lies on a 32-byte boundary by the choice of `a`
    spx_cv_short8 v;
    if ((reinterpret_cast<uintptr_t>(src + e_lo) & 15) == 0) {
      v = *reinterpret_cast<const spx_cv_short8*>(src + e_lo);
    } else {
#pragma unroll
      for (int i = 0; i < SPX_CV_VALUES; i++) v[i] = src[e_lo + i];
    }
    spx_cv_float4 p, q;
#pragma unroll
    for (int i = 0; i < 4; i++) { p[i] = (float)v[i] / 32767.0f; q[i] = (float)v[4 + i] / 32767.0f; }
    *reinterpret_cast<spx_cv_float4*>(dst + e_lo) = p;
    *reinterpret_cast<spx_cv_float4*>(dst + e_lo + 4) = q;
  } else {
    for (int64_t e = e_lo; e < e_hi; e++) dst[e] = (float)src[e] / 32767.0f;
  }
}

// The job table's way into the workspace: 32-bit words from the pinned slot (one small kernel, as the engine stages its tables).
__global__ void __launch_bounds__(256) spx_conv_table_kernel(const unsigned* __restrict__ src, unsigned* __restrict__ dst, unsigned n) {
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

// Blocks that cover `vals` values wherever the stream starts in the destination; -1: more than a grid's first dimension holds.
static int64_t conv_blocks(int64_t vals) {
  const int64_t per = SPX_CV_THREADS * SPX_CV_VALUES;
  return (vals + (SPX_CV_VALUES - 1) + per - 1) / per;
}

// The conversion table of a job table, written into `tab` (pinned host memory), and the two grids' first dimensions.  -1: a stream
// has more values than one launch covers.
static int conv_fill(SpxConvJob* tab, const spx_stream_job* jobs, int n, int* max_in, int* max_out) {
  int64_t mi = 1, mo = 1;
  for (int i = 0; i < n; i++) {
    const spx_stream_job& j = jobs[i];
    SpxConvJob& J = tab[i];
    J.in_off = j.in_off; J.in_vals = j.n_in * j.channels;
    J.out_off = j.out_off; J.out_cap = j.out_cap;
    J.channels = j.channels; J.nonlinear = j.nonlinear != 0.0f ? 1 : 0;
    const int64_t bi = conv_blocks(J.in_vals), bo = conv_blocks(j.out_cap * j.channels);
    if (bi > 0x7fffffff || bo > 0x7fffffff) return -1;
    J.in_blocks = J.in_vals > 0 ? (int)bi : 0;
    J.out_blocks = j.out_cap > 0 ? (int)bo : 0;
    mi = std::max<int64_t>(mi, J.in_blocks);
    mo = std::max<int64_t>(mo, J.out_blocks);
  }
  *max_in = (int)mi; *max_out = (int)mo;
  return 0;
}
static void conv_upload(const void* pinned, SpxConvJob* d_tab, int n, hipStream_t st) {
  const unsigned words = (unsigned)(sizeof(SpxConvJob) * (size_t)n / sizeof(unsigned));
  hipLaunchKernelGGL(spx_conv_table_kernel, dim3((words + 255) / 256 < 64 ? (words + 255) / 256 : 64), dim3(256), 0, st,
                     static_cast<const unsigned*>(pinned), reinterpret_cast<unsigned*>(d_tab), words);
}
static void conv_launch_in(const SpxConvJob* d_tab, int n, int max_in, const float* in, int16_t* st_in, hipStream_t st) {
  SpxConvJob none;
  memset(&none, 0, sizeof(none));
  for (int s0 = 0; s0 < n; s0 += 65535) {   // (the grid's second dimension holds 65 535)
    const int m = n - s0 < 65535 ? n - s0 : 65535;
    hipLaunchKernelGGL(spx_float_to_short_kernel, dim3((unsigned)max_in, (unsigned)m), dim3(SPX_CV_THREADS), 0, st, d_tab, none, s0, in, st_in);
  }
}
static void conv_launch_out(const SpxConvJob* d_tab, int n, int max_out, const int64_t* n_out, const int16_t* st_out, float* out, hipStream_t st) {
  SpxConvJob none;
  memset(&none, 0, sizeof(none));
  for (int s0 = 0; s0 < n; s0 += 65535) {
    const int m = n - s0 < 65535 ? n - s0 : 65535;
    hipLaunchKernelGGL(spx_short_to_float_kernel, dim3((unsigned)max_out, (unsigned)m), dim3(SPX_CV_THREADS), 0, st, d_tab, none, s0, n_out,
                       st_out, out);
  }
}

// The same four steps for the pipeline object on float samples (spx_pipeline.hip, SPX_PIPELINE_FLOAT): the table lives in a buffer
// set's own pinned and device memory, the stagings are the buffer set's d_in / d_out.  The kernels and their arithmetic are these.
size_t spx_conv_table_bytes(int n) { return sizeof(SpxConvJob) * (size_t)n; }
int spx_conv_table_fill(void* pinned, const spx_stream_job* jobs, int n, int* max_in, int* max_out) {
  return conv_fill(static_cast<SpxConvJob*>(pinned), jobs, n, max_in, max_out);
}
void spx_conv_table_upload(const void* pinned, void* d_tab, int n, hipStream_t st) { conv_upload(pinned, static_cast<SpxConvJob*>(d_tab), n, st); }
void spx_conv_launch_in(const void* d_tab, int n, int max_in, const float* in, int16_t* st_in, hipStream_t st) {
  conv_launch_in(static_cast<const SpxConvJob*>(d_tab), n, max_in, in, st_in, st);
}
void spx_conv_launch_out(const void* d_tab, int n, int max_out, const int64_t* n_out, const int16_t* st_out, float* out, hipStream_t st) {
  conv_launch_out(static_cast<const SpxConvJob*>(d_tab), n, max_out, n_out, st_out, out, st);
}

// Workspace of a float call: the int16 call's own workspace at the front (spx_batch_read_steps finds its records there) |
// SpxConvJob[n] | the int16 input staging, max(in_off + n_in * channels) + 64 values (the padding the kernels' window loads may
// touch) | the int16 output staging, max(out_off + out_cap * channels) values; every part on a 256-byte boundary.
struct FloatLayout { size_t base, off_table, off_in, off_out, total; };
static int float_layout(spx_plan_t plan, const spx_stream_job* jobs, const float* rates, int n, FloatLayout& FL) {
  // everything the int16 call refuses about a job or a rate, once: with rates, spx_batch_workspace_bytes_rate asks (0 with the message)
  if (!rates && spx_check_jobs(plan, jobs, n)) return -1;
  FL.base = spx_batch_workspace_bytes_rate(plan, jobs, rates, n);
  if (FL.base == 0) return -1;
  int64_t in_vals = 0, out_vals = 0;
  for (int i = 0; i < n; i++) {
    const spx_stream_job& j = jobs[i];
    // the float path's own limits: the stagings' extents below must not overflow
    if (j.in_off >= (1ll << 46) || j.out_off >= (1ll << 46) || j.out_cap >= (1ll << 40) || j.channels > (1 << 15))
      return fail(-1, "spx_batch: bad job (an offset of 2^46, a capacity of 2^40 or more than 2^15 channels: too large for the float call's stagings)");
    in_vals = std::max(in_vals, j.in_off + j.n_in * j.channels);
    out_vals = std::max(out_vals, j.out_off + j.out_cap * j.channels);
  }
  SpxCarve ws(FL.base);
  FL.off_table = ws.take(sizeof(SpxConvJob) * (size_t)n);
  FL.off_in = ws.take(sizeof(int16_t) * (size_t)(in_vals + 64));
  FL.off_out = ws.take(sizeof(int16_t) * (size_t)out_vals);
  FL.total = ws.o;
  return 0;
}

static int conv_one(int64_t n, int nonlinear, SpxConvJob& J) {
  memset(&J, 0, sizeof(J));
  const int64_t b = conv_blocks(n);
  if (b > 0x7fffffff) return fail(-1, "spx conversion: too many values for one call");
  J.in_vals = n; J.out_cap = n; J.channels = 1; J.nonlinear = nonlinear;
  J.in_blocks = J.out_blocks = (int)b;
  return 0;
}

extern "C" {
int spx_float_to_short(const float* in, int16_t* out, size_t n, int nonlinear_scale, void* hs) {
  if (n == 0) return 0;
  if (!in || !out || (reinterpret_cast<uintptr_t>(in) & 3) || (reinterpret_cast<uintptr_t>(out) & 1) || n > ((size_t)1 << 46))
    return fail(-1, "spx_float_to_short: bad arguments (null, misaligned, or too many values)");
  SpxConvJob J;
  if (conv_one((int64_t)n, nonlinear_scale ? 1 : 0, J)) return -1;
  hipLaunchKernelGGL(spx_float_to_short_kernel, dim3((unsigned)J.in_blocks), dim3(SPX_CV_THREADS), 0, static_cast<hipStream_t>(hs),
                     static_cast<const SpxConvJob*>(nullptr), J, 0, in, out);
  HIPCHK(hipGetLastError());
  return 0;
}
int spx_short_to_float(const int16_t* in, float* out, size_t n, void* hs) {
  if (n == 0) return 0;
  if (!in || !out || (reinterpret_cast<uintptr_t>(in) & 1) || (reinterpret_cast<uintptr_t>(out) & 3) || n > ((size_t)1 << 46))
    return fail(-1, "spx_short_to_float: bad arguments (null, misaligned, or too many values)");
  SpxConvJob J;
  if (conv_one((int64_t)n, 0, J)) return -1;
  hipLaunchKernelGGL(spx_short_to_float_kernel, dim3((unsigned)J.out_blocks), dim3(SPX_CV_THREADS), 0, static_cast<hipStream_t>(hs),
                     static_cast<const SpxConvJob*>(nullptr), J, 0, static_cast<const int64_t*>(nullptr), in, out);
  HIPCHK(hipGetLastError());
  return 0;
}

size_t spx_batch_workspace_bytes_float(spx_plan_t plan, const spx_stream_job* jobs, const float* rates, int n_streams) {
  FloatLayout FL;
  if (float_layout(plan, jobs, rates, n_streams, FL)) return 0;
  return FL.total;
}

}  // extern "C"

// spx_batch_run_float, and (with_map) spx_batch_run_float_map: the same layers, the map handed through to the int16 call.
static int run_float(spx_plan_t plan, const spx_stream_job* jobs, const float* rates, int n, const float* in, float* out,
                     int64_t* n_out, bool with_map, int64_t* map, void* ws, size_t ws_bytes, const spx_taps* taps, void* hs) {
  // ---- everything that is refused is refused before the first launch ----
  if (!plan || !jobs || n <= 0 || !in || !out || !n_out || !ws) return fail(-1, "spx_batch_run_float: bad arguments (a null pointer or no streams)");
  if ((reinterpret_cast<uintptr_t>(in) & 3) || (reinterpret_cast<uintptr_t>(out) & 3))
    return fail(-1, "spx_batch_run_float: in and out must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(-1, "spx_batch_run_float: the workspace must be 256-byte aligned");
  FloatLayout FL;
  if (float_layout(plan, jobs, rates, n, FL)) return -1;   // a job or a rate that is refused
  if (ws_bytes < FL.total) return fail(-1, "spx_batch_run_float: workspace too small (spx_batch_workspace_bytes_float)");
  if (with_map) {   // what the int16 call with a map refuses on top of that -- asked here, ahead of the input conversion's launch
    if (!map) return fail(-1, "spx_batch_run_float_map: map is NULL");
    int64_t rows = 0;
    for (int i = 0; i < n; i++) rows += spx_map_rows(plan->dev, jobs[i].n_in, jobs[i].nonlinear != 0.0f);
    if (rows > 0x7fffffff) return fail(-1, "spx_batch_run_float_map: more than 2^31 - 1 map rows in one call");
  }
  hipStream_t st = static_cast<hipStream_t>(hs);
  unsigned char* w = static_cast<unsigned char*>(ws);
  SpxConvJob* d_tab = reinterpret_cast<SpxConvJob*>(w + FL.off_table);
  int16_t* st_in = reinterpret_cast<int16_t*>(w + FL.off_in);
  int16_t* st_out = reinterpret_cast<int16_t*>(w + FL.off_out);

  // ---- the table: through a per-thread pinned slot (two, taking turns), reused once the kernel that last read it has retired ----
  static thread_local SpxStagePair stage;
  SpxStage& G = stage.take();
  if (G.acquire(sizeof(SpxConvJob) * (size_t)n)) return -2;
  int max_in = 1, max_out = 1;
  if (conv_fill(static_cast<SpxConvJob*>(G.p), jobs, n, &max_in, &max_out)) return fail(-1, "spx_batch_run_float: out_cap too large for one launch");
  SpxRange range_("spx_batch_run_float");
  conv_upload(G.p, d_tab, n, st);
  if (G.release(st)) return -2;

  // ---- input conversion | the int16 call on the stagings | output conversion, all on hip_stream ----
  conv_launch_in(d_tab, n, max_in, in, st_in, st);
  const int rc = with_map ? spx_batch_run_rate_map(plan, jobs, rates, n, st_in, st_out, n_out, map, ws, FL.base, taps, hs)
                          : spx_batch_run_rate(plan, jobs, rates, n, st_in, st_out, n_out, ws, FL.base, taps, hs);
  if (rc) return rc;
  conv_launch_out(d_tab, n, max_out, n_out, st_out, out, st);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" {
int spx_batch_run_float(spx_plan_t plan, const spx_stream_job* jobs, const float* rates, int n, const float* in, float* out,
                        int64_t* n_out, void* ws, size_t ws_bytes, const spx_taps* taps, void* hs) {
  return run_float(plan, jobs, rates, n, in, out, n_out, false, nullptr, ws, ws_bytes, taps, hs);
}
int spx_batch_run_float_map(spx_plan_t plan, const spx_stream_job* jobs, const float* rates, int n, const float* in, float* out,
                            int64_t* n_out, int64_t* map, void* ws, size_t ws_bytes, const spx_taps* taps, void* hs) {
  return run_float(plan, jobs, rates, n, in, out, n_out, true, map, ws, ws_bytes, taps, hs);
}
}  // extern "C"
