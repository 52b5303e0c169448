// Time map of a batch call (include/speedy_hip.h: spx_plan_map_rows, spx_batch_run_map, spx_map_lookup): which output frame each
// 10 ms of input lands on.
//
// The rows come from the general walk kernel's map instantiation (spx_walk.hip, spx_walk_map_kernel): row k of a nonlinear job is
// the number of frames the time-scale stage has produced when ring buffer k -- input frames [kB, (k+1)B) -- is about to be handed
// to it, the last row is the job's final count; a linear job has the final count alone.  spx_batch_run_map is spx_batch_run with
// SpxCallOpts::map set (run_impl: the whole batch on the general kernel, kernels in sequence on the caller's stream).
// spx_batch_run_rate_map (spx_engine.hip) is spx_batch_run_rate with the same option: the rows conversion kernel below follows the
// rate kernel and turns the speed-stage rows into final frames.
//
// The lookup kernel interpolates between the nodes in exact int64 arithmetic:
//   R = complete ring buffers of a nonlinear job (0 for a linear one)
//   R >= 1:  X = [0, B, .., (R-1)B, n_in],  Y = the stream's R + 1 rows
//   R == 0:  X = [0, n_in],                 Y = [0, the one row]
// One thread per query, grid over (query block, stream); the query counts live in device memory (q_off), so the grid has a fixed
// width and a thread strides over its stream's queries.  Forward: the segment is t / B, one division.  Inverse: a binary search
// over the stream's rows for the last node at or below u -- about ten dependent 8-byte loads for a 10 s stream, all of them in
// the 8 KB the stream's rows occupy, which the queries of a block share through the cache; no LDS staging (nothing measured
// that would justify it).
#include "spx_engine.h"

#define SPX_MAP_THREADS 256

// What the lookup kernel knows of a stream (HOST table in pinned memory, read once per block through the scalar cache).
struct SpxMapStream {
  int64_t n_in;
  int64_t row0;   // index of the stream's first row in `map`
  int64_t R;      // nodes = R + 1 (R >= 1) or 2 (R == 0)
};

__global__ void __launch_bounds__(SPX_MAP_THREADS)
spx_map_lookup_kernel(const SpxMapStream* __restrict__ streams, int stream0, int B, const int64_t* __restrict__ map,
                      const int64_t* __restrict__ q_off, const int64_t* __restrict__ q, int64_t* __restrict__ r, int inverse) {
  const int s = stream0 + (int)blockIdx.y;
  const SpxMapStream S = streams[s];
  const int64_t q0 = q_off[s], q1 = q_off[s + 1];
  const int64_t* __restrict__ rows = map + S.row0;
  const int64_t n_in = S.n_in, R = S.R;
  const int64_t L = R >= 1 ? R + 1 : 2;                  // nodes
  const int64_t y_last = R >= 1 ? rows[R] : rows[0];
  const int64_t stride = (int64_t)gridDim.x * SPX_MAP_THREADS;
  for (int64_t i = q0 + (int64_t)blockIdx.x * SPX_MAP_THREADS + threadIdx.x; i < q1; i += stride) {
    int64_t v = q[i], ans;
    if (!inverse) {
      if (v < 0) v = 0;
      if (v > n_in) v = n_in;
      if (n_in == 0) {
        ans = 0;
      } else {
        int64_t j = v / B;
        if (j > L - 2) j = L - 2;
        const int64_t x0 = j * B, x1 = (j + 1 < L - 1) ? (j + 1) * B : n_in;   // (x1 - x0 >= B, or n_in > 0 where R == 0)
        const int64_t y0 = R >= 1 ? rows[j] : 0, y1 = R >= 1 ? rows[j + 1] : y_last;
        ans = y0 + (v - x0) * (y1 - y0) / (x1 - x0);
      }
    } else {
      if (v < 0) v = 0;
      if (v >= y_last) {
        ans = n_in;
      } else {
        // the largest node index with Y <= v: Y[0] = 0 <= v < Y[L - 1]; a flat run resolves to its last node
        int64_t lo = 0, hi = L - 1;
        while (hi - lo > 1) {
          const int64_t mid = (lo + hi) >> 1;
          const int64_t ym = R >= 1 ? rows[mid] : (mid == 0 ? 0 : y_last);
          if (ym <= v) lo = mid; else hi = mid;
        }
        const int64_t x0 = lo * B, x1 = (lo + 1 < L - 1) ? (lo + 1) * B : n_in;
        const int64_t y0 = R >= 1 ? rows[lo] : 0, y1 = R >= 1 ? rows[lo + 1] : y_last;
        // (rows that do not rise -- those of a job whose count came back negative are unspecified -- never divide by zero)
        ans = y1 > y0 ? x0 + (v - y0) * (x1 - x0) / (y1 - y0) : x0;
      }
    }
    r[i] = ans;
  }
}

// Rows of a call with playback rates (spx_batch_run_rate_map), converted in place behind the rate kernel: the walk kernel has written
// SPEED-STAGE rows (its flush untruncated where a rate stage follows), the caller is owed FINAL frames.  The rate stage is a closed
// form (spx_rate_batch.hip): after m frames of the speed stage F(m) = 0 for m < 2, else ceil((m - 1) * new / old) final frames
// exist.  Rows 0 .. R-1 become F(row); the last row (a linear job's only one) is the final count the rate kernel left in n_out.
// A stream with rate 1 (bypass) keeps the rows spx_batch_run_map gives it.
// Grid over (row block, stream) as the lookup kernel's; the stream's SpxRateJob record and the last time chunk's SpxStreamDev
// record (map_row, the whole n_in) are the ones the call has staged in the workspace.  One 8-byte load and one 8-byte store per
// row.  A negative row (INT64_MIN included: a job whose result is unspecified) takes the m < 2 branch: nothing is indexed by a
// row, and the one divisor is the record's old_rate (>= 1: rate_ratio).
__global__ void __launch_bounds__(SPX_MAP_THREADS)
spx_map_rate_rows_kernel(const SpxRateJob* __restrict__ jobs, const SpxStreamDev* __restrict__ streams, int stream0, int B,
                         const int64_t* __restrict__ n_out, int64_t* __restrict__ map) {
  const int s = stream0 + (int)blockIdx.y;
  const SpxRateJob J = jobs[s];
  if (J.bypass) return;
  const int64_t R = streams[s].nonlinear != 0.0f ? streams[s].n_in / B : 0;
  int64_t* __restrict__ rows = map + streams[s].map_row;
  const int64_t newR = J.new_rate, oldR = J.old_rate;
  const int64_t stride = (int64_t)gridDim.x * SPX_MAP_THREADS;
  for (int64_t k = (int64_t)blockIdx.x * SPX_MAP_THREADS + threadIdx.x; k <= R; k += stride) {
    if (k == R) {
      rows[k] = n_out[s];
    } else {
      const int64_t m = rows[k];
      rows[k] = m >= 2 ? ((m - 1) * newR + oldR - 1) / oldR : 0;
    }
  }
}

// streams: DEVICE, the call's LAST time chunk's records; max_rows: the longest stream's row count (the grid's width: a thread
// strides over what 64 blocks do not cover).
void spx_launch_map_rate_rows(const SpxRateJob* jobs, const SpxStreamDev* streams, int n_streams, int B, int64_t max_rows,
                              const int64_t* n_out, int64_t* map, hipStream_t hs) {
  int64_t gx = (max_rows + SPX_MAP_THREADS - 1) / SPX_MAP_THREADS;
  gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
  for (int s0 = 0; s0 < n_streams; s0 += 65535) {   // (the grid's second dimension holds 65 535)
    const int m = n_streams - s0 < 65535 ? n_streams - s0 : 65535;
    hipLaunchKernelGGL(spx_map_rate_rows_kernel, dim3((unsigned)gx, (unsigned)m), dim3(SPX_MAP_THREADS), 0, hs, jobs, streams, s0, B,
                       n_out, map);
  }
}

static std::atomic<int> g_last_lookup_gx{0}, g_last_lookup_launches{0};   // spx_debug_last_lookup_grid

extern "C" {

int spx_debug_last_lookup_grid(int* launches) {
  if (launches) *launches = g_last_lookup_launches.load(std::memory_order_relaxed);
  return g_last_lookup_gx.load(std::memory_order_relaxed);
}

int64_t spx_plan_map_rows(spx_plan_t plan, int64_t n_in, float nonlinear) {
  if (!plan || n_in < 0) { fail(-1, "spx_plan_map_rows: bad arguments"); return -1; }
  return spx_map_rows(plan->dev, n_in, nonlinear != 0.0f);
}

int spx_batch_run_map(spx_plan_t plan, const spx_stream_job* jobs, int n, const int16_t* in, int16_t* out, int64_t* n_out,
                      int64_t* map, void* ws, size_t ws_bytes, const spx_taps* taps, void* hs) {
  // what spx_batch_run refuses, with its messages, before anything else is looked at
  if (spx_check_jobs(plan, jobs, n, true)) return -1;
  if (!map) return fail(-1, "spx_batch_run_map: map is NULL");
  if (!in || !out || !n_out) return fail(-1, "spx_batch_run_map: bad arguments");
  int64_t rows = 0;
  for (int i = 0; i < n; i++) rows += spx_map_rows(plan->dev, jobs[i].n_in, jobs[i].nonlinear != 0.0f);
  if (rows > 0x7fffffff) return fail(-1, "spx_batch_run_map: more than 2^31 - 1 map rows in one call");
  SpxCallOpts o;
  o.map = map;
  return run_impl({plan, jobs, n, in, out, n_out, ws, ws_bytes, taps, hs}, o);
}

int spx_map_lookup(spx_plan_t plan, const spx_stream_job* jobs, int n, const int64_t* map, const int64_t* q_off, const int64_t* q,
                   int64_t* r, int inverse, void* hs) {
  if (spx_check_jobs(plan, jobs, n, true)) return -1;
  if (!map || !q_off || !q || !r) return fail(-1, "spx_map_lookup: bad arguments");
  const int B = plan->dev.B;
  std::vector<SpxMapStream> tab((size_t)n);
  int64_t row = 0;
  for (int i = 0; i < n; i++) {
    const bool nonlinear = jobs[i].nonlinear != 0.0f;
    tab[i].n_in = jobs[i].n_in;
    tab[i].row0 = row;
    tab[i].R = nonlinear ? jobs[i].n_in / B : 0;
    row += spx_map_rows(plan->dev, jobs[i].n_in, nonlinear);
  }
  hipStream_t st = static_cast<hipStream_t>(hs);
  std::lock_guard<std::mutex> plan_lock(plan->mu);
  // the table: through one of the plan's two pinned staging slots (SpxStage, spx_engine.h)
  SpxStage& G = plan->stage.take();
  if (G.acquire(sizeof(SpxMapStream) * (size_t)n)) return -2;
  memcpy(G.p, tab.data(), sizeof(SpxMapStream) * (size_t)n);
  // query blocks per stream: the counts are the device's to know -- enough blocks to fill the device for a few streams, a
  // handful for many (a thread strides over what is left)
  int gx = 4096 / n;
  gx = gx < 4 ? 4 : (gx > 1024 ? 1024 : gx);
  g_last_lookup_gx.store(gx, std::memory_order_relaxed);
  g_last_lookup_launches.store((n + 65534) / 65535, std::memory_order_relaxed);
  for (int s0 = 0; s0 < n; s0 += 65535) {   // (the grid's second dimension holds 65 535)
    const int m = n - s0 < 65535 ? n - s0 : 65535;
    hipLaunchKernelGGL(spx_map_lookup_kernel, dim3((unsigned)gx, (unsigned)m), dim3(SPX_MAP_THREADS), 0, st,
                       static_cast<const SpxMapStream*>(G.p), s0, B, map, q_off, q, r, inverse);
  }
  if (G.release(st)) return -2;
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
