// Batch dynamic time warping (include/speedy_hip.h "BATCH DTW": spx_dtw_workspace_bytes, spx_batch_dtw): for every pair of float
// sequences the accumulated cost, the warp path, its least-squares slope and the mean and deviation of its local slopes -- the
// reference's perceptual check (dynamic_time_warping.cc:60-132, sonic_test.cc:86-133, 200-209) as two kernels, one workgroup per pair.
// tests/dtw_ref.py is the definition both are held to, bit for bit.
//
// spx_dtw_forward_kernel walks the pair's cost matrix in tiles of 64 x 64 cells, tile rows outermost.  Per tile
//   phase 1  all four waves: the tile's 4 096 local costs.  The 64 rows of a and of b are staged through LDS 32 values of k at a
//            time, TRANSPOSED ([k][row], stride 68 words): a thread owns 4 x 4 cells and reads its four a values and its four b
//            values of a k with ONE 16-byte LDS read each (a: four addresses per wave, broadcast; b: sixteen consecutive slots, one
//            bank row), then 16 x (subtract, multiply, add) -- k ascending, one float accumulator per cell, no fused multiply-add
//            (the build's -ffp-contract=off), as EuclideanDistance adds them.  sqrtf (correctly rounded by the build's flag) of
//            the sums goes to an LDS tile of stride 66 words.
//   phase 2  wave 0: the recurrence over the tile's 127 anti-diagonals, lane = row.  At step t lane r owns column t - r: `left` is
//            the lane's own previous value and stays in its register -- across tiles of a tile row too, so no right column is ever
//            stored --, `up` is the value lane r - 1 computed one step earlier (one DPP wave shift), `diag` is the `up` of the
//            lane's previous step.  Lane 0 takes `up` from the tile's top row (lane t's register, v_readlane).  The cost tile is
//            read at word 65 r + t, conflict-free, eight steps' values at a time.  The matrix's borders are +infinity neighbours,
//            and a 0 diagonal neighbour for cell (0, 0): the same minimum and the same strict comparisons then give the
//            reference's border rows (d + left, +1; d + up, -1; d, 0).
//   carried  the bottom row of a tile row in a per-pair array of n_b floats in the workspace (one coalesced load and store per
//            tile: it lives in L2), the corner C(i0 - 1, j0 - 1) in a register.
//   stored   the directions, TWO BITS per cell (0 diagonal, 1 up = the reference's -1, 2 left = +1): a lane shifts the 64 of its
//            row through four registers and writes them with one 16-byte store per tile.  The cost matrix itself never leaves LDS.
// The other three waves wait in phase 2 -- about 40 % of the kernel at dim = 120 with one pair per CU (profiles/dtw.txt); with more
// pairs than CUs the workgroups of other pairs fill the CU meanwhile (34 KB of LDS each).  The overlap inside one workgroup (phase 1
// of the next tile beside phase 2 of this one, a second cost tile) is not built: the follow-up the profile argues for.
//
// spx_dtw_tail_kernel (behind it on the same stream)
//   * walks the directions backwards: the 1 KB of packed directions of the tile the walk is in are staged in LDS, every thread
//     walks the same steps on them (uniform control, LDS broadcasts) and thread 0 writes the entries, reversed, to the workspace;
//   * copies them forwards into `path`, 1 024 entries at a time through LDS, where thread 0 adds the four float sums of
//     LinearSlope in path order;
//   * gives every thread one window of LinearSlopeEverywhere at a time (2 h entries, read from `path`), 1 024 windows per round,
//     and has thread 0 add them in order in a double (VectorMean); a third round the same way for the squared differences
//     (VectorStandardDeviation).  Serial sums read LDS, never memory.
#include "spx_engine.h"

#define SPX_DTW_THREADS 256
#define SPX_DTW_TILE 64
#define SPX_DTW_KC 32          // values of k staged at a time
#define SPX_DTW_KS 68          // words between two k of the staged rows (64 rows + 4: 16-byte reads stay aligned)
#define SPX_DTW_DS 66          // words between two rows of the cost tile (phase 2 reads word 65 r + t)
#define SPX_DTW_CHUNK 1024     // path entries / windows per round of the tail
#define SPX_DTW_MAX_DIM 65536
#define SPX_DTW_MAX_CELLS ((int64_t)1 << 30)
// -DSPX_DTW_PHASES=1 / =2: a diagnostic build whose forward kernel runs phase 1 / phase 2 alone (wrong results; for the time split of
// profiles/dtw.txt only, never shipped)
#ifndef SPX_DTW_PHASES
#define SPX_DTW_PHASES 3
#endif

// What the kernels know of a pair (HOST table in pinned memory).  dirs .. slopes: bytes from the workspace's (aligned) base.
struct SpxDtwPair {
  int64_t a_off, b_off, path_off;
  int64_t dirs;      // uint4 [n_a][tiles_b]: row i's directions of tile column tj, two bits per cell
  int64_t brow;      // float [n_b]: the bottom row of the tile row above
  int64_t rev;       // int2 [n_a + n_b - 1]: the path as the back-trace finds it
  int64_t slopes;    // float [n_a + n_b - 1]: the local slopes
  int32_t n_a, n_b;
};

// lane l's value in lane l + 1 (lane 0 keeps its own)
__device__ __forceinline__ float dtw_from_lane_below(float v) {
  const int x = __builtin_bit_cast(int, v);
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(x, x, 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}
__device__ __forceinline__ void dtw_wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ void __launch_bounds__(SPX_DTW_THREADS)
spx_dtw_forward_kernel(const SpxDtwPair* __restrict__ pairs, int dim, int ld_a, int ld_b, const float* __restrict__ a,
                       const float* __restrict__ b, spx_dtw_result* __restrict__ results, unsigned char* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float s_a[SPX_DTW_KC * SPX_DTW_KS];
  __shared__ __attribute__((aligned(16))) float s_b[SPX_DTW_KC * SPX_DTW_KS];
  __shared__ __attribute__((aligned(16))) float s_d[SPX_DTW_TILE * SPX_DTW_DS];
  __shared__ float s_bot[2 * SPX_DTW_TILE];   // the tile's bottom row, and a word per lane for the other lanes' stores
  const SpxDtwPair P = pairs[blockIdx.x];
  const int n_a = P.n_a, n_b = P.n_b;
  const float* __restrict__ A = a + P.a_off;
  const float* __restrict__ B = b + P.b_off;
  uint4* __restrict__ dirs = reinterpret_cast<uint4*>(ws + P.dirs);
  float* brow = reinterpret_cast<float*>(ws + P.brow);
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tr = tid >> 4, tc = tid & 15;          // phase 1: rows 4 tr .., columns 4 tc ..
  const int kk = tid & 31, r0 = tid >> 5;          // staging: value k0 + kk of rows r0 + 8 q
  const int TA = (n_a + SPX_DTW_TILE - 1) / SPX_DTW_TILE, TB = (n_b + SPX_DTW_TILE - 1) / SPX_DTW_TILE;
  const float inf = __builtin_inff();
  float left = inf, corner_next = inf;             // wave 0, across the tiles of a tile row

  for (int ti = 0; ti < TA; ti++) {
    const int i0 = ti * SPX_DTW_TILE;
    const int rows = n_a - i0 < SPX_DTW_TILE ? n_a - i0 : SPX_DTW_TILE;
    for (int tj = 0; tj < TB; tj++) {
      const int j0 = tj * SPX_DTW_TILE;
      const int cols = n_b - j0 < SPX_DTW_TILE ? n_b - j0 : SPX_DTW_TILE;
      // ---- phase 1: the tile's local costs (rows and columns outside the matrix read as zeros and are never used)
      float acc[4][4];
#pragma unroll
      for (int x = 0; x < 4; x++)
#pragma unroll
        for (int y = 0; y < 4; y++) acc[x][y] = 0.0f;
      for (int k0 = 0; k0 < ((SPX_DTW_PHASES & 1) ? dim : 1); k0 += SPX_DTW_KC) {
        const int kn = dim - k0 < SPX_DTW_KC ? dim - k0 : SPX_DTW_KC;
        __syncthreads();   // the staged rows are free -- and, the first time round, wave 0 is through with the last tile
#pragma unroll
        for (int q = 0; q < 8; q++) {
          const int r = r0 + 8 * q;
          float va = 0.0f, vb = 0.0f;
          if (kk < kn) {
            if (r < rows) va = A[(int64_t)(i0 + r) * ld_a + k0 + kk];
            if (r < cols) vb = B[(int64_t)(j0 + r) * ld_b + k0 + kk];
          }
          s_a[kk * SPX_DTW_KS + r] = va;
          s_b[kk * SPX_DTW_KS + r] = vb;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < kn; k++) {
          const float4 av = *reinterpret_cast<const float4*>(&s_a[k * SPX_DTW_KS + 4 * tr]);
          const float4 bv = *reinterpret_cast<const float4*>(&s_b[k * SPX_DTW_KS + 4 * tc]);
          const float ar[4] = {av.x, av.y, av.z, av.w}, bc[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
          for (int x = 0; x < 4; x++)
#pragma unroll
            for (int y = 0; y < 4; y++) {
              const float t = ar[x] - bc[y];
              acc[x][y] = acc[x][y] + t * t;
            }
        }
      }
#pragma unroll
      for (int x = 0; x < 4; x++) {
        float* row = &s_d[(4 * tr + x) * SPX_DTW_DS + 4 * tc];
        *reinterpret_cast<float2*>(row) = make_float2(sqrtf(acc[x][0]), sqrtf(acc[x][1]));
        *reinterpret_cast<float2*>(row + 2) = make_float2(sqrtf(acc[x][2]), sqrtf(acc[x][3]));
      }
      float topv = inf;
      if (wave == 0 && ti > 0 && lane < cols) topv = brow[j0 + lane];   // the top row: lane = column
      __syncthreads();
      if (wave != 0) continue;

      // ---- phase 2 (wave 0): the recurrence, lane = row i0 + lane
      const float corner = tj == 0 ? (ti == 0 ? 0.0f : inf) : corner_next;
      corner_next = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, topv), 63));   // C(i0 - 1, j0 + 63)
      if (tj == 0) left = inf;
      float diag = dtw_from_lane_below(left);
      if (lane == 0) diag = corner;
      float val = 0.0f;
      // the directions of the lane's row: a 128-bit shift register, two bits in at the top per column (four v_alignbit)
      unsigned w0 = 0u, w1 = 0u, w2 = 0u, w3 = 0u;
      const float* drow = &s_d[lane * (SPX_DTW_DS - 1)];
      const int steps = (SPX_DTW_PHASES & 2) ? rows + cols - 1 : 0;
      // lane 63's values are the tile's bottom row; the other lanes' stores go to a word of their own behind it (no branch)
      const int bot_at = lane == SPX_DTW_TILE - 1 ? -(SPX_DTW_TILE - 1) : SPX_DTW_TILE + lane;
      const int bot_step = lane == SPX_DTW_TILE - 1 ? 1 : 0;
      // eight steps at a time: their eight local costs are read from LDS together, one wait for all (a read per step, waited for
      // on the spot, was most of a step: profiles/dtw.txt).  Word 65 lane + t0 + 7 <= 65 * 63 + 127 lies inside the tile.  A lane
      // is active while its column t - lane is one of the tile's `cols`: steps past rows + cols - 2 touch no row of the matrix.
      for (int t0 = 0; t0 < steps; t0 += 8) {
        float dv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) dv[u] = drow[t0 + u];
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const int t = t0 + u;
          // lane 0's `up` is the top row's column t: lane t's register (t is uniform; lane 0 is past the tile at t >= 64)
          const int tv = __builtin_amdgcn_readlane(__builtin_bit_cast(int, topv), t & 63);
          float up = dtw_from_lane_below(val);
          if (lane == 0) up = __builtin_bit_cast(float, tv);
          const int c = t - lane;
          float m = left < up ? left : up;            // std::min(std::min(up, left), diag)
          m = diag < m ? diag : m;
          const float v = dv[u] + m;
          const unsigned code = (up < diag && up < left) ? 1u : ((left < up && left < diag) ? 2u : 0u);
          if ((unsigned)c < (unsigned)cols) {
            diag = up;
            left = v;
            val = v;
            w0 = __builtin_amdgcn_alignbit(w1, w0, 2);
            w1 = __builtin_amdgcn_alignbit(w2, w1, 2);
            w2 = __builtin_amdgcn_alignbit(w3, w2, 2);
            w3 = __builtin_amdgcn_alignbit(code, w3, 2);
            s_bot[bot_at + t * bot_step] = v;
          }
        }
      }
      // `left` is the row's last column now: the pair's cost, in the last row of the last tile
      if (i0 + lane == n_a - 1 && tj == TB - 1) results[blockIdx.x].cost = left;
      // a row of `cols` columns has shifted 2 cols bits in: column c's two bits belong at bit 2 c
      unsigned long long lo = ((unsigned long long)w1 << 32) | w0, hi = ((unsigned long long)w3 << 32) | w2;
      const int sh = 2 * (SPX_DTW_TILE - cols);
      if (sh >= 64) { lo = hi >> (sh - 64); hi = 0ull; } else if (sh > 0) { lo = (lo >> sh) | (hi << (64 - sh)); hi >>= sh; }
      if (lane < rows) dirs[(int64_t)(i0 + lane) * TB + tj] = make_uint4((unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32));
      if (ti + 1 < TA) {   // (the tile has 64 rows then: lane 63 has written every column)
        dtw_wave_lds_sync();
        if (lane < cols) brow[j0 + lane] = s_bot[lane];
      }
    }
  }
}

// the direction of cell (i, j) from the staged tile: row i & 63, column j & 63
__device__ __forceinline__ unsigned dtw_dir(const unsigned* s_dir, int i, int j) {
  const int c = j & 63;
  return (s_dir[(i & 63) * 4 + (c >> 4)] >> (2 * (c & 15))) & 3u;
}

// LinearSlope (sonic_test.cc:86-99) over `n` entries of the path from `xy`
__device__ __forceinline__ float dtw_slope(const int2* xy, int n) {
  float sx = 0.0f, sy = 0.0f, sxy = 0.0f, sx2 = 0.0f;
  for (int k = 0; k < n; k++) {
    const int2 e = xy[k];
    sx = sx + (float)e.x;
    sy = sy + (float)e.y;
    sxy = sxy + (float)((long long)e.x * e.y);
    sx2 = sx2 + (float)((long long)e.x * e.x);
  }
  return ((float)n * sxy - sx * sy) / ((float)n * sx2 - sx * sx);
}

__global__ void __launch_bounds__(SPX_DTW_THREADS)
spx_dtw_tail_kernel(const SpxDtwPair* __restrict__ pairs, int half_width, spx_dtw_result* __restrict__ results,
                    int32_t* __restrict__ path_base, unsigned char* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) unsigned s_dir[SPX_DTW_TILE * 4];
  __shared__ int2 s_xy[SPX_DTW_CHUNK];
  __shared__ float s_f[SPX_DTW_CHUNK];
  __shared__ float s_bcast;
  const SpxDtwPair P = pairs[blockIdx.x];
  const int n_a = P.n_a, n_b = P.n_b;
  const int tid = (int)threadIdx.x;
  const int TB = (n_b + SPX_DTW_TILE - 1) / SPX_DTW_TILE;
  const uint4* __restrict__ dirs = reinterpret_cast<const uint4*>(ws + P.dirs);
  int2* rev = reinterpret_cast<int2*>(ws + P.rev);
  float* slopes = reinterpret_cast<float*>(ws + P.slopes);
  int2* path = reinterpret_cast<int2*>(path_base) + P.path_off;

  // ---- the back-trace (dynamic_time_warping.cc:102-132): every thread the same steps, thread 0 writes
  int i = n_a - 1, j = n_b - 1, n_path = 0;
  while (i >= 0 && j >= 0) {
    const int ti = i >> 6, tj = j >> 6;
    __syncthreads();
    if (tid < SPX_DTW_TILE && ti * SPX_DTW_TILE + tid < n_a)
      reinterpret_cast<uint4*>(s_dir)[tid] = dirs[(int64_t)(ti * SPX_DTW_TILE + tid) * TB + tj];
    __syncthreads();
    while (i >= 0 && j >= 0 && (i >> 6) == ti && (j >> 6) == tj) {
      if (tid == 0) rev[n_path] = make_int2(i, j);
      n_path++;
      const unsigned code = dtw_dir(s_dir, i, j);
      if (code != 2u) i--;
      if (code != 1u) j--;
    }
  }

  // ---- the path forwards, and LinearSlope over all of it (thread 0, in path order, from LDS)
  float sx = 0.0f, sy = 0.0f, sxy = 0.0f, sx2 = 0.0f;
  for (int p0 = 0; p0 < n_path; p0 += SPX_DTW_CHUNK) {
    const int m = n_path - p0 < SPX_DTW_CHUNK ? n_path - p0 : SPX_DTW_CHUNK;
    __syncthreads();   // (the first: thread 0's entries are visible to the workgroup)
    for (int k = tid; k < m; k += SPX_DTW_THREADS) {
      const int2 e = rev[n_path - 1 - (p0 + k)];
      path[p0 + k] = e;
      s_xy[k] = e;
    }
    __syncthreads();
    if (tid == 0) {
      for (int k = 0; k < m; k++) {
        const int2 e = s_xy[k];
        sx = sx + (float)e.x;
        sy = sy + (float)e.y;
        sxy = sxy + (float)((long long)e.x * e.y);
        sx2 = sx2 + (float)((long long)e.x * e.x);
      }
    }
  }
  __syncthreads();   // `path` is visible to the workgroup

  // ---- LinearSlopeEverywhere, VectorMean, VectorStandardDeviation (sonic_test.cc:101-133)
  const int h = half_width;
  const int n_local = n_path - 2 * (int64_t)h > 0 ? n_path - 2 * h : 0;
  double sum = 0.0;
  for (int w0 = 0; w0 < n_local; w0 += SPX_DTW_CHUNK) {
    const int m = n_local - w0 < SPX_DTW_CHUNK ? n_local - w0 : SPX_DTW_CHUNK;
    __syncthreads();
    for (int k = tid; k < m; k += SPX_DTW_THREADS) {
      const float s = dtw_slope(path + w0 + k, 2 * h);   // window p = w0 + k + h: entries p - h .. p + h - 1
      s_f[k] = s;
      slopes[w0 + k] = s;
    }
    __syncthreads();
    if (tid == 0)
      for (int k = 0; k < m; k++) sum += (double)s_f[k];
  }
  __syncthreads();
  if (tid == 0) s_bcast = (float)sum / (float)n_local;
  __syncthreads();
  const float mean = s_bcast;
  double sq = 0.0;
  for (int w0 = 0; w0 < n_local; w0 += SPX_DTW_CHUNK) {
    const int m = n_local - w0 < SPX_DTW_CHUNK ? n_local - w0 : SPX_DTW_CHUNK;
    __syncthreads();
    for (int k = tid; k < m; k += SPX_DTW_THREADS) {   // (a thread reads back the slopes it wrote itself)
      const float diff = slopes[w0 + k] - mean;
      s_f[k] = diff * diff;
    }
    __syncthreads();
    if (tid == 0)
      for (int k = 0; k < m; k++) sq += (double)s_f[k];
  }
  if (tid == 0) {
    spx_dtw_result* R = results + blockIdx.x;   // (cost: the forward kernel's)
    R->slope = ((float)n_path * sxy - sx * sy) / ((float)n_path * sx2 - sx * sx);
    R->local_mean = mean;
    R->local_std = sqrtf((float)sq / (float)n_local);
    R->n_path = n_path;
    R->n_local = n_local;
  }
}

// The one place that judges a call's pair table and lays its workspace out (SpxCarve, spx_engine.h).  tab (may be null) gets the
// kernels' records.  Returns the bytes, 0 with the broken rule in spx_last_error.
static size_t dtw_layout(const spx_dtw_job* jobs, int n, int dim, SpxDtwPair* tab) {
  if (!jobs) { fail(-1, "spx_batch_dtw: a NULL pointer"); return 0; }
  if (n < 1) { fail(-1, "spx_batch_dtw: n_pairs is below 1"); return 0; }
  if (dim < 1 || dim > SPX_DTW_MAX_DIM) { fail(-1, "spx_batch_dtw: dim is outside 1 .. 65536"); return 0; }
  SpxCarve carve;
  for (int i = 0; i < n; i++) {
    const spx_dtw_job& j = jobs[i];
    if (j.n_a < 1 || j.n_b < 1) { fail(-1, "spx_batch_dtw: a pair with n_a or n_b below 1"); return 0; }
    if ((int64_t)j.n_a * j.n_b > SPX_DTW_MAX_CELLS) { fail(-1, "spx_batch_dtw: a pair of more than 2^30 cells"); return 0; }
    if (j.a_off < 0 || j.b_off < 0 || j.path_off < 0) { fail(-1, "spx_batch_dtw: a negative offset"); return 0; }
    const size_t tb = ((size_t)j.n_b + SPX_DTW_TILE - 1) / SPX_DTW_TILE;
    const size_t entries = (size_t)j.n_a + (size_t)j.n_b - 1;
    const size_t dirs = carve.take((size_t)j.n_a * tb * sizeof(uint4));
    const size_t brow = carve.take((size_t)j.n_b * sizeof(float));
    const size_t rev = carve.take(entries * sizeof(int2));
    const size_t slopes = carve.take(entries * sizeof(float));
    if (tab) tab[i] = {j.a_off, j.b_off, j.path_off, (int64_t)dirs, (int64_t)brow, (int64_t)rev, (int64_t)slopes, j.n_a, j.n_b};
  }
  return carve.o + 256;   // (the caller's base is rounded up to 256 bytes)
}

// HIP events around a launch while spx_set_timing is on: kind 5 = the forward kernel, 6 = the tail (spx_timing_collect sorts them)
struct DtwTimed {
  hipEvent_t a = nullptr, b = nullptr;
  hipStream_t s;
  int kind;
  static hipEvent_t take() {
    std::lock_guard<std::mutex> g(g_tmu);
    if (!g_ev_free.empty()) { hipEvent_t e = g_ev_free.back(); g_ev_free.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
  }
  DtwTimed(int kind_, hipStream_t s_) : s(s_), kind(kind_) {
    if (g_timing) { a = take(); b = take(); (void)hipEventRecord(a, s); }
  }
  ~DtwTimed() {
    if (!a) return;
    (void)hipEventRecord(b, s);
    std::lock_guard<std::mutex> g(g_tmu);
    g_ev_pending.push_back({a, b, kind});
  }
};

static std::atomic<int> g_last_dtw_gx{0}, g_last_dtw_launches{0};   // spx_debug_last_dtw_grid

extern "C" {

int spx_debug_last_dtw_grid(int* launches) {
  if (launches) *launches = g_last_dtw_launches.load(std::memory_order_relaxed);
  return g_last_dtw_gx.load(std::memory_order_relaxed);
}

size_t spx_dtw_workspace_bytes(const spx_dtw_job* jobs, int n_pairs, int dim) { return dtw_layout(jobs, n_pairs, dim, nullptr); }

int spx_batch_dtw(spx_plan_t plan, const spx_dtw_job* jobs, int n, int dim, int ld_a, int ld_b, int half_width, const float* a,
                  const float* b, spx_dtw_result* results, int32_t* path, void* ws, size_t ws_bytes, void* hs) {
  if (!plan || !jobs || !a || !b || !results || !path || !ws) return fail(-1, "spx_batch_dtw: a NULL pointer");
  if (n < 1) return fail(-1, "spx_batch_dtw: n_pairs is below 1");
  std::vector<SpxDtwPair> tab((size_t)n);
  const size_t need = dtw_layout(jobs, n, dim, tab.data());
  if (!need) return -1;
  if (ld_a < dim || ld_b < dim) return fail(-1, "spx_batch_dtw: a row stride below dim");
  if (half_width < 1) return fail(-1, "spx_batch_dtw: half_width is below 1");
  if (ws_bytes < need) return fail(-1, "spx_batch_dtw: the workspace is smaller than spx_dtw_workspace_bytes");
  unsigned char* base = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255);
  hipStream_t st = static_cast<hipStream_t>(hs);
  std::lock_guard<std::mutex> plan_lock(plan->mu);
  // the table: through one of the plan's two pinned staging slots (SpxStage, spx_engine.h), as spx_edit_replay's
  SpxStage& G = plan->stage.take();
  if (G.acquire(sizeof(SpxDtwPair) * (size_t)n)) return -2;
  memcpy(G.p, tab.data(), sizeof(SpxDtwPair) * (size_t)n);
  const SpxDtwPair* d_tab = static_cast<const SpxDtwPair*>(G.p);
  g_last_dtw_gx.store(n, std::memory_order_relaxed);   // one workgroup per pair, in both kernels
  g_last_dtw_launches.store(2, std::memory_order_relaxed);
  {
    DtwTimed t(5, st);
    hipLaunchKernelGGL(spx_dtw_forward_kernel, dim3((unsigned)n), dim3(SPX_DTW_THREADS), 0, st, d_tab, dim, ld_a, ld_b, a, b, results, base);
  }
  {
    DtwTimed t(6, st);
    hipLaunchKernelGGL(spx_dtw_tail_kernel, dim3((unsigned)n), dim3(SPX_DTW_THREADS), 0, st, d_tab, half_width, results, path, base);
  }
  if (G.release(st)) return -2;
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
