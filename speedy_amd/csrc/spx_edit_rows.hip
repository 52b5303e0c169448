// Row tracks through an edit list (include/speedy_hip.h "EDIT LIST, ROW TRACKS": spx_edit_rows, spx_edit_warp_rows,
// spx_edit_unwarp_rows): labels, flags and feature rows at a frame rate -- one row per `hop` key frames -- brought from the input's
// timeline onto the output's (warp) and back (unwarp).  tests/edit_rows_ref.py states the definition in Python integers and
// np.float32 scalars; the kernel is held to it byte for byte.
//
// One kernel template over (direction, mode), spx_edit_lookup_kernel's launch shape: grid (row block, stream), a fixed grid width and
// a stride loop over the rows, every count read on the device.  A block that has rows first copies the column it searches -- the
// records' out_at for a warp, the index G for an unwarp -- into LDS where the stream has at most 4 096 records, and probes there; a
// longer list is searched where it lies.
//   search   each lane runs the binary search of ONE row and keeps what the move needs: the source row (or -1: a row of zeros) and,
//            for a cross-fade of two different rows in BLEND mode, the second row, t and n.
//   move     the wave walks its 64 rows, 2^lg lanes to a row and 64 >> lg rows to a pass (lg chosen on the host from the row's
//            bytes: one lane for a row of at most 16 bytes, the whole wave from 1 KB on); the few integers come from the owning lane
//            by __shfl.  A row moves in the widest power of two that its addresses allow -- 16 bytes where the row's source and
//            destination are aligned to 16 -- and a tail of single elements.  A row of zeros is stored, not loaded; a cross-fade
//            row loads two rows.
//   shape    rows above 64 bytes (lg >= 3): a block takes 64 rows, its four waves search the same 64 and share the passes --
//            four times the blocks in flight for rows that take many passes.  Smaller rows: a block takes 256, a wave its own 64.
// Whatever the records hold: every record index stays inside [0, n_ops) of the stream's region of ops and index, every source row
// inside [0, n_rows) of the track, every destination row inside the count the stream reports; positions are int64 until they are
// checked.  The float cross-fade is spx_edit_replay_scaled's: each operation rounded to float (-ffp-contract=off), the division
// correctly rounded.
#include "spx_engine.h"

#define SPX_EROWS_THREADS 256
#define SPX_EROWS_SLOTS 4096                       // records of a stream whose searched column a block stages in LDS
#define SPX_EROWS_NONE (-0x7fffffff - 1)           // second row of a row that is not a blend
#define SPX_EROWS_MAX_HOP (1 << 20)
#define SPX_EROWS_MAX_DIM 65536
#define SPX_EROWS_MAX_LD (1LL << 28)               // (row index * stride * element size stays far inside int64)

// What the kernel knows of a stream (HOST table in pinned memory).
struct SpxEditRowsStream {
  int64_t op0, op_cap;       // index of the stream's first record in `ops` (and of its first value in `index`), records its region holds
  int64_t limit, key_cap;    // L;  jobs[i].out_cap, in key frames
  int64_t in_off, out_off;   // the track's first element in y_in / y_out
  int64_t n_rows, out_cap;   // rows the track has;  rows its output region holds
};

__host__ __device__ static inline int64_t erows_count(int64_t x, int64_t hop, int64_t phase) {
  return x > phase ? (x - phase + hop - 1) / hop : 0;
}

typedef unsigned erows_u4 __attribute__((ext_vector_type(4)));
typedef unsigned erows_u2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned erows_xfade(unsigned a, unsigned b, float down_w, float up_w, float fn) {
  const float down = __uint_as_float(a) * down_w;
  const float up = __uint_as_float(b) * up_w;
  return __float_as_uint((down + up) / fn);
}
__device__ __forceinline__ erows_u4 erows_xfade(erows_u4 a, erows_u4 b, float down_w, float up_w, float fn) {
  erows_u4 r;
  r.x = erows_xfade(a.x, b.x, down_w, up_w, fn);
  r.y = erows_xfade(a.y, b.y, down_w, up_w, fn);
  r.z = erows_xfade(a.z, b.z, down_w, up_w, fn);
  r.w = erows_xfade(a.w, b.w, down_w, up_w, fn);
  return r;
}

// `count` values of type V of one row, lanes l, l + lanes, ..: a copy of ia, zeros (ia == nullptr), or -- blend -- the cross-fade of
// ia and ib, either of which may be a row of zeros.
template <class V>
__device__ __forceinline__ void erows_span(char* __restrict__ out, const char* __restrict__ ia, int count, int l, int lanes) {
  V* __restrict__ o = reinterpret_cast<V*>(out);
  if (ia) {
    const V* __restrict__ a = reinterpret_cast<const V*>(ia);
    for (int c = l; c < count; c += lanes) o[c] = a[c];
  } else {
    for (int c = l; c < count; c += lanes) o[c] = V(0);
  }
}
template <class V>
__device__ __forceinline__ void erows_span_blend(char* __restrict__ out, const char* __restrict__ ia, const char* __restrict__ ib,
                                                 int count, int l, int lanes, float down_w, float up_w, float fn) {
  V* __restrict__ o = reinterpret_cast<V*>(out);
  const V* __restrict__ a = reinterpret_cast<const V*>(ia);
  const V* __restrict__ b = reinterpret_cast<const V*>(ib);
  for (int c = l; c < count; c += lanes) o[c] = erows_xfade(ia ? a[c] : V(0), ib ? b[c] : V(0), down_w, up_w, fn);
}

// `bytes` of a row in accesses of `width` bytes (a power of two that divides every address involved and `bytes`).
__device__ __forceinline__ void erows_move(int width, char* __restrict__ out, const char* __restrict__ ia, int bytes, int l, int lanes) {
  switch (width) {
    case 16: erows_span<erows_u4>(out, ia, bytes >> 4, l, lanes); break;
    case 8: erows_span<erows_u2>(out, ia, bytes >> 3, l, lanes); break;
    case 4: erows_span<unsigned>(out, ia, bytes >> 2, l, lanes); break;
    case 2: erows_span<unsigned short>(out, ia, bytes >> 1, l, lanes); break;
    default: erows_span<unsigned char>(out, ia, bytes, l, lanes); break;
  }
}

template <bool UNWARP, bool BLEND>
__global__ void __launch_bounds__(SPX_EROWS_THREADS)
spx_edit_rows_kernel(const SpxEditRowsStream* __restrict__ streams, int stream0, const int4* __restrict__ ops,
                     const int64_t* __restrict__ n_ops, const int64_t* __restrict__ n_out, const int32_t* __restrict__ index, int hop,
                     int phase, int row_bytes, int64_t ld_in_bytes, int64_t ld_out_bytes, int elem_bytes, int lg, int share,
                     const char* __restrict__ y_in, char* __restrict__ y_out, int64_t* __restrict__ n_rows_out) {
  __shared__ int s_col[SPX_EROWS_SLOTS];
  const int s = stream0 + (int)blockIdx.y;
  const SpxEditRowsStream S = streams[s];
  const int64_t nk64 = n_ops[s];
  int64_t no64 = n_out[s];
  const bool reports = blockIdx.x == 0 && threadIdx.x == 0;
  // nothing for a stream whose list did not fit or is empty, a warp without output, an unwarp whose output did not fit
  if (nk64 <= 0 || nk64 > S.op_cap || (UNWARP ? no64 < 0 : no64 <= 0)) {
    if (reports) n_rows_out[s] = 0;
    return;
  }
  if (no64 > S.key_cap) no64 = S.key_cap;
  if (no64 > 0x7fffffff) no64 = 0x7fffffff;
  if (no64 < 0) no64 = 0;
  const int no = (int)no64, nk = (int)nk64;
  const int L = (int)(S.limit > 0x7fffffff ? 0x7fffffff : (S.limit < 0 ? 0 : S.limit));
  const int64_t R = erows_count(UNWARP ? L : no, hop, phase);
  if (R > S.out_cap) {
    if (reports) n_rows_out[s] = -R;
    return;
  }
  if (reports) n_rows_out[s] = R;
  const int chunk = share ? 64 : SPX_EROWS_THREADS;
  if ((int64_t)blockIdx.x * chunk >= R) return;      // (the whole block: no row to move, nothing to stage)
  const int4* __restrict__ gops = ops + S.op0;
  const int32_t* __restrict__ G = UNWARP ? index + S.op0 : nullptr;
  const bool staged = nk <= SPX_EROWS_SLOTS;
  if (staged) {
    for (int j = threadIdx.x; j < nk; j += SPX_EROWS_THREADS) s_col[j] = UNWARP ? G[j] : gops[j].x;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lanes = 1 << lg, rows_per_pass = 64 >> lg, l = lane & (lanes - 1);
  const int64_t n_rows = S.n_rows;
  const char* __restrict__ yin = y_in + S.in_off * elem_bytes;
  char* __restrict__ yout = y_out + S.out_off * elem_bytes;
  // a source frame as a row of the track, -1 where it reads as zeros
  const auto row_of = [&](int64_t src) -> int {
    if (src < 0 || src >= L) return -1;
    const int64_t r = src / hop;
    return r < n_rows ? (int)r : -1;
  };
  for (int64_t base = (int64_t)blockIdx.x * chunk; base < R; base += (int64_t)gridDim.x * chunk) {
    // ---- search: one row per lane ----
    const int64_t j = base + (share ? lane : (int)threadIdx.x);
    int ra = -1, rb = SPX_EROWS_NONE, xt = 0, xn = 1;
    if (j < R) {
      const int64_t pos = j * hop + phase;           // below no (warp) or L (unwarp): it fits int32
      if (!UNWARP) {
        const int u = (int)pos;
        int lo = 0, hi = nk;                         // the largest record with out_at <= u (record 0 where there is none)
        while (hi - lo > 1) {
          const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
          if ((staged ? s_col[mid] : gops[mid].x) <= u) lo = mid; else hi = mid;
        }
        const int4 op = gops[lo];
        const int64_t a = op.y, b = op.z, n = op.w;
        const int64_t t = (int64_t)u - op.x;
        if (!BLEND || b < 0) {
          ra = row_of((b < 0 || t < ((n + 1) >> 1)) ? a + t : b + t);
        } else {
          ra = row_of(a + t);
          const int r2 = row_of(b + t);
          if (r2 != ra) {                            // (the same row, or zeros twice: the row itself, no arithmetic)
            rb = r2;
            xt = t > 0x7fffffff ? 0x7fffffff : (t < -0x7fffffffLL ? -0x7fffffff : (int)t);
            xn = op.w;
          }
        }
      } else {
        const int p = (int)pos;
        int lo = 0, hi = nk;                         // the first record with G >= p
        while (lo < hi) {
          const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
          if ((staged ? s_col[mid] : G[mid]) >= p) hi = mid; else lo = mid + 1;
        }
        if (lo < nk) {
          const int4 op = gops[lo];
          const int64_t a = op.y, b = op.z, n = op.w;
          int64_t t = p > a ? p - a : 0;
          if (b >= 0) {
            const int64_t h = (n + 1) >> 1;
            if (t >= h) t = p - b > h ? p - b : h;
          }
          const int64_t o = (int64_t)op.x + t;
          if (o >= 0 && o < no) {
            const int64_t r = o / hop;
            if (r < n_rows) ra = (int)r;
          }
        }
      }
    }
    // ---- move: the wave walks its rows, `lanes` lanes to a row ----
    const int64_t wbase = base + (share ? 0 : wave * 64);
    for (int pass = share ? wave : 0; pass < lanes; pass += share ? SPX_EROWS_THREADS / 64 : 1) {
      if (wbase + (int64_t)pass * rows_per_pass >= R) break;       // (the same for every lane of the wave)
      const int owner = pass * rows_per_pass + (lane >> lg);
      const int era = __shfl(ra, owner);
      int erb = SPX_EROWS_NONE, et = 0, en = 1;
      if (BLEND) {
        erb = __shfl(rb, owner);
        et = __shfl(xt, owner);
        en = __shfl(xn, owner);
      }
      const int64_t jr = wbase + owner;
      if (jr >= R) continue;
      char* __restrict__ out = yout + jr * ld_out_bytes;
      const char* __restrict__ ia = era >= 0 ? yin + (int64_t)era * ld_in_bytes : nullptr;
      const char* __restrict__ ib = BLEND && erb >= 0 ? yin + (int64_t)erb * ld_in_bytes : nullptr;
      const uintptr_t m = reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(ia) | reinterpret_cast<uintptr_t>(ib);
      const int width = (m & 15) ? (int)(m & (~m + 1)) : 16;       // the largest power of two, at most 16, that divides all three
      const int body = row_bytes & ~(width - 1);
      if (BLEND && erb != SPX_EROWS_NONE) {
        const float down_w = (float)((int64_t)en - et), up_w = (float)et, fn = (float)en;
        const int wide = width == 16 ? body : 0;                  // (float rows: 16 bytes or single values)
        erows_span_blend<erows_u4>(out, ia, ib, wide >> 4, l, lanes, down_w, up_w, fn);
        erows_span_blend<unsigned>(out + wide, ia ? ia + wide : nullptr, ib ? ib + wide : nullptr, (row_bytes - wide) >> 2, l, lanes,
                                   down_w, up_w, fn);
      } else {
        erows_move(width, out, ia, body, l, lanes);
        if (body < row_bytes) erows_move(elem_bytes, out + body, ia ? ia + body : nullptr, row_bytes - body, l, lanes);
      }
    }
  }
}

static std::atomic<int> g_last_rows_gx{0}, g_last_rows_launches{0};   // spx_debug_last_rows_grid

// Both calls behind their names: the checks, the streams' table, its trip through the plan's pinned staging slot, the launches.
static int edit_rows_run(const char* who, bool unwarp, spx_plan_t plan, const spx_stream_job* jobs, int n, const spx_edit_op* ops,
                         const int64_t* ops_cap, const int64_t* n_ops, const int64_t* n_out, const int32_t* index,
                         const spx_edit_rows_track* tracks, int32_t hop, int32_t phase, int32_t dim, int64_t ld_in, int64_t ld_out,
                         int elem_bytes, int mode, const void* y_in, void* y_out, int64_t* n_rows_out, void* hs) {
  const auto refuse = [who](const char* why) { return fail(-1, std::string(who) + ": " + why); };
  if (spx_check_jobs(plan, jobs, n, true)) return -1;
  if (!ops || !ops_cap || !n_ops || !n_out || !tracks || !y_in || !y_out || !n_rows_out) return refuse("a NULL pointer");
  if (unwarp && !index) return refuse("an unwarp needs the index (spx_edit_index); index is NULL");
  if (hop < 1 || hop > SPX_EROWS_MAX_HOP) return refuse("hop is outside 1 .. 2^20");
  if (phase < 0 || phase >= hop) return refuse("phase is outside [0, hop)");
  if (dim < 1 || dim > SPX_EROWS_MAX_DIM) return refuse("dim is outside 1 .. 65536");
  if (ld_in < dim || ld_out < dim) return refuse("a row stride below dim");
  if (ld_in > SPX_EROWS_MAX_LD || ld_out > SPX_EROWS_MAX_LD) return refuse("a row stride above 2^28 elements");
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8) return refuse("elem_bytes is none of 1, 2, 4, 8");
  if (mode != SPX_ROWS_NEAREST && mode != SPX_ROWS_BLEND) return refuse("an unknown mode");
  if (mode == SPX_ROWS_BLEND && elem_bytes != 4) return refuse("SPX_ROWS_BLEND takes float32 rows: elem_bytes must be 4");
  if (reinterpret_cast<uintptr_t>(ops) & 15) return refuse("ops is not aligned to 16 bytes");
  const uintptr_t amask = (uintptr_t)elem_bytes - 1;
  if ((reinterpret_cast<uintptr_t>(y_in) & amask) || (reinterpret_cast<uintptr_t>(y_out) & amask))
    return refuse("y_in or y_out is not aligned to the element size");
  const int B = plan->dev.B;
  const int row_bytes = dim * elem_bytes;
  int lg = 0;                                        // 2^lg lanes to a row: one 16-byte access each where the row is aligned
  while (lg < 6 && (16 << lg) < row_bytes) lg++;
  const int share = lg >= 3;
  const int chunk = share ? 64 : SPX_EROWS_THREADS;
  std::vector<SpxEditRowsStream> tab((size_t)n);
  int64_t row = 0, blocks = 1;
  for (int i = 0; i < n; i++) {
    const spx_edit_rows_track& t = tracks[i];
    if (t.in_off < 0 || t.out_off < 0) return refuse("a negative track offset");
    if (t.n_rows < 0 || t.out_cap < 0) return refuse("a negative n_rows or out_cap");
    if (ops_cap[i] < 0) return refuse("a negative capacity");
    SpxEditRowsStream& s = tab[i];
    s.op0 = row; s.op_cap = ops_cap[i];
    s.limit = jobs[i].nonlinear != 0.0f ? jobs[i].n_in / B * B : jobs[i].n_in;
    s.key_cap = jobs[i].out_cap;
    s.in_off = t.in_off; s.out_off = t.out_off; s.n_rows = t.n_rows; s.out_cap = t.out_cap;
    if (ops_cap[i] > 0x7fffffff || (row += ops_cap[i]) > 0x7fffffff) return refuse("more than 2^31 - 1 records of capacity in one call");
    // the rows the stream can have at most: what the grid is sized for (a stream with more than out_cap rows writes none)
    int64_t frames = unwarp ? s.limit : s.key_cap;
    frames = frames > 0x7fffffff ? 0x7fffffff : frames;
    int64_t r = erows_count(frames, hop, phase);
    if (r > t.out_cap) r = t.out_cap;
    if ((r + chunk - 1) / chunk > blocks) blocks = (r + chunk - 1) / chunk;
  }
  hipStream_t st = static_cast<hipStream_t>(hs);
  std::lock_guard<std::mutex> plan_lock(plan->mu);
  SpxStage& G = plan->stage.take();
  if (G.acquire(sizeof(SpxEditRowsStream) * (size_t)n)) return -2;
  memcpy(G.p, tab.data(), sizeof(SpxEditRowsStream) * (size_t)n);
  // row blocks per stream, as spx_edit_lookup chooses them -- and no more than the longest stream can use
  int gx = 4096 / n;
  gx = gx < 4 ? 4 : (gx > 1024 ? 1024 : gx);
  if (blocks < gx) gx = (int)blocks;
  g_last_rows_gx.store(gx, std::memory_order_relaxed);
  g_last_rows_launches.store((n + 65534) / 65535, std::memory_order_relaxed);
  const int4* ops4 = reinterpret_cast<const int4*>(ops);
  const char* yi = static_cast<const char*>(y_in);
  char* yo = static_cast<char*>(y_out);
  const int64_t ldi = ld_in * elem_bytes, ldo = ld_out * elem_bytes;
  for (int s0 = 0; s0 < n; s0 += 65535) {   // (the grid's second dimension holds 65 535)
    const int m = n - s0 < 65535 ? n - s0 : 65535;
    const dim3 grid((unsigned)gx, (unsigned)m), block(SPX_EROWS_THREADS);
    const SpxEditRowsStream* T = static_cast<const SpxEditRowsStream*>(G.p);
    if (unwarp)
      hipLaunchKernelGGL((spx_edit_rows_kernel<true, false>), grid, block, 0, st, T, s0, ops4, n_ops, n_out, index, hop, phase, row_bytes,
                         ldi, ldo, elem_bytes, lg, share, yi, yo, n_rows_out);
    else if (mode == SPX_ROWS_BLEND)
      hipLaunchKernelGGL((spx_edit_rows_kernel<false, true>), grid, block, 0, st, T, s0, ops4, n_ops, n_out, index, hop, phase, row_bytes,
                         ldi, ldo, elem_bytes, lg, share, yi, yo, n_rows_out);
    else
      hipLaunchKernelGGL((spx_edit_rows_kernel<false, false>), grid, block, 0, st, T, s0, ops4, n_ops, n_out, index, hop, phase, row_bytes,
                         ldi, ldo, elem_bytes, lg, share, yi, yo, n_rows_out);
  }
  if (G.release(st)) return -2;
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" {

int spx_debug_last_rows_grid(int* launches) {
  if (launches) *launches = g_last_rows_launches.load(std::memory_order_relaxed);
  return g_last_rows_gx.load(std::memory_order_relaxed);
}

int64_t spx_edit_rows(int64_t frames, int32_t hop, int32_t phase) {
  if (frames < 0 || hop < 1 || hop > SPX_EROWS_MAX_HOP || phase < 0 || phase >= hop) return -1;
  return erows_count(frames, hop, phase);
}

int spx_edit_warp_rows(spx_plan_t plan, const spx_stream_job* jobs, int n, const spx_edit_op* ops, const int64_t* ops_cap,
                       const int64_t* n_ops, const int64_t* n_out, const spx_edit_rows_track* tracks, int32_t hop, int32_t phase,
                       int32_t dim, int64_t ld_in, int64_t ld_out, int elem_bytes, int mode, const void* y_in, void* y_out,
                       int64_t* n_rows_out, void* hs) {
  return edit_rows_run("spx_edit_warp_rows", false, plan, jobs, n, ops, ops_cap, n_ops, n_out, nullptr, tracks, hop, phase, dim, ld_in,
                       ld_out, elem_bytes, mode, y_in, y_out, n_rows_out, hs);
}

int spx_edit_unwarp_rows(spx_plan_t plan, const spx_stream_job* jobs, int n, const spx_edit_op* ops, const int64_t* ops_cap,
                         const int64_t* n_ops, const int64_t* n_out, const int32_t* index, const spx_edit_rows_track* tracks,
                         int32_t hop, int32_t phase, int32_t dim, int64_t ld_in, int64_t ld_out, int elem_bytes, const void* y_in,
                         void* y_out, int64_t* n_rows_out, void* hs) {
  return edit_rows_run("spx_edit_unwarp_rows", true, plan, jobs, n, ops, ops_cap, n_ops, n_out, index, tracks, hop, phase, dim, ld_in,
                       ld_out, elem_bytes, SPX_ROWS_NEAREST, y_in, y_out, n_rows_out, hs);
}

}  // extern "C"
