// Sample-exact position lookup over an edit list (include/speedy_hip.h "EDIT LIST": spx_edit_index, spx_edit_lookup): which output
// frame an input frame is first heard at, and which input frame an output frame plays.  tests/edit_lookup_ref.py states the
// definition in Python integers; both kernels are held to it answer for answer.
//
// The SOURCE of output frame out_at + t of a record (out_at, a, b, n): a + t for a copy; for a cross-fade a + t while the ramp going
// down has the larger weight (2 t < n, i.e. t < h = (n + 1) / 2), b + t from there on.  It is not monotone over the output -- a
// slow-down plays input twice -- so the forward search runs over
//   R_k = the largest source inside record k,   G_k = max(R_0 .. R_k)   (the INDEX: one int32 per record, laid out as `ops` is)
// and the first record with G_k >= p holds the first output frame whose source is at or above p; where in the record is a closed
// form.  The inverse search runs over the out_at column of the records themselves and needs no index.
//
// Index kernel: one workgroup per stream, one record per thread and pass.  The running maximum goes across a wave by DPP (row
// shifts of 1, 2, 4 and 8 lanes, then the two row broadcasts), across the four waves through 16 bytes of LDS, and from one pass of
// 256 records to the next in a register.  One 16-byte load and one 4-byte store per record, exactly min(n_ops, ops_cap) of them.
//
// Lookup kernel: spx_map_lookup_kernel's shape -- one thread per query, grid over (query block, stream), a fixed grid width and a
// stride loop, the query counts read on the device.  A query is a binary search (about eleven dependent probes for a 10 s stream)
// and one 16-byte load of the record it lands on.  A block that has queries first copies the column it searches -- G, or the
// records' out_at -- into LDS, where the stream has at most 4 096 records (16 KB; a 10 s stream has about 1 000: 4 KB), and probes
// there; a longer list is searched where it lies, through the cache.  Chosen by measurement, against the form that always searches
// in memory (-DSPX_EDIT_LOOKUP_LDS=0 below): 256 streams x 100 000 queries 0.32 against 0.51 ms forward, 0.32 against 0.59 ms
// inverse; x 1 000 queries 0.022 against 0.027 and 0.030 ms (profiles/edit_lookup.txt).
// Whatever the records hold, every index stays inside [0, min(n_ops, ops_cap)) of the stream's region of `ops` and `index`; int64
// queries are clamped before they are narrowed; the arithmetic on a record's fields is int64.  Nothing else is read: no track, no
// audio.
#include "spx_engine.h"

#define SPX_ELOOK_THREADS 256
#define SPX_EIDX_THREADS 256
#define SPX_EIDX_WAVES (SPX_EIDX_THREADS / 64)
// -DSPX_EDIT_LOOKUP_LDS=0: the other form of the lookup kernel, for A/B runs (profiles/edit_lookup.txt has both): no staging, every
// probe of the binary search a load from memory.
#ifndef SPX_EDIT_LOOKUP_LDS
#define SPX_EDIT_LOOKUP_LDS 1
#endif
#define SPX_ELOOK_SLOTS 4096                       // records of a stream whose searched column a block stages in LDS

// What both kernels know of a stream (HOST table in pinned memory).
struct SpxEditLookupStream {
  int64_t op0, op_cap;   // index of the stream's first record in `ops` (and of its first value in `index`), records its region holds
  int64_t limit;         // L: n_in for a linear job, (n_in / B) * B for a nonlinear one
};

__device__ __forceinline__ int sat32(int64_t v) {
  return v > 0x7fffffffLL ? 0x7fffffff : (v < -0x7fffffffLL - 1 ? (int)(-0x7fffffffLL - 1) : (int)v);
}

// R: the largest source inside a record.  (Every position of a list spx_batch_run_edits wrote fits int32; a planted one saturates.)
__device__ __forceinline__ int edit_record_max(const int4 op) {
  const int64_t a = op.y, b = op.z, n = op.w;
  if (b < 0) return sat32(a + n - 1);
  const int64_t h = (n + 1) >> 1;
  const int64_t ra = a + h - 1, rb = b + n - 1;
  return sat32(n > h && rb > ra ? rb : ra);
}

// Inclusive running maximum over the 64 lanes of a wave, every lane active.  A lane that a shift leaves without a source -- the
// first lanes of a row, the rows a broadcast does not address -- keeps `old`, the identity.
#define SPX_DPP_MAX(v, ctrl, row_mask)                                                            \
  do {                                                                                            \
    const int o_ = __builtin_amdgcn_update_dpp((int)0x80000000, (v), (ctrl), (row_mask), 0xf, false); \
    (v) = o_ > (v) ? o_ : (v);                                                                    \
  } while (0)
__device__ __forceinline__ int wave_running_max(int v) {
  SPX_DPP_MAX(v, 0x111, 0xf);   // row_shr:1
  SPX_DPP_MAX(v, 0x112, 0xf);   // row_shr:2
  SPX_DPP_MAX(v, 0x114, 0xf);   // row_shr:4
  SPX_DPP_MAX(v, 0x118, 0xf);   // row_shr:8   -- every row of 16 lanes is done
  SPX_DPP_MAX(v, 0x142, 0xa);   // row_bcast:15 into rows 1 and 3
  SPX_DPP_MAX(v, 0x143, 0xc);   // row_bcast:31 into rows 2 and 3
  return v;
}

__global__ void __launch_bounds__(SPX_EIDX_THREADS)
spx_edit_index_kernel(const SpxEditLookupStream* __restrict__ streams, int stream0, const int4* __restrict__ ops,
                      const int64_t* __restrict__ n_ops, int32_t* __restrict__ index) {
  __shared__ int s_tot[2][SPX_EIDX_WAVES];
  const int s = stream0 + (int)blockIdx.x;
  const SpxEditLookupStream S = streams[s];
  int64_t nk64 = n_ops[s];
  if (nk64 <= 0) return;                           // (a list that did not fit: its index region stays what it was)
  if (nk64 > S.op_cap) nk64 = S.op_cap;
  const int nk = (int)nk64;                        // (op_cap <= 2^31 - 1: the call checks it)
  const int4* __restrict__ gops = ops + S.op0;
  int32_t* __restrict__ gidx = index + S.op0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = (int)0x80000000;
  int buf = 0;
  // (base runs in 64 bits: nk may lie within 256 of 2^31.  The trip count is the workgroup's: every lane takes part in the DPP steps.)
  for (int64_t base = 0; base < nk; base += SPX_EIDX_THREADS, buf ^= 1) {
    const int64_t k = base + threadIdx.x;
    const int r = k < nk ? edit_record_max(gops[k]) : (int)0x80000000;
    const int v = wave_running_max(r);
    if (lane == 63) s_tot[buf][wave] = v;
    // one barrier per pass: the totals alternate between two rows, and a wave reaches the row's next use only through the barrier
    // of the pass in between, behind every read of this one
    __syncthreads();
    int pre = carry, all = carry;
#pragma unroll
    for (int w = 0; w < SPX_EIDX_WAVES; w++) {
      const int t = s_tot[buf][w];
      all = t > all ? t : all;
      if (w < wave) pre = t > pre ? t : pre;
    }
    if (k < nk) gidx[k] = v > pre ? v : pre;
    carry = all;
  }
}

__global__ void __launch_bounds__(SPX_ELOOK_THREADS)
spx_edit_lookup_kernel(const SpxEditLookupStream* __restrict__ streams, int stream0, const int4* __restrict__ ops,
                       const int64_t* __restrict__ n_ops, const int64_t* __restrict__ n_out, const int32_t* __restrict__ index,
                       const int64_t* __restrict__ q_off, const int64_t* __restrict__ q, int64_t* __restrict__ r,
                       int32_t* __restrict__ rec, int inverse) {
  const int s = stream0 + (int)blockIdx.y;
  const SpxEditLookupStream S = streams[s];
  const int64_t q0 = q_off[s], q1 = q_off[s + 1];
  int64_t nk64 = n_ops[s], no64 = n_out[s];
  const bool dead = nk64 < 0 || no64 < 0;          // the list did not fit, or the output did not: -1 throughout
  if (nk64 > S.op_cap) nk64 = S.op_cap;
  if (no64 > 0x7fffffff) no64 = 0x7fffffff;
  const int nk = dead ? 0 : (int)nk64, no = dead ? 0 : (int)no64;
  const int L = (int)S.limit;
  const int4* __restrict__ gops = ops + S.op0;
  const int32_t* __restrict__ G = index ? index + S.op0 : nullptr;
  const int64_t stride = (int64_t)gridDim.x * SPX_ELOOK_THREADS;
#if SPX_EDIT_LOOKUP_LDS
  __shared__ int s_col[SPX_ELOOK_SLOTS];
  if (q0 + (int64_t)blockIdx.x * SPX_ELOOK_THREADS >= q1) return;   // (the whole block: nothing to answer, nothing to stage)
  const bool staged = nk <= SPX_ELOOK_SLOTS;
  if (staged) {
    for (int j = threadIdx.x; j < nk; j += SPX_ELOOK_THREADS) s_col[j] = inverse ? gops[j].x : G[j];
    __syncthreads();
  }
#define SPX_ELOOK_G(j) (staged ? s_col[j] : G[j])
#define SPX_ELOOK_AT(j) (staged ? s_col[j] : gops[j].x)
#else
#define SPX_ELOOK_G(j) G[j]
#define SPX_ELOOK_AT(j) gops[j].x
#endif
  for (int64_t i = q0 + (int64_t)blockIdx.x * SPX_ELOOK_THREADS + threadIdx.x; i < q1; i += stride) {
    int64_t v = q[i], ans;
    int k;
    if (dead) {
      ans = -1; k = -1;
    } else if (!inverse) {
      const int p = v < 0 ? 0 : (v > L ? L : (int)v);
      int lo = 0, hi = nk;                          // the first record with G >= p: lo <= mid < hi <= nk
      while (lo < hi) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (SPX_ELOOK_G(mid) >= p) hi = mid; else lo = mid + 1;
      }
      if (lo >= nk) {
        ans = no; k = -1;
      } else {
        const int4 op = gops[lo];
        const int64_t a = op.y, b = op.z, n = op.w;
        int64_t t = p > a ? p - a : 0;
        if (b >= 0) {
          const int64_t h = (n + 1) >> 1;
          if (t >= h) t = p - b > h ? p - b : h;
        }
        const int64_t o = (int64_t)op.x + t;
        if (o >= no) { ans = no; k = -1; } else { ans = o; k = lo; }   // (a record behind the flush's cut, or reaching across it)
      }
    } else {
      if (v < 0) v = 0;
      if (v >= no || nk == 0) {
        ans = L; k = -1;
      } else {
        const int u = (int)v;
        int lo = 0, hi = nk;                        // the largest record with out_at <= u (record 0 where there is none)
        while (hi - lo > 1) {
          const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
          if (SPX_ELOOK_AT(mid) <= u) lo = mid; else hi = mid;
        }
        const int4 op = gops[lo];
        const int64_t a = op.y, b = op.z, n = op.w;
        const int64_t t = (int64_t)u - op.x;
        const int64_t src = (b < 0 || t < ((n + 1) >> 1)) ? a + t : b + t;
        ans = src < L ? src : L;                    // (a frame that plays the flush's padding answers L)
        k = lo;
      }
    }
    r[i] = ans;
    if (rec) rec[i] = k;
  }
}

static std::atomic<int> g_last_elook_gx{0}, g_last_elook_launches{0};   // spx_debug_last_edit_lookup_grid

// The checks both calls share, and the streams' table.  0, or -1 with spx_last_error.
static int edit_lookup_table(const char* who, spx_plan_t plan, const spx_stream_job* jobs, int n, const void* ops, const int64_t* ops_cap,
                             std::vector<SpxEditLookupStream>& tab) {
  if (reinterpret_cast<uintptr_t>(ops) & 15) return fail(-1, std::string(who) + ": ops is not aligned to 16 bytes");
  const int B = plan->dev.B;
  tab.resize((size_t)n);
  int64_t row = 0;
  for (int i = 0; i < n; i++) {
    if (ops_cap[i] < 0) return fail(-1, std::string(who) + ": a negative capacity");
    tab[i].op0 = row;
    tab[i].op_cap = ops_cap[i];
    tab[i].limit = jobs[i].nonlinear != 0.0f ? jobs[i].n_in / B * B : jobs[i].n_in;
    if (ops_cap[i] > 0x7fffffff || (row += ops_cap[i]) > 0x7fffffff)
      return fail(-1, std::string(who) + ": more than 2^31 - 1 records of capacity in one call");
  }
  return 0;
}

extern "C" {

int spx_debug_last_edit_lookup_grid(int* launches) {
  if (launches) *launches = g_last_elook_launches.load(std::memory_order_relaxed);
  return g_last_elook_gx.load(std::memory_order_relaxed);
}

int spx_edit_index(spx_plan_t plan, const spx_stream_job* jobs, int n, const spx_edit_op* ops, const int64_t* ops_cap,
                   const int64_t* n_ops, int32_t* index, void* hs) {
  if (spx_check_jobs(plan, jobs, n, true)) return -1;
  if (!ops || !ops_cap || !n_ops || !index) return fail(-1, "spx_edit_index: a NULL pointer");
  std::vector<SpxEditLookupStream> tab;
  if (edit_lookup_table("spx_edit_index", plan, jobs, n, ops, ops_cap, tab)) return -1;
  hipStream_t st = static_cast<hipStream_t>(hs);
  std::lock_guard<std::mutex> plan_lock(plan->mu);
  // the table: through one of the plan's two pinned staging slots (SpxStage, spx_engine.h), as spx_map_lookup's
  SpxStage& G = plan->stage.take();
  if (G.acquire(sizeof(SpxEditLookupStream) * (size_t)n)) return -2;
  memcpy(G.p, tab.data(), sizeof(SpxEditLookupStream) * (size_t)n);
  hipLaunchKernelGGL(spx_edit_index_kernel, dim3((unsigned)n), dim3(SPX_EIDX_THREADS), 0, st,
                     static_cast<const SpxEditLookupStream*>(G.p), 0, reinterpret_cast<const int4*>(ops), n_ops, index);
  if (G.release(st)) return -2;
  HIPCHK(hipGetLastError());
  return 0;
}

int spx_edit_lookup(spx_plan_t plan, const spx_stream_job* jobs, int n, const spx_edit_op* ops, const int64_t* ops_cap,
                    const int64_t* n_ops, const int64_t* n_out, const int32_t* index, const int64_t* q_off, const int64_t* q,
                    int64_t* r, int32_t* rec, int inverse, void* hs) {
  if (spx_check_jobs(plan, jobs, n, true)) return -1;
  if (!ops || !ops_cap || !n_ops || !n_out || !q_off || !q || !r) return fail(-1, "spx_edit_lookup: a NULL pointer");
  if (!inverse && !index) return fail(-1, "spx_edit_lookup: a forward lookup needs the index (spx_edit_index); index is NULL");
  std::vector<SpxEditLookupStream> tab;
  if (edit_lookup_table("spx_edit_lookup", plan, jobs, n, ops, ops_cap, tab)) return -1;
  hipStream_t st = static_cast<hipStream_t>(hs);
  std::lock_guard<std::mutex> plan_lock(plan->mu);
  SpxStage& G = plan->stage.take();
  if (G.acquire(sizeof(SpxEditLookupStream) * (size_t)n)) return -2;
  memcpy(G.p, tab.data(), sizeof(SpxEditLookupStream) * (size_t)n);
  // query blocks per stream, as spx_map_lookup chooses them: the counts are the device's to know
  int gx = 4096 / n;
  gx = gx < 4 ? 4 : (gx > 1024 ? 1024 : gx);
  g_last_elook_gx.store(gx, std::memory_order_relaxed);
  g_last_elook_launches.store((n + 65534) / 65535, std::memory_order_relaxed);
  for (int s0 = 0; s0 < n; s0 += 65535) {   // (the grid's second dimension holds 65 535)
    const int m = n - s0 < 65535 ? n - s0 : 65535;
    hipLaunchKernelGGL(spx_edit_lookup_kernel, dim3((unsigned)gx, (unsigned)m), dim3(SPX_ELOOK_THREADS), 0, st,
                       static_cast<const SpxEditLookupStream*>(G.p), s0, reinterpret_cast<const int4*>(ops), n_ops, n_out, index, q_off,
                       q, r, rec, inverse);
  }
  if (G.release(st)) return -2;
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
