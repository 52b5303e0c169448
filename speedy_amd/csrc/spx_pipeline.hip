// spx_pipeline (include/speedy_hip.h): batch after batch, host memory to host memory, with everything in between owned by the
// library -- `depth` sets of device buffers, the pinned output buffers, two HIP streams, the events.
//
// The table given at creation is the pipeline's CAPACITY: where every lane's output lies (out_off), how many frames it holds
// (out_cap), the lane's channel count and plan, the input's extent and the workspace size -- every buffer is sized from these and
// none changes afterwards.  What a batch RUNS is a job table per ticket: the creation table itself (spx_pipeline_submit), or the
// caller's for this batch (spx_pipeline_submit_jobs) once pipeline_check has found that every lane's job fits its lane.  The
// engine takes a fresh table with every call anyway (run_impl rebuilds layout, speed class, launch mode and staged tables from
// it), and the gather kernels read the counts from the device and the capacities from d_tab, which stays valid.
//
// What one submit enqueues (nothing waits on the host except for the batch `depth` tickets back):
//   copy stream   wait(kernels of the batch that last used this buffer set)  ->  H2D of the input  ->  record(in)
//   library       the batch call in its overlapped order (spx_engine.hip): staging, analysis, tension kernels behind `in` on the
//                 device's side stream, the walk kernel on one of the two walk streams
//   run stream    [wait(walk kernel): the engine's]  ->  gather kernel: every stream's produced frames, densely packed at 64-byte
//                 boundaries, written STRAIGHT into the slot's pinned host buffer, with the offsets and the counts  ->  record(done)
// The reference's caller owns one buffer and one loop (speedy_wave.cc:154-242: write a chunk, read what is ready); this is that
// loop for a caller whose unit is a batch of streams.
//
// Why the gather kernel writes host memory itself: the produced size is known on the device only.  A device-to-host copy of the
// exact size needs the host to wait for the batch first (round 4's bench loop did, and the wait kept it from running ahead:
// 2.3-3.5 ms per batch with the pipelined calls); a copy of the capacity moves three times the bytes.  The kernel needs neither,
// and it is narrow (pack_wgs workgroups): PCIe writes are posted, a few waves keep the link busy, and the CUs stay with the
// chains of the next batches' walk kernels -- the runtime's own copy kernel is launched full-width.
// Measured against it (round 5, profiles/r05/r5s_copy_out.txt): the gathered frames to HBM first and out by hipMemcpyAsync, sized
// from the last batch that came back (the rest of a batch that outgrew the copy fetched at wait time) -- the runtime performs
// that copy with its full-width shader kernel (__amd_rocclr_copyBuffer, 0.53 - 0.56 ms per 27 MB), and the leg read 1.78 - 1.83 ms
// per batch against 1.67 - 1.70.  Not kept.
//
// FLOAT samples (SPX_PIPELINE_FLOAT): the same pipeline with a conversion at either end; the engine, its kernels and the int16
// buffers between them are untouched, and a pipeline without the flag takes none of this code.
//   copy stream   [H2D of extent x 4 bytes into the slot's float staging]  ->  this batch's conversion table (spx_convert.hip's
//                 SpxConvJob records: in_off, values and scale per lane, from the slot's pinned copy)  ->  spx_float_to_short_kernel
//                 over (block, lane) into the slot's int16 staging  ->  record(in)
//   run stream    host output: spx_pipe_copy_float_kernel instead of spx_pipe_copy_kernel -- it converts while it packs and writes
//                 floats straight into the slot's pinned float buffer;  SPX_PIPELINE_DEVICE_OUT: spx_short_to_float_kernel (the form
//                 that reads n_out on the device) behind the walk kernel into the slot's float d_out
// The input conversion goes on the COPY stream, not behind `in` on the run stream or one of the engine's: it is the natural
// continuation of the copy it depends on (stream order, no event between them), `in` then means "the int16 staging is complete" and
// the engine is called exactly as for an int16 batch -- and the run stream's head is the previous batch's gather, which waits for
// that batch's walk kernel: a conversion queued there would hold this batch's producers back by a whole batch.  A device input is
// converted there too (nothing to copy): the conversion, not the walk kernel's window loads, reads the caller's buffer, exactly over
// the jobs' values, and `in` says when it has been read.  No stream is added to the five the library holds.
// Measured (profiles/pipeline_float.txt, 256 x 10 s): the conversions take 55 and 24 us, the float gather 0.99 ms for 53.5 MB (the int16
// one 0.49 for half the bytes: the link's rate both); host to host 3.36 ms per batch over a 2.88 ms copy of the 164 MB input.
//
// PLAYBACK RATES (spx_pipeline_create_rate): a one-plan pipeline whose capacities count FINAL frames (spx_plan_out_capacity_rate at the
// rate each lane is sized for) and whose workspace holds the rate call's TSM staging of EVERY lane.  A ticket carries a rate per lane
// beside its job table.  All ones: nothing above changes.  One rate other than 1: the engine runs the batch as spx_batch_run_rate does
// (spx_engine.hip spx_internal_run_rate: the same builder, the plain call) on the RUN stream behind `in`; the tails follow as they are.
//   copy stream   as above (float: with the conversion)  ->  record(in)
//   run stream    wait(in)  ->  staging, analysis, tension, general walk kernel (no flush truncation, into the slot's workspace),
//                 spx_rate_batch_kernel into the slot's d_out  ->  offsets + gather (or the float conversion)  ->  record(done)
// Never detached; no stream is added.  DESIGN.md "The rate pipeline" says where the order against neighbouring overlapped calls
// comes from.
#include "spx_engine.h"   // the engine's entries this file calls ("what the pipeline object calls")

#define SPX_PIPE_MAX_DEPTH 8
#define PIPE_ALIGN 32   // int16 values: every stream's region starts at a 64-byte boundary, in device and in host memory

// Offsets of the packed output: exclusive prefix sums of the streams' produced values, each rounded up to PIPE_ALIGN; written
// to device memory (for the copy kernel) and, with the counts, to the slot's pinned host table.  One workgroup.
__global__ void __launch_bounds__(256)
spx_pipe_offsets_kernel(const int64_t* __restrict__ n_out, const int* __restrict__ channels, const int64_t* __restrict__ caps, int n,
                        int64_t* __restrict__ d_offsets, int64_t* __restrict__ h_offsets, int64_t* __restrict__ h_counts) {
  __shared__ int64_t sh[256];
  __shared__ int64_t carry;
  const int t = threadIdx.x;
  if (t == 0) carry = 0;
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + t;
    int64_t v = 0;
    if (i < n) {
      const int64_t k = n_out[i];
      h_counts[i] = k;
      // a negative count flags an overflowed stream: the frames that fitted its capacity are there; INT64_MIN a lost producer
      int64_t f = (k == INT64_MIN ? 0 : (k > 0 ? k : -k));
      if (f > caps[i]) f = caps[i];
      v = (f * channels[i] + (PIPE_ALIGN - 1)) & ~(int64_t)(PIPE_ALIGN - 1);
    }
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const int64_t add = (t >= d) ? sh[t - d] : 0;
      __syncthreads();
      sh[t] += add;
      __syncthreads();
    }
    const int64_t base = carry;
    if (i < n) { const int64_t o = base + sh[t] - v; d_offsets[i] = o; h_offsets[i] = o; }
    __syncthreads();
    if (t == 255) carry = base + sh[255];
    __syncthreads();
  }
  if (t == 0) { d_offsets[n] = carry; h_offsets[n] = carry; }
}
// The copy: workgroup b takes streams b, b + gridDim.x, ...; 16 bytes per lane and load, four loads in flight (source and
// destination regions start at 64-byte boundaries and are padded to them: the last vector of a stream may carry up to 31 values
// of the capacity region behind the produced frames -- inside the buffers on both sides).
__global__ void __launch_bounds__(256)
spx_pipe_copy_kernel(const int16_t* __restrict__ out, const int64_t* __restrict__ out_offs, const int64_t* __restrict__ d_offsets, int n,
                     int16_t* __restrict__ dst) {
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const uint4* __restrict__ s = reinterpret_cast<const uint4*>(out + out_offs[i]);
    uint4* __restrict__ d = reinterpret_cast<uint4*>(dst + d_offsets[i]);
    const int64_t nv = (d_offsets[i + 1] - d_offsets[i]) / 8;   // 16-byte vectors
    for (int64_t e0 = threadIdx.x; e0 < nv; e0 += 4 * 256) {
      uint4 v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) { const int64_t e = e0 + u * 256; if (e < nv) v[u] = s[e]; }
#pragma unroll
      for (int u = 0; u < 4; u++) { const int64_t e = e0 + u * 256; if (e < nv) d[e] = v[u]; }
    }
  }
}
// The same on float samples: per step a lane loads one 16-byte vector of 8 int16 and stores two 16-byte vectors of floats, every
// value int16 / 32767.0f (the IEEE quotient: -fhip-fp32-correctly-rounded-divide-sqrt, as spx_short_to_float_kernel has it).  The
// packed offsets count values, so a stream's floats start at a 128-byte boundary of dst; the last vectors of a stream may carry the
// images of up to 31 capacity-region values -- dst holds out_values + 64 floats.
typedef short spx_pipe_short8 __attribute__((ext_vector_type(8)));
typedef float spx_pipe_float4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256)
spx_pipe_copy_float_kernel(const int16_t* __restrict__ out, const int64_t* __restrict__ out_offs, const int64_t* __restrict__ d_offsets, int n,
                           float* __restrict__ dst) {
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const spx_pipe_short8* __restrict__ s = reinterpret_cast<const spx_pipe_short8*>(out + out_offs[i]);
    spx_pipe_float4* __restrict__ d = reinterpret_cast<spx_pipe_float4*>(dst + d_offsets[i]);
    const int64_t nv = (d_offsets[i + 1] - d_offsets[i]) / 8;   // 16-byte vectors of the source
    for (int64_t e0 = threadIdx.x; e0 < nv; e0 += 4 * 256) {
      spx_pipe_short8 v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) { const int64_t e = e0 + u * 256; if (e < nv) v[u] = s[e]; }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int64_t e = e0 + u * 256;
        if (e < nv) {
          spx_pipe_float4 a, b;
#pragma unroll
          for (int k = 0; k < 4; k++) { a[k] = (float)v[u][k] / 32767.0f; b[k] = (float)v[u][4 + k] / 32767.0f; }
          d[2 * e] = a;
          d[2 * e + 1] = b;
        }
      }
    }
  }
}

struct SpxPipeSlot {
  int16_t* d_in = nullptr;
  int16_t* d_out = nullptr;
  int64_t* d_nout = nullptr;
  int64_t* d_offsets = nullptr;   // [n + 1] packed offsets (device copy, for the gather kernel)
  void* ws = nullptr;
  int16_t* h_in = nullptr;        // pinned staging a caller may fill (spx_pipeline_host_input), allocated on first use
  int16_t* h_out = nullptr;       // pinned: the packed output
  int64_t* h_meta = nullptr;      // pinned: offsets[n + 1], counts[n]
  hipEvent_t ev_in = nullptr;     // the input has arrived in d_in
  hipEvent_t ev_done = nullptr;   // kernels and gather done: the output is in host memory, d_in / d_out may be reused
  std::vector<spx_stream_job> jobs;   // the table this ticket was submitted with (the pipeline's out_off / out_cap in it): kept for the
                                      // record -- the engine stages what it needs before its call returns, nothing reads this later
  // SPX_PIPELINE_FLOAT (everything below stays null without the flag)
  float* d_inf = nullptr;         // float staging of a host input, allocated on first use as d_in is
  float* d_outf = nullptr;        // SPX_PIPELINE_DEVICE_OUT: the float output in the static layout
  float* h_inf = nullptr;         // pinned float staging a caller may fill (spx_pipeline_host_input_float)
  float* h_outf = nullptr;        // pinned: the packed float output (no h_out then)
  void* h_cv = nullptr;           // pinned: this ticket's conversion table, and its device copy
  void* d_cv = nullptr;
  int64_t ticket = -1;
  bool in_recorded = false;       // ev_in has been recorded at least once (h_in / d_in have a copy to wait for)
  bool in_host = false;           // this ticket's input came from host memory: consumed once ev_in has passed (device input: ev_done);
                                  // set for a float input of either kind: its conversion, in front of ev_in, is what reads it
};
struct spx_pipeline {
  std::vector<spx_plan_t> plans;
  std::vector<int> plan_index;
  bool mixed = false;
  bool rate_kind = false;             // made by spx_pipeline_create_rate: capacities in final frames, every lane's TSM staging in the workspace
  std::vector<float> rates;           // ... and the rate every lane was sized for: the rates of spx_pipeline_submit
  int n = 0, depth = 0;
  unsigned flags = 0;
  int device = 0;
  std::vector<spx_stream_job> jobs;   // the creation table with the pipeline's own out_off / out_cap: every lane's CAPACITY (out_off,
                                      // out_cap, channels; with in_values and ws_bytes below), and the table of spx_pipeline_submit
  std::vector<int64_t> static_offsets;   // SPX_PIPELINE_DEVICE_OUT: the fixed layout of d_out (offsets[n] = its extent)
  size_t in_values = 0, out_values = 0, ws_bytes = 0;
  hipStream_t s_h2d = nullptr, s_run = nullptr;
  int64_t* d_tab = nullptr;           // out_off[n], cap[n] (int64), channels[n] (int)
  std::vector<SpxPipeSlot> slots;
  int64_t next_ticket = 0;
  int pack_wgs = 64;
};

static int pfail(int code, const std::string& msg) { spx_internal_set_error(msg.c_str()); return code; }
#define PCHK(expr)                                                                             \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) return pfail(-2, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

static void pipeline_free(spx_pipeline* p) {
  if (!p) return;
  (void)hipStreamSynchronize(p->s_run);
  if (p->s_h2d) (void)hipStreamSynchronize(p->s_h2d);
  for (auto& S : p->slots) {
    if (S.ev_done) { if (S.ticket >= 0) (void)hipEventSynchronize(S.ev_done); (void)hipEventDestroy(S.ev_done); }
    if (S.ev_in) (void)hipEventDestroy(S.ev_in);
    if (S.d_in) (void)hipFree(S.d_in);
    if (S.d_out) (void)hipFree(S.d_out);
    if (S.d_nout) (void)hipFree(S.d_nout);
    if (S.d_offsets) (void)hipFree(S.d_offsets);
    if (S.ws) (void)hipFree(S.ws);
    if (S.h_in) (void)hipHostFree(S.h_in);
    if (S.h_out) (void)hipHostFree(S.h_out);
    if (S.h_meta) (void)hipHostFree(S.h_meta);
    if (S.d_inf) (void)hipFree(S.d_inf);
    if (S.d_outf) (void)hipFree(S.d_outf);
    if (S.d_cv) (void)hipFree(S.d_cv);
    if (S.h_inf) (void)hipHostFree(S.h_inf);
    if (S.h_outf) (void)hipHostFree(S.h_outf);
    if (S.h_cv) (void)hipHostFree(S.h_cv);
  }
  if (p->d_tab) (void)hipFree(p->d_tab);
  if (p->s_run) (void)hipStreamDestroy(p->s_run);
  if (p->s_h2d) (void)hipStreamDestroy(p->s_h2d);
  (void)hipGetLastError();
  delete p;
}

// The int16 calls on a float pipeline, the _float calls on an int16 one: refused before anything is waited for, copied or enqueued.
static int wrong_kind(const spx_pipeline* p, bool float_call, const char* who) {
  const bool flt = (p->flags & SPX_PIPELINE_FLOAT) != 0;
  if (flt == float_call) return 0;
  return pfail(-1, std::string(who) + (flt ? ": the pipeline was created with SPX_PIPELINE_FLOAT and takes the _float calls only"
                                           : ": the pipeline was created without SPX_PIPELINE_FLOAT and takes the int16 calls only"));
}
static int lane_fail(int lane, const std::string& what) { return pfail(-1, "spx_pipeline: lane " + std::to_string(lane) + ": " + what); }
// A lane's job by the engine's rules (spx_jobs.h), in the engine's words, with the lane in front
static int lane_check(const spx_pipeline* p, int lane, const spx_stream_job& j) {
  const SpxJobFault f = spx_check_job(spx_job_limits(p->plans[p->mixed ? p->plan_index[lane] : 0]), j);
  return f == SPX_JOB_OK ? 0 : lane_fail(lane, spx_job_fault_text(f));
}

// A lane's rate by spx_batch_run_rate's rule, in its words, with the lane and the rate in front
static int lane_rate_check(const spx_pipeline* p, int lane, float rate) {
  if (spx_internal_rate_check(p->plans[0], rate) == 0) return 0;
  return lane_fail(lane, "rate " + std::to_string(rate) + ": " + spx_last_error());
}

static int pipeline_build(spx_pipeline* p) {
  const int n = p->n;
  PCHK(hipGetDevice(&p->device));
  // the pipeline's own output layout: capacity per stream as spx_plan_out_capacity_for (a rate pipeline: _rate, FINAL frames at the
  // rate the lane is sized for), regions at 64-byte boundaries
  int64_t oo = 0;
  size_t in_values = 0;
  std::vector<int64_t> tab((size_t)2 * n);
  std::vector<int> chans((size_t)n);
  p->static_offsets.resize((size_t)n + 1);
  for (int i = 0; i < n; i++) {
    spx_stream_job& j = p->jobs[i];
    j.out_off = j.out_cap = 0;   // (the caller's are not read: the pipeline lays its own output out below)
    if (lane_check(p, i, j)) return -1;
    spx_plan_t pl = p->plans[p->mixed ? p->plan_index[i] : 0];
    if (p->rate_kind && lane_rate_check(p, i, p->rates[i])) return -1;
    j.out_cap = p->rate_kind ? spx_plan_out_capacity_rate(pl, j.n_in, j.speed, j.nonlinear, p->rates[i])
                             : spx_plan_out_capacity_for(pl, j.n_in, j.speed, j.nonlinear);
    if (j.out_cap < 0) return lane_fail(i, spx_last_error());
    j.out_off = oo;
    p->static_offsets[i] = oo;
    tab[i] = oo; tab[(size_t)n + i] = j.out_cap; chans[i] = j.channels;
    oo += (j.out_cap * j.channels + (PIPE_ALIGN - 1)) & ~(int64_t)(PIPE_ALIGN - 1);
    const size_t end = (size_t)j.in_off + (size_t)j.n_in * j.channels;
    if (end > in_values) in_values = end;
  }
  p->static_offsets[n] = oo;
  p->in_values = in_values;
  p->out_values = (size_t)oo;
  // (a rate pipeline: the rate call's workspace with the TSM staging of EVERY lane, also of those sized for rate 1 -- any lane may
  // resample in some batch; it begins with the plain call's workspace, which is what a batch of ones runs in)
  p->ws_bytes = p->mixed ? spx_batch_workspace_bytes_mixed(p->plans.data(), (int)p->plans.size(), p->jobs.data(), p->plan_index.data(), n)
                         : (p->rate_kind ? spx_internal_rate_workspace_all(p->plans[0], p->jobs.data(), n)
                                         : spx_batch_workspace_bytes(p->plans[0], p->jobs.data(), n));
  if (!p->ws_bytes) return -1;
  PCHK(hipStreamCreateWithFlags(&p->s_run, hipStreamNonBlocking));
  PCHK(hipStreamCreateWithFlags(&p->s_h2d, hipStreamNonBlocking));
  const size_t tab_bytes = (size_t)n * (2 * sizeof(int64_t) + sizeof(int));
  PCHK(spx_dev_alloc(&p->d_tab, tab_bytes));
  PCHK(hipMemcpy(p->d_tab, tab.data(), (size_t)n * 2 * sizeof(int64_t), hipMemcpyHostToDevice));
  PCHK(hipMemcpy(reinterpret_cast<unsigned char*>(p->d_tab) + (size_t)n * 2 * sizeof(int64_t), chans.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  p->slots.resize((size_t)p->depth);
  const bool host_out = !(p->flags & SPX_PIPELINE_DEVICE_OUT);
  const bool flt = (p->flags & SPX_PIPELINE_FLOAT) != 0;
  for (auto& S : p->slots) {
    // (d_in: allocated by the first submit of host memory -- a caller whose input is device-resident never needs it)
    // (cleared once as always; under spx_debug_set_alloc_fill filled with its byte instead: spx_dev_alloc)
    PCHK(spx_dev_alloc(&S.d_out, (p->out_values + 64) * sizeof(int16_t), true));
    PCHK(spx_dev_alloc(&S.d_nout, (size_t)n * sizeof(int64_t), true));
    PCHK(spx_dev_alloc(&S.d_offsets, ((size_t)n + 1) * sizeof(int64_t)));
    PCHK(spx_dev_alloc(&S.ws, p->ws_bytes, true));
    if (host_out) {
      if (flt) PCHK(hipHostMalloc(reinterpret_cast<void**>(&S.h_outf), (p->out_values + 64) * sizeof(float), hipHostMallocDefault));
      else PCHK(hipHostMalloc(reinterpret_cast<void**>(&S.h_out), (p->out_values + 64) * sizeof(int16_t), hipHostMallocDefault));
      PCHK(hipHostMalloc(reinterpret_cast<void**>(&S.h_meta), ((size_t)2 * n + 1) * sizeof(int64_t), hipHostMallocDefault));
    }
    if (flt) {
      // the int16 staging the engine reads, + 64 values as always, zeroed once (the conversion writes the jobs' values only)
      PCHK(spx_dev_alloc(&S.d_in, (p->in_values + 64) * sizeof(int16_t), true));
      PCHK(hipHostMalloc(&S.h_cv, spx_conv_table_bytes(n), hipHostMallocDefault));
      PCHK(spx_dev_alloc(&S.d_cv, spx_conv_table_bytes(n)));
      if (!host_out) {
        PCHK(spx_dev_alloc(&S.d_outf, (p->out_values + 64) * sizeof(float), true));
      }
    }
    PCHK(hipEventCreateWithFlags(&S.ev_in, hipEventDisableTiming));
    PCHK(hipEventCreateWithFlags(&S.ev_done, hipEventDisableTiming));
  }
  PCHK(hipDeviceSynchronize());   // the memsets above ran on the null stream; the pipeline's streams do not wait for it
  return 0;
}

extern "C" {

spx_pipeline_t spx_pipeline_create_mixed(const spx_plan_t* plans, int n_plans, const spx_stream_job* jobs, const int* plan_index,
                                         int n_streams, int depth, unsigned flags) {
  if (!plans || n_plans < 1 || n_plans > 8 || !jobs || n_streams < 1 || depth < 0 || depth == 1 || depth > SPX_PIPE_MAX_DEPTH) {
    pfail(-1, "spx_pipeline_create: bad arguments (depth 0 or 2 .. 8)");
    return nullptr;
  }
  spx_pipeline* p = new spx_pipeline();
  p->plans.assign(plans, plans + n_plans);
  p->mixed = plan_index != nullptr || n_plans > 1;
  if (p->mixed) {
    p->plan_index.resize((size_t)n_streams, 0);
    for (int i = 0; i < n_streams; i++) {
      p->plan_index[i] = plan_index ? plan_index[i] : 0;
      if (p->plan_index[i] < 0 || p->plan_index[i] >= n_plans) { delete p; pfail(-1, "spx_pipeline_create: plan_index out of range"); return nullptr; }
    }
  }
  p->n = n_streams;
  p->depth = depth ? depth : 4;
  p->flags = flags;
  p->jobs.assign(jobs, jobs + n_streams);
  if (pipeline_build(p)) { pipeline_free(p); return nullptr; }
  return p;
}
spx_pipeline_t spx_pipeline_create(spx_plan_t plan, const spx_stream_job* jobs, int n_streams, int depth, unsigned flags) {
  if (!plan) { pfail(-1, "spx_pipeline_create: no plan"); return nullptr; }
  return spx_pipeline_create_mixed(&plan, 1, jobs, nullptr, n_streams, depth, flags);
}
spx_pipeline_t spx_pipeline_create_rate(spx_plan_t plan, const spx_stream_job* jobs, const float* rates, int n_streams, int depth,
                                        unsigned flags) {
  if (!plan) { pfail(-1, "spx_pipeline_create_rate: no plan"); return nullptr; }
  if (!jobs || n_streams < 1 || depth < 0 || depth == 1 || depth > SPX_PIPE_MAX_DEPTH) {
    pfail(-1, "spx_pipeline_create_rate: bad arguments (depth 0 or 2 .. 8)");
    return nullptr;
  }
  spx_pipeline* p = new spx_pipeline();
  p->plans.assign(1, plan);
  p->rate_kind = true;
  if (rates) p->rates.assign(rates, rates + n_streams);
  else p->rates.assign((size_t)n_streams, 1.0f);
  p->n = n_streams;
  p->depth = depth ? depth : 4;
  p->flags = flags;
  p->jobs.assign(jobs, jobs + n_streams);
  if (pipeline_build(p)) { pipeline_free(p); return nullptr; }
  return p;
}
void spx_pipeline_destroy(spx_pipeline_t p) { pipeline_free(p); }
int spx_pipeline_depth(spx_pipeline_t p) { return p ? p->depth : 0; }
size_t spx_pipeline_input_values(spx_pipeline_t p) { return p ? p->in_values : 0; }

int16_t* spx_pipeline_host_input(spx_pipeline_t p) {
  if (!p) return nullptr;
  if (wrong_kind(p, false, "spx_pipeline_host_input")) return nullptr;
  SpxPipeSlot& S = p->slots[(size_t)(p->next_ticket % p->depth)];
  if (!S.h_in) {
    if (hipHostMalloc(reinterpret_cast<void**>(&S.h_in), (p->in_values + 64) * sizeof(int16_t), hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      pfail(-2, "spx_pipeline_host_input: pinned allocation failed");
      return nullptr;
    }
  }
  if (S.in_recorded && hipEventSynchronize(S.ev_in) != hipSuccess) { (void)hipGetLastError(); return nullptr; }   // the copy that last read it
  return S.h_in;
}
float* spx_pipeline_host_input_float(spx_pipeline_t p) {
  if (!p) return nullptr;
  if (wrong_kind(p, true, "spx_pipeline_host_input_float")) return nullptr;
  SpxPipeSlot& S = p->slots[(size_t)(p->next_ticket % p->depth)];
  if (!S.h_inf) {
    if (hipHostMalloc(reinterpret_cast<void**>(&S.h_inf), (p->in_values + 16) * sizeof(float), hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      pfail(-2, "spx_pipeline_host_input_float: pinned allocation failed");
      return nullptr;
    }
  }
  if (S.in_recorded && hipEventSynchronize(S.ev_in) != hipSuccess) { (void)hipGetLastError(); return nullptr; }   // the copy that last read it
  return S.h_inf;
}

}  // extern "C"

// SPX_PIPELINE_FLOAT: what a submit enqueues on the copy stream in place of the int16 copy -- the copy of a host input into the float
// staging, this batch's conversion table, the conversion into the int16 staging -- with ev_in recorded behind the conversion.
static int pipeline_float_input(spx_pipeline_t p, SpxPipeSlot& S, size_t extent, const float* in, int in_is_device, int* max_out) {
  // (the slot's pinned table was last read by a kernel in front of an ev_in that the batch behind ev_done waited for: free to rewrite)
  int max_in = 1;
  if (spx_conv_table_fill(S.h_cv, S.jobs.data(), p->n, &max_in, max_out)) return pfail(-1, "spx_pipeline: a lane too large for one conversion launch");
  const float* src = in;
  if (!in_is_device) {
    if (!S.d_inf) PCHK(spx_dev_alloc_on(&S.d_inf, (p->in_values + 16) * sizeof(float), p->s_h2d, false, false));   // (+ 16: never empty)
    if (extent) PCHK(hipMemcpyAsync(S.d_inf, in, extent * sizeof(float), hipMemcpyHostToDevice, p->s_h2d));
    src = S.d_inf;
  }
  spx_conv_table_upload(S.h_cv, S.d_cv, p->n, p->s_h2d);
  spx_conv_launch_in(S.d_cv, p->n, max_in, src, S.d_in, p->s_h2d);
  PCHK(hipEventRecord(S.ev_in, p->s_h2d));
  S.in_recorded = true;
  return 0;
}

// One batch with the table `jobs` (the pipeline's own layout in it) and `extent` values of input: int16, or float on a pipeline
// created with SPX_PIPELINE_FLOAT.
// rates (a rate pipeline's batch; null = every rate 1): a batch of ones takes the overlapped order every pipeline batch takes; with one
// rate other than 1 the engine runs the batch as spx_batch_run_rate does -- general walk kernel into the TSM staging of the slot's
// workspace, rate kernel into the slot's d_out, kernels in sequence on the run stream behind ev_in -- and the tails follow unchanged.
static int64_t pipeline_submit(spx_pipeline_t p, const spx_stream_job* jobs, const float* rates, size_t extent, const void* in_any,
                               int in_is_device) {
  const bool flt = (p->flags & SPX_PIPELINE_FLOAT) != 0;
  bool resample = false;
  for (int i = 0; rates && i < p->n; i++) resample = resample || rates[i] != 1.0f;
  const int16_t* in = flt ? nullptr : static_cast<const int16_t*>(in_any);
  const int64_t ticket = p->next_ticket;
  SpxPipeSlot& S = p->slots[(size_t)(ticket % p->depth)];
  // at most `depth` batches in flight: the batch that last used this buffer set has finished (its output, if nobody asked for
  // it, is dropped here)
  if (S.ticket >= 0) PCHK(hipEventSynchronize(S.ev_done));
  S.jobs.assign(jobs, jobs + p->n);
  const int16_t* dev_in = in;
  void* in_ready = nullptr;
  int cv_max_out = 1;
  if (flt) {
    const int frc = pipeline_float_input(p, S, extent, static_cast<const float*>(in_any), in_is_device, &cv_max_out);
    if (frc) { (void)hipDeviceSynchronize(); (void)hipGetLastError(); S.ticket = -1; return frc; }
    dev_in = S.d_in;
    in_ready = S.ev_in;
  } else if (!in_is_device) {
    // (the kernels that last read d_in are behind ev_done, waited for above: the copy may start at once)
    // ONE copy stream: with two taking turns -- so that the next 82 MB copy starts while the previous one still runs and the
    // 50 - 80 us between two chained copies go -- the leg read 1.73 - 1.75 ms per batch against 1.67 (profiles/r05/r5o_copy_streams.txt).
    if (!S.d_in) {
      // + 64 values behind the input: the walk kernels' aligned window refill may read a few frames past a stream's end; zeroed
      // once, never written again
      PCHK(spx_dev_alloc_on(&S.d_in, (p->in_values + 64) * sizeof(int16_t), p->s_h2d, true, false));
    }
    // (this batch's extent only: what lies behind it in d_in -- an earlier batch's samples -- is padding no lane of this batch reads)
    if (extent) PCHK(hipMemcpyAsync(S.d_in, in, extent * sizeof(int16_t), hipMemcpyHostToDevice, p->s_h2d));
    PCHK(hipEventRecord(S.ev_in, p->s_h2d));
    S.in_recorded = true;
    dev_in = S.d_in;
    in_ready = S.ev_in;
  }
  int rc;
  const bool host_out = !(p->flags & SPX_PIPELINE_DEVICE_OUT);
  // With the outputs left on the device nothing of a batch has to run behind its walk kernel: the call is DETACHED from the run
  // stream (spx_engine.hip SpxCallOpts) -- the batch's event is recorded on the walk stream itself and the run stream stays empty.
  // (SPX_PIPELINE_FLOAT | SPX_PIPELINE_DEVICE_OUT: the output conversion runs behind the walk kernel on the run stream, so the call
  // cannot be detached from it and takes the order the host-output pipeline takes)
  bool event_recorded = false;
  const bool detach = !host_out && !flt;
  const SpxCall call = {p->plans[0], S.jobs.data(), p->n, dev_in, S.d_out, S.d_nout, S.ws, p->ws_bytes, nullptr, p->s_run};
  if (resample) {
    // (never detached: the rate kernel ends the call on the run stream, where the slot's event is recorded below.  The rates are read
    // before the call returns: they reach the device inside the SpxRateJob records, through the engine's staging kernel)
    rc = spx_internal_run_rate(call, rates, in_ready, nullptr);
  } else if (p->mixed) {
    // (round 6: detached like a one-plan batch -- the groups' walk kernels on the library's walk streams, two calls' worth in flight)
    rc = spx_internal_run_mixed(p->plans.data(), (int)p->plans.size(), S.jobs.data(), p->plan_index.data(), p->n, dev_in, S.d_out, S.d_nout,
                                S.ws, p->ws_bytes, p->s_run, true, in_ready, detach ? S.ev_done : nullptr, detach);
    event_recorded = detach;
  } else {
    rc = spx_internal_run(call, true, true, in_ready, detach ? S.ev_done : nullptr, detach);
    event_recorded = detach;
  }
  if (rc) {
    // part of the batch may have been enqueued on this buffer set: nothing of it is handed out, and nothing is left in flight
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    S.ticket = -1;
    return rc;
  }
  S.in_host = flt || !in_is_device;   // (a float input of either kind is consumed by its conversion, in front of ev_in)
  if (host_out) {
    const int n = p->n;
    const int64_t* d_off = p->d_tab;
    const int64_t* d_cap = p->d_tab + n;
    const int* d_ch = reinterpret_cast<const int*>(p->d_tab + 2 * (size_t)n);
    hipLaunchKernelGGL(spx_pipe_offsets_kernel, dim3(1), dim3(256), 0, p->s_run, S.d_nout, d_ch, d_cap, n, S.d_offsets, S.h_meta, S.h_meta + n + 1);
    const int wgs = n < p->pack_wgs ? n : p->pack_wgs;
    if (flt) hipLaunchKernelGGL(spx_pipe_copy_float_kernel, dim3(wgs), dim3(256), 0, p->s_run, S.d_out, d_off, S.d_offsets, n, S.h_outf);
    else hipLaunchKernelGGL(spx_pipe_copy_kernel, dim3(wgs), dim3(256), 0, p->s_run, S.d_out, d_off, S.d_offsets, n, S.h_out);
  } else if (flt) {
    // (the table went to the device on the copy stream in front of ev_in, which every kernel of the batch is behind; said once more
    // for the run stream, whatever order the engine chose)
    PCHK(hipStreamWaitEvent(p->s_run, S.ev_in, 0));
    spx_conv_launch_out(S.d_cv, p->n, cv_max_out, S.d_nout, S.d_out, S.d_outf, p->s_run);
  }
  if (!event_recorded) PCHK(hipEventRecord(S.ev_done, p->s_run));
  PCHK(hipGetLastError());
  S.ticket = ticket;
  p->next_ticket++;
  return ticket;
}

// Does the caller's table fit the pipeline?  0 with `table` = the caller's jobs in the pipeline's own output layout and `extent` =
// the int16 values of input the batch reads, or -1 with the lane and the limit in spx_last_error.  Host arithmetic only.
// The limits are the pipeline's own: the lane's channel count, the input buffer, the lane's output capacity, the workspace.
// A job's VALUES are judged by the engine's rules (lane_check: spx_jobs.h, the rules every batch call applies at its top), asked
// here per lane so that the message names the lane and comes before the wait for the buffer set and the copy in.
// rates (a rate pipeline only; null = every rate 1): each one spx_batch_run_rate takes, the capacity rule in FINAL frames
// (spx_plan_out_capacity_rate at THIS batch's rate against the lane's capacity at creation -- the inequality itself, not "rate >=
// creation rate": rate_ratio halves both sample rates to 14 bits, so the capacity is not promised monotone in the rate), and the
// workspace rule against spx_batch_workspace_bytes_rate of the table with these rates.
static int pipeline_check(spx_pipeline_t p, const spx_stream_job* jobs, const float* rates, std::vector<spx_stream_job>& table, size_t* extent) {
  const int n = p->n;
  table.assign(jobs, jobs + n);
  size_t ext = 0;
  for (int i = 0; i < n; i++) {
    spx_stream_job& j = table[i];
    const spx_stream_job& c = p->jobs[i];
    if (j.channels != c.channels)
      return lane_fail(i, std::to_string(j.channels) + " channels, the lane was created with " + std::to_string(c.channels));
    j.out_off = c.out_off;
    j.out_cap = c.out_cap;
    if (lane_check(p, i, j)) return -1;
    if (rates && lane_rate_check(p, i, rates[i])) return -1;
    if ((uint64_t)j.in_off > p->in_values || (uint64_t)j.n_in * (uint64_t)j.channels > p->in_values - (uint64_t)j.in_off)
      return lane_fail(i, "in_off " + std::to_string(j.in_off) + " + n_in " + std::to_string(j.n_in) + " x " + std::to_string(j.channels) +
                              " channels ends behind the pipeline's input of " + std::to_string(p->in_values) + " values (spx_pipeline_input_values)");
    const size_t end = (size_t)j.in_off + (size_t)j.n_in * (size_t)j.channels;
    if (end > ext) ext = end;
    if (rates && rates[i] != 1.0f) {
      const int64_t fin = spx_plan_out_capacity_rate(p->plans[0], j.n_in, j.speed, j.nonlinear, rates[i]);
      if (fin < 0) return lane_fail(i, spx_last_error());
      if (fin > c.out_cap)
        return lane_fail(i, "n_in " + std::to_string(j.n_in) + " at speed " + std::to_string(j.speed) + (j.nonlinear != 0.0f ? " nonlinear" : " linear") +
                                " and rate " + std::to_string(rates[i]) + " needs an output capacity of " + std::to_string(fin) +
                                " final frames (spx_plan_out_capacity_rate), the lane was created with " + std::to_string(c.out_cap));
      continue;
    }
    const int64_t need = spx_plan_out_capacity_for(p->plans[p->mixed ? p->plan_index[i] : 0], j.n_in, j.speed, j.nonlinear);
    if (need > c.out_cap)
      return lane_fail(i, "n_in " + std::to_string(j.n_in) + " at speed " + std::to_string(j.speed) + (j.nonlinear != 0.0f ? " nonlinear" : " linear") +
                              " needs an output capacity of " + std::to_string(need) + " frames (spx_plan_out_capacity_for), the lane was created with " +
                              std::to_string(c.out_cap));
  }
  const size_t ws = p->mixed ? spx_batch_workspace_bytes_mixed(p->plans.data(), (int)p->plans.size(), table.data(), p->plan_index.data(), n)
                             : (rates ? spx_batch_workspace_bytes_rate(p->plans[0], table.data(), rates, n)
                                      : spx_batch_workspace_bytes(p->plans[0], table.data(), n));
  if (!ws) return -1;   // (the engine could not lay the table out: its own message stands)
  if (ws > p->ws_bytes && rates) {
    // a rate batch's workspace also holds the speed stage's output of the lanes that resample: name the first lane that has more
    // analysis frames, or more speed-stage frames to stage, than it was created with
    int lane = 0;
    for (int i = 0; i < n; i++) {
      const spx_stream_job &j = table[i], &c = p->jobs[i];
      const int64_t now = j.nonlinear != 0.0f ? spx_plan_frames(p->plans[0], j.n_in) : 0;
      const int64_t then = c.nonlinear != 0.0f ? spx_plan_frames(p->plans[0], c.n_in) : 0;
      if (now > then || spx_plan_out_capacity_for(p->plans[0], j.n_in, j.speed, j.nonlinear) > spx_plan_out_capacity_for(p->plans[0], c.n_in, c.speed, c.nonlinear)) { lane = i; break; }
    }
    return lane_fail(lane, "more analysis frames or more speed-stage frames to resample than the lane was created with: the batch needs a workspace of " +
                               std::to_string(ws) + " bytes (spx_batch_workspace_bytes_rate), the pipeline's holds " + std::to_string(p->ws_bytes));
  }
  if (ws > p->ws_bytes) {
    // the workspace grows with the analysis frames of the nonlinear lanes: name the first lane that has more of them than it was created with
    int lane = 0;
    for (int i = 0; i < n; i++) {
      spx_plan_t pl = p->plans[p->mixed ? p->plan_index[i] : 0];
      const int64_t now = table[i].nonlinear != 0.0f ? spx_plan_frames(pl, table[i].n_in) : 0;
      const int64_t then = p->jobs[i].nonlinear != 0.0f ? spx_plan_frames(pl, p->jobs[i].n_in) : 0;
      if (now > then) { lane = i; break; }
    }
    return lane_fail(lane, "more analysis frames than the lane was created with (a linear lane turned nonlinear, or a longer one): the batch needs a workspace of " +
                               std::to_string(ws) + " bytes (spx_batch_workspace_bytes), the pipeline's holds " + std::to_string(p->ws_bytes));
  }
  *extent = ext;
  return 0;
}
static int pipeline_current(spx_pipeline_t p, const char* who) {
  int cur = 0;
  if (hipGetDevice(&cur) == hipSuccess && cur != p->device) return pfail(-1, std::string(who) + ": the pipeline's device is not the current one");
  return 0;
}

extern "C" {

int64_t spx_pipeline_submit(spx_pipeline_t p, const int16_t* in, int in_is_device) {
  if (!p || !in) return pfail(-1, "spx_pipeline_submit: bad arguments");
  if (wrong_kind(p, false, "spx_pipeline_submit") || pipeline_current(p, "spx_pipeline_submit")) return -1;
  return pipeline_submit(p, p->jobs.data(), p->rate_kind ? p->rates.data() : nullptr, p->in_values, in, in_is_device);
}
static int float_aligned(const float* in, const char* who) {
  if (reinterpret_cast<uintptr_t>(in) & 3) return pfail(-1, std::string(who) + ": in must be 4-byte aligned");
  return 0;
}
int64_t spx_pipeline_submit_float(spx_pipeline_t p, const float* in, int in_is_device) {
  if (!p || !in) return pfail(-1, "spx_pipeline_submit_float: bad arguments");
  if (wrong_kind(p, true, "spx_pipeline_submit_float") || float_aligned(in, "spx_pipeline_submit_float") ||
      pipeline_current(p, "spx_pipeline_submit_float")) return -1;
  return pipeline_submit(p, p->jobs.data(), p->rate_kind ? p->rates.data() : nullptr, p->in_values, in, in_is_device);
}
int spx_pipeline_jobs_fit(spx_pipeline_t p, const spx_stream_job* jobs) {
  if (!p || !jobs) return pfail(-1, "spx_pipeline_jobs_fit: bad arguments");
  std::vector<spx_stream_job> table;
  size_t extent = 0;
  return pipeline_check(p, jobs, nullptr, table, &extent);
}
int64_t spx_pipeline_submit_jobs(spx_pipeline_t p, const spx_stream_job* jobs, const int16_t* in, int in_is_device) {
  if (!p || !jobs || !in) return pfail(-1, "spx_pipeline_submit_jobs: bad arguments");
  if (wrong_kind(p, false, "spx_pipeline_submit_jobs") || pipeline_current(p, "spx_pipeline_submit_jobs")) return -1;
  std::vector<spx_stream_job> table;
  size_t extent = 0;
  if (pipeline_check(p, jobs, nullptr, table, &extent)) return -1;   // (before anything is waited for, copied or enqueued: no ticket is used up)
  return pipeline_submit(p, table.data(), nullptr, extent, in, in_is_device);
}
int64_t spx_pipeline_submit_jobs_float(spx_pipeline_t p, const spx_stream_job* jobs, const float* in, int in_is_device) {
  if (!p || !jobs || !in) return pfail(-1, "spx_pipeline_submit_jobs_float: bad arguments");
  if (wrong_kind(p, true, "spx_pipeline_submit_jobs_float") || float_aligned(in, "spx_pipeline_submit_jobs_float") ||
      pipeline_current(p, "spx_pipeline_submit_jobs_float")) return -1;
  std::vector<spx_stream_job> table;
  size_t extent = 0;
  if (pipeline_check(p, jobs, nullptr, table, &extent)) return -1;
  return pipeline_submit(p, table.data(), nullptr, extent, in, in_is_device);
}

// ---- the _rate calls: a rate pipeline's batch with its own rate per lane (rates == NULL: every rate 1) ----
static int rate_pipeline_only(const spx_pipeline* p, const char* who) {
  if (p->rate_kind) return 0;
  return pfail(-1, std::string(who) + ": the pipeline takes no playback rates: create it with spx_pipeline_create_rate");
}
int spx_pipeline_jobs_fit_rate(spx_pipeline_t p, const spx_stream_job* jobs, const float* rates) {
  if (!p || !jobs) return pfail(-1, "spx_pipeline_jobs_fit_rate: bad arguments");
  if (rate_pipeline_only(p, "spx_pipeline_jobs_fit_rate")) return -1;
  std::vector<spx_stream_job> table;
  size_t extent = 0;
  return pipeline_check(p, jobs, rates, table, &extent);
}
int64_t spx_pipeline_submit_jobs_rate(spx_pipeline_t p, const spx_stream_job* jobs, const float* rates, const int16_t* in, int in_is_device) {
  if (!p || !jobs || !in) return pfail(-1, "spx_pipeline_submit_jobs_rate: bad arguments");
  if (rate_pipeline_only(p, "spx_pipeline_submit_jobs_rate") || wrong_kind(p, false, "spx_pipeline_submit_jobs_rate") ||
      pipeline_current(p, "spx_pipeline_submit_jobs_rate")) return -1;
  std::vector<spx_stream_job> table;
  size_t extent = 0;
  if (pipeline_check(p, jobs, rates, table, &extent)) return -1;   // (before anything is waited for, copied or enqueued: no ticket is used up)
  return pipeline_submit(p, table.data(), rates, extent, in, in_is_device);
}
int64_t spx_pipeline_submit_jobs_rate_float(spx_pipeline_t p, const spx_stream_job* jobs, const float* rates, const float* in, int in_is_device) {
  if (!p || !jobs || !in) return pfail(-1, "spx_pipeline_submit_jobs_rate_float: bad arguments");
  if (rate_pipeline_only(p, "spx_pipeline_submit_jobs_rate_float") || wrong_kind(p, true, "spx_pipeline_submit_jobs_rate_float") ||
      float_aligned(in, "spx_pipeline_submit_jobs_rate_float") || pipeline_current(p, "spx_pipeline_submit_jobs_rate_float")) return -1;
  std::vector<spx_stream_job> table;
  size_t extent = 0;
  if (pipeline_check(p, jobs, rates, table, &extent)) return -1;
  return pipeline_submit(p, table.data(), rates, extent, in, in_is_device);
}

static SpxPipeSlot* slot_of(spx_pipeline_t p, int64_t ticket) {
  if (!p || ticket < 0 || ticket >= p->next_ticket) return nullptr;
  SpxPipeSlot& S = p->slots[(size_t)(ticket % p->depth)];
  return S.ticket == ticket ? &S : nullptr;
}
int spx_pipeline_input_consumed(spx_pipeline_t p, int64_t ticket) {
  SpxPipeSlot* S = slot_of(p, ticket);
  if (!S) return pfail(-1, "spx_pipeline_input_consumed: unknown ticket, or its buffers have been handed to a later batch");
  // host input: the copy in has read it; device input: the kernels read it until the batch is done (the walk kernel copies from it);
  // a float input of either kind: its conversion, in front of ev_in, has read it (in_host is set for both)
  if (S->in_host) PCHK(hipEventSynchronize(S->ev_in));
  else PCHK(hipEventSynchronize(S->ev_done));
  return 0;
}
int spx_pipeline_wait(spx_pipeline_t p, int64_t ticket, const int16_t** out, const int64_t** offsets, const int64_t** counts) {
  if (p && wrong_kind(p, false, "spx_pipeline_wait")) return -1;
  SpxPipeSlot* S = slot_of(p, ticket);
  if (!S) return pfail(-1, "spx_pipeline_wait: unknown ticket, or its buffers have been handed to a later batch");
  PCHK(hipEventSynchronize(S->ev_done));
  const bool host_out = !(p->flags & SPX_PIPELINE_DEVICE_OUT);
  if (out) *out = host_out ? S->h_out : S->d_out;
  if (offsets) *offsets = host_out ? S->h_meta : p->static_offsets.data();
  if (counts) *counts = host_out ? S->h_meta + p->n + 1 : S->d_nout;
  return 0;
}

int spx_pipeline_wait_float(spx_pipeline_t p, int64_t ticket, const float** out, const int64_t** offsets, const int64_t** counts) {
  if (p && wrong_kind(p, true, "spx_pipeline_wait_float")) return -1;
  SpxPipeSlot* S = slot_of(p, ticket);
  if (!S) return pfail(-1, "spx_pipeline_wait_float: unknown ticket, or its buffers have been handed to a later batch");
  PCHK(hipEventSynchronize(S->ev_done));
  const bool host_out = !(p->flags & SPX_PIPELINE_DEVICE_OUT);
  if (out) *out = host_out ? S->h_outf : S->d_outf;
  if (offsets) *offsets = host_out ? S->h_meta : p->static_offsets.data();
  if (counts) *counts = host_out ? S->h_meta + p->n + 1 : S->d_nout;
  return 0;
}

void* spx_host_alloc(size_t bytes) {
  void* q = nullptr;
  if (hipHostMalloc(&q, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); pfail(-2, "spx_host_alloc failed"); return nullptr; }
  return q;
}
void spx_host_free(void* q) { if (q) (void)hipHostFree(q); }

}  // extern "C"
