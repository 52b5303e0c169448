/* spx_batch_dtw as a program: plain C99 over include/speedy_hip.h, no HIP headers.
 *
 *   batch_dtw_example IN.raw RATE SPEED NONLINEAR [HALF_WIDTH]
 *
 * IN.raw = mono int16 PCM; NONLINEAR in (0, 1] (the spectrogram tap belongs to the nonlinear path).  Audits one stream on the
 * device: spx_batch_run compresses it with the spectrogram tap on, spx_batch_analyze takes the same tap of the OUTPUT, and
 * spx_batch_dtw aligns the two taps where they lie -- row stride N = spx_plan_fft_size, the low N / 4 bins of every row, as the
 * reference's ComputeSpectrogram keeps them (sonic_test.cc:211-240).  Only the output's length and the 24 bytes of the result come
 * back to the host.  Prints
 *   rows A B        analysis frames of the input and of the output
 *   cost C          accumulated cost of the best warp path
 *   slope S         least-squares slope of the path (output rows per input row: about 1 / SPEED)
 *   local_mean M    mean and
 *   local_std D     deviation of the slopes of windows of 2 * HALF_WIDTH path entries
 *   n_path P        entries of the path
 *   n_local W       windows
 * Exit code 0 = ok.  Used by tests/test_gpu_dtw.py. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "speedy_hip.h"

#define CHECK(call)                                                \
  do {                                                             \
    if ((call) != 0) {                                             \
      fprintf(stderr, "%s failed: %s\n", #call, spx_last_error()); \
      return 2;                                                    \
    }                                                              \
  } while (0)

static int16_t* read_raw(const char* path, long* bytes) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); return NULL; }
  fseek(f, 0, SEEK_END);
  *bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  int16_t* p = (int16_t*)malloc((size_t)*bytes + 2);
  if (!p || fread(p, 1, (size_t)*bytes, f) != (size_t)*bytes) { fprintf(stderr, "%s: short read\n", path); fclose(f); free(p); return NULL; }
  fclose(f);
  return p;
}

int main(int argc, char** argv) {
  if (argc != 5 && argc != 6) {
    fprintf(stderr, "usage: %s IN.raw RATE SPEED NONLINEAR [HALF_WIDTH]\n", argv[0]);
    return 1;
  }
  const int rate = atoi(argv[2]);
  const float speed = (float)atof(argv[3]), nonlinear = (float)atof(argv[4]);
  const int half_width = argc == 6 ? atoi(argv[5]) : 10;
  long bytes = 0;
  int16_t* x = read_raw(argv[1], &bytes);
  if (!x) return 1;
  if (nonlinear == 0.0f) { fprintf(stderr, "NONLINEAR must not be 0: a linear job has no analysis frames\n"); return 1; }
  const int64_t n_in = bytes / 2;

  spx_plan_t plan = spx_plan_create(rate, /*match_matlab=*/0);
  if (!plan) { fprintf(stderr, "spx_plan_create: %s\n", spx_last_error()); return 2; }
  const int N = spx_plan_fft_size(plan);
  const int64_t cap = spx_plan_out_capacity_for(plan, n_in, speed, nonlinear);
  const int64_t rows_in = spx_plan_frames(plan, n_in);
  spx_stream_job job;
  job.in_off = 0;
  job.n_in = n_in;
  job.out_off = 0;
  job.out_cap = cap;
  job.channels = 1;
  job.speed = speed;
  job.nonlinear = nonlinear;
  job.feedback = 0.0f;
  /* the output is analysed as a stream of its own: at most `cap` frames, so its tap and workspace are sized for that */
  spx_stream_job job_out = job;
  job_out.n_in = cap;
  const int64_t rows_cap = spx_plan_frames(plan, cap);
  const size_t wsb_in = spx_batch_workspace_bytes(plan, &job, 1), wsb_cap = spx_batch_workspace_bytes(plan, &job_out, 1);
  const size_t wsb = wsb_in > wsb_cap ? wsb_in : wsb_cap;
  void* ws = spx_device_alloc(wsb);
  int16_t* d_in = (int16_t*)spx_device_alloc((size_t)n_in * sizeof(int16_t) + 128);    /* window loads: 64 values of padding */
  int16_t* d_out = (int16_t*)spx_device_alloc((size_t)cap * sizeof(int16_t) + 128);    /* (it is an input too, further down) */
  int64_t* d_nout = (int64_t*)spx_device_alloc(sizeof(int64_t));
  float* d_spec_in = (float*)spx_device_alloc((size_t)(rows_in > 0 ? rows_in : 1) * (size_t)N * sizeof(float));
  float* d_spec_out = (float*)spx_device_alloc((size_t)(rows_cap > 0 ? rows_cap : 1) * (size_t)N * sizeof(float));
  if (!ws || !d_in || !d_out || !d_nout || !d_spec_in || !d_spec_out) { fprintf(stderr, "device allocation failed\n"); return 2; }
  CHECK(spx_copy_to_device(d_in, x, (size_t)n_in * sizeof(int16_t), NULL));

  spx_taps taps;
  memset(&taps, 0, sizeof(taps));
  taps.spectrogram = d_spec_in;
  CHECK(spx_batch_run(plan, &job, 1, d_in, d_out, d_nout, ws, wsb, &taps, NULL));
  int64_t n_out = 0;
  CHECK(spx_copy_to_host(&n_out, d_nout, sizeof(n_out), NULL));
  CHECK(spx_stream_synchronize(NULL));
  if (n_out < 0) { fprintf(stderr, "output capacity exceeded\n"); return 3; }

  job_out.n_in = n_out;
  const int64_t rows_out = spx_plan_frames(plan, n_out);
  if (rows_in < 1 || rows_out < 1) { fprintf(stderr, "too short: %lld and %lld analysis frames\n", (long long)rows_in, (long long)rows_out); return 3; }
  taps.spectrogram = d_spec_out;
  CHECK(spx_batch_analyze(plan, &job_out, 1, d_out, ws, wsb, &taps, NULL));

  spx_dtw_job pair;
  pair.a_off = 0;
  pair.b_off = 0;
  pair.path_off = 0;
  pair.n_a = (int32_t)rows_in;
  pair.n_b = (int32_t)rows_out;
  const int dim = N / 4;
  const size_t dtw_wsb = spx_dtw_workspace_bytes(&pair, 1, dim);
  if (!dtw_wsb) { fprintf(stderr, "spx_dtw_workspace_bytes: %s\n", spx_last_error()); return 2; }
  void* dtw_ws = spx_device_alloc(dtw_wsb);
  spx_dtw_result* d_res = (spx_dtw_result*)spx_device_alloc(sizeof(spx_dtw_result));
  int32_t* d_path = (int32_t*)spx_device_alloc((size_t)(rows_in + rows_out - 1) * 2 * sizeof(int32_t));
  if (!dtw_ws || !d_res || !d_path) { fprintf(stderr, "device allocation failed\n"); return 2; }
  CHECK(spx_batch_dtw(plan, &pair, 1, dim, /*ld_a=*/N, /*ld_b=*/N, half_width, d_spec_in, d_spec_out, d_res, d_path, dtw_ws, dtw_wsb, NULL));
  spx_dtw_result res;
  CHECK(spx_copy_to_host(&res, d_res, sizeof(res), NULL));
  CHECK(spx_stream_synchronize(NULL));

  printf("rows %lld %lld\n", (long long)rows_in, (long long)rows_out);
  printf("cost %.9g\n", (double)res.cost);
  printf("slope %.9g\n", (double)res.slope);
  printf("local_mean %.9g\n", (double)res.local_mean);
  printf("local_std %.9g\n", (double)res.local_std);
  printf("n_path %d\n", (int)res.n_path);
  printf("n_local %d\n", (int)res.n_local);

  spx_device_free(ws); spx_device_free(d_in); spx_device_free(d_out); spx_device_free(d_nout); spx_device_free(d_spec_in);
  spx_device_free(d_spec_out); spx_device_free(dtw_ws); spx_device_free(d_res); spx_device_free(d_path);
  spx_plan_destroy(plan);
  free(x);
  return 0;
}
