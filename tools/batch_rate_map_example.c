/* spx_batch_run_rate_map as a program: plain C99 over include/speedy_hip.h, no HIP headers.
 *
 *   batch_rate_map_example IN.raw RATE CHANNELS SPEED NONLINEAR PLAYBACK_RATE T0 T1
 *
 * IN.raw = interleaved int16 PCM: one clip, compressed at SPEED and played at PLAYBACK_RATE (sonicSetRate; 1.25 in the tests) in one
 * call that also writes the clip's time map.  T0 and T1 are two caption times in INPUT frames.  Prints
 *   frames N                        the clip's final count (n_out)
 *   row K V                         every row of the map, in FINAL frames -- the unit of the output buffer
 *   caption I in T out U back V     spx_map_lookup forward (T -> U, where the caption lands in the output) and inverse (U -> V)
 * Exit code 0 = ok.  Used by tests/test_gpu_time_map_rate.py. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "speedy_hip.h"

#define CHECK(call)                                                \
  do {                                                             \
    if ((call) != 0) {                                             \
      fprintf(stderr, "%s failed: %s\n", #call, spx_last_error()); \
      return 2;                                                    \
    }                                                              \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 9) {
    fprintf(stderr, "usage: %s IN.raw RATE CHANNELS SPEED NONLINEAR PLAYBACK_RATE T0 T1\n", argv[0]);
    return 1;
  }
  const int rate = atoi(argv[2]), channels = atoi(argv[3]);
  const float speed = (float)atof(argv[4]), nonlinear = (float)atof(argv[5]);
  float rates[1];
  int64_t captions[2];
  rates[0] = (float)atof(argv[6]);
  captions[0] = (int64_t)atoll(argv[7]);
  captions[1] = (int64_t)atoll(argv[8]);
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  int16_t* host_in = (int16_t*)malloc((size_t)bytes + 2);
  if (fread(host_in, 1, (size_t)bytes, f) != (size_t)bytes) { fprintf(stderr, "short read\n"); return 1; }
  fclose(f);
  const int64_t n_in = bytes / 2 / channels;

  spx_plan_t plan = spx_plan_create(rate, /*match_matlab=*/0);
  if (!plan) { fprintf(stderr, "spx_plan_create: %s\n", spx_last_error()); return 2; }
  spx_stream_job job;
  /* the capacity counts FINAL frames, and so will the map's rows */
  const int64_t cap = spx_plan_out_capacity_rate(plan, n_in, speed, nonlinear, rates[0]);
  const int64_t rows = spx_plan_map_rows(plan, n_in, nonlinear);
  if (cap < 0 || rows < 0) { fprintf(stderr, "%s\n", spx_last_error()); return 2; }
  job.in_off = 0;
  job.n_in = n_in;
  job.out_off = 0;
  job.out_cap = cap;
  job.channels = channels;
  job.speed = speed;
  job.nonlinear = nonlinear;
  job.feedback = 0.0f;
  const size_t in_bytes = (size_t)n_in * (size_t)channels * sizeof(int16_t);
  const size_t wsb = spx_batch_workspace_bytes_rate(plan, &job, rates, 1);
  if (wsb == 0) { fprintf(stderr, "spx_batch_workspace_bytes_rate: %s\n", spx_last_error()); return 2; }
  void* ws = spx_device_alloc(wsb);
  int16_t* d_in = (int16_t*)spx_device_alloc(in_bytes + 128);
  int16_t* d_out = (int16_t*)spx_device_alloc((size_t)cap * (size_t)channels * sizeof(int16_t) + 16);
  int64_t* d_nout = (int64_t*)spx_device_alloc(sizeof(int64_t));
  int64_t* d_map = (int64_t*)spx_device_alloc((size_t)rows * sizeof(int64_t));
  int64_t* d_q = (int64_t*)spx_device_alloc(6 * sizeof(int64_t)); /* q_off[2] | q[2] | r[2] */
  if (!ws || !d_in || !d_out || !d_nout || !d_map || !d_q) { fprintf(stderr, "device allocation failed\n"); return 2; }
  CHECK(spx_copy_to_device(d_in, host_in, in_bytes, NULL));
  CHECK(spx_batch_run_rate_map(plan, &job, rates, 1, d_in, d_out, d_nout, d_map, ws, wsb, NULL, NULL));

  int64_t host_nout = 0;
  int64_t* host_map = (int64_t*)malloc((size_t)rows * sizeof(int64_t));
  CHECK(spx_copy_to_host(&host_nout, d_nout, sizeof(int64_t), NULL));
  CHECK(spx_copy_to_host(host_map, d_map, (size_t)rows * sizeof(int64_t), NULL));
  CHECK(spx_stream_synchronize(NULL));
  if (host_nout < 0) { fprintf(stderr, "output capacity exceeded\n"); return 3; }
  printf("frames %lld\n", (long long)host_nout);
  for (int64_t k = 0; k < rows; k++) printf("row %lld %lld\n", (long long)k, (long long)host_map[k]);

  /* the captions: input frames -> final output frames, and back */
  int64_t q[4], fwd[2], back[2];
  q[0] = 0; q[1] = 2; q[2] = captions[0]; q[3] = captions[1];
  CHECK(spx_copy_to_device(d_q, q, sizeof(q), NULL));
  CHECK(spx_map_lookup(plan, &job, 1, d_map, d_q, d_q + 2, d_q + 4, /*inverse=*/0, NULL));
  CHECK(spx_copy_to_host(fwd, d_q + 4, sizeof(fwd), NULL));
  CHECK(spx_stream_synchronize(NULL));
  CHECK(spx_copy_to_device(d_q + 2, fwd, sizeof(fwd), NULL));
  CHECK(spx_map_lookup(plan, &job, 1, d_map, d_q, d_q + 2, d_q + 4, /*inverse=*/1, NULL));
  CHECK(spx_copy_to_host(back, d_q + 4, sizeof(back), NULL));
  CHECK(spx_stream_synchronize(NULL));
  for (int i = 0; i < 2; i++)
    printf("caption %d in %lld out %lld back %lld\n", i, (long long)captions[i], (long long)fwd[i], (long long)back[i]);

  spx_device_free(ws); spx_device_free(d_in); spx_device_free(d_out); spx_device_free(d_nout); spx_device_free(d_map);
  spx_device_free(d_q);
  spx_plan_destroy(plan);
  free(host_in); free(host_map);
  return 0;
}
