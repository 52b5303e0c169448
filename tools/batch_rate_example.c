/* spx_batch_run_rate as a program: plain C99 over include/speedy_hip.h, no HIP headers.
 *
 *   batch_rate_example IN.raw RATE CHANNELS SPEED NONLINEAR PLAYBACK_RATE [PLAYBACK_RATE ...]
 *
 * IN.raw = interleaved int16 PCM.  The utterance is submitted once per PLAYBACK_RATE as the independent streams of ONE call,
 * each with its own sonicSetRate value (1 = the stream spx_batch_run would produce).  Prints one line per stream:
 *   stream I rate R frames N crc32 XXXXXXXX
 * (CRC-32 of the stream's int16 output bytes, the zlib polynomial).  Exit code 0 = ok.
 * Used by tests/test_gpu_batch_rate.py::test_c_example_prints_the_oracles_counts_and_crcs. */
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

static uint32_t crc32_of(const unsigned char* p, size_t n) {
  uint32_t c = 0xffffffffu;
  for (size_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
  }
  return ~c;
}

int main(int argc, char** argv) {
  if (argc < 7) {
    fprintf(stderr, "usage: %s IN.raw RATE CHANNELS SPEED NONLINEAR PLAYBACK_RATE [PLAYBACK_RATE ...]\n", argv[0]);
    return 1;
  }
  const int rate = atoi(argv[2]), channels = atoi(argv[3]), n = argc - 6;
  const float speed = (float)atof(argv[4]), nonlinear = (float)atof(argv[5]);
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
  spx_stream_job* jobs = (spx_stream_job*)calloc((size_t)n, sizeof(spx_stream_job));
  float* rates = (float*)calloc((size_t)n, sizeof(float));
  int64_t out_values = 0;
  for (int i = 0; i < n; i++) {
    rates[i] = (float)atof(argv[6 + i]);
    /* the capacity counts FINAL frames: what the rate stage can make of the speed stage's output */
    const int64_t cap = spx_plan_out_capacity_rate(plan, n_in, speed, nonlinear, rates[i]);
    if (cap < 0) { fprintf(stderr, "stream %d: %s\n", i, spx_last_error()); return 2; }
    jobs[i].in_off = 0; /* every stream reads the same utterance */
    jobs[i].n_in = n_in;
    jobs[i].out_off = out_values;
    jobs[i].out_cap = cap;
    jobs[i].channels = channels;
    jobs[i].speed = speed;
    jobs[i].nonlinear = nonlinear;
    jobs[i].feedback = 0.0f;
    out_values += cap * channels;
  }
  const size_t in_bytes = (size_t)n_in * (size_t)channels * sizeof(int16_t);
  const size_t wsb = spx_batch_workspace_bytes_rate(plan, jobs, rates, n);
  if (wsb == 0) { fprintf(stderr, "spx_batch_workspace_bytes_rate: %s\n", spx_last_error()); return 2; }
  void* ws = spx_device_alloc(wsb);
  int16_t* d_in = (int16_t*)spx_device_alloc(in_bytes + 128);
  int16_t* d_out = (int16_t*)spx_device_alloc((size_t)out_values * sizeof(int16_t) + 16);
  int64_t* d_nout = (int64_t*)spx_device_alloc((size_t)n * sizeof(int64_t));
  if (!ws || !d_in || !d_out || !d_nout) { fprintf(stderr, "device allocation failed\n"); return 2; }
  CHECK(spx_copy_to_device(d_in, host_in, in_bytes, NULL));
  CHECK(spx_batch_run_rate(plan, jobs, rates, n, d_in, d_out, d_nout, ws, wsb, NULL, NULL));
  int64_t* host_nout = (int64_t*)malloc((size_t)n * sizeof(int64_t));
  int16_t* host_out = (int16_t*)malloc((size_t)out_values * sizeof(int16_t) + 2);
  CHECK(spx_copy_to_host(host_nout, d_nout, (size_t)n * sizeof(int64_t), NULL));
  CHECK(spx_copy_to_host(host_out, d_out, (size_t)out_values * sizeof(int16_t), NULL));
  CHECK(spx_stream_synchronize(NULL));
  for (int i = 0; i < n; i++) {
    if (host_nout[i] < 0) { fprintf(stderr, "stream %d: output capacity exceeded\n", i); return 3; }
    printf("stream %d rate %g frames %lld crc32 %08x\n", i, (double)rates[i], (long long)host_nout[i],
           (unsigned)crc32_of((const unsigned char*)(host_out + jobs[i].out_off),
                              (size_t)host_nout[i] * (size_t)channels * sizeof(int16_t)));
  }
  spx_device_free(ws); spx_device_free(d_in); spx_device_free(d_out); spx_device_free(d_nout);
  spx_plan_destroy(plan);
  free(jobs); free(rates); free(host_in); free(host_nout); free(host_out);
  return 0;
}
