/* The rate pipeline as a program: plain C99 over include/speedy_hip.h, no HIP headers.
 *
 *   pipeline_rate_example IN.raw RATE CHANNELS SPEED NONLINEAR PLAYBACK_RATE [PLAYBACK_RATE ...]
 *
 * IN.raw = interleaved int16 PCM.  A pipeline of one lane per PLAYBACK_RATE (spx_pipeline_create_rate), every lane holding the
 * same utterance, runs TWO batches: the first with the rates as given, the second with the list reversed -- a lane's rate changes
 * from one batch to the next, so every lane is created with the smaller of its two rates (the larger capacity).  Prints one line
 * per lane and batch:
 *   batch B stream I rate R frames N crc32 XXXXXXXX
 * (CRC-32 of the lane's int16 output bytes, the zlib polynomial).  Exit code 0 = ok.
 * Used by tests/test_gpu_pipeline_rate.py::test_c_example_prints_the_oracles_counts_and_crcs. */
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
  int16_t* utterance = (int16_t*)malloc((size_t)bytes + 2);
  if (fread(utterance, 1, (size_t)bytes, f) != (size_t)bytes) { fprintf(stderr, "short read\n"); return 1; }
  fclose(f);
  const int64_t n_in = bytes / 2 / channels;
  const size_t lane_values = (size_t)n_in * (size_t)channels;

  spx_plan_t plan = spx_plan_create(rate, /*match_matlab=*/0);
  if (!plan) { fprintf(stderr, "spx_plan_create: %s\n", spx_last_error()); return 2; }
  spx_stream_job* jobs = (spx_stream_job*)calloc((size_t)n, sizeof(spx_stream_job));
  float* rates[2];
  float* sized_for = (float*)calloc((size_t)n, sizeof(float));
  rates[0] = (float*)calloc((size_t)n, sizeof(float));
  rates[1] = (float*)calloc((size_t)n, sizeof(float));
  for (int i = 0; i < n; i++) {
    rates[0][i] = (float)atof(argv[6 + i]);
    rates[1][n - 1 - i] = rates[0][i];
  }
  for (int i = 0; i < n; i++) {
    /* the pipeline lays the outputs out itself (out_off / out_cap are not read); lane i's input starts at in_off */
    jobs[i].in_off = (int64_t)((size_t)i * lane_values);
    jobs[i].n_in = n_in;
    jobs[i].channels = channels;
    jobs[i].speed = speed;
    jobs[i].nonlinear = nonlinear;
    jobs[i].feedback = 0.0f;
    /* sizing advice of the header: the smallest rate the lane will see */
    sized_for[i] = rates[0][i] < rates[1][i] ? rates[0][i] : rates[1][i];
  }
  spx_pipeline_t pipe = spx_pipeline_create_rate(plan, jobs, sized_for, n, /*depth=*/2, 0u);
  if (!pipe) { fprintf(stderr, "spx_pipeline_create_rate: %s\n", spx_last_error()); return 2; }
  if (spx_pipeline_input_values(pipe) != (size_t)n * lane_values) { fprintf(stderr, "unexpected input size\n"); return 3; }

  int64_t tickets[2];
  for (int b = 0; b < 2; b++) {
    /* the pinned staging of the NEXT submit: both batches are in flight before the first is waited for */
    int16_t* host_in = spx_pipeline_host_input(pipe);
    if (!host_in) { fprintf(stderr, "spx_pipeline_host_input: %s\n", spx_last_error()); return 2; }
    for (int i = 0; i < n; i++) memcpy(host_in + (size_t)i * lane_values, utterance, lane_values * sizeof(int16_t));
    CHECK(spx_pipeline_jobs_fit_rate(pipe, jobs, rates[b]));
    tickets[b] = spx_pipeline_submit_jobs_rate(pipe, jobs, rates[b], host_in, /*in_is_device=*/0);
    if (tickets[b] != b) { fprintf(stderr, "spx_pipeline_submit_jobs_rate: ticket %lld: %s\n", (long long)tickets[b], spx_last_error()); return 2; }
  }
  for (int b = 0; b < 2; b++) {
    const int16_t* out;
    const int64_t *offsets, *counts;
    CHECK(spx_pipeline_wait(pipe, tickets[b], &out, &offsets, &counts));
    for (int i = 0; i < n; i++) {
      if (counts[i] < 0) { fprintf(stderr, "batch %d stream %d: output capacity exceeded\n", b, i); return 3; }
      printf("batch %d stream %d rate %g frames %lld crc32 %08x\n", b, i, (double)rates[b][i], (long long)counts[i],
             (unsigned)crc32_of((const unsigned char*)(out + offsets[i]), (size_t)counts[i] * (size_t)channels * sizeof(int16_t)));
    }
  }
  spx_pipeline_destroy(pipe);
  spx_plan_destroy(plan);
  free(jobs); free(rates[0]); free(rates[1]); free(sized_for); free(utterance);
  return 0;
}
