/* spx_batch_run_twopass as a program: plain C99 over include/speedy_hip.h, no HIP headers.
 *
 *   batch_twopass_example IN.raw RATE CHANNELS NONLINEAR TARGET [TARGET ...]
 *
 * IN.raw = interleaved int16 PCM.  The utterance is submitted once per TARGET as the independent streams of ONE call:
 *   TARGET = lSECONDS   length mode: the stream is brought to SECONDS of audio (speedy_wave --length SECONDS)
 *   TARGET = mSPEED     match mode: the final pass runs at the speed a nonlinear pass at SPEED achieves
 *                       (speedy_wave --match_nonlinear --speed SPEED; NONLINEAR 0 gives the linear control)
 * Prints one line per stream:
 *   stream I probe P speed XXXXXXXX frames N crc32 XXXXXXXX
 * (the probe pass's count, the second-pass speed's float bits, the final count, CRC-32 of the int16 output bytes).
 * Exit code 0 = ok.  Used by tests/test_gpu_twopass.py::test_c_example. */
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
  if (argc < 6) {
    fprintf(stderr, "usage: %s IN.raw RATE CHANNELS NONLINEAR lSECONDS|mSPEED [...]\n", argv[0]);
    return 1;
  }
  const int rate = atoi(argv[2]), channels = atoi(argv[3]), n = argc - 5;
  const float nonlinear = (float)atof(argv[4]);
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
  double* seconds = (double*)calloc((size_t)n, sizeof(double));
  int64_t out_values = 0;
  for (int i = 0; i < n; i++) {
    const char* t = argv[5 + i];
    double want;
    if (t[0] == 'l') {
      seconds[i] = atof(t + 1);
      /* the speed the probe pass runs at: the call works it out the same way */
      want = (double)((float)n_in / (float)rate) / seconds[i];
    } else if (t[0] == 'm') {
      seconds[i] = 0.0;
      want = atof(t + 1);
    } else {
      fprintf(stderr, "target %s: lSECONDS or mSPEED\n", t);
      return 1;
    }
    /* one capacity for both passes: the probe's output passes through the same buffer */
    const int64_t cap = spx_plan_out_capacity_twopass(plan, n_in, want, nonlinear);
    if (cap < 0) { fprintf(stderr, "stream %d: %s\n", i, spx_last_error()); return 2; }
    jobs[i].in_off = 0; /* every stream reads the same utterance */
    jobs[i].n_in = n_in;
    jobs[i].out_off = out_values;
    jobs[i].out_cap = cap;
    jobs[i].channels = channels;
    jobs[i].speed = (float)want; /* read in match mode only */
    jobs[i].nonlinear = nonlinear;
    jobs[i].feedback = 0.0f;
    out_values += cap * channels;
  }
  const size_t in_bytes = (size_t)n_in * (size_t)channels * sizeof(int16_t);
  const size_t wsb = spx_batch_workspace_bytes_twopass(plan, jobs, seconds, n);
  if (wsb == 0) { fprintf(stderr, "spx_batch_workspace_bytes_twopass: %s\n", spx_last_error()); return 2; }
  void* ws = spx_device_alloc(wsb);
  int16_t* d_in = (int16_t*)spx_device_alloc(in_bytes + 128);
  int16_t* d_out = (int16_t*)spx_device_alloc((size_t)out_values * sizeof(int16_t) + 16);
  int64_t* d_nout = (int64_t*)spx_device_alloc((size_t)n * sizeof(int64_t));
  int64_t* d_probe = (int64_t*)spx_device_alloc((size_t)n * sizeof(int64_t));
  float* d_speeds = (float*)spx_device_alloc((size_t)n * sizeof(float));
  if (!ws || !d_in || !d_out || !d_nout || !d_probe || !d_speeds) { fprintf(stderr, "device allocation failed\n"); return 2; }
  CHECK(spx_copy_to_device(d_in, host_in, in_bytes, NULL));
  /* both passes and the speed between them: one call, nothing comes back to the host in between */
  CHECK(spx_batch_run_twopass(plan, jobs, seconds, n, d_in, d_out, d_nout, d_probe, d_speeds, ws, wsb, NULL, NULL));
  int64_t* host_nout = (int64_t*)malloc((size_t)n * sizeof(int64_t));
  int64_t* host_probe = (int64_t*)malloc((size_t)n * sizeof(int64_t));
  float* host_speeds = (float*)malloc((size_t)n * sizeof(float));
  int16_t* host_out = (int16_t*)malloc((size_t)out_values * sizeof(int16_t) + 2);
  CHECK(spx_copy_to_host(host_nout, d_nout, (size_t)n * sizeof(int64_t), NULL));
  CHECK(spx_copy_to_host(host_probe, d_probe, (size_t)n * sizeof(int64_t), NULL));
  CHECK(spx_copy_to_host(host_speeds, d_speeds, (size_t)n * sizeof(float), NULL));
  CHECK(spx_copy_to_host(host_out, d_out, (size_t)out_values * sizeof(int16_t), NULL));
  CHECK(spx_stream_synchronize(NULL));
  for (int i = 0; i < n; i++) {
    uint32_t bits;
    if (host_nout[i] < 0) { fprintf(stderr, "stream %d: output capacity exceeded\n", i); return 3; }
    memcpy(&bits, &host_speeds[i], sizeof(bits));
    printf("stream %d probe %lld speed %08x frames %lld crc32 %08x\n", i, (long long)host_probe[i], (unsigned)bits,
           (long long)host_nout[i],
           (unsigned)crc32_of((const unsigned char*)(host_out + jobs[i].out_off),
                              (size_t)host_nout[i] * (size_t)channels * sizeof(int16_t)));
  }
  spx_device_free(ws); spx_device_free(d_in); spx_device_free(d_out); spx_device_free(d_nout);
  spx_device_free(d_probe); spx_device_free(d_speeds);
  spx_plan_destroy(plan);
  free(jobs); free(seconds); free(host_in); free(host_nout); free(host_probe); free(host_speeds); free(host_out);
  return 0;
}
