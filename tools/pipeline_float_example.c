/* The pipeline object on float samples as a program: plain C99 over include/speedy_hip.h, no HIP headers.
 *
 *   pipeline_float_example IN.wav OUT.f32 SPEED NONLINEAR
 *
 * IN.wav = 16-bit PCM.  Its samples are scaled to float (v / 32768.0f, exact) -- the float32 a decoding loader would hold in host
 * memory -- written into the pipeline's pinned float staging and run as the ONE lane of a pipeline created with SPX_PIPELINE_FLOAT,
 * through spx_pipeline_submit_jobs_float; both conversions happen on the GPU.  OUT.f32 receives the float output, interleaved, raw
 * little-endian float32.  Prints
 *   rate R channels C frames_in N frames_out M
 * Exit code 0 = ok.  Used by tests/test_gpu_pipeline_float.py::test_c_example_writes_the_oracles_float_stream. */
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

static uint32_t le32(const unsigned char* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static unsigned le16(const unsigned char* p) { return (unsigned)p[0] | ((unsigned)p[1] << 8); }

/* The "fmt " and "data" chunks of a RIFF/WAVE file held in memory: 0, or -1 for anything but 16-bit PCM. */
static int parse_wav(const unsigned char* b, size_t n, int* rate, int* channels, const unsigned char** data, size_t* data_bytes) {
  size_t pos = 12;
  int have_fmt = 0;
  if (n < 12 || memcmp(b, "RIFF", 4) != 0 || memcmp(b + 8, "WAVE", 4) != 0) return -1;
  while (pos + 8 <= n) {
    const size_t len = le32(b + pos + 4);
    const unsigned char* body = b + pos + 8;
    if (memcmp(b + pos, "fmt ", 4) == 0 && len >= 16 && pos + 8 + 16 <= n) {
      if (le16(body) != 1 || le16(body + 14) != 16) return -1;
      *channels = (int)le16(body + 2);
      *rate = (int)le32(body + 4);
      have_fmt = 1;
    } else if (memcmp(b + pos, "data", 4) == 0) {
      if (!have_fmt) return -1;
      *data = body;
      *data_bytes = len <= n - (pos + 8) ? len : n - (pos + 8);
      return 0;
    }
    pos += 8 + len + (len & 1);
  }
  return -1;
}

int main(int argc, char** argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: %s IN.wav OUT.f32 SPEED NONLINEAR\n", argv[0]);
    return 1;
  }
  const float speed = (float)atof(argv[3]), nonlinear = (float)atof(argv[4]);
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  unsigned char* file = (unsigned char*)malloc((size_t)bytes + 1);
  if (fread(file, 1, (size_t)bytes, f) != (size_t)bytes) { fprintf(stderr, "short read\n"); return 1; }
  fclose(f);
  int rate = 0, channels = 0;
  const unsigned char* pcm = NULL;
  size_t pcm_bytes = 0;
  if (parse_wav(file, (size_t)bytes, &rate, &channels, &pcm, &pcm_bytes) != 0 || channels < 1) {
    fprintf(stderr, "%s: not a 16-bit PCM WAV file\n", argv[1]);
    return 1;
  }
  const int64_t n_in = (int64_t)(pcm_bytes / 2 / (size_t)channels);
  const size_t in_values = (size_t)n_in * (size_t)channels;

  spx_plan_t plan = spx_plan_create(rate, /*match_matlab=*/0);
  if (!plan) { fprintf(stderr, "spx_plan_create: %s\n", spx_last_error()); return 2; }
  /* the table is the int16 pipeline's: in_off counts float values here; the pipeline lays the output out itself */
  spx_stream_job job;
  memset(&job, 0, sizeof(job));
  job.in_off = 0;
  job.n_in = n_in;
  job.channels = channels;
  job.speed = speed;
  job.nonlinear = nonlinear;
  job.feedback = 0.0f;
  spx_pipeline_t pipe = spx_pipeline_create(plan, &job, 1, /*depth=*/2, SPX_PIPELINE_FLOAT);
  if (!pipe) { fprintf(stderr, "spx_pipeline_create: %s\n", spx_last_error()); return 2; }
  if (spx_pipeline_input_values(pipe) != in_values) { fprintf(stderr, "unexpected input size\n"); return 3; }
  /* an int16 call on a float pipeline is refused and uses up no ticket */
  if (spx_pipeline_host_input(pipe) != NULL) { fprintf(stderr, "the int16 staging of a float pipeline was handed out\n"); return 3; }
  float* host_in = spx_pipeline_host_input_float(pipe);
  if (!host_in) { fprintf(stderr, "spx_pipeline_host_input_float: %s\n", spx_last_error()); return 2; }
  for (size_t i = 0; i < in_values; i++) {
    const unsigned u = le16(pcm + 2 * i);
    const int v = u >= 32768u ? (int)u - 65536 : (int)u;
    host_in[i] = (float)v / 32768.0f;
  }
  CHECK(spx_pipeline_jobs_fit(pipe, &job));
  const int64_t ticket = spx_pipeline_submit_jobs_float(pipe, &job, host_in, /*in_is_device=*/0);
  if (ticket != 0) { fprintf(stderr, "spx_pipeline_submit_jobs_float: ticket %lld: %s\n", (long long)ticket, spx_last_error()); return 2; }
  const float* out;
  const int64_t *offsets, *counts;
  CHECK(spx_pipeline_wait_float(pipe, ticket, &out, &offsets, &counts));
  const int64_t n_out = counts[0];
  if (n_out < 0) { fprintf(stderr, "output capacity exceeded\n"); return 3; }
  const size_t got = (size_t)n_out * (size_t)channels;
  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror(argv[2]); return 1; }
  for (size_t i = 0; i < got; i++) {
    uint32_t u;
    unsigned char le[4];
    memcpy(&u, out + offsets[0] + i, 4);
    le[0] = (unsigned char)(u & 255u); le[1] = (unsigned char)((u >> 8) & 255u);
    le[2] = (unsigned char)((u >> 16) & 255u); le[3] = (unsigned char)(u >> 24);
    if (fwrite(le, 1, 4, o) != 4) { fprintf(stderr, "short write\n"); return 1; }
  }
  fclose(o);
  printf("rate %d channels %d frames_in %lld frames_out %lld\n", rate, channels, (long long)n_in, (long long)n_out);
  spx_pipeline_destroy(pipe);
  spx_plan_destroy(plan);
  free(file);
  return 0;
}
