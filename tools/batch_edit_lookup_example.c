/* spx_edit_index and spx_edit_lookup as a program: plain C99 over include/speedy_hip.h, no HIP headers.
 *
 *   batch_edit_lookup_example KEY.raw RATE CHANNELS SPEED NONLINEAR CUE [CUE ...]
 *
 * KEY.raw = interleaved int16 PCM; every CUE an input frame (a word's start, a caption cue, a cut point).  One call compresses the
 * recording and records its edit list, one builds the list's index, one lookup takes the cues forward -- the output frame at which
 * each is first heard, to the sample -- and one takes those answers back to the input frame each plays.  Nothing but the printed
 * numbers comes back to the host.  Prints
 *   frames N ops K
 *   cue P out O rec R back P2          one line per cue: R = the record of the edit list that emits output frame O (-1: behind the
 *                                      end), P2 = the input frame output frame O plays (>= P: P itself, or the first surviving
 *                                      audio behind it)
 * Exit code 0 = ok.  Used by tests/test_gpu_edit_lookup.py. */
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
  if (argc < 7) {
    fprintf(stderr, "usage: %s KEY.raw RATE CHANNELS SPEED NONLINEAR CUE [CUE ...]\n", argv[0]);
    return 1;
  }
  const int rate = atoi(argv[2]), kc = atoi(argv[3]);
  const float speed = (float)atof(argv[4]), nonlinear = (float)atof(argv[5]);
  const int n_cues = argc - 6;
  long kbytes = 0;
  int16_t* key = read_raw(argv[1], &kbytes);
  if (!key || kc < 1) return 1;
  const int64_t n_in = kbytes / 2 / kc;

  spx_plan_t plan = spx_plan_create(rate, /*match_matlab=*/0);
  if (!plan) { fprintf(stderr, "spx_plan_create: %s\n", spx_last_error()); return 2; }
  const int64_t cap = spx_plan_out_capacity_for(plan, n_in, speed, nonlinear);
  const int64_t ops_cap = spx_plan_edit_ops(plan, n_in, speed, nonlinear);
  if (ops_cap < 0) { fprintf(stderr, "spx_plan_edit_ops: %s\n", spx_last_error()); return 2; }
  spx_stream_job job;
  job.in_off = 0;
  job.n_in = n_in;
  job.out_off = 0;
  job.out_cap = cap;
  job.channels = kc;
  job.speed = speed;
  job.nonlinear = nonlinear;
  job.feedback = 0.0f;
  const size_t key_bytes = (size_t)n_in * (size_t)kc * sizeof(int16_t);
  const size_t wsb = spx_batch_workspace_bytes(plan, &job, 1);
  const size_t n_rec = (size_t)(ops_cap > 0 ? ops_cap : 1), q_bytes = (size_t)n_cues * sizeof(int64_t);
  void* ws = spx_device_alloc(wsb);
  int16_t* d_key = (int16_t*)spx_device_alloc(key_bytes + 128);   /* the walk kernel's window loads: 64 values of padding */
  int16_t* d_out = (int16_t*)spx_device_alloc((size_t)cap * (size_t)kc * sizeof(int16_t) + 16);
  int64_t* d_counts = (int64_t*)spx_device_alloc(2 * sizeof(int64_t)); /* n_out | n_ops */
  spx_edit_op* d_ops = (spx_edit_op*)spx_device_alloc(n_rec * sizeof(spx_edit_op));
  int32_t* d_index = (int32_t*)spx_device_alloc(n_rec * sizeof(int32_t));
  int64_t* d_qoff = (int64_t*)spx_device_alloc(2 * sizeof(int64_t));
  int64_t* d_cue = (int64_t*)spx_device_alloc(q_bytes);
  int64_t* d_fwd = (int64_t*)spx_device_alloc(q_bytes);
  int64_t* d_back = (int64_t*)spx_device_alloc(q_bytes);
  int32_t* d_rec = (int32_t*)spx_device_alloc((size_t)n_cues * sizeof(int32_t));
  int64_t* cue = (int64_t*)malloc(q_bytes);
  int64_t* fwd = (int64_t*)malloc(q_bytes);
  int64_t* back = (int64_t*)malloc(q_bytes);
  int32_t* rec = (int32_t*)malloc((size_t)n_cues * sizeof(int32_t));
  if (!ws || !d_key || !d_out || !d_counts || !d_ops || !d_index || !d_qoff || !d_cue || !d_fwd || !d_back || !d_rec || !cue || !fwd ||
      !back || !rec) {
    fprintf(stderr, "allocation failed\n");
    return 2;
  }
  for (int i = 0; i < n_cues; i++) cue[i] = (int64_t)atoll(argv[6 + i]);
  int64_t q_off[2];
  q_off[0] = 0;
  q_off[1] = n_cues;
  CHECK(spx_copy_to_device(d_key, key, key_bytes, NULL));
  CHECK(spx_copy_to_device(d_qoff, q_off, sizeof(q_off), NULL));
  CHECK(spx_copy_to_device(d_cue, cue, q_bytes, NULL));

  /* the job and its list; the index over the list; the cues forward, with their records; the answers back */
  CHECK(spx_batch_run_edits(plan, &job, 1, d_key, d_out, d_counts, d_ops, &ops_cap, d_counts + 1, ws, wsb, NULL, NULL));
  CHECK(spx_edit_index(plan, &job, 1, d_ops, &ops_cap, d_counts + 1, d_index, NULL));
  CHECK(spx_edit_lookup(plan, &job, 1, d_ops, &ops_cap, d_counts + 1, d_counts, d_index, d_qoff, d_cue, d_fwd, d_rec, /*inverse=*/0, NULL));
  CHECK(spx_edit_lookup(plan, &job, 1, d_ops, &ops_cap, d_counts + 1, d_counts, NULL, d_qoff, d_fwd, d_back, NULL, /*inverse=*/1, NULL));

  int64_t counts[2];
  CHECK(spx_copy_to_host(counts, d_counts, sizeof(counts), NULL));
  CHECK(spx_copy_to_host(fwd, d_fwd, q_bytes, NULL));
  CHECK(spx_copy_to_host(back, d_back, q_bytes, NULL));
  CHECK(spx_copy_to_host(rec, d_rec, (size_t)n_cues * sizeof(int32_t), NULL));
  CHECK(spx_stream_synchronize(NULL));
  if (counts[0] < 0) { fprintf(stderr, "output capacity exceeded\n"); return 3; }
  if (counts[1] < 0) { fprintf(stderr, "the edit list has %lld records, the capacity holds %lld\n", (long long)-counts[1], (long long)ops_cap); return 3; }
  printf("frames %lld ops %lld\n", (long long)counts[0], (long long)counts[1]);
  for (int i = 0; i < n_cues; i++)
    printf("cue %lld out %lld rec %d back %lld\n", (long long)cue[i], (long long)fwd[i], (int)rec[i], (long long)back[i]);

  spx_device_free(ws); spx_device_free(d_key); spx_device_free(d_out); spx_device_free(d_counts); spx_device_free(d_ops);
  spx_device_free(d_index); spx_device_free(d_qoff); spx_device_free(d_cue); spx_device_free(d_fwd); spx_device_free(d_back);
  spx_device_free(d_rec);
  spx_plan_destroy(plan);
  free(key); free(cue); free(fwd); free(back); free(rec);
  return 0;
}
