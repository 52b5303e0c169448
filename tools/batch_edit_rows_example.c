/* spx_edit_warp_rows and spx_edit_unwarp_rows as a program: plain C99 over include/speedy_hip.h, no HIP headers.
 *
 *   batch_edit_rows_example KEY.raw RATE SPEED NONLINEAR LABELS.i32 FEATURES.f32 DIM
 *
 * KEY.raw = mono int16 PCM; LABELS.i32 = one int32 label per 160 key frames (a phone or word id per 10 ms at 16 kHz), on the
 * recording's own timeline; FEATURES.f32 = one row of DIM floats per 160 key frames.  One call compresses the recording and records
 * its edit list; one warp brings the labels onto the output's timeline (nearest row), one the features (rows inside a cross-fade
 * are the cross-fade of their two source rows); the index is built, and one unwarp takes the warped labels back onto the
 * recording's timeline.  Rows stand for the frame in their middle (phase 80).  Prints
 *   frames N ops K
 *   labels rows R sum S              R = spx_edit_rows(N, 160, 80) rows on the output's timeline, S their sum
 *   features rows R bits X           X = the sum of the rows' float bit patterns, modulo 2^64
 *   back rows Q sum S2 same M        Q = spx_edit_rows(L, 160, 80) rows back on the input's timeline, M of them the original label
 * Exit code 0 = ok.  Used by tests/test_gpu_edit_rows.py. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "speedy_hip.h"

#define HOP 160
#define PHASE 80

#define CHECK(call)                                                \
  do {                                                             \
    if ((call) != 0) {                                             \
      fprintf(stderr, "%s failed: %s\n", #call, spx_last_error()); \
      return 2;                                                    \
    }                                                              \
  } while (0)

static void* read_raw(const char* path, long* bytes) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); return NULL; }
  fseek(f, 0, SEEK_END);
  *bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  void* p = malloc((size_t)*bytes + 8);
  if (!p || fread(p, 1, (size_t)*bytes, f) != (size_t)*bytes) { fprintf(stderr, "%s: short read\n", path); fclose(f); free(p); return NULL; }
  fclose(f);
  return p;
}

int main(int argc, char** argv) {
  if (argc != 8) {
    fprintf(stderr, "usage: %s KEY.raw RATE SPEED NONLINEAR LABELS.i32 FEATURES.f32 DIM\n", argv[0]);
    return 1;
  }
  const int rate = atoi(argv[2]), dim = atoi(argv[7]);
  const float speed = (float)atof(argv[3]), nonlinear = (float)atof(argv[4]);
  long kbytes = 0, lbytes = 0, fbytes = 0;
  int16_t* key = (int16_t*)read_raw(argv[1], &kbytes);
  int32_t* labels = (int32_t*)read_raw(argv[5], &lbytes);
  float* feats = (float*)read_raw(argv[6], &fbytes);
  if (!key || !labels || !feats || dim < 1) return 1;
  const int64_t n_in = kbytes / 2;
  const int64_t label_rows = lbytes / 4, feat_rows = fbytes / 4 / dim;

  spx_plan_t plan = spx_plan_create(rate, /*match_matlab=*/0);
  if (!plan) { fprintf(stderr, "spx_plan_create: %s\n", spx_last_error()); return 2; }
  const int64_t cap = spx_plan_out_capacity_for(plan, n_in, speed, nonlinear);
  const int64_t ops_cap = spx_plan_edit_ops(plan, n_in, speed, nonlinear);
  if (ops_cap < 0) { fprintf(stderr, "spx_plan_edit_ops: %s\n", spx_last_error()); return 2; }
  const int64_t B = spx_plan_frame_step(plan);
  const int64_t limit = nonlinear != 0.0f ? n_in / B * B : n_in;                 /* L */
  const int64_t out_rows = spx_edit_rows(cap, HOP, PHASE), back_rows = spx_edit_rows(limit, HOP, PHASE);
  spx_stream_job job;
  job.in_off = 0;
  job.n_in = n_in;
  job.out_off = 0;
  job.out_cap = cap;
  job.channels = 1;
  job.speed = speed;
  job.nonlinear = nonlinear;
  job.feedback = 0.0f;
  const size_t key_bytes = (size_t)n_in * sizeof(int16_t);
  const size_t wsb = spx_batch_workspace_bytes(plan, &job, 1);
  const size_t n_rec = (size_t)(ops_cap > 0 ? ops_cap : 1);
  const size_t lab_out_bytes = (size_t)(out_rows + 1) * 4, feat_out_bytes = (size_t)(out_rows + 1) * (size_t)dim * 4;
  const size_t back_bytes = (size_t)(back_rows + 1) * 4;
  void* ws = spx_device_alloc(wsb);
  int16_t* d_key = (int16_t*)spx_device_alloc(key_bytes + 128);   /* the walk kernel's window loads: 64 values of padding */
  int16_t* d_out = (int16_t*)spx_device_alloc((size_t)cap * sizeof(int16_t) + 16);
  int64_t* d_counts = (int64_t*)spx_device_alloc(5 * sizeof(int64_t)); /* n_out | n_ops | rows: labels, features, back */
  spx_edit_op* d_ops = (spx_edit_op*)spx_device_alloc(n_rec * sizeof(spx_edit_op));
  int32_t* d_index = (int32_t*)spx_device_alloc(n_rec * sizeof(int32_t));
  int32_t* d_lab = (int32_t*)spx_device_alloc((size_t)lbytes + 4);
  float* d_feat = (float*)spx_device_alloc((size_t)fbytes + 4);
  int32_t* d_lab_out = (int32_t*)spx_device_alloc(lab_out_bytes);
  float* d_feat_out = (float*)spx_device_alloc(feat_out_bytes);
  int32_t* d_back = (int32_t*)spx_device_alloc(back_bytes);
  int32_t* lab_out = (int32_t*)malloc(lab_out_bytes);
  uint32_t* feat_out = (uint32_t*)malloc(feat_out_bytes);
  int32_t* back = (int32_t*)malloc(back_bytes);
  if (!ws || !d_key || !d_out || !d_counts || !d_ops || !d_index || !d_lab || !d_feat || !d_lab_out || !d_feat_out || !d_back ||
      !lab_out || !feat_out || !back) {
    fprintf(stderr, "allocation failed\n");
    return 2;
  }
  CHECK(spx_copy_to_device(d_key, key, key_bytes, NULL));
  if (lbytes) CHECK(spx_copy_to_device(d_lab, labels, (size_t)lbytes, NULL));
  if (fbytes) CHECK(spx_copy_to_device(d_feat, feats, (size_t)fbytes, NULL));
  for (int64_t j = 0; j <= out_rows; j++) lab_out[j] = 0;
  CHECK(spx_copy_to_device(d_lab_out, lab_out, lab_out_bytes, NULL));

  /* the tracks: labels and features on the input's timeline; then the warped labels, on the output's */
  spx_edit_rows_track lab_track, feat_track, back_track;
  lab_track.in_off = 0; lab_track.out_off = 0; lab_track.n_rows = label_rows; lab_track.out_cap = out_rows;
  feat_track.in_off = 0; feat_track.out_off = 0; feat_track.n_rows = feat_rows; feat_track.out_cap = out_rows;
  back_track.in_off = 0; back_track.out_off = 0; back_track.n_rows = out_rows; back_track.out_cap = back_rows;

  CHECK(spx_batch_run_edits(plan, &job, 1, d_key, d_out, d_counts, d_ops, &ops_cap, d_counts + 1, ws, wsb, NULL, NULL));
  CHECK(spx_edit_warp_rows(plan, &job, 1, d_ops, &ops_cap, d_counts + 1, d_counts, &lab_track, HOP, PHASE, 1, 1, 1, 4, SPX_ROWS_NEAREST,
                           d_lab, d_lab_out, d_counts + 2, NULL));
  CHECK(spx_edit_warp_rows(plan, &job, 1, d_ops, &ops_cap, d_counts + 1, d_counts, &feat_track, HOP, PHASE, dim, dim, dim, 4,
                           SPX_ROWS_BLEND, d_feat, d_feat_out, d_counts + 3, NULL));
  CHECK(spx_edit_index(plan, &job, 1, d_ops, &ops_cap, d_counts + 1, d_index, NULL));
  /* (the warped track is handed over with the rows its region holds, out_rows: the count the warp wrote stays on the device.  The
   *  last output frames can lie in a row whose middle is behind n_out, which the warp did not write: the region was zeroed above) */
  CHECK(spx_edit_unwarp_rows(plan, &job, 1, d_ops, &ops_cap, d_counts + 1, d_counts, d_index, &back_track, HOP, PHASE, 1, 1, 1, 4,
                             d_lab_out, d_back, d_counts + 4, NULL));

  int64_t counts[5];
  CHECK(spx_copy_to_host(counts, d_counts, sizeof(counts), NULL));
  CHECK(spx_copy_to_host(lab_out, d_lab_out, lab_out_bytes, NULL));
  CHECK(spx_copy_to_host(feat_out, d_feat_out, feat_out_bytes, NULL));
  CHECK(spx_copy_to_host(back, d_back, back_bytes, NULL));
  CHECK(spx_stream_synchronize(NULL));
  if (counts[0] < 0) { fprintf(stderr, "output capacity exceeded\n"); return 3; }
  if (counts[1] < 0) { fprintf(stderr, "the edit list has %lld records, the capacity holds %lld\n", (long long)-counts[1], (long long)ops_cap); return 3; }
  if (counts[2] < 0 || counts[3] < 0 || counts[4] < 0) { fprintf(stderr, "a row track's capacity was exceeded\n"); return 3; }
  long long sum = 0, sum2 = 0, same = 0;
  unsigned long long bits = 0;
  for (int64_t j = 0; j < counts[2]; j++) sum += lab_out[j];
  for (int64_t j = 0; j < counts[3] * dim; j++) bits += feat_out[j];
  for (int64_t j = 0; j < counts[4]; j++) {
    sum2 += back[j];
    same += j < label_rows && back[j] == labels[j];
  }
  printf("frames %lld ops %lld\n", (long long)counts[0], (long long)counts[1]);
  printf("labels rows %lld sum %lld\n", (long long)counts[2], sum);
  printf("features rows %lld bits %llu\n", (long long)counts[3], bits);
  printf("back rows %lld sum %lld same %lld\n", (long long)counts[4], sum2, same);

  spx_device_free(ws); spx_device_free(d_key); spx_device_free(d_out); spx_device_free(d_counts); spx_device_free(d_ops);
  spx_device_free(d_index); spx_device_free(d_lab); spx_device_free(d_feat); spx_device_free(d_lab_out); spx_device_free(d_feat_out);
  spx_device_free(d_back);
  spx_plan_destroy(plan);
  free(key); free(labels); free(feats); free(lab_out); free(feat_out); free(back);
  return 0;
}
