/* spx_batch_run_edits and spx_edit_replay as a program: plain C99 over include/speedy_hip.h, no HIP headers.
 *
 *   batch_edits_example KEY.raw TRACK.raw RATE KEY_CHANNELS TRACK_CHANNELS SPEED NONLINEAR OUT_KEY.raw OUT_TRACK.raw
 *
 * KEY.raw and TRACK.raw = interleaved int16 PCM of the same number of frames: the key (say, the noisy recording) decides speed and
 * pitch, the track (the clean one, a stem, a mask) is cut in exactly the same places.  One call compresses the key and records its
 * edit list, a second replays the list on the track; nothing comes back to the host in between.  Prints
 *   frames N     the key's output frames (n_out) -- the track's too
 *   ops K        the records of the key's edit list
 * and writes both outputs.  Exit code 0 = ok.  Used by tests/test_gpu_edit_list.py. */
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

static int write_raw(const char* path, const int16_t* p, size_t values) {
  FILE* f = fopen(path, "wb");
  if (!f) { perror(path); return 1; }
  const size_t done = fwrite(p, sizeof(int16_t), values, f);
  fclose(f);
  return done != values;
}

int main(int argc, char** argv) {
  if (argc != 10) {
    fprintf(stderr, "usage: %s KEY.raw TRACK.raw RATE KEY_CHANNELS TRACK_CHANNELS SPEED NONLINEAR OUT_KEY.raw OUT_TRACK.raw\n", argv[0]);
    return 1;
  }
  const int rate = atoi(argv[3]), kc = atoi(argv[4]), tc = atoi(argv[5]);
  const float speed = (float)atof(argv[6]), nonlinear = (float)atof(argv[7]);
  long kbytes = 0, tbytes = 0;
  int16_t* key = read_raw(argv[1], &kbytes);
  int16_t* track = read_raw(argv[2], &tbytes);
  if (!key || !track || kc < 1 || tc < 1) return 1;
  const int64_t n_in = kbytes / 2 / kc;
  if (tbytes / 2 / tc != n_in) { fprintf(stderr, "the key has %lld frames, the track %lld\n", (long long)n_in, (long long)(tbytes / 2 / tc)); return 1; }

  spx_plan_t plan = spx_plan_create(rate, /*match_matlab=*/0);
  if (!plan) { fprintf(stderr, "spx_plan_create: %s\n", spx_last_error()); return 2; }
  const int64_t cap = spx_plan_out_capacity_for(plan, n_in, speed, nonlinear);
  int64_t ops_cap = spx_plan_edit_ops(plan, n_in, speed, nonlinear);
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
  spx_edit_track tr;
  tr.in_off = 0;
  tr.out_off = 0;
  tr.channels = tc;
  tr.reserved = 0;
  const size_t key_bytes = (size_t)n_in * (size_t)kc * sizeof(int16_t), track_bytes = (size_t)n_in * (size_t)tc * sizeof(int16_t);
  const size_t wsb = spx_batch_workspace_bytes(plan, &job, 1);
  void* ws = spx_device_alloc(wsb);
  int16_t* d_key = (int16_t*)spx_device_alloc(key_bytes + 128);   /* the walk kernel's window loads: 64 values of padding */
  int16_t* d_track = (int16_t*)spx_device_alloc(track_bytes + 2); /* the replay reads the track's frames and nothing else */
  int16_t* d_out = (int16_t*)spx_device_alloc((size_t)cap * (size_t)kc * sizeof(int16_t) + 16);
  int16_t* d_yout = (int16_t*)spx_device_alloc((size_t)cap * (size_t)tc * sizeof(int16_t) + 16);
  int64_t* d_counts = (int64_t*)spx_device_alloc(2 * sizeof(int64_t)); /* n_out | n_ops */
  spx_edit_op* d_ops = (spx_edit_op*)spx_device_alloc((size_t)(ops_cap > 0 ? ops_cap : 1) * sizeof(spx_edit_op));
  if (!ws || !d_key || !d_track || !d_out || !d_yout || !d_counts || !d_ops) { fprintf(stderr, "device allocation failed\n"); return 2; }
  CHECK(spx_copy_to_device(d_key, key, key_bytes, NULL));
  CHECK(spx_copy_to_device(d_track, track, track_bytes, NULL));

  int64_t counts[2];
  for (int attempt = 0; attempt < 2; attempt++) {
    CHECK(spx_batch_run_edits(plan, &job, 1, d_key, d_out, d_counts, d_ops, &ops_cap, d_counts + 1, ws, wsb, NULL, NULL));
    CHECK(spx_copy_to_host(counts, d_counts, sizeof(counts), NULL));
    CHECK(spx_stream_synchronize(NULL));
    if (counts[1] >= 0) break;
    /* a job whose steps fail can outgrow spx_plan_edit_ops: the negative count says how many records it has */
    spx_device_free(d_ops);
    ops_cap = -counts[1];
    d_ops = (spx_edit_op*)spx_device_alloc((size_t)ops_cap * sizeof(spx_edit_op));
    if (!d_ops) { fprintf(stderr, "device allocation failed\n"); return 2; }
  }
  if (counts[0] < 0) { fprintf(stderr, "output capacity exceeded\n"); return 3; }
  if (counts[1] < 0) { fprintf(stderr, "the edit list did not fit\n"); return 3; }
  CHECK(spx_edit_replay(plan, &job, 1, d_ops, &ops_cap, d_counts + 1, d_counts, &tr, d_track, d_yout, NULL));

  int16_t* out = (int16_t*)malloc((size_t)counts[0] * (size_t)kc * sizeof(int16_t) + 2);
  int16_t* yout = (int16_t*)malloc((size_t)counts[0] * (size_t)tc * sizeof(int16_t) + 2);
  if (!out || !yout) return 2;
  if (counts[0] > 0) {
    CHECK(spx_copy_to_host(out, d_out, (size_t)counts[0] * (size_t)kc * sizeof(int16_t), NULL));
    CHECK(spx_copy_to_host(yout, d_yout, (size_t)counts[0] * (size_t)tc * sizeof(int16_t), NULL));
  }
  CHECK(spx_stream_synchronize(NULL));
  printf("frames %lld\n", (long long)counts[0]);
  printf("ops %lld\n", (long long)counts[1]);
  if (write_raw(argv[8], out, (size_t)counts[0] * (size_t)kc) || write_raw(argv[9], yout, (size_t)counts[0] * (size_t)tc)) return 1;

  spx_device_free(ws); spx_device_free(d_key); spx_device_free(d_track); spx_device_free(d_out); spx_device_free(d_yout);
  spx_device_free(d_counts); spx_device_free(d_ops);
  spx_plan_destroy(plan);
  free(key); free(track); free(out); free(yout);
  return 0;
}
