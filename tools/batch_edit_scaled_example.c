/* spx_batch_run_edits and spx_edit_replay_scaled as a program: plain C99 over include/speedy_hip.h, no HIP headers.
 *
 *   batch_edit_scaled_example [SPEED [NONLINEAR]]        (3.5 and 1 by default)
 *
 * Deciding at 16 kHz, rendering the master: a synthetic voiced signal is made twice -- a 48 kHz stereo FLOAT master and the 16 kHz
 * mono int16 key an analysis would be given (every third frame of the master's left channel; the signal has nothing above 2 kHz).
 * One call compresses the key and records its edit list, a second replays the list on the master at 3 / 1; nothing comes back to
 * the host in between.  Prints
 *   frames N          the key's output frames (n_out)
 *   ops K             the records of the key's edit list
 *   master_frames M   the master's output frames (n_out_y): M = spx_edit_scale(N, 3, 1)
 *   xfade o v         one value inside a cross-fade, frame o of the right channel, as the device computed it
 * and checks that value against the header's formula on the host.  Exit code 0 = ok.  Used by tests/test_gpu_edit_scaled.py. */
#include <math.h>
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

#define KEY_RATE 16000
#define P 3 /* master rate / key rate = 48000 / 16000 */
#define Q 1
#define SECONDS 2
#define MASTER_CHANNELS 2

/* a voiced sound: harmonics of a gliding pitch under a syllable envelope, in -0.6 .. 0.6; the right channel a little different */
static float master_value(int64_t frame, int channel) {
  const double t = (double)frame / (double)(KEY_RATE * P);
  const double f0 = 110.0 + 30.0 * sin(2.0 * 3.141592653589793 * 0.7 * t);
  const double env = 0.55 + 0.45 * sin(2.0 * 3.141592653589793 * 3.1 * t);
  double v = 0.0;
  for (int h = 1; h <= 8; h++) v += sin(2.0 * 3.141592653589793 * f0 * h * t + 0.3 * h * channel) / (h + 1);
  return (float)(0.6 * env * v);
}

int main(int argc, char** argv) {
  const float speed = argc > 1 ? (float)atof(argv[1]) : 3.5f, nonlinear = argc > 2 ? (float)atof(argv[2]) : 1.0f;
  const int64_t n_key = (int64_t)KEY_RATE * SECONDS, n_master = n_key * P / Q;
  float* master = (float*)malloc((size_t)n_master * MASTER_CHANNELS * sizeof(float));
  int16_t* key = (int16_t*)malloc((size_t)n_key * sizeof(int16_t));
  if (!master || !key) return 2;
  for (int64_t f = 0; f < n_master; f++)
    for (int c = 0; c < MASTER_CHANNELS; c++) master[f * MASTER_CHANNELS + c] = master_value(f, c);
  for (int64_t f = 0; f < n_key; f++) key[f] = (int16_t)lrintf(32767.0f * master[f * P * MASTER_CHANNELS]);

  spx_plan_t plan = spx_plan_create(KEY_RATE, /*match_matlab=*/0);
  if (!plan) { fprintf(stderr, "spx_plan_create: %s\n", spx_last_error()); return 2; }
  const int64_t cap = spx_plan_out_capacity_for(plan, n_key, speed, nonlinear);
  int64_t ops_cap = spx_plan_edit_ops(plan, n_key, speed, nonlinear);
  if (cap < 0 || ops_cap < 0) { fprintf(stderr, "the plan refuses the job: %s\n", spx_last_error()); return 2; }
  spx_stream_job job;
  job.in_off = 0;
  job.n_in = n_key;
  job.out_off = 0;
  job.out_cap = cap;
  job.channels = 1;
  job.speed = speed;
  job.nonlinear = nonlinear;
  job.feedback = 0.0f;
  spx_edit_master tr;
  tr.in_off = 0;
  tr.out_off = 0;
  tr.n_in = n_master;
  tr.out_cap = spx_edit_scale(cap, P, Q);
  tr.channels = MASTER_CHANNELS;
  tr.reserved = 0;
  const size_t key_bytes = (size_t)n_key * sizeof(int16_t), master_bytes = (size_t)n_master * MASTER_CHANNELS * sizeof(float);
  const size_t yout_bytes = (size_t)tr.out_cap * MASTER_CHANNELS * sizeof(float);
  const size_t wsb = spx_batch_workspace_bytes(plan, &job, 1);
  void* ws = spx_device_alloc(wsb);
  int16_t* d_key = (int16_t*)spx_device_alloc(key_bytes + 128);    /* the walk kernel's window loads: 64 values of padding */
  float* d_master = (float*)spx_device_alloc(master_bytes + 4);    /* the replay reads the master's frames and nothing else */
  int16_t* d_out = (int16_t*)spx_device_alloc((size_t)cap * sizeof(int16_t) + 16);
  float* d_yout = (float*)spx_device_alloc(yout_bytes + 16);
  int64_t* d_counts = (int64_t*)spx_device_alloc(3 * sizeof(int64_t)); /* n_out | n_ops | n_out_y */
  spx_edit_op* d_ops = (spx_edit_op*)spx_device_alloc((size_t)(ops_cap > 0 ? ops_cap : 1) * sizeof(spx_edit_op));
  if (!ws || !d_key || !d_master || !d_out || !d_yout || !d_counts || !d_ops) { fprintf(stderr, "device allocation failed\n"); return 2; }
  CHECK(spx_copy_to_device(d_key, key, key_bytes, NULL));
  CHECK(spx_copy_to_device(d_master, master, master_bytes, NULL));

  /* decide at 16 kHz, render at 48 kHz: two calls on one stream, the counts stay on the device */
  CHECK(spx_batch_run_edits(plan, &job, 1, d_key, d_out, d_counts, d_ops, &ops_cap, d_counts + 1, ws, wsb, NULL, NULL));
  CHECK(spx_edit_replay_scaled(plan, &job, 1, d_ops, &ops_cap, d_counts + 1, d_counts, &tr, P, Q, SPX_SAMPLES_FLOAT, d_master, d_yout,
                               d_counts + 2, NULL));
  int64_t counts[3];
  CHECK(spx_copy_to_host(counts, d_counts, sizeof(counts), NULL));
  CHECK(spx_stream_synchronize(NULL));
  if (counts[0] < 0) { fprintf(stderr, "output capacity exceeded\n"); return 3; }
  if (counts[1] < 0) { fprintf(stderr, "the edit list did not fit (a job whose steps fail: call again with %lld records)\n", (long long)-counts[1]); return 3; }
  if (counts[2] != spx_edit_scale(counts[0], P, Q)) { fprintf(stderr, "n_out_y is %lld\n", (long long)counts[2]); return 3; }
  printf("frames %lld\n", (long long)counts[0]);
  printf("ops %lld\n", (long long)counts[1]);
  printf("master_frames %lld\n", (long long)counts[2]);

  /* one cross-fade value against the formula: the middle frame of the first cross-fade that lies whole in front of the cut */
  spx_edit_op* ops = (spx_edit_op*)malloc((size_t)(counts[1] > 0 ? counts[1] : 1) * sizeof(spx_edit_op));
  float* yout = (float*)malloc(yout_bytes + 4);
  if (!ops || !yout) return 2;
  if (counts[1] > 0) CHECK(spx_copy_to_host(ops, d_ops, (size_t)counts[1] * sizeof(spx_edit_op), NULL));
  if (counts[2] > 0) CHECK(spx_copy_to_host(yout, d_yout, (size_t)counts[2] * MASTER_CHANNELS * sizeof(float), NULL));
  CHECK(spx_stream_synchronize(NULL));
  const int64_t L = nonlinear != 0.0f ? n_key / spx_plan_frame_step(plan) * spx_plan_frame_step(plan) : n_key;
  int64_t Lm = spx_edit_scale(L, P, Q);
  if (Lm > tr.n_in) Lm = tr.n_in;
  int checked = 0;
  for (int64_t k = 0; k < counts[1] && !checked; k++) {
    const spx_edit_op op = ops[k];
    if (op.b < 0 || (int64_t)op.out_at + op.n > counts[0]) continue;
    const int64_t at = spx_edit_scale(op.out_at, P, Q), n = spx_edit_scale((int64_t)op.out_at + op.n, P, Q) - at;
    const int64_t a = spx_edit_scale(op.a, P, Q), b = spx_edit_scale(op.b, P, Q), t = n / 2;
    const int c = MASTER_CHANNELS - 1;
    const float ya = a + t < Lm ? master[(a + t) * MASTER_CHANNELS + c] : 0.0f;
    const float yb = b + t < Lm ? master[(b + t) * MASTER_CHANNELS + c] : 0.0f;
    /* every operation rounded to float, one after the other */
    volatile float down = ya * (float)(n - t);
    volatile float up = yb * (float)t;
    volatile float sum = down + up;
    const float want = sum / (float)n;
    const float got = yout[(at + t) * MASTER_CHANNELS + c];
    printf("xfade %lld %.9g\n", (long long)(at + t), (double)got);
    if (got != want) { fprintf(stderr, "the cross-fade at master frame %lld is %.9g, the formula gives %.9g\n", (long long)(at + t), (double)got, (double)want); return 4; }
    checked = 1;
  }
  if (!checked) { fprintf(stderr, "the list has no cross-fade in front of the cut\n"); return 4; }

  spx_device_free(ws); spx_device_free(d_key); spx_device_free(d_master); spx_device_free(d_out); spx_device_free(d_yout);
  spx_device_free(d_counts); spx_device_free(d_ops);
  spx_plan_destroy(plan);
  free(master); free(key); free(ops); free(yout);
  return 0;
}
