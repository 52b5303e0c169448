/* spx_pipeline_submit_jobs as a program: plain C99 over include/speedy_hip.h, no HIP headers, no C++.
 *
 *   pipeline_jobs_example IN.raw RATE CHANNELS LANES DEPTH
 *
 * IN.raw = interleaved int16 PCM, one utterance.  ONE pipeline of LANES lanes is created for the whole utterance per lane at
 * 3.5x nonlinear -- that table is the pipeline's CAPACITY -- and three batches of different shapes go through it:
 *   ticket 0   the creation table itself: every lane the whole utterance, 3.5x nonlinear
 *   ticket 1   lane i the first (i + 1) / LANES of the utterance, speeds 1.5 / 2.0 / 3.5 taking turns, nonlinear
 *   ticket 2   the lengths of ticket 1 in reverse order, every lane LINEAR at 2x, the last lane EMPTY (n_in = 0: a batch with
 *              fewer live streams than lanes)
 * All three are submitted before the first is waited for.  A table that does not fit (a lane longer than created) is refused in
 * between and must leave the ticket numbers alone.  Prints one line per ticket and lane:
 *   ticket T lane I in N speed S nonlinear X frames K crc32 XXXXXXXX
 * (CRC-32 of the lane's int16 output bytes, the zlib polynomial).  Exit code 0 = ok.
 * Used by tests/test_gpu_pipeline_jobs.py::test_c_example_prints_the_oracles_counts_and_crcs. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "speedy_hip.h"

static uint32_t crc32_of(const unsigned char* p, size_t n) {
  uint32_t c = 0xffffffffu;
  for (size_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
  }
  return ~c;
}

int main(int argc, char** argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: %s IN.raw RATE CHANNELS LANES DEPTH\n", argv[0]);
    return 1;
  }
  const int rate = atoi(argv[2]), channels = atoi(argv[3]), lanes = atoi(argv[4]), depth = atoi(argv[5]);
  if (lanes < 1 || channels < 1) { fprintf(stderr, "LANES and CHANNELS must be at least 1\n"); return 1; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  int16_t* pcm = (int16_t*)malloc((size_t)bytes + 2);
  if (fread(pcm, 1, (size_t)bytes, f) != (size_t)bytes) { fprintf(stderr, "short read\n"); return 1; }
  fclose(f);
  const int64_t n_in = bytes / 2 / channels;
  const size_t per_lane = (size_t)n_in * (size_t)channels;

  spx_plan_t plan = spx_plan_create(rate, /*match_matlab=*/0);
  if (!plan) { fprintf(stderr, "spx_plan_create: %s\n", spx_last_error()); return 2; }
  /* three tables over the same lanes: in_off stays where the lane was created, n_in / speed / nonlinear change per batch */
  static const float turns[3] = {1.5f, 2.0f, 3.5f};
  spx_stream_job* tab[3];
  for (int b = 0; b < 3; b++) {
    tab[b] = (spx_stream_job*)calloc((size_t)lanes, sizeof(spx_stream_job));
    for (int i = 0; i < lanes; i++) {
      spx_stream_job* j = &tab[b][i];
      j->in_off = (int64_t)i * (int64_t)per_lane;
      j->channels = channels;
      j->feedback = 0.0f;
      if (b == 0) { j->n_in = n_in; j->speed = 3.5f; j->nonlinear = 1.0f; }
      if (b == 1) { j->n_in = n_in * (i + 1) / lanes; j->speed = turns[i % 3]; j->nonlinear = 1.0f; }
      if (b == 2) { j->n_in = i == lanes - 1 ? 0 : n_in * (lanes - i) / lanes; j->speed = 2.0f; j->nonlinear = 0.0f; }
    }
  }
  spx_pipeline_t pipe = spx_pipeline_create(plan, tab[0], lanes, depth, /*flags=*/0);
  if (!pipe) { fprintf(stderr, "spx_pipeline_create: %s\n", spx_last_error()); return 2; }
  const size_t in_values = spx_pipeline_input_values(pipe);
  if (in_values != per_lane * (size_t)lanes) { fprintf(stderr, "unexpected input size\n"); return 3; }
  /* every lane reads the front of the utterance: one input buffer serves all three batches (pinned: the copy runs at the link's rate) */
  int16_t* in = (int16_t*)spx_host_alloc((in_values ? in_values : 1) * sizeof(int16_t));
  if (!in) { fprintf(stderr, "spx_host_alloc: %s\n", spx_last_error()); return 2; }
  for (int i = 0; i < lanes; i++) memcpy(in + (size_t)i * per_lane, pcm, per_lane * sizeof(int16_t));

  int64_t tickets[3];
  for (int b = 0; b < 3; b++) {
    if (spx_pipeline_jobs_fit(pipe, tab[b]) != 0) { fprintf(stderr, "table %d does not fit: %s\n", b, spx_last_error()); return 3; }
    tickets[b] = spx_pipeline_submit_jobs(pipe, tab[b], in, /*in_is_device=*/0);
    if (tickets[b] != b) { fprintf(stderr, "spx_pipeline_submit_jobs (table %d): ticket %lld: %s\n", b, (long long)tickets[b], spx_last_error()); return 2; }
    if (b == 0 && n_in > 0) {
      /* a lane longer than it was created: refused, with the lane and the limit named; nothing is enqueued, no ticket is used up */
      spx_stream_job* big = (spx_stream_job*)malloc((size_t)lanes * sizeof(spx_stream_job));
      memcpy(big, tab[0], (size_t)lanes * sizeof(spx_stream_job));
      big[lanes - 1].n_in = n_in + 1;
      if (spx_pipeline_jobs_fit(pipe, big) == 0 || spx_pipeline_submit_jobs(pipe, big, in, 0) >= 0) {
        fprintf(stderr, "a lane longer than the pipeline's capacity was accepted\n");
        return 3;
      }
      fprintf(stderr, "refused as expected: %s\n", spx_last_error());
      free(big);
    }
  }
  for (int b = 0; b < 3; b++) {
    const int16_t* out;
    const int64_t *offsets, *counts;
    if (spx_pipeline_wait(pipe, tickets[b], &out, &offsets, &counts) != 0) { fprintf(stderr, "spx_pipeline_wait: %s\n", spx_last_error()); return 2; }
    for (int i = 0; i < lanes; i++) {
      if (counts[i] < 0) { fprintf(stderr, "ticket %d lane %d: output capacity exceeded\n", b, i); return 3; }
      if (offsets[i] % 32 != 0) { fprintf(stderr, "ticket %d lane %d: offset not at a 64-byte boundary\n", b, i); return 3; }
      if (tab[b][i].n_in == 0 && counts[i] != 0) { fprintf(stderr, "ticket %d lane %d: an empty lane produced frames\n", b, i); return 3; }
      printf("ticket %d lane %d in %lld speed %g nonlinear %g frames %lld crc32 %08x\n", b, i, (long long)tab[b][i].n_in,
             (double)tab[b][i].speed, (double)tab[b][i].nonlinear, (long long)counts[i],
             (unsigned)crc32_of((const unsigned char*)(out + offsets[i]), (size_t)counts[i] * (size_t)channels * sizeof(int16_t)));
    }
  }
  spx_pipeline_destroy(pipe);
  spx_host_free(in);
  spx_plan_destroy(plan);
  for (int b = 0; b < 3; b++) free(tab[b]);
  free(pcm);
  return 0;
}
