/* speedy_hip.h — the thin C-ABI between host code and the hand-written HIP (gfx950) kernels of the
 * Speedy hot path:   analysis -> tension -> speed -> pitch-synchronous overlap-add.
 *
 * Plain C: pointers and sizes only, no HIP/torch types.  `hip_stream` arguments are a hipStream_t cast
 * to void* (NULL = the default stream).  Every pointer marked DEVICE must be HBM-resident on the
 * current device; HOST pointers are ordinary host memory.
 *
 * What each entry point replaces in the reference (google/speedy):
 *   spx_plan_create        speedyCreateStream's tables (speedy.c:206-299: window :256-258, FFT plan
 *                          :269-277, filter alphas :287-292) + libsonic's period limits
 *   spx_batch_analyze      speedyAddDataShort ... speedyComputeLocalEnergy for every frame of every
 *                          stream (speedy.c:553-565,416-425,438-473,510-523), the mono mix of
 *                          sonicSendDataToSpeedy (soniclib.c:262-287) and the per-frame part of
 *                          speedyComputeSpectralDifference (speedy.c:628-647,705-719)
 *   spx_batch_walk         the frame-sequential rest: filters, hysteresis, tension, speed
 *                          (speedy.c:73-76,590-610,682-728,752-788; soniclib.c:339-345) and the TSM stage the
 *                          reference reaches through sonicIntSetSpeed / sonicIntWriteShortToStream /
 *                          sonicIntFlushStream (soniclib.c:354,369,538-551)
 *   spx_batch_run          = analyze + walk: one whole sonicWriteShortToStream ... sonicFlushStream
 *                          life cycle (speedy_wave.cc:154-242) for N independent streams at once
 * The reference-compatible streaming API on top of this is include/sonic2.h.
 */
#ifndef SPEEDY_HIP_H_
#define SPEEDY_HIP_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#ifndef SPX_FEATURE_COUNT
#define SPX_FEATURE_COUNT 15 /* speedy.h:115 */
#endif

typedef struct spx_plan* spx_plan_t;

/* Per-stream job description (HOST array).  Offsets are in int16 elements from the batch base pointers. */
typedef struct {
  int64_t in_off;   /* first input sample of this stream, in shorts, inside `in`                      */
  int64_t n_in;     /* input length in multi-channel sample frames (sonic2.h:56-59 units)             */
  int64_t out_off;  /* first output sample, in shorts, inside `out`                                   */
  int64_t out_cap;  /* output capacity in multi-channel sample frames                                 */
  int32_t channels; /* interleaved channel count                                                      */
  float speed;      /* sonicSetSpeed                (soniclib.c:177)                                  */
  float nonlinear;  /* sonicEnableNonlinearSpeedup  (soniclib.c:555); 0 = linear: TSM stage only      */
  float feedback;   /* sonicSetDurationFeedbackStrength (soniclib.c:565)                              */
} spx_stream_job;

/* Optional debug taps (DEVICE, any may be NULL): the reference's five callbacks (sonic2.h:104-125).
 * Row r of stream s lives at index tap_off[s] + r, with tap_off[s] = sum over earlier streams of their
 * analysis-frame counts (spx_plan_frames).  Taps are excluded from the roofline byte count. */
typedef struct {
  float* tension;     /* [frames]        tension of read-buffer k  (soniclib.c:320-324)                */
  float* speed;       /* [frames]        speed handed to the TSM stage (soniclib.c:349-354)            */
  float* features;    /* [frames][15]    speedyGetInternalState at tension time (soniclib.c:325-329)   */
  float* spectrogram; /* [frames][N]     |DFT| of analysis frame j (soniclib.c:297-302)                */
  float* normalized;  /* [frames][N/2]   normalised spectrum used for tension k (speedy.c:673-675)     */
} spx_taps;

/* ---- errors: 0 = ok; otherwise a negative code, text via spx_last_error() (thread-local) ---- */
const char* spx_last_error(void);
int spx_abi_version(void);

/* ---- plan: tables for one (sample rate, hysteresis mode) pair ---- */
spx_plan_t spx_plan_create(int sample_rate, int match_matlab);
void spx_plan_destroy(spx_plan_t plan);
int spx_plan_frame_step(spx_plan_t plan);   /* speedyInputFrameStep, speedy.c:335-338 */
int spx_plan_window_size(spx_plan_t plan);  /* speedyInputFrameSize, speedy.c:330-333 */
int spx_plan_fft_size(spx_plan_t plan);     /* speedyFFTSize,        speedy.c:340-343 */
int spx_plan_future(spx_plan_t plan);       /* kTemporalHysteresisFuture, speedy.h:136-146 */
int spx_plan_max_required(spx_plan_t plan); /* libsonic maxRequired = 2*(rate/65) */
/* Number of analysis frames the shim schedules for n_in input frames (soniclib.c:440-444). */
int64_t spx_plan_frames(spx_plan_t plan, int64_t n_in);
/* Safe output capacity (frames) for n_in input frames at `speed`: n_in + slack for speed >= 1; for a slow-down
 * (n_in + flush padding) * 2/s + slack with s = speed for a linear job and s = 0.01 (the kMinimumSpeed clamp,
 * speedy.c:92,776) when the nonlinear path may drive the speed.  The three-argument form assumes nonlinear. */
int64_t spx_plan_out_capacity(spx_plan_t plan, int64_t n_in, float speed);
int64_t spx_plan_out_capacity_for(spx_plan_t plan, int64_t n_in, float speed, float nonlinear);

/* ---- batch execution ---- */
/* Bytes of DEVICE scratch needed for a batch (depends only on the jobs' lengths). */
size_t spx_batch_workspace_bytes(spx_plan_t plan, const spx_stream_job* jobs, int n_streams);

/* Whole life cycle for n_streams independent streams, asynchronous on hip_stream:
 *   in   DEVICE  int16 input samples (read once)
 *   out  DEVICE  int16 output samples (written once)
 *   n_out DEVICE int64[n_streams]: produced frames per stream (negative = out_cap overflow)
 * Returns 0 when the launches were enqueued.
 * What the workspace, out, n_out and the taps hold when the call is made does not matter, nor what lies in `in` between the jobs'
 * streams and in the 64 values behind the last one: every state the kernels keep starts from the call's own staging (memory fresh
 * from hipMalloc, a workspace another table's call has used).  in, out and the taps need the alignment of their element type only;
 * nothing is written outside out_off .. out_off + out_cap * channels of a job and the job's rows of the taps.  That holds for every
 * batch call below (tests/test_gpu_dirty_memory.py).
 * The reference stores any float as speed, nonlinear factor or feedback strength and has no defined behaviour for most of them.
 * Here a job is taken if channels >= 1, no count or offset is negative, the speed is finite and > 0, the nonlinear factor lies in
 * [0, 1], the feedback strength is finite, n_in < 2^30 and -- a nonlinear job -- the plan's analysis tile fits one CU's LDS;
 * a batch if the walk kernel's window of its largest channel count fits a CU's LDS.  The whole table is judged by these rules
 * before anything is enqueued: -1 with the first broken rule in spx_last_error, nothing launched, the plan as it was.  That
 * holds for every batch call below -- _ahead / _overlapped (also where the call is cut into sub-batches), _mixed*, _rate, _float, _map:
 * the bad job may be the last of the last group -- and the rate / float workspace and capacity queries answer 0 / -1 for such
 * a table; spx_pipeline_create* and spx_pipeline_submit_jobs / _jobs_fit apply the same rules per lane and name the lane. */
int spx_batch_run(spx_plan_t plan, const spx_stream_job* jobs, int n_streams, const int16_t* in,
                  int16_t* out, int64_t* n_out, void* workspace, size_t workspace_bytes,
                  const spx_taps* taps, void* hip_stream);

/* spx_batch_run with a PLAYBACK RATE per stream: sonicSetRate before the first write (sonic2.h:70; the reference forwards it to
 * the TSM dependency, whose adjustRate resamples what the speed stage produced, soniclib.c:169-175).
 *   rates  HOST float[n_streams], NULL = every rate 1 (the call IS spx_batch_run then, as it is with every entry 1).
 * out / n_out hold the FINAL frames -- behind the rate stage -- and out_cap counts final frames (spx_plan_out_capacity_rate);
 * n_out[i] negative = out_cap was too small (nothing is written past out_off + out_cap * channels).  A job with rates[i] == 1 gets
 * the bytes and the count spx_batch_run gives it, in the same call as jobs with other rates.  Taps are spx_batch_run's (the rate
 * stage lies behind everything they observe); spx_batch_pack_outputs and spx_batch_read_steps work on the result unchanged.
 * A rate <= 0, not finite, or so large that (int)(sample rate / rate) < 1 is refused: -1, spx_last_error, nothing launched.
 * The workspace (spx_batch_workspace_bytes_rate) also holds the speed stage's output of the jobs with a rate other than 1; its
 * contents on entry do not matter.
 * Asynchronous on hip_stream like spx_batch_run, kernels in sequence; the plain call only (no _ahead / _overlapped / _mixed form).
 * The pipeline object takes a rate per lane and per batch: spx_pipeline_create_rate below.  Any channel count the walk kernel's window takes: the 16 of the streaming API's rate
 * stage do not apply. */
int spx_batch_run_rate(spx_plan_t plan, const spx_stream_job* jobs, const float* rates, int n_streams, const int16_t* in,
                       int16_t* out, int64_t* n_out, void* workspace, size_t workspace_bytes,
                       const spx_taps* taps, void* hip_stream);
/* 0 (spx_last_error) for a rate or a job spx_batch_run_rate would refuse. */
size_t spx_batch_workspace_bytes_rate(spx_plan_t plan, const spx_stream_job* jobs, const float* rates, int n_streams);
/* spx_plan_out_capacity_for behind the rate stage: safe capacity in FINAL frames; -1 (spx_last_error) for a rate, speed,
 * nonlinear factor or n_in that is refused. */
int64_t spx_plan_out_capacity_rate(spx_plan_t plan, int64_t n_in, float speed, float nonlinear, float rate);

/* ---- TIME MAP: which output frame each 10 ms of input lands on ----
 * A nonlinear speed-up changes its speed every 10 ms; spx_batch_run_map is spx_batch_run that also writes down where the input
 * went, for callers whose audio carries timestamps (captions, word or phone labels, a video track).  With B = spx_plan_frame_step
 * and R = n_in / B (integer division) a job's rows M are
 *   nonlinear != 0   R + 1 rows: M[k], k < R, = the output frames the time-scale stage has produced when ring buffer k -- input
 *                    frames [kB, (k+1)B) -- is about to be handed to it; M[R] = the job's final count, the value of n_out
 *   nonlinear == 0   one row, M[0] = n_out.
 * spx_plan_map_rows returns that row count (-1 for a null plan or a negative n_in).  M[0] = 0 where R >= 1, and the rows never
 * decrease; consecutive rows are often equal, because the time-scale stage works in whole pitch periods.  It also holds back up to
 * about spx_plan_max_required input frames before it emits anything for them: the map is LATE by at most that much INPUT -- a few
 * tens of milliseconds; measured against spx_edit_lookup, 480 to 490 of 492 frames at 16 kHz -- and never early.  In OUTPUT frames
 * the lag is that input at the speed of the moment: up to 221 frames at 3.5x, 428 at 1.2x and 1 579 at 0.5x on the directed 16 kHz
 * jobs (profiles/edit_lookup.txt).  (The integral of 1 / speed over the speed tap is no substitute: it drifts from these rows.)
 *   map  DEVICE int64; stream i's rows start at the sum of spx_plan_map_rows of the streams in front of it, in job order.
 * out, n_out and the taps are byte for byte spx_batch_run's for the same table; the workspace is spx_batch_workspace_bytes (its contents
 * on entry, like those of out, n_out, the taps and `map`, do not matter).  The
 * call refuses what spx_batch_run refuses, with the same messages, and a NULL map -- -1, spx_last_error, nothing enqueued.  The rows
 * of a job whose n_out comes back negative are unspecified.
 * COST: the whole batch runs on the GENERAL walk kernel (the speed-up kernels write no map yet), kernels in sequence on hip_stream,
 * as spx_batch_run_rate does: profiles/time_map.txt.  The plain call only.  OUT OF SCOPE: a map on the _ahead, _overlapped,
 * _mixed* and _twopass calls, on the pipeline object and on the streaming API (include/sonic2.h).
 *
 * WITH PLAYBACK RATES, AND ON FLOAT SAMPLES: spx_batch_run_rate_map is spx_batch_run_rate, and spx_batch_run_float_map is
 * spx_batch_run_float, with the same map beside it.  spx_plan_map_rows and the row layout are unchanged (the rate stage changes no
 * row count); the rows count FINAL frames -- behind the rate stage, the unit of out, n_out and out_cap of these calls.  With
 * (new, old) = (int)(sample rate / rates[i]) computed in float and the sample rate, halved together until both fit 14 bits, and
 *   F(m) = 0 for m < 2, else ((m - 1) * new + old - 1) / old in int64     (the frames behind the rate stage after m frames of the speed stage)
 *   nonlinear != 0, rates[i] != 1   M[k] = F(the row spx_batch_run_map writes for the same job), k < R; M[R] = n_out[i]
 *   nonlinear == 0, rates[i] != 1   M[0] = n_out[i]
 *   rates[i] == 1, or rates == NULL the rows of spx_batch_run_map, unchanged, in the same call as jobs with other rates
 * Row k is what a streaming caller with sonicSetRate set sees in sonicSamplesAvailable at that hand-off (nothing read in between),
 * and the rows never decrease, the last one included.  The rows of a job whose n_out comes back negative are unspecified.
 * out, n_out and the taps are byte for byte spx_batch_run_rate's (spx_batch_run_float's) for the same table, and the workspace is
 * spx_batch_workspace_bytes_rate (_float), unchanged: the rows are converted in place in `map`, by one small kernel behind the rate
 * kernel.  With every rate 1 or rates == NULL spx_batch_run_rate_map IS spx_batch_run_map.  Refused with -1 and spx_last_error,
 * nothing enqueued, the plan as it was: everything spx_batch_run_rate (_float) refuses, with its messages; a NULL map; more than
 * 2^31 - 1 rows in one call.  The plain call only, kernels in sequence on hip_stream (profiles/time_map_rate.txt).
 *
 * spx_map_lookup converts positions on the device, asynchronous on hip_stream, in exact integer arithmetic (int64, floor division).
 *   jobs     HOST   the table the map was made with (n_in and nonlinear are read)
 *   map      DEVICE the rows spx_batch_run_map wrote -- or spx_batch_run_rate_map / _float_map: the lookup interpolates whatever rows
 *                   it is given, and on a map from those calls the output side (Y, forward's answers, inverse's queries) is in FINAL frames
 *   q_off    DEVICE int64[n_streams + 1]: stream i's queries are q[q_off[i] .. q_off[i + 1]) (an empty range is fine)
 *   q, r     DEVICE int64: positions in, positions out, same indices
 *   inverse  0: input frame -> output frame; otherwise output frame -> input frame
 * Nodes: X = [0, B, .., (R-1)B, n_in], Y = M for R >= 1;  X = [0, n_in], Y = [0, M[0]] for R = 0 (a linear job, or one shorter
 * than a ring buffer).  L = the number of nodes.
 *   forward  t clamped to [0, n_in]; n_in = 0 gives 0; else j = min(t / B, L - 2) and
 *            Y[j] + (t - X[j]) * (Y[j+1] - Y[j]) / (X[j+1] - X[j])
 *   inverse  u clamped to [0, Y[L-1]]; u >= Y[L-1] gives n_in; else j = the largest index with Y[j] <= u (a flat run resolves
 *            to its last node, so Y[j+1] > u) and  X[j] + (u - Y[j]) * (X[j+1] - X[j]) / (Y[j+1] - Y[j])
 * Both are non-decreasing, and forward(inverse(u)) <= u.  Returns 0, or -1 (spx_last_error) for a null pointer or a table
 * spx_batch_run refuses.
 * DOMAIN: the lookups are exact where n_in * Y[L-1] < 2^63.  Precisely: neither product exceeds its segment's
 * (X[j+1] - X[j]) * (Y[j+1] - Y[j]) -- the forward one reaches it in the last segment, at t = n_in, and stays below it elsewhere
 * (t < X[j+1] there); the inverse one stops at (Y[j+1] - Y[j] - 1) times the segment's width -- so the answers are exact while that
 * product is at most 2^63 - 1 in every segment; a segment is at most n_in wide (R = 0) or 2B - 1 (R >= 1) and rises by at most
 * Y[L-1].  Every map spx_batch_run_map writes lies far inside (n_in < 2^30, and the walk kernel counts at most 2^31 - 1 output
 * frames).  Outside the domain, and on rows that decrease or are negative, the answers are unspecified; the indices stay inside
 * the stream's rows and no divisor is zero. */
int64_t spx_plan_map_rows(spx_plan_t plan, int64_t n_in, float nonlinear);
int spx_batch_run_map(spx_plan_t plan, const spx_stream_job* jobs, int n_streams, const int16_t* in,
                      int16_t* out, int64_t* n_out, int64_t* map, void* workspace, size_t workspace_bytes,
                      const spx_taps* taps, void* hip_stream);
int spx_map_lookup(spx_plan_t plan, const spx_stream_job* jobs, int n_streams, const int64_t* map, const int64_t* q_off,
                   const int64_t* q, int64_t* r, int inverse, void* hip_stream);
int spx_batch_run_rate_map(spx_plan_t plan, const spx_stream_job* jobs, const float* rates, int n_streams, const int16_t* in,
                           int16_t* out, int64_t* n_out, int64_t* map, void* workspace, size_t workspace_bytes,
                           const spx_taps* taps, void* hip_stream);
int spx_batch_run_float_map(spx_plan_t plan, const spx_stream_job* jobs, const float* rates, int n_streams, const float* in,
                            float* out, int64_t* n_out, int64_t* map, void* workspace, size_t workspace_bytes,
                            const spx_taps* taps, void* hip_stream);

/* ---- EDIT LIST: the copies and cross-fades a job performed, and their replay on other tracks ----
 * Every output frame of a job is either a run of input frames copied through or a cross-fade of two runs.  spx_batch_run_edits is
 * spx_batch_run that also writes that list down, and spx_edit_replay applies a list to any other track of the same length -- a clean
 * recording beside the noisy one, stems, a dubbed language, a per-sample mask -- so that speed and pitch are decided on ONE track
 * and every companion is cut in exactly the same places.  Decide once, render many times: each further track costs a pass over its
 * bytes, not another walk (profiles/edit_list.txt).
 *
 * A record (spx_edit_op, 16 bytes, n >= 1):
 *   b <  0   a copy:        output frame out_at + t = source frame a + t, t < n
 *   b >= 0   a cross-fade:  per channel, output frame out_at + t = (y[a + t] * (n - t) + y[b + t] * t) / n, truncated toward zero
 *            (a: the ramp going down, b: the ramp coming up)
 * A source frame at or behind L reads as 0: L = n_in for a linear job, (n_in / B) * B for a nonlinear one (B = spx_plan_frame_step:
 * the trailing partial ring buffer is dropped, and the flush pads with zeros).  Records come in the order the time-scale stage emits
 * them -- a speed-up step is one cross-fade; a slow-down step a copy and then a cross-fade (a step that fails leaves its copy); every
 * piece of a pending copy-through, at most spx_plan_max_required frames, a copy; a write at unity speed one copy of everything
 * pending -- and are contiguous: ops[0].out_at = 0, ops[k + 1].out_at = ops[k].out_at + ops[k].n.  The flush's cut removes no
 * record: frames at or behind n_out are not part of the output.  Every position fits int32 (n_in < 2^30 plus padding; the walk
 * kernel counts at most 2^31 - 1 output frames).
 *
 * spx_batch_run_edits
 *   ops      DEVICE, aligned to 16 bytes; stream i's records start at the sum of ops_cap of the streams in front of it
 *   ops_cap  HOST   int64[n_streams], records per stream (spx_plan_edit_ops, or any value >= 0)
 *   n_ops    DEVICE int64[n_streams]: the number of records of each job.  A job that has more than ops_cap[i] comes back as MINUS the
 *            number it has: the kernel keeps counting and stops storing, nothing is written behind the stream's region, out and
 *            n_out are unaffected -- call again with that capacity.  Where n_out[i] is negative the stream's records are unspecified.
 * out, n_out and the taps are byte for byte spx_batch_run's for the same table; the workspace is spx_batch_workspace_bytes (its contents
 * on entry, like those of out, n_out, the taps, ops and n_ops, do not matter).  Refused
 * with -1 and spx_last_error, nothing enqueued, the plan as it was: everything spx_batch_run refuses, with its messages; a NULL or
 * misaligned ops, a NULL ops_cap or n_ops; a negative capacity; more than 2^31 - 1 records of capacity in one call.
 * COST: as spx_batch_run_map -- the whole batch on the GENERAL walk kernel, kernels in sequence on hip_stream -- plus one 16-byte
 * store per record.  The plain call only.  OUT OF SCOPE: an edit list on the _rate, _float, _map, _twopass, _ahead, _overlapped and
 * _mixed* calls, on the pipeline object and on the streaming API; float tracks.
 *
 * spx_plan_edit_ops returns a capacity that holds every record of a job NONE OF WHOSE STEPS FAILS (-1 for values spx_batch_run
 * refuses).  A step fails when its cross-fade would have no frame: with minPeriod = sample rate / 400, a linear job with
 * 1 / minPeriod <= speed <= minPeriod has no failed step, and a nonlinear job has none while every speed of its speed tap lies in
 * that range -- the library cannot know those speeds before the call, so for a nonlinear job the value is a capacity that holds
 * unless the tension drives an event's speed outside the range.  A job whose steps fail processes its pending input again at the next
 * event (the stage consumes nothing on a failure), so no bound linear in the length covers it: the negative count in n_ops is the
 * answer there.
 *
 * spx_edit_replay runs asynchronously on hip_stream: for each stream, out_y[o], o < n_out[i], is the value of the record that covers
 * o, computed on the track y -- any channel count, n_in frames.  Replaying a job's list on the job's own input gives the job's out,
 * byte for byte.
 *   jobs     HOST   the table the list was made with (n_in, nonlinear and out_cap are read)
 *   ops, ops_cap, n_ops, n_out   as spx_batch_run_edits took and left them (n_ops, n_out: DEVICE -- nothing comes back to the host)
 *   tracks   HOST   one per stream: in_off / out_off in int16 values from y_in / y_out, channels in 1 .. 65535; out_off addresses
 *            jobs[i].out_cap frames of `channels` values
 *   y_in     DEVICE read only below L frames per stream: no padding behind the last track is needed (unlike spx_batch_run's `in`)
 *   y_out    DEVICE a stream with n_out[i] <= 0 or n_ops[i] < 0 gets nothing written; no other gets more than n_out[i] frames
 * Refused with -1 and spx_last_error before anything is enqueued: a NULL pointer; a track with channels < 1 (or above 65535) or a
 * negative offset; a misaligned ops; a table spx_batch_run refuses.
 *
 * POSITION LOOKUP, TO THE SAMPLE: spx_edit_index and spx_edit_lookup answer "where did this input frame go" and "which input frame
 * plays here" from the records themselves -- exact, and not late, where spx_map_lookup answers to 10 ms and up to about
 * spx_plan_max_required frames late.  For word or phone labels, caption cues, an editor's cut points, a click in the sped-up audio
 * that must land on the source.  tests/edit_lookup_ref.py states the definition in Python integers.
 *   The SOURCE of output frame out_at + t of a record, with h = (n + 1) / 2 (the number of t with 2 t < n):
 *     copy         a + t
 *     cross-fade   a + t for t < h (the ramp going down still has the larger weight), b + t from there on (a tie in weight goes
 *                  to the ramp coming up)
 *   inverse  (output frame u -> input frame)  u below 0 counts as 0; u >= n_out answers L with record -1; otherwise k = the record
 *            that covers u, the largest k with out_at(k) <= u, and the answer is min(source, L) with record k -- a frame that plays
 *            the flush's padding answers L.
 *   forward  (input frame p -> output frame)  p clamped to [0, L]; the answer is the smallest output frame o < n_out whose source
 *            is >= p -- the first moment at which p itself is heard, or the first surviving audio behind it -- with its record; n_out
 *            with record -1 if there is none.
 * The source is not monotone over the output (a slow-down plays input twice), so forward searches the INDEX: with R_k = the largest
 * source inside record k (a + n - 1 for a copy; a + h - 1, or max(a + h - 1, b + n - 1) where n > h, for a cross-fade),
 * G_k = max(R_0 .. R_k).  The first record with G_k >= p holds the answer, at t = max(0, p - a) for a copy, and for a cross-fade
 * t1 = max(0, p - a) if t1 < h, else max(h, p - b); the answer is min(out_at + t, n_out) -- records behind the flush's cut are in
 * the list, the min handles them -- and its record is -1 when the answer is n_out.
 * forward is non-decreasing, forward(inverse(o)) <= o, and inverse(forward(p)) >= p where forward(p) < n_out.
 *
 * spx_edit_index writes G, asynchronously on hip_stream; n_ops is read on the device.
 *   jobs, ops, ops_cap, n_ops   as spx_edit_replay takes them
 *   index    DEVICE int32, laid out as ops: stream i's values start at the sum of ops_cap of the streams in front of it, one per
 *            record; exactly min(n_ops[i], ops_cap[i]) are written, none for a stream with a negative n_ops
 * spx_edit_lookup converts positions, asynchronously on hip_stream.
 *   n_out    DEVICE as spx_batch_run_edits left it
 *   index    DEVICE what spx_edit_index wrote for these records; may be NULL where inverse != 0
 *   q_off, q, r   DEVICE int64, exactly as spx_map_lookup takes them
 *   rec      DEVICE int32, same indices as r, or NULL: the index of the answer's record in the stream's list (-1: none), so that a
 *            caller can read both ramps and the weight of a cross-fade from ops itself
 *   inverse  0: input frame -> output frame; otherwise output frame -> input frame
 * A stream whose n_ops[i] or n_out[i] is negative gets -1 for every answer and every record, and disturbs no other stream.
 * Refused with -1 and spx_last_error before anything is enqueued: a NULL pointer other than rec and (inverse != 0) index; a forward
 * call without an index; a misaligned ops; a negative capacity; more than 2^31 - 1 records of capacity in one call; a table
 * spx_batch_run refuses.  Whatever the records hold, the kernels read nothing outside the stream's region of ops and index (no
 * track, no audio) and write nothing outside r, rec and that region of index; on records that are not contiguous from 0 or whose
 * positions do not fit int32 the answers are unspecified.
 * COST: the index one workgroup per stream in one pass; a lookup one binary search per query (profiles/edit_lookup.txt).
 * OUT OF SCOPE: lookups behind a rate stage; lookups on the _float, _twopass, _ahead and _mixed* calls, on the pipeline object and on
 * the streaming API (none of them records a list); fractional answers inside a cross-fade. */
typedef struct { int32_t out_at, a, b, n; } spx_edit_op;
typedef struct { int64_t in_off, out_off; int32_t channels, reserved; } spx_edit_track;
int64_t spx_plan_edit_ops(spx_plan_t plan, int64_t n_in, float speed, float nonlinear);
int spx_batch_run_edits(spx_plan_t plan, const spx_stream_job* jobs, int n_streams, const int16_t* in, int16_t* out, int64_t* n_out,
                        spx_edit_op* ops, const int64_t* ops_cap, int64_t* n_ops, void* workspace, size_t workspace_bytes,
                        const spx_taps* taps, void* hip_stream);
int spx_edit_replay(spx_plan_t plan, const spx_stream_job* jobs, int n_streams, const spx_edit_op* ops, const int64_t* ops_cap,
                    const int64_t* n_ops, const int64_t* n_out, const spx_edit_track* tracks, const int16_t* y_in, int16_t* y_out,
                    void* hip_stream);
int spx_edit_index(spx_plan_t plan, const spx_stream_job* jobs, int n_streams, const spx_edit_op* ops, const int64_t* ops_cap,
                   const int64_t* n_ops, int32_t* index, void* hip_stream);
int spx_edit_lookup(spx_plan_t plan, const spx_stream_job* jobs, int n_streams, const spx_edit_op* ops, const int64_t* ops_cap,
                    const int64_t* n_ops, const int64_t* n_out, const int32_t* index, const int64_t* q_off, const int64_t* q,
                    int64_t* r, int32_t* rec, int inverse, void* hip_stream);

/* ---- EDIT LIST, SCALED: replay on tracks at a higher sample rate, int16 or float ----
 * The most common companion of a key is the master it was made from: a 44.1 or 48 kHz stereo float mix beside the 16 kHz mono track
 * the analysis wants.  spx_edit_replay_scaled is spx_edit_replay for such a track: speed and pitch are decided once, at the key's
 * rate, and the master is cut in the same places -- the cheap run plus one pass over the master's bytes (profiles/edit_scaled.txt).
 * tests/edit_scaled_ref.py states the definition below in Python integers.
 *
 * p / q is the master's rate over the key's (3/1, 2/1, 441/160, 320/147, 1/1 ...).  The library reduces it by its gcd and requires
 * 1 <= q <= p <= 32 q and p <= 32768 after the reduction.  S(x) = floor(x p / q); spx_edit_scale returns it on the host (-1 for a
 * ratio that is refused or x < 0).
 *
 * For stream i, with L as in spx_edit_replay: no = min(n_out[i], jobs[i].out_cap), N' = S(no), L' = min(S(L), tracks[i].n_in).
 * Record (out_at, a, b, n) covers master frames [S(out_at), S(out_at + n)), cut at N':
 *   n' = S(out_at + n) - S(out_at) -- at least 1 because p >= q: the extents tile [0, N') --, a' = S(a), b' = S(b), and output
 *   frame o of the record has t = o - S(out_at).  A source frame at or behind L' reads as 0 (+0.0f).
 *   copy                  y[a' + t]
 *   cross-fade, int16     (y[a' + t] * (n' - t) + y[b' + t] * t) / n', truncated toward zero; exact for every n' <= 65535 (the ratio
 *                         cap keeps every list the walk kernel writes far inside that)
 *   cross-fade, float     ((ya * (float)(n' - t)) + (yb * (float)t)) / (float)n': every operation rounded to float, no fused
 *                         multiply-add, the division correctly rounded; non-finite inputs give what IEEE arithmetic gives
 * At a non-integer ratio a' and b' are floored SEPARATELY, so the two ramps of a cross-fade can sit up to one master frame off the
 * exact ratio; at integer ratios the positions are exact.  At p == q with int16 the output is spx_edit_replay's, byte for byte.
 *
 *   jobs, ops, ops_cap, n_ops, n_out   exactly what spx_edit_replay takes (n_ops, n_out: DEVICE -- nothing comes back to the host)
 *   tracks   HOST   one per stream: in_off / out_off in ELEMENTS of the sample format from y_in / y_out; n_in / out_cap the track's
 *            own length and output capacity in frames at the master's rate; channels in 1 .. 65535
 *   sample_format   SPX_SAMPLES_INT16 (y_in, y_out: int16_t) or SPX_SAMPLES_FLOAT (float)
 *   y_in     DEVICE read only inside [0, L') of each track
 *   y_out    DEVICE nothing is written outside a stream's N' frames
 *   n_out_y  DEVICE int64[n_streams], written by the call:
 *              N'    the stream was rendered, N' frames
 *              -N'   N' > tracks[i].out_cap: nothing written for that stream
 *              0     n_out[i] <= 0, n_ops[i] <= 0 or n_ops[i] > ops_cap[i]: nothing written
 * No stream disturbs another; whatever the records hold, nothing is read outside [0, L') of a track or outside the stream's region
 * of ops.  Refused with -1 and spx_last_error before anything is enqueued, the outputs and the plan untouched: everything
 * spx_edit_replay refuses; a ratio outside the rule; an unknown sample_format; a NULL n_out_y; a negative n_in or out_cap; y_in or
 * y_out not aligned to the sample size; a stream with S(min(jobs[i].out_cap, 2^31 - 1)) or S(L) above 2^31 - 1 (master positions
 * fit int32 inside the kernel, as the key's do in spx_edit_replay's).
 * COST: one pass over the master's bytes, spx_edit_replay's kernel shape with the records scaled once per block.
 * OUT OF SCOPE: resampling the master down to the key, which stays the caller's job; lookups in master frames (scale the queries of
 * spx_edit_lookup with spx_edit_scale); the pipeline object.  (Tracks BELOW the key's rate -- labels, flags, feature rows -- are
 * "EDIT LIST, ROW TRACKS" below.) */
#define SPX_SAMPLES_INT16 0
#define SPX_SAMPLES_FLOAT 1
typedef struct { int64_t in_off, out_off, n_in, out_cap; int32_t channels, reserved; } spx_edit_master;
int64_t spx_edit_scale(int64_t x, int32_t p, int32_t q);
int spx_edit_replay_scaled(spx_plan_t plan, const spx_stream_job* jobs, int n_streams, const spx_edit_op* ops,
                           const int64_t* ops_cap, const int64_t* n_ops, const int64_t* n_out, const spx_edit_master* tracks,
                           int32_t p, int32_t q, int sample_format, const void* y_in, void* y_out, int64_t* n_out_y,
                           void* hip_stream);

/* ---- EDIT LIST, ROW TRACKS: warp label and feature tracks to the output's time and back ----
 * The companion a speech pipeline most often has sits BELOW the key's rate: phone or word labels at 100 Hz, VAD flags, filter-bank
 * or pitch features at a 10 ms hop, 20 ms encoder frames of 768 floats, a per-frame loss mask.  spx_edit_warp_rows brings such a
 * track from the INPUT's timeline onto the OUTPUT's (labels that fit the sped-up audio: speed augmentation with frame-level
 * targets); spx_edit_unwarp_rows brings a track on the OUTPUT's timeline (posteriors, VAD or embeddings a model computed on the
 * sped-up audio) back onto the INPUT's.  One search per row, whole rows moved; tests/edit_rows_ref.py states the definition below
 * in Python integers and np.float32 scalars.
 *
 * A ROW TRACK has hop H >= 1 key frames per row and a phase 0 <= phase < H: row j describes key frames [j H, (j + 1) H), and frame
 * j H + phase stands for it.  rows(x) = (x - phase + H - 1) / H for x > phase, else 0 -- the number of rows whose representative
 * frame lies below x; spx_edit_rows returns it on the host (-1 for frames < 0, a hop outside 1 .. 2^20 or a phase outside
 * [0, hop)).  A row has dim elements of elem_bytes (1, 2, 4 or 8) and is never interpreted outside BLEND mode; rows lie ld_in /
 * ld_out >= dim elements apart, and elements at or behind column dim are never read and never written.
 *
 * L, n_out, the SOURCE of an output frame, forward and inverse are those of POSITION LOOKUP above; no = min(n_out[i],
 * jobs[i].out_cap).  A ZERO ROW is dim elements of zero bytes.
 *
 * WARP (input time -> output time): stream i gets Ro = rows(no) rows.  For row j: u = j H + phase, k = the record that covers u
 * (the largest k with out_at(k) <= u), t = u - out_at(k).
 *   SPX_ROWS_NEAREST (any elem_bytes)   s = the source of the record at t; the row is input row s / H -- a zero row where s >= L
 *                      (the replay's "a source frame at or behind L reads as 0"; likewise s < 0, which no job's list holds) or
 *                      s / H >= the track's n_rows.
 *   SPX_ROWS_BLEND   (elem_bytes 4, float32)   a copy record gives NEAREST.  A cross-fade has two sources, a + t and b + t, each a
 *                      row (a + t) / H, (b + t) / H or a zero row by the same rule.  Where both are the same row (or both zero
 *                      rows) the output is that row, bit for bit; otherwise, per element,
 *                      ((ya * (float)(n - t)) + (yb * (float)t)) / (float)n: every operation rounded to float, no fused
 *                      multiply-add, the division correctly rounded -- spx_edit_replay_scaled's float cross-fade; non-finite
 *                      inputs give what IEEE arithmetic gives.
 * UNWARP (output time -> input time, NEAREST only): stream i gets Ri = rows(L) rows, a number the host knows.  For row r:
 * p = r H + phase, (o, k) = forward(p); the row is track row o / H -- a zero row where k = -1 (o = n_out: nothing at or behind p
 * survives) or o / H >= the track's n_rows.  It needs the index spx_edit_index wrote.
 *
 *   jobs, ops, ops_cap, n_ops, n_out   exactly what spx_edit_lookup takes (n_ops, n_out: DEVICE -- nothing comes back to the host)
 *   index    DEVICE what spx_edit_index wrote for these records (the unwarp only)
 *   tracks   HOST   one per stream: in_off / out_off in ELEMENTS from y_in / y_out; n_rows = the rows the track has at in_off;
 *            out_cap = the rows its region at out_off holds
 *   y_in, y_out   DEVICE, aligned to elem_bytes only; the two do not overlap.  Rows move in 16-byte accesses where a row's source
 *            and destination are aligned to 16, in the widest power of two they share otherwise
 *   n_rows_out   DEVICE int64[n_streams], written by the call: the number of rows written; MINUS that number where it exceeds
 *            tracks[i].out_cap, nothing written for that stream; 0, nothing written, for a stream with n_ops[i] <= 0 or
 *            n_ops[i] > ops_cap[i], for a warp with n_out[i] <= 0, for an unwarp with n_out[i] < 0
 * No stream disturbs another; whatever the records hold, nothing is read outside a track's n_rows rows or the stream's region of
 * ops and index, and nothing is written outside the rows counted.  Asynchronous on hip_stream.  Refused with -1 and spx_last_error,
 * nothing enqueued, the outputs untouched: everything spx_edit_lookup refuses; a NULL pointer (an unwarp without index says that it
 * needs spx_edit_index); hop < 1 or above 2^20; phase outside [0, hop); dim < 1 or above 65536; a stride below dim or above 2^28; an
 * elem_bytes outside the four; SPX_ROWS_BLEND with elem_bytes != 4; an unknown mode; a negative offset, n_rows or out_cap; y_in or
 * y_out misaligned for the element.
 * COST: one binary search per row in LDS and one pass over the rows' bytes (profiles/edit_rows.txt).
 * OUT OF SCOPE: blending in the unwarp direction; rows behind a rate stage; a hop per stream; a pipeline-object form; lists from
 * calls that record none; fractional row positions. */
#define SPX_ROWS_NEAREST 0
#define SPX_ROWS_BLEND 1
typedef struct { int64_t in_off, out_off, n_rows, out_cap; } spx_edit_rows_track;   /* HOST: offsets in elements, counts in rows */
int64_t spx_edit_rows(int64_t frames, int32_t hop, int32_t phase);
int spx_edit_warp_rows(spx_plan_t plan, const spx_stream_job* jobs, int n_streams, const spx_edit_op* ops, const int64_t* ops_cap,
                       const int64_t* n_ops, const int64_t* n_out, const spx_edit_rows_track* tracks, int32_t hop, int32_t phase,
                       int32_t dim, int64_t ld_in, int64_t ld_out, int elem_bytes, int mode, const void* y_in, void* y_out,
                       int64_t* n_rows_out, void* hip_stream);
int spx_edit_unwarp_rows(spx_plan_t plan, const spx_stream_job* jobs, int n_streams, const spx_edit_op* ops, const int64_t* ops_cap,
                         const int64_t* n_ops, const int64_t* n_out, const int32_t* index, const spx_edit_rows_track* tracks,
                         int32_t hop, int32_t phase, int32_t dim, int64_t ld_in, int64_t ld_out, int elem_bytes, const void* y_in,
                         void* y_out, int64_t* n_rows_out, void* hip_stream);

/* ---- BATCH DTW: align pairs of feature sequences on the device -- cost, warp path and slopes per pair ----
 * The reference's perceptual check (TestSpeechSample, sonic_test.cc:639-724) aligns the spectrogram of the output to that of the
 * input by dynamic time warping (dynamic_time_warping.{h,cc}) and asks whether the warp path has the slope the speed promised.
 * spx_batch_dtw does that for a batch of pairs in device memory -- the `spectrogram` tap of spx_batch_run / spx_batch_analyze can be
 * handed over where it lies -- and leaves cost, path and slope figures in device memory.  tests/dtw_ref.py states the definition
 * in Python float32 scalars; the kernels are held to it bit for bit.
 *
 * For sequences a (n_a rows) and b (n_b rows) of dim floats:
 *   local cost   d(i, j): s = 0; for k = 0 .. dim - 1 IN THIS ORDER: t = a[i][k] - b[j][k], s = s + t * t; d = sqrtf(s).  Every
 *                operation rounded to float, no fused multiply-add, the square root correctly rounded (EuclideanDistance,
 *                sonic_test.cc:200-209).
 *   recurrence   (dynamic_time_warping.cc:76-100)  C(0,0) = d(0,0), direction 0; first row C(0,j) = d(0,j) + C(0,j-1), direction
 *                +1; first column C(i,0) = d(i,0) + C(i-1,0), direction -1; elsewhere, with up = C(i-1,j), left = C(i,j-1),
 *                diag = C(i-1,j-1): C(i,j) = d(i,j) + min(min(up, left), diag), direction -1 if up < diag && up < left, +1 if
 *                left < up && left < diag, else 0 -- strict comparisons, ties go along the diagonal.  cost = C(n_a-1, n_b-1).
 *   path         (:102-132)  from (n_a-1, n_b-1): record (i, j); direction -1: i--, 0: i--, j--, +1: j--; until an index is below
 *                0.  Reversed: n_path <= n_a + n_b - 1 pairs, the first (0, 0).
 *   slope        (LinearSlope, sonic_test.cc:86-99)  x = the path's a indices, y = its b indices; four float sums added in path
 *                order, x*y and x*x formed as exact integers and then converted; slope = (n*sumXY - sumX*sumY) / (n*sumX2 -
 *                sumX*sumX) in float, n = (float)n_path.
 *   local slopes (LinearSlopeEverywhere, VectorMean, VectorStandardDeviation, :101-133)  window p = the same slope over path
 *                entries p - h .. p + h - 1, p = h .. n_path - h - 1: n_local = max(0, n_path - 2 h) of them.  local_mean: the
 *                slopes added in order in a double, rounded to float, divided by (float)n_local.  local_std: diff = slope - mean
 *                and diff * diff in float, added in order in a double, rounded to float, divided by (float)n_local, sqrtf.
 * A zero denominator -- n_path = 1, a window in which a does not advance, n_local = 0 -- gives what IEEE arithmetic gives: NaN or
 * an infinity.  DOMAIN: finite inputs whose accumulated costs stay finite; outside it the results are unspecified.
 *
 *   jobs      HOST   one per pair: a_off / b_off = the first value of the pair's rows, in floats from a / b; path_off = its first
 *                    path entry, in entries (int32 pairs: a index, b index) from `path`; n_a, n_b >= 1 rows, n_a * n_b <= 2^30
 *   dim       values per row that take part, 1 .. 65536;  ld_a, ld_b >= dim: floats from one row to the next.  Values at or behind
 *             column dim of a row are never read: with ld = N (spx_plan_fft_size) and dim = N / 4 the spectrogram tap is aligned
 *             in place on its low bins, as the reference's ComputeSpectrogram keeps them.
 *   a, b      DEVICE float rows;  results  DEVICE [n_pairs];  path  DEVICE: n_a + n_b - 1 entries per pair from path_off -- the
 *             regions are the caller's, not checked for overlap; entries at or behind n_path are not written
 *   workspace DEVICE, spx_dtw_workspace_bytes (0 with spx_last_error for a table the call refuses): two bits per cell of direction,
 *             rounded up to 64 columns, and 16 bytes per row and column -- the cost matrix itself is never stored.  Its contents
 *             on entry do not matter (a partial tile writes its own cells' bits and zeros in the rest of its words), nor do
 *             those of results and path
 *   plan      the device, and the staging of the job table: what spx_edit_replay and spx_map_lookup use it for.  The sample rate
 *             plays no part.
 * Asynchronous on hip_stream; nothing comes back to the host.  Refused with -1 and spx_last_error, nothing enqueued, the outputs
 * untouched: a NULL pointer; n_pairs < 1; dim < 1 or above 65536; a row stride below dim; half_width < 1; n_a or n_b below 1;
 * n_a * n_b > 2^30; a negative offset; a workspace below spx_dtw_workspace_bytes.
 * COST: one workgroup per pair -- a pair's recurrence is one chain -- in two launches; profiles/dtw.txt.
 * OUT OF SCOPE: a distance other than the Euclidean one; banded or windowed warping; a pipeline-object form; DTW inside the _run
 * calls. */
typedef struct { int64_t a_off, b_off; int64_t path_off; int32_t n_a, n_b; } spx_dtw_job;                             /* HOST, 32 bytes */
typedef struct { float cost, slope, local_mean, local_std; int32_t n_path, n_local; } spx_dtw_result;                 /* DEVICE, 24 bytes */
size_t spx_dtw_workspace_bytes(const spx_dtw_job* jobs, int n_pairs, int dim);
int spx_batch_dtw(spx_plan_t plan, const spx_dtw_job* jobs, int n_pairs, int dim, int ld_a, int ld_b, int half_width,
                  const float* a, const float* b, spx_dtw_result* results, int32_t* path,
                  void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- TWO PASSES IN ONE CALL: every stream to a target length, or the linear control at the nonlinear duration ----
 * The reference's CLI has two two-pass drivers (speedy_wave.cc:424-462): --length runs a nonlinear pass at the requested speed,
 * measures what came out and runs the final pass at want * (want / achieved), so that the output lands on the requested duration;
 * --match_nonlinear runs the same measuring pass and then the final (normally linear) pass at exactly the achieved speed.
 * spx_batch_run_twopass is both, per stream, for a whole batch -- asynchronous on hip_stream, with NO host wait and no
 * device-to-host copy between the passes: the second-pass speeds are worked out on the device.
 *   seconds  HOST double[n_streams] or NULL.  Per stream i, with T = jobs[i].n_in and rate = the plan's sample rate:
 *     MATCH   seconds == NULL or seconds[i] == 0:   want = (double)jobs[i].speed
 *     LENGTH  seconds[i] > 0:   want = (double)((float)T / (float)rate) / seconds[i]   (jobs[i].speed is ignored)
 *   probe pass   the job with speed (float)want, nonlinear 1 and the job's feedback; its count goes to n_probe[i]
 *   achieved     got = (double)T / (double)n_probe[i]
 *   speeds[i]    MATCH (float)got;  LENGTH (float)(want * (want / got));  n_probe[i] <= 0 (an empty stream, one too short to emit
 *                anything, out_cap too small for the probe, a lost producer): (float)want.  IEEE double arithmetic, each operation
 *                rounded once; the types and rounding points of tools/speedy_wave_hip.cpp:179-191.
 *   final pass   the job as given, at speed speeds[i]
 *   n_probe, speeds   DEVICE int64[n_streams], float[n_streams]: written by the call, for the caller to read behind it
 * out, n_out and the taps are byte for byte what spx_batch_run gives the final table (the jobs with speeds[i] as their speed): a
 * negative n_out where out_cap is too small, nothing written past out_off + out_cap * channels.  The probe pass's audio passes
 * through the same out region first (at most out_cap frames of it); values of the region behind the final count are unspecified.
 * Refused with -1 and spx_last_error, nothing enqueued, the plan as it was: whatever spx_batch_run refuses in the probe table or in
 * the final table; a NULL n_probe or speeds; a seconds[i] that is negative or not finite; a want whose float value is not finite and
 * > 0 (LENGTH on an empty stream is one); a stream with want * want * (out_cap + 1) >= 1e18 -- the bound that keeps every speed the
 * device can compute inside the range the walk kernels serve; a workspace smaller than spx_batch_workspace_bytes_twopass (the probe
 * table's spx_batch_workspace_bytes and the retarget table behind it; 0 with spx_last_error for a table that is refused;
 * what it, out, n_out, n_probe, speeds and the taps hold on entry does not matter).
 * CAPACITY: spx_plan_out_capacity_twopass(n_in, want, nonlinear) is the larger of spx_plan_out_capacity_for(n_in, (float)want, 1)
 * -- the probe -- and spx_plan_out_capacity_for(n_in, (float)want, nonlinear); -1 for values spx_batch_run refuses.  What that covers
 * of the final pass, whose speed is not known beforehand:
 *   want >= 1   n_in + slack: a second-pass speed >= 1, nonlinear or linear.  MATCH stays there (a nonlinear probe at a speed >= 1
 *               never emits more than it consumes, so got >= 1 up to the flush padding of a stream of a few hundred frames); LENGTH
 *               leaves it when got > want * want, that is when the probe overshot a want close to 1 by more than want itself.
 *   want < 1    (n_in + flush padding) * 200 + slack: every second-pass speed of a nonlinear job, and of a linear job down to 0.01.
 * Outside of that the final count may come back negative -- never a write past the region.
 * COST: where every final job is nonlinear the second pass runs WITHOUT an analysis launch, on the frame records the first pass
 * left in the workspace (spx_debug_last_twopass bit 0) -- the analysis does not depend on the speed; a batch with a linear final job
 * runs the second pass's analysis for whatever is nonlinear.  The second pass's kernels run in sequence on hip_stream, and its walk
 * kernel is the any-speed instantiation (the speed class cannot be read off a speed the host does not know).  Measured, 256 x 10 s,
 * 16 kHz mono, LENGTH at 3.5x, call after call (profiles/twopass.txt): this call 4.03 ms; the loop a caller writes without it --
 * spx_batch_run, the counts to the host, the formula, spx_batch_run -- 3.55 ms; one spx_batch_run 1.72 ms.  So for such a batch the
 * call is 0.48 ms SLOWER than the loop: both of the loop's calls run their three kernels side by side on the speed-up-only walk
 * kernel, where the analysis hides beside the walk kernel (saving its launch saves nothing a step waits for), and the loop's idle gap
 * is only about 0.1 ms.  The second pass here takes 2.31 ms, and a kernel trace says where: retarget kernel 5 us, tension kernel
 * 33 us, no gap between the passes, and a walk kernel of 2.19 ms in its any-speed instantiation against 1.71 in the speed-up-only
 * one -- the whole 0.48 ms.  What the call offers today is its shape -- one asynchronous call, no host wait between the passes -- not
 * time; a speed class decided on the device (the speed-up-only kernel where every patched speed is above 1) is the follow-up.  Consecutive calls: the second pass's job table waits, on the host, for the staging kernel of the
 * previous call's second pass (the plan's two pinned staging slots taking turns), that is until the previous call's first pass has
 * finished -- the GPU still has the previous second pass to run by then.
 * The plain call only.  OUT OF SCOPE: the _rate, _float, _map, _ahead / _overlapped and _mixed* forms, the pipeline object, a probe
 * that writes no audio, more than one correction step. */
size_t spx_batch_workspace_bytes_twopass(spx_plan_t plan, const spx_stream_job* jobs, const double* seconds, int n_streams);
int64_t spx_plan_out_capacity_twopass(spx_plan_t plan, int64_t n_in, double want, float nonlinear);
int spx_batch_run_twopass(spx_plan_t plan, const spx_stream_job* jobs, const double* seconds, int n_streams, const int16_t* in,
                          int16_t* out, int64_t* n_out, int64_t* n_probe, float* speeds, void* workspace, size_t workspace_bytes,
                          const spx_taps* taps, void* hip_stream);
/* Diagnostics: bit 0 = the last two-pass call reused the first pass's analysis. */
int spx_debug_last_twopass(void);

/* spx_batch_run_rate on FLOAT samples in device memory (sonicWriteFloatToStream / sonicReadFloatFromStream, sonic2.h:64-68).
 *   in   DEVICE  float input samples in (-1, 1), 4-byte aligned; read once, exactly the jobs' values: no padding behind the end
 *   out  DEVICE  float output samples, 4-byte aligned (every value an int16 / 32767.0f, the IEEE quotient)
 * The job table is the same 48-byte table: in_off / out_off count FLOAT VALUES inside in / out, n_in / out_cap are frames as always,
 * capacities come from spx_plan_out_capacity_for / _rate unchanged.  rates == NULL: every rate 1.  n_out has exactly
 * spx_batch_run_rate's meaning: negative = out_cap was too small, and then exactly out_cap frames were written.
 * The INPUT SCALE is per job, as the reference has it: nonlinear != 0 gives (double)x * 32768.0 (soniclib.c:496), nonlinear == 0
 * gives x * 32767.0f in float (the TSM dependency's own scale).  The conversion to int16 is DEFINED here, because the C cast is
 * undefined outside the short range: truncate toward zero to a 32-bit integer and keep the low 16 bits -- what the streaming API's
 * host loop does on x86; full scale 1.0f on a nonlinear job gives -32768 -- and a product that is NaN or of magnitude >= 2^31
 * gives 0.
 * A layer on top of the int16 call: the call enqueues, on hip_stream and without a host wait, the job table's way into the
 * workspace and the input conversion, then spx_batch_run_rate (spx_batch_run when every rate is 1: the int16 work is that call's,
 * bit for bit) on int16 stagings inside the workspace, then the output conversion, which reads n_out on the device.  Taps are
 * passed through.  The workspace (spx_batch_workspace_bytes_float, 256-byte aligned as every device allocation is) begins with the
 * int16 call's own workspace, so spx_batch_read_steps works on it; behind it lie the table and the two stagings.
 * Its contents on entry do not matter, nor those of out, n_out and the taps.
 * Refused with -1 and spx_last_error, nothing launched: everything the int16 call refuses (a bad speed, rate, nonlinear factor ...),
 * a null pointer, in or out not 4-byte aligned, a workspace that is too small.
 * NOT offered on float samples: the _ahead / _overlapped / _mixed* forms on caller-owned buffers and spx_batch_pack_outputs.  (The
 * pipeline object takes float samples: SPX_PIPELINE_FLOAT below.) */
size_t spx_batch_workspace_bytes_float(spx_plan_t plan, const spx_stream_job* jobs, const float* rates, int n_streams);
int spx_batch_run_float(spx_plan_t plan, const spx_stream_job* jobs, const float* rates, int n_streams, const float* in,
                        float* out, int64_t* n_out, void* workspace, size_t workspace_bytes,
                        const spx_taps* taps, void* hip_stream);
/* The two conversions on their own, n contiguous values, asynchronous on hip_stream.
 * nonlinear_scale != 0: the 32768.0 double scale, else 32767.0f. */
int spx_float_to_short(const float* in, int16_t* out, size_t n, int nonlinear_scale, void* hip_stream);
int spx_short_to_float(const int16_t* in, float* out, size_t n, void* hip_stream);

/* spx_batch_run for a caller that issues batch after batch (round 4): consecutive calls are software-pipelined.  This call's
 * analysis and tension kernels are enqueued on a stream of the library's and start AT ONCE -- beside the walk kernel of the
 * previous call, which is still running on hip_stream -- and its own walk kernel follows on hip_stream with every speed ready.
 * Same results as spx_batch_run.  The caller's side of the contract:
 *   - `in` is complete in device memory when the call is made (the analysis does not wait for work queued on hip_stream), and
 *     nothing still pending on hip_stream touches workspace, taps, out or n_out: the call's staging, analysis and tension kernels
 *     write the workspace and the taps on the library's stream at once;
 *   - consecutive calls alternate (at least) two workspaces / out / n_out buffers; a call that hands over the previous call's
 *     workspace again waits for that call to finish instead (correct, no overlap);
 *   - hip_stream is the same stream call after call; when it has drained, every kernel of every call issued on it has.
 * Batches that do not fit the shape (kernels that do not fit side by side ...) run exactly as spx_batch_run would -- with one
 * exception since round 6: a call of more than two streams per CU (two time ranges, kernels in sequence) still starts its PRODUCERS
 * at once on the library's stream, so that call k + 1's first analysis range runs beside call k's last walk range (2 048 x 10 s per
 * call, call after call: 6.21 -> 5.85 ms); the contract above is what makes that legal. */
int spx_batch_run_ahead(spx_plan_t plan, const spx_stream_job* jobs, int n_streams, const int16_t* in,
                        int16_t* out, int64_t* n_out, void* workspace, size_t workspace_bytes,
                        const spx_taps* taps, void* hip_stream);

/* spx_batch_run_ahead with the WALK kernels of consecutive calls overlapping as well: a call's walk kernel runs on a stream of
 * the library's (two, taking turns) and hip_stream only waits for it, so the walk of call k + 1 starts as soon as its own
 * speeds are there, beside the walk of call k -- two walk workgroups per CU run at nearly full speed each, and the longest
 * chains of one batch no longer hold the next batch back (BASELINE configs[3]: 1.60 -> 1.39 ms per batch with two buffer sets
 * taking turns, 1.16 with three: a call's producers then start while the walk kernels of both previous calls are running, and
 * the walk kernel is launched in its lean form, which leaves the analysis kernel two waves per SIMD beside two walk workgroups).
 * The price is a RELAXED stream order, on top of spx_batch_run_ahead's contract:
 *   - work the caller enqueues on hip_stream AFTER call k is ordered behind call k's kernels as always (it sees call k's output),
 *     but call k + 1's walk kernel is ordered only behind what was on hip_stream when call k was MADE: whatever the caller
 *     enqueues between call k and call k + 1 must not touch call k + 1's buffers (two buffer sets taking turns, each consumed
 *     right behind its own call, satisfy this by construction; a call that hands over the previous call's out / n_out or
 *     workspace again is ordered behind everything, as spx_batch_run_ahead would order it).
 * Everything else as spx_batch_run_ahead; shapes outside the mode run as spx_batch_run would. */
int spx_batch_run_overlapped(spx_plan_t plan, const spx_stream_job* jobs, int n_streams, const int16_t* in,
                             int16_t* out, int64_t* n_out, void* workspace, size_t workspace_bytes,
                             const spx_taps* taps, void* hip_stream);

/* The same for input that is still on its way when the call is made (a host-to-device copy on another stream):
 * in_ready_event is a hipEvent_t the caller has recorded behind whatever completes `in`; the call's producers wait for it
 * (NULL: as spx_batch_run_ahead). */
int spx_batch_run_ahead_when(spx_plan_t plan, const spx_stream_job* jobs, int n_streams, const int16_t* in,
                             int16_t* out, int64_t* n_out, void* workspace, size_t workspace_bytes,
                             const spx_taps* taps, void* hip_stream, void* in_ready_event);

/* ---- the owning pipeline (round 5): batch after batch, host memory to host memory ----
 * What the reference's caller loop does per stream -- write a chunk, read what is ready, again (speedy_wave.cc:154-242) -- for a
 * caller that feeds BATCHES: spx_pipeline_submit hands over one batch of input (host or device memory), spx_pipeline_wait returns
 * that batch's output.  The object OWNS everything in between: `depth` sets of device buffers (input, output, workspace), pinned
 * host buffers for the output, its HIP streams and events.  Inside, the library issues the host-to-device copy, the three kernels
 * in the overlapped order of spx_batch_run_overlapped (batch k + 1's analysis beside batch k's walk kernel, the walk kernels of
 * consecutive batches overlapping) and a gather kernel that writes the produced frames of all streams, densely packed, straight
 * into pinned host memory -- no device-to-host copy is enqueued and no host thread waits inside submit, so copies in, kernels and
 * copies out of up to `depth` batches are in flight at once.  The relaxed stream order that spx_batch_run_overlapped asks its
 * caller to respect is an implementation detail here: nobody else can touch the buffers.
 *   jobs      the shape of every batch of spx_pipeline_submit, and the CAPACITY of the pipeline for spx_pipeline_submit_jobs: n_in,
 *             channels, speed, nonlinear, feedback and in_off (where stream i -- lane i -- starts in a batch's input, in int16
 *             values); out_off / out_cap are ignored (the pipeline lays the outputs out itself, capacity =
 *             spx_plan_out_capacity_for)
 *   plans / plan_index   as in spx_batch_run_mixed, for batches that mix sample rates (spx_pipeline_create: one plan)
 *   depth     buffer sets, 2 .. 8 (0 = the default, 4); 3 or more let the walk kernels of consecutive batches overlap fully
 *   flags     SPX_PIPELINE_DEVICE_OUT: the outputs stay in device memory (no gather, no copy out).  Such a pipeline's calls are
 *             detached from its run stream, and since round 6 that holds for mixed-rate batches too: the groups' walk kernels of
 *             consecutive batches overlap on the library's walk streams (BASELINE configs[4] shard: 1.87 - 1.97 -> 1.56 ms per batch).
 *             With SPX_PIPELINE_FLOAT as well the output conversion runs behind a batch's walk kernel, so such a batch cannot be
 *             detached: it takes the engine order the host-output pipeline takes.
 *             SPX_PIPELINE_FLOAT: a pipeline on float samples (the _float calls further down); combines with the above.
 * NULL with spx_last_error ("spx_pipeline: lane N: " and the rule) for a creation table with a job spx_batch_run would refuse.
 * Not thread-safe: one host thread (or external locking) per pipeline; several pipelines may be alive at once. */
typedef struct spx_pipeline* spx_pipeline_t;
#define SPX_PIPELINE_DEVICE_OUT 1u
#define SPX_PIPELINE_FLOAT 2u   /* flags of spx_pipeline_create / spx_pipeline_create_mixed; combines with SPX_PIPELINE_DEVICE_OUT */
spx_pipeline_t spx_pipeline_create(spx_plan_t plan, const spx_stream_job* jobs, int n_streams, int depth, unsigned flags);
spx_pipeline_t spx_pipeline_create_mixed(const spx_plan_t* plans, int n_plans, const spx_stream_job* jobs, const int* plan_index,
                                         int n_streams, int depth, unsigned flags);
void spx_pipeline_destroy(spx_pipeline_t p);
int spx_pipeline_depth(spx_pipeline_t p);
/* int16 values of one batch's input: max over streams of in_off + n_in * channels. */
size_t spx_pipeline_input_values(spx_pipeline_t p);
/* Pinned host staging (spx_pipeline_input_values() int16 values) for the batch the NEXT submit hands over: a caller that produces
 * its input there saves a host copy and gets the full link rate.  Blocks until the copy that last read this buffer (`depth`
 * submits ago) has finished.  Any other host pointer (pinned or pageable) may be given to submit as well. */
int16_t* spx_pipeline_host_input(spx_pipeline_t p);
/* Hand over one batch.  in: HOST memory (in_is_device = 0) -- must stay unchanged until the batch's input has been copied
 * (spx_pipeline_input_consumed, or the batch's spx_pipeline_wait) -- or DEVICE memory (in_is_device = 1), complete when the call is
 * made and unchanged until the batch's spx_pipeline_wait returns; a device buffer is passed to the kernels as it is, and their
 * aligned window loads may touch up to 64 int16 values behind the last stream's end: it must be ALLOCATED for
 * spx_pipeline_input_values() + 64 values (the content of the padding does not matter; the same holds for the `in` of the
 * spx_batch_* calls).  Returns the batch's ticket (0, 1, 2 ...) or a negative error.
 * At most `depth` batches are in flight: the call waits for the batch `depth` tickets back first. */
int64_t spx_pipeline_submit(spx_pipeline_t p, const int16_t* in, int in_is_device);
/* spx_pipeline_submit with THIS batch's job table.  The table given to spx_pipeline_create becomes the pipeline's CAPACITY: lane i
 * takes any job that fits what lane i was created with.  (spx_pipeline_submit(p, in, d) is this call with the creation table.)
 *   jobs   HOST array of exactly the n_streams the pipeline was created with; copied before the call returns.  Read: in_off, n_in,
 *          speed, nonlinear, feedback and channels.  out_off / out_cap are ignored: the pipeline keeps the output layout and the
 *          capacities of its creation and hands those to the engine.  channels must be the lane's channel count at creation; the
 *          lane's plan (plan_index of a mixed pipeline) is fixed as well.  n_in = 0 is an empty lane (count 0, no room in the packed
 *          output): a batch with fewer live streams than lanes.
 * The table is accepted if and only if, for every lane,
 *   - the job is one spx_batch_run takes (speed finite and > 0, nonlinear in [0, 1], feedback finite, fewer than 2^30 frames ...),
 *   - in_off >= 0 and in_off + n_in * channels <= spx_pipeline_input_values(p),
 *   - spx_plan_out_capacity_for(the lane's plan, n_in, speed, nonlinear) <= the lane's capacity at creation,
 * and spx_batch_workspace_bytes (_mixed) of the table <= that of the creation table: the workspace grows with the number of analysis
 * frames, so linear lanes turned nonlinear can exceed it where no lane exceeds its output capacity.
 * SIZING: for speed >= 1 the capacity is n_in + slack whatever the speed -- a pipeline created with the longest n_in per lane and
 * nonlinear = 1 admits every shorter job at any speed >= 1, linear or nonlinear.  A slow-down lane must be created with the
 * smallest speed it will see (and nonlinear, if it will ever be: the nonlinear capacity of a slow-down assumes the 0.01 clamp).
 * A table that is refused returns -1 with spx_last_error naming the lane and the limit, BEFORE anything is waited for, copied or
 * enqueued: no ticket number is used up, batches in flight are untouched, the pipeline stays fully usable.
 * HOST input is copied up to this batch's extent only -- max over lanes of in_off + n_in * channels -- and need not be longer; DEVICE
 * input is allocated for spx_pipeline_input_values() + 64 values as always.  Values behind a short lane's end may hold another
 * lane's samples or an earlier batch's: padding, whose content does not matter.
 * Tickets, depth, spx_pipeline_wait, spx_pipeline_input_consumed and spx_pipeline_host_input as for spx_pipeline_submit; with
 * SPX_PIPELINE_DEVICE_OUT the offsets stay the static capacity layout.  Results per stream are those of spx_batch_run on the same
 * job and samples; fixed-shape and varying batches may be mixed freely on one pipeline.  (A table whose speed class differs from
 * the previous batch's -- a lane at speed < 1 behind speed-up batches -- takes other walk kernels and may take another launch
 * order: slower or faster, the same bytes.) */
int64_t spx_pipeline_submit_jobs(spx_pipeline_t p, const spx_stream_job* jobs, const int16_t* in, int in_is_device);
/* 0 if spx_pipeline_submit_jobs would accept this table, else -1 and spx_last_error names the lane and the limit.  Enqueues nothing,
 * waits for nothing. */
int spx_pipeline_jobs_fit(spx_pipeline_t p, const spx_stream_job* jobs);
/* Blocks until the input handed over with `ticket` may be overwritten: the copy in has finished (host input), the batch's kernels
 * have finished (device input: they read it to the end).  On a float pipeline (SPX_PIPELINE_FLOAT) an input of EITHER kind is
 * consumed once its conversion has run -- the call returns then, not at the end of the batch: a device tensor may be reused a whole
 * batch earlier than on an int16 pipeline.  0, or a negative error (unknown ticket). */
int spx_pipeline_input_consumed(spx_pipeline_t p, int64_t ticket);
/* Wait for a batch.  On return
 *   *out      the output samples: pinned HOST memory owned by the pipeline (DEVICE memory with SPX_PIPELINE_DEVICE_OUT)
 *   *offsets  HOST int64[n_streams + 1]: stream i's samples are out[offsets[i] .. offsets[i] + counts[i] * channels[i]); every
 *             offset is a multiple of 32 values (64 bytes); offsets[n_streams] = the extent of the packed output
 *   *counts   int64[n_streams]: produced frames per stream as spx_batch_run's n_out (negative = capacity overflow); HOST memory,
 *             DEVICE memory with SPX_PIPELINE_DEVICE_OUT
 * valid until `depth` more batches have been submitted.  Tickets may be waited for in any order, each at most once per buffer
 * life; a ticket whose buffers have been handed to a later batch returns an error. */
int spx_pipeline_wait(spx_pipeline_t p, int64_t ticket, const int16_t** out, const int64_t** offsets, const int64_t** counts);

/* ---- the pipeline object on FLOAT samples: spx_pipeline_create / _create_mixed with SPX_PIPELINE_FLOAT ----
 * sonicWriteFloatToStream / sonicReadFloatFromStream (sonic2.h:64-68) for a caller that feeds batches of float audio -- a loader's
 * float32 in host memory, a model's waveform in device memory -- with both conversions on the GPU, inside the pipeline's own order.
 * CREATION AND FIT are those of every pipeline: the same tables, the same capacity rules, the same "lane N:" messages;
 * spx_pipeline_input_values() counts FLOAT values and is the same number as for int16; in_off counts float values inside `in`;
 * spx_pipeline_jobs_fit works unchanged.  The conversions do not depend on a plan: spx_pipeline_create_mixed takes the flag too.
 * INPUT CONVERSION: spx_batch_run_float's rule exactly, per lane, by the nonlinear factor of THIS BATCH's job: nonlinear != 0 gives
 * (double)x * 32768.0, nonlinear == 0 gives x * 32767.0f; then truncate toward zero to 32 bits and keep the low 16 bits; a product
 * that is NaN or of magnitude >= 2^31 gives 0.  OUTPUT: every value is an int16 / 32767.0f, the IEEE quotient.
 * What a submit enqueues, without a host wait beyond the one for the batch `depth` tickets back: on the pipeline's copy stream the
 * copy in (host input), this batch's conversion table and one conversion launch over (block, lane) into the int16 staging the engine
 * reads; the engine as for an int16 batch; and on the run stream a gather kernel that converts while it packs and writes floats
 * straight into pinned host memory (SPX_PIPELINE_DEVICE_OUT: a conversion behind the walk kernel into a float buffer on the device).
 *   HOST input    is copied up to the batch's extent only: extent x 4 bytes (spx_pipeline_submit_float: the creation table's).
 *   DEVICE input  is read exactly over the jobs' values, by the conversion and not by the walk kernel's window loads: NO 64-value
 *                 padding is needed, only 4-byte alignment; complete when the call is made, unchanged until
 *                 spx_pipeline_input_consumed (above: it returns once the conversion has run, for either kind of input).
 * spx_pipeline_wait_float, host output: *out is pinned HOST memory holding floats; *offsets count float values and, with *counts,
 * are the SAME NUMBERS the int16 pipeline reports for the same batch -- every offset a multiple of 32 values, here 128 bytes; an empty
 * lane takes no room; the values between a stream's last frame and the next offset are unspecified.  With SPX_PIPELINE_DEVICE_OUT:
 * *out is a float buffer in DEVICE memory in the static capacity layout (the creation offsets), *counts are in device memory.
 * A negative count converts min(|count|, capacity) frames and a lost producer none, as in the int16 gather.
 * WRONG-KIND CALLS -- spx_pipeline_submit, _submit_jobs, _wait, _host_input on a float pipeline; the _float calls on an int16 one --
 * return -1 (NULL) with a message that names the flag, before anything is waited for, copied or enqueued: no ticket is used up and
 * the pipeline stays fully usable.  A float pointer that is not 4-byte aligned is refused the same way.
 * Playback rates on float samples: spx_pipeline_create_rate with the flag and spx_pipeline_submit_jobs_rate_float, further down.
 * STILL OUT OF SCOPE: float _ahead / _overlapped / _mixed* calls on caller-owned buffers, a float spx_batch_pack_outputs. */
/* Pinned host staging of spx_pipeline_input_values() floats for the next submit, as spx_pipeline_host_input. */
float* spx_pipeline_host_input_float(spx_pipeline_t p);
int64_t spx_pipeline_submit_float(spx_pipeline_t p, const float* in, int in_is_device);
int64_t spx_pipeline_submit_jobs_float(spx_pipeline_t p, const spx_stream_job* jobs, const float* in, int in_is_device);
int spx_pipeline_wait_float(spx_pipeline_t p, int64_t ticket, const float** out, const int64_t** offsets, const int64_t** counts);

/* ---- the RATE PIPELINE: a playback rate per lane and per batch (sonicSetRate before the first write, sonic2.h:70) ----
 * A one-plan pipeline whose lanes each carry a playback rate, which may differ from batch to batch as the job table may.  A lane's
 * output is byte for byte what spx_batch_run_rate gives the same job, rate and samples (on float samples: spx_batch_run_float).
 * CREATION  spx_pipeline_create with one more table:
 *   rates   HOST float[n_streams]: the rate each lane is SIZED FOR; NULL = every rate 1, as in spx_batch_run_rate
 *   flags   SPX_PIPELINE_DEVICE_OUT and SPX_PIPELINE_FLOAT, in any combination
 * A lane's capacity, in FINAL frames (behind the rate stage), is spx_plan_out_capacity_rate(plan, n_in, speed, nonlinear, rate); the
 * output layout is every pipeline's (regions at multiples of 32 values).  The workspace is sized so that EVERY lane can resample,
 * the lanes created at rate 1 included: it reserves the speed stage's staging of all its lanes, and a lane created at rate 1 takes
 * rate 2 in the next batch.  NULL with spx_last_error, "spx_pipeline: lane N: " and the rule, for a job spx_batch_run refuses or a
 * rate spx_batch_run_rate refuses (not finite, <= 0, (int)(sample rate / rate) < 1).  There is no mixed-sample-rate form, as
 * spx_batch_run_rate has none.
 * FIT  spx_pipeline_jobs_fit_rate, which both submit calls below apply before anything is waited for, copied or enqueued.  A table
 * with its rates (NULL = every rate 1) is accepted if and only if
 *   - every rule of spx_pipeline_jobs_fit holds (channels, the engine's job rules, the input's extent), its capacity rule in final
 *     frames:  spx_plan_out_capacity_rate(plan, n_in, speed, nonlinear, rates[i]) <= the lane's capacity at creation,
 *   - every rate is one spx_batch_run_rate takes,
 *   - spx_batch_workspace_bytes_rate of the table with these rates <= the pipeline's workspace.
 * A refusal returns -1 and names the lane and the limit -- the rate itself, the capacity in final frames with both numbers, or the
 * workspace -- uses up no ticket and leaves the batches in flight untouched.  The rule is the inequality, not "rate >= the creation
 * rate": the rate stage works with both sample rates halved until they fit 14 bits, so the capacity is not promised monotone in the
 * rate.  SIZING, as advice: create a lane with the longest n_in, the smallest speed if below 1, and the smallest rate it will see.
 * THE OTHER CALLS on a rate pipeline: spx_pipeline_submit / _submit_float run the creation table at the creation rates;
 * spx_pipeline_submit_jobs / _submit_jobs_float / _jobs_fit mean "every rate 1" (the _rate call with rates == NULL); wait,
 * wait_float, input_consumed, host_input(_float), input_values and depth are unchanged, and so is the int16 / float wrong-kind rule.
 * Offsets and counts are in final frames and values, offsets multiples of 32, an empty lane takes no room; with
 * SPX_PIPELINE_DEVICE_OUT the offsets are the static layout and the counts are in device memory.
 * The three _rate calls on a pipeline NOT made by spx_pipeline_create_rate return -1 with a message that names
 * spx_pipeline_create_rate, before anything is waited for or enqueued; spx_pipeline_create / _create_mixed are what they were.
 * WHAT A SUBMIT ENQUEUES  A batch whose rates are all 1 is an ordinary pipeline batch: the overlapped order (detached where an
 * ordinary batch is), and the bytes, counts and offsets of a pipeline made by spx_pipeline_create from the same table.  A batch with
 * at least one rate other than 1: the copy stream does what it always does (copy in, on float samples the conversion); then, on the
 * run stream and behind the input, the engine runs the batch AS spx_batch_run_rate RUNS IT -- analysis, tension, the general walk
 * kernel without flush truncation into the speed-stage staging of the slot's workspace, the rate kernel into the slot's output,
 * kernels in sequence, rate-1 lanes bypassed as in the batch call -- and behind it the gather (or the float conversion) every batch
 * ends with.  Such a batch is never detached.  Batches of both kinds alternate freely on one pipeline.
 * COST, plainly: a rate batch costs about what spx_batch_run_rate costs -- 4.86 ms of kernels for 256 x 10 s against 1.73 ms for the
 * plain call (profiles/batch_rate.txt): the general walk kernel, and no overlap between the kernels of consecutive rate batches.
 * What the pipeline adds is what it owns: buffers, layout, packing, and copies in that run beside the neighbours' kernels
 * (profiles/pipeline_rate.txt has the measurement against the loop around spx_batch_run_rate that a caller had to write before). */
spx_pipeline_t spx_pipeline_create_rate(spx_plan_t plan, const spx_stream_job* jobs, const float* rates, int n_streams, int depth,
                                        unsigned flags);
int spx_pipeline_jobs_fit_rate(spx_pipeline_t p, const spx_stream_job* jobs, const float* rates);
int64_t spx_pipeline_submit_jobs_rate(spx_pipeline_t p, const spx_stream_job* jobs, const float* rates, const int16_t* in,
                                      int in_is_device);
int64_t spx_pipeline_submit_jobs_rate_float(spx_pipeline_t p, const spx_stream_job* jobs, const float* rates, const float* in,
                                            int in_is_device);

/* Pinned host memory for callers without HIP headers (the input of spx_pipeline_submit at the full link rate). */
void* spx_host_alloc(size_t bytes);
void spx_host_free(void* p);

/* The two stages separately (same arguments); spx_batch_run = analyze then walk. */
int spx_batch_analyze(spx_plan_t plan, const spx_stream_job* jobs, int n_streams, const int16_t* in,
                      void* workspace, size_t workspace_bytes, const spx_taps* taps, void* hip_stream);
int spx_batch_walk(spx_plan_t plan, const spx_stream_job* jobs, int n_streams, const int16_t* in,
                   int16_t* out, int64_t* n_out, void* workspace, size_t workspace_bytes,
                   const spx_taps* taps, void* hip_stream);

/* One call for a batch whose streams differ in SAMPLE RATE (the reference fixes the rate per handle, soniclib.c:93 /
 * speedy.c:213-214, so any mix can be alive at once; BASELINE configs[4] mixes 16 kHz and 22.05 kHz).  plans[k] serves the
 * jobs with plan_index[i] == k (all plans on the current device, at most 8); in / out / n_out as in spx_batch_run, n_out
 * indexed like jobs.  All groups are launched together -- the walk workgroups of every group are resident at the same
 * time -- forked from and joined to hip_stream.  Results per stream are those of spx_batch_run on its own plan. */
size_t spx_batch_workspace_bytes_mixed(const spx_plan_t* plans, int n_plans, const spx_stream_job* jobs,
                                       const int* plan_index, int n_streams);
int spx_batch_run_mixed(const spx_plan_t* plans, int n_plans, const spx_stream_job* jobs, const int* plan_index,
                        int n_streams, const int16_t* in, int16_t* out, int64_t* n_out, void* workspace,
                        size_t workspace_bytes, void* hip_stream);

/* The same with the debug taps.  Row order: streams grouped by plan index ascending, job order inside a group; row r of a
 * stream lives at index tap_off[s] + r with tap_off[s] = the analysis-frame counts (spx_plan_frames on the stream's own plan,
 * 0 for a linear job) of every stream in front of it in THAT order.  spectrogram / normalized rows are as wide as the
 * stream's own plan makes them (N, W): their element offsets are the sums of frames x width of the streams in front. */
int spx_batch_run_mixed_taps(const spx_plan_t* plans, int n_plans, const spx_stream_job* jobs, const int* plan_index,
                             int n_streams, const int16_t* in, int16_t* out, int64_t* n_out, void* workspace,
                             size_t workspace_bytes, const spx_taps* taps, void* hip_stream);
/* spx_batch_run_mixed for a caller that issues mixed batch after mixed batch (see spx_batch_run_ahead: same contract -- `in`
 * complete when the call is made, two workspaces / out / n_out taking turns, one hip_stream, and the same plans[0] call after
 * call): every group's analysis and tension kernels start at once on a stream of the library's, beside the previous call's walk
 * kernels.  Calls of more streams than the device has CUs run exactly as spx_batch_run_mixed would. */
int spx_batch_run_mixed_ahead(const spx_plan_t* plans, int n_plans, const spx_stream_job* jobs, const int* plan_index,
                              int n_streams, const int16_t* in, int16_t* out, int64_t* n_out, void* workspace,
                              size_t workspace_bytes, void* hip_stream);

/* Timing hooks for bench.py: while enabled, every spx_batch_run records HIP events on hip_stream around
 * each of its kernels (no host synchronisation is added to the call).  spx_timing_collect waits for the
 * recorded events, returns the summed kernel milliseconds (over all launches of each kernel) and the number of
 * spx_batch_run calls since the last collect. */
void spx_set_timing(int enabled);
/* spx_batch_run splits every stream into `chunks` consecutive time ranges and overlaps the analysis of range c+1 (on an internal
 * HIP stream) with the walk of range c (on hip_stream); results are identical for any value, the state record is carried exactly
 * as in the streaming API.  NEVER CALLED: the library chooses -- one range up to two streams per CU (on MI355X the extra launch
 * tails cost more than the overlap gains at 256 x 10 s), two above that.  A count set here is binding for every later call of the
 * process, 1 included (a call of 2 048 streams then runs as one range: 6.31 instead of 6.21 ms). */
void spx_set_pipeline_chunks(int chunks);
/* Concurrent mode of spx_batch_run (default on): the analysis kernel and the frame-rate (tension) kernel run on two
 * internal HIP streams, the walk kernel at the same time on hip_stream; tiles of frames and then per-frame speeds are
 * handed over through device-scope flags as they become ready.  Results are identical with it on or off. */
void spx_set_concurrent(int on);
/* Which frame-rate (tension) kernel a batch call launches.  0 (default): a launch that hands over no tile flags -- kernels in
 * sequence, pipelined and overlapped calls, time chunks, sub-batches -- takes spx_tension_seq_kernel (one pass over LDS, the three
 * recurrences side by side), the concurrent mode spx_tension_kernel (it polls the tile flags).  1: spx_tension_kernel always.
 * Results are identical bit for bit; the switch is for differential tests and for A/B runs of one library. */
void spx_set_tension_form(int form);
/* Diagnostics: the tension kernel the last batch call of this process launched, 0 = spx_tension_kernel, 1 = spx_tension_seq_kernel
 * (the streaming and unit-level APIs always launch the former and leave this value alone). */
int spx_debug_last_tension_form(void);
/* Diagnostics: the number of time chunks the last whole batch call of this process (analysis and walk in one call: spx_batch_run and
 * its _rate, _map, _float, _twopass, _ahead and _overlapped forms) ran in -- 1, 2 above two streams per CU, or what
 * spx_set_pipeline_chunks asked for; 0 before the first such call. */
int spx_debug_last_call_chunks(void);
/* Diagnostics: the query blocks per stream of the last spx_map_lookup of this process (4 .. 1 024); *launches (may be NULL) = the
 * kernel launches it took (one per 65 535 streams); 0 before the first call. */
int spx_debug_last_lookup_grid(int* launches);
/* ... and the output blocks per stream of the last spx_edit_replay (4 096 int16 values each), with its launches. */
int spx_debug_last_replay_grid(int* launches);
/* ... and the query blocks per stream of the last spx_edit_lookup (4 .. 1 024, chosen as spx_map_lookup chooses them), with its launches. */
int spx_debug_last_edit_lookup_grid(int* launches);
/* ... and the output blocks per stream of the last spx_edit_replay_scaled (4 096 values each, int16 or float), with its launches. */
int spx_debug_last_scaled_grid(int* launches);
/* ... and the row blocks per stream of the last spx_edit_warp_rows or spx_edit_unwarp_rows (at most spx_edit_lookup's choice, and
 * no more than the longest stream can use: 64 rows a block where a row has more than 64 bytes, else 256), with its launches. */
int spx_debug_last_rows_grid(int* launches);
/* ... and the workgroups of the last spx_batch_dtw: one per pair, in each of its two launches (*launches = 2). */
int spx_debug_last_dtw_grid(int* launches);
int spx_timing_collect(double* sum_ms_analyze, double* sum_ms_walk, int* n_calls);
/* "analysis;tension;walk": the kernels (template arguments included, as a profiler prints them) that serve a batch of
 * n_streams streams with at most max_channels channels; speedup_only = every job has speed > 1. */
const char* spx_batch_kernel_names(spx_plan_t plan, int n_streams, int max_channels, int speedup_only);
/* The same with the walk kernel in its lean form (what spx_batch_run_overlapped launches when three or more workspaces take turns). */
const char* spx_batch_kernel_names_lean(spx_plan_t plan, int n_streams, int max_channels, int speedup_only);
/* Diagnostics: the form of the walk kernel launched last in this process, 16 * search waves + output waves (68 = the usual
 * 4 + 4, 64 = the lean form of the concurrent mode at 22.05 kHz mono, 32 = the throughput form), 0 = the general kernel. */
int spx_debug_last_walk_form(void);
/* Diagnostics: allocated VGPRs (hipFuncGetAttributes, rounded up to the granule of 8) of the kernels whose register budgets
 * decide the concurrent mode.  which: 0 tension, 1 walk 16 kHz mono (4 + 4 waves, long window), 2 walk 22.05 kHz mono lean
 * (4 + 0), 3 analysis 16 kHz, 4 analysis 22.05 kHz, 5 walk 16 kHz multi-channel (4 + 4).  -1 for an unknown index. */
int spx_debug_kernel_vgprs(int which);
/* Diagnostics: the walk kernel a batch of this shape would be served by -- out[0] allocated VGPRs, out[1] scratch bytes per lane
 * (spilled registers), out[2] LDS bytes per workgroup, out[3] its form (as spx_debug_last_walk_form), out[4] waves per workgroup --
 * and the analysis kernel of a sample rate (out[0 .. 2] alike, out[2] for a launch whose streams are all mono; out[3] the waves
 * that transform frames: 4, 2 or 1).
 * tests/test_gpu_parity.py pins these per (rate, channels, batch size): the engine's choice of launch mode is arithmetic
 * over them. */
int spx_debug_walk_info(int sample_rate, int channels, int n_streams, int speedup_only, int short_jobs, int lean, int* out5);
int spx_debug_analysis_info(int sample_rate, int* out4);
/* Diagnostics, host code only (no GPU needed): the lane-major constant table of the 16 kHz analysis kernel as a plan of this
 * sample rate holds it (15 entries x 64 lanes x 16 bytes into out) and the tables it is filled from (tw, tw2: 480 doubles each,
 * win: 240 floats).  Returns the table's size in bytes, 0 for a rate whose window is not 240 samples, -1 on a null pointer. */
int spx_debug_lane_consts(int sample_rate, void* out, double* tw, double* tw2, float* win);
/* Diagnostics: the 22 resource numbers the engine's launch-mode decision (speedy_amd/csrc/spx_mode.h, a pure function) is fed for a
 * batch of this shape: CUs, LDS per CU, the walk kernel's form as picked and in its lean form (LDS, waves, VGPRs, fast kernel?, output
 * waves; lean form exists?), the tension kernel's LDS and VGPRs, the analysis tiles (the plan's, 16, 8 frames) and the analysis
 * kernel's LDS and VGPRs with the plan's tile and with the small one.  profiles/kernel_resources.json holds them for the shapes
 * tests/test_mode_table.py decides on the CPU. */
int spx_debug_mode_resources(int sample_rate, int channels, int n_streams, int speedup_only, long long* out22);
/* Diagnostics: the walk kernel's five-instruction division for the candidate step lengths against the IEEE quotient, for
 * `denominators` random speeds (speed - 1 log-uniform in [2^exp_lo, 2^exp_hi)) x every count 1 .. 4096 x both numerator forms;
 * returns the number of mismatches (0 is the only acceptable answer), -1 on a runtime error. */
long long spx_debug_fdiv_check(unsigned seed, unsigned denominators, int exp_lo, int exp_hi);
/* The cross-fade's quotient (spx_walk_fast.hip xfade_quot: reciprocal by Newton steps, fused multiply-add, truncating conversion)
 * against the integer division, for every n in [n_lo, n_hi] (1 .. 4096) and every numerator k n + {-1, 0, 1}, |k| <= 32768.
 * Returns the number of mismatches, -1 on a bad range or a runtime error. */
long long spx_debug_xfade_check(int n_lo, int n_hi);
/* The same for the analysis kernel's scale-free fp32 / fp64 divisions and its fp64 square root (spx_log.h): `threads` x
 * `per_thread` pseudo-random operands of the ranges the kernel feeds them; the number of results that differ from the IEEE
 * sequences' (0 is the only acceptable answer), -1 on a runtime error. */
long long spx_debug_arith_check(unsigned seed, unsigned threads, unsigned per_thread);
/* The walk kernels' lag selectors on sums the caller supplies (all pointers HOST): the arg-min of d / lag over lags p0 .. p0 + n_lags
 * - 1, first lag among equal ratios, as the kernels compute it -- one wave per vector.
 * spx_debug_select_check: the speed-up kernel's selector, one lag per lane (n_lags <= 64, rows of 64 words) or two (n_lags <= 128, rows
 * of 128 words); ties of the integer key are rescanned exactly where max_period^2 >= 65536, as in the kernel.  lag_index[v] = the winner's
 * index, kmin[v] = floor(d 2^16 / lag) of the winner.
 * spx_debug_select_fold_check: the general kernel's selector, folded 64 lags at a time (rows of n_lags rounded up to a multiple of 64
 * words, p0 >= 10); want_max: the arg-max as well; fresh: the first fold in the form that takes its first candidate without a
 * comparison.  out3[3 v ..] = best lag, minDiff, maxDiff (the floor quotients; maxDiff = 0 without want_max).
 * Every word of a row is read: the lanes beyond n_lags may hold anything.  Return 0; -1 on a bad argument, on a sum above 65535 lag in a
 * valid lane (checked on the host before anything is launched) or on a runtime error. */
int spx_debug_select_check(const unsigned* d, int n_vectors, int p0, int n_lags, int max_period, int two_per_lane, int* lag_index,
                           unsigned* kmin);
int spx_debug_select_fold_check(const unsigned* d, int n_vectors, int p0, int n_lags, int want_max, int fresh, int* out3);
/* The analysis kernel's natural log ("log spec v2", DESIGN.md 4a: its argument is always a float quotient, speedy.c:716-717) over
 * EVERY positive normal float: block b = the 2^20 float patterns b << 20 ..; sums[b] (HOST uint64[2040], blocks 8 .. 2039 filled) =
 * the sum of the results' bit patterns modulo 2^64.  The oracle computes the same sums (oracle/orc_logcheck.c): equal sums, block
 * for block, are bit-equality on the whole domain.  Returns 0, negative on error. */
int spx_debug_log_check(unsigned first_block, unsigned end_block, unsigned long long* sums);
/* Diagnostics: 1 if the last spx_batch_run / analyze+walk call of this process took the concurrent three-kernel mode, 2 if it was
 * pipelined with the previous call (spx_batch_run_ahead), 0 if it launched its kernels in sequence (another process holds the
 * device's concurrent-mode lock, spx_set_concurrent(0), the batch shape). */
int spx_debug_last_call_concurrent(void);
/* Diagnostics: what the library's own long-lived device allocations hold when they are new -- pipeline slots, the pool's workspace,
 * block cache and record arrays, the state of the drop-in stream API and of the unit-level API.  byte = 0 .. 255: every such block
 * allocated from now on is filled with that byte before anything else uses it (in place of the clearing some of them get);
 * -1 (the default, and any other value): off, the library makes exactly the calls it makes without the switch.  Read when a block is
 * allocated, never on a launch path.  Results must not depend on it (tests/test_gpu_dirty_owned.py). */
void spx_debug_set_alloc_fill(int byte);
/* Sum over the same calls of the frame-rate (tension) kernel's time, as of the last spx_timing_collect. */
double spx_timing_last_tension_ms(void);
/* ... and of the rate kernel's (spx_batch_run_rate calls with a rate other than 1). */
double spx_timing_last_rate_ms(void);
/* ... and of the kernel that converts a time map's rows to final frames (spx_batch_run_rate_map / _float_map calls with a rate other than 1). */
double spx_timing_last_map_rows_ms(void);
/* ... and of the two kernels of the spx_batch_dtw calls made while spx_set_timing was on, and the share of the second (the
 * back-trace and the slopes). */
double spx_timing_last_dtw_ms(void);
double spx_timing_last_dtw_tail_ms(void);

/* Diagnostics: the number of pitch searches (libsonic's findPitchPeriod calls) each stream's walk has run since the stream started (a batch job starts it) -- the length of the stream's chain of dependent steps, which is what bounds a call with one stream per CU.
 *   workspace  DEVICE  the workspace that call ran with;  steps  HOST  int32[n_streams].  Waits for hip_stream first. */
int spx_batch_read_steps(spx_plan_t plan, const spx_stream_job* jobs, int n_streams, const void* workspace,
                         int32_t* steps, void* hip_stream);
int spx_batch_read_steps_mixed(const spx_plan_t* plans, int n_plans, const spx_stream_job* jobs, const int* plan_index,
                               int n_streams, const void* workspace, int32_t* steps, void* hip_stream);

/* ---- plain device-memory helpers (so that C/C++ hosts need no HIP headers) ---- */
void* spx_device_alloc(size_t bytes);
void spx_device_free(void* p);
/* Gather the produced frames of a finished batch into one contiguous buffer so that a single device-to-host copy
 * moves them: packed[offsets[i] .. offsets[i+1]) = the n_out[i]*channels[i] int16 values of stream i.
 *   jobs      HOST  the job table the batch ran with (out_off, channels)
 *   out,n_out DEVICE as written by spx_batch_run
 *   packed    DEVICE int16, at least sum(max(n_out,0)*channels) values (the size of `out` always suffices)
 *   offsets   DEVICE int64[n_streams + 1], written here: exclusive prefix sums in int16 values
 * Runs on hip_stream after the batch; returns 0 or a negative error. */
int spx_batch_pack_outputs(const spx_stream_job* jobs, int n_streams, const int16_t* out, const int64_t* n_out,
                           int16_t* packed, int64_t* offsets, void* hip_stream);
int spx_copy_to_device(void* dst, const void* src, size_t bytes, void* hip_stream);
int spx_copy_to_host(void* dst, const void* src, size_t bytes, void* hip_stream);
int spx_stream_synchronize(void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SPEEDY_HIP_H_ */
