// Which jobs (spx_stream_job, include/speedy_hip.h) a batch call takes: the rules, once, as a pure function -- no HIP, so that the
// engine, the pipeline object and the host-only table library (spx_mode_table.cpp; tests/test_job_rules.py replays the rules on
// the CPU) all include it.  Every entry point asks BEFORE it enqueues anything (spx_check_jobs, spx_engine.hip); the one rule that
// needs a kernel's resources -- the walk kernel's LDS window of the batch's shape -- is applied there, behind these.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/speedy_hip.h"

// What a rule needs of the plan: the analysis window and frame step in samples (frames_for, spx_engine.h), and whether the analysis
// tile fits one CU's LDS (spx_internal_analysis_fits: false above about 61 kHz).
struct SpxJobLimits { int W, B; bool analysis_fits; };

// In the order the rules are applied: the first broken one is the one reported.
enum SpxJobFault { SPX_JOB_OK = 0, SPX_JOB_COUNTS, SPX_JOB_SPEED, SPX_JOB_NONLINEAR, SPX_JOB_FEEDBACK, SPX_JOB_RATE_TOO_HIGH, SPX_JOB_TOO_LONG };

static inline SpxJobFault spx_check_job(const SpxJobLimits& L, const spx_stream_job& j) {
  if (j.channels < 1 || j.n_in < 0 || j.in_off < 0 || j.out_off < 0 || j.out_cap < 0) return SPX_JOB_COUNTS;
  // The reference takes any float here and has no defined behaviour for most of them (a speed <= 0 makes the TSM
  // stage's step counts negative).  A job is refused unless every speed the TSM stage can be given is positive:
  if (!(j.speed > 0.0f) || !isfinite(j.speed)) return SPX_JOB_SPEED;
  if (!(j.nonlinear >= 0.0f && j.nonlinear <= 1.0f)) return SPX_JOB_NONLINEAR;
  if (!isfinite(j.feedback)) return SPX_JOB_FEEDBACK;
  if (j.nonlinear != 0.0f && !L.analysis_fits) return SPX_JOB_RATE_TOO_HIGH;
  // (also bounds the analysis frames, a 32-bit count in the tables: (n_in - W - 1) / B + 1 <= n_in for W >= 0 and B >= 1)
  if (j.n_in >= (1ll << 30)) return SPX_JOB_TOO_LONG;
  return SPX_JOB_OK;
}

// The rule's words, without a caller's prefix ("spx_batch: ", "spx_pipeline: lane 3: "); "" for SPX_JOB_OK.
static inline const char* spx_job_fault_text(SpxJobFault f) {
  switch (f) {
    case SPX_JOB_COUNTS: return "bad job (channels < 1 or a negative count / offset)";
    case SPX_JOB_SPEED: return "speed must be finite and > 0";
    case SPX_JOB_NONLINEAR: return "nonlinear factor outside [0, 1] (sonic2.h:73-76; the blended speed could reach 0)";
    case SPX_JOB_FEEDBACK: return "feedback strength is not finite";
    case SPX_JOB_RATE_TOO_HIGH: return "sample rate too high for the nonlinear path (the analysis tile does not fit one CU's LDS); linear jobs only";
    case SPX_JOB_TOO_LONG: return "stream of 2^30 frames or more (in-kernel positions are 32-bit)";
    case SPX_JOB_OK: break;
  }
  return "";
}
