// picp_sim3_host.h -- one Sim(3) RANSAC run on the device (picp_sim3.hip), as picp_pnp_host.h has
// the P3P's.  Not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "picp_c.h"
#include "picp_host.h"
#include "picp_internal.h"
#include "picp_ransac_host.h"

#pragma GCC visibility push(hidden)

// The arguments, the score grid and the device buffers of one run.  The caller fills I (device
// pointers) after sim3_args; the results stay on the device until the caller copies them out.
struct Sim3Run {
  Sim3Args A;
  Sim3Items I;
  RansacGrid grid;
  DevBuf<int32_t> samples, hyp_valid, cnt, win, inliers, found, refit_count;
  DevBuf<float> hyp_S, S, scale, rms, refit_S;
  DevBuf<uint8_t> mask;  // allocated when asked for
};

// checks the parameters (PICP_ERR_ARG) and fills A; prm null: the defaults
int sim3_args(Sim3Args* A, const picp_sim3_params* prm, int n_problems);
// the score grid of the problems' sizes (host offsets, n_problems + 1) and every buffer; debug:
// the refits' transforms and counts are kept
int sim3_prepare(Sim3Run* R, hipStream_t st, const int64_t* offs, bool want_mask, bool debug);
// the five launches; spans (nullable): five TimedSpans (samples, hypotheses, score, select, refit), span `rep` of each
hipError_t sim3_enqueue(Sim3Run* R, hipStream_t st, TimedSpans* spans, int rep);

#pragma GCC visibility pop
