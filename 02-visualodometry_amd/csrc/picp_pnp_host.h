// picp_pnp_host.h -- one P3P RANSAC run on the device (picp_pnp.hip), shared by the stateless
// batch calls (picp_pnp_runtime.cpp) and the single-problem handle (picp_handle.cpp).  Not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "picp_c.h"
#include "picp_host.h"
#include "picp_internal.h"
#include "picp_ransac_host.h"

#pragma GCC visibility push(hidden)

// The arguments, the score grid and the device buffers of one run.  The caller fills I (device
// pointers) after pnp_args; the results stay on the device until the caller copies them out.
struct PnpRun {
  PnpArgs A;
  PnpItems I;
  RansacGrid grid;  // kept between calls: picp_relocalize runs frames of one size again and again
  DevBuf<int32_t> samples, n_roots, cnt, inliers, found;
  DevBuf<float> hyp_T, T;
  DevBuf<uint8_t> mask;  // allocated when asked for
};

// checks the parameters and the camera (PICP_ERR_ARG) and fills A; prm null: the defaults
int pnp_args(PnpArgs* A, const float K[9], int rows, int cols, const picp_pnp_params* prm, int n_problems);
// the score grid of the problems' sizes (host offsets, n_problems + 1) and every buffer
int pnp_prepare(PnpRun* R, hipStream_t st, const int64_t* offs, bool want_mask);
// the four launches; spans (nullable): four TimedSpans (samples, solve, score, select), span `rep` of each
hipError_t pnp_enqueue(PnpRun* R, hipStream_t st, TimedSpans* spans, int rep);

#pragma GCC visibility pop
