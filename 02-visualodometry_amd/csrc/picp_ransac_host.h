// picp_ransac_host.h -- the host side the batched RANSAC solvers share (picp_pnp_runtime.cpp,
// picp_sim3_runtime.cpp).  Every message names its caller, which passes the name.  Not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "picp_host.h"
#include "picp_ransac_plan.h"

#pragma GCC visibility push(hidden)

#define RANSAC_MAX_HYP (1 << 24)  // hypotheses of one call
static_assert(sizeof(RansacBlock) == sizeof(int2), "the plan's table is uploaded as int2");

// The score grid of a run (its plan: picp_ransac_plan.h) and its block table on the device.
struct RansacGrid {
  int nb = 0;      // blocks: grid x
  int hsplit = 1;  // hypothesis slices: grid y
  DevBuf<int2> blk;
  std::vector<int64_t> offs;  // the offsets blk was built for
};

// Plans the grid of the problems' sizes (host offsets, n_problems + 1); builds and uploads the
// table only when the offsets are not those of the last call (picp_relocalize keeps its table).
inline int ransac_grid_prepare(RansacGrid* G, hipStream_t st, const int64_t* offs, int n_problems, int hyp,
                               int score_tile, int hyp_tile, const char* what, const char* items) {
  const bool same = G->offs.size() == (size_t)n_problems + 1 && std::equal(G->offs.begin(), G->offs.end(), offs);
  std::vector<RansacBlock> blk;
  const char* err =
      picp_ransac_plan(offs, n_problems, hyp, score_tile, hyp_tile, &G->nb, &G->hsplit, same ? nullptr : &blk);
  if (err) return picp_set_err(PICP_ERR_ARG, err, what, items);
  const int rc = G->blk.grow(G->nb);
  if (rc) return rc;
  if (G->nb && !same) {
    HIP_TRY(hipMemcpyAsync(G->blk, blk.data(), blk.size() * sizeof(int2), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // blk is a local
    G->offs.assign(offs, offs + n_problems + 1);
  }
  return PICP_OK;
}

// a ragged batch: offsets from 0, ascending, at most INT32_MAX items each; no null array unless empty
inline int check_ragged_batch(const char* what, int n_problems, const int64_t* offs, const void* a, const void* b) {
  if (offs[0] != 0) return picp_set_err(PICP_ERR_ARG, "%s: offsets must start at 0", what);
  for (int i = 0; i < n_problems; ++i)
    if (offs[i + 1] < offs[i] || offs[i + 1] - offs[i] > INT32_MAX)
      return picp_set_err(PICP_ERR_ARG, "%s: bad offsets", what);
  if (offs[n_problems] != 0 && !(a && b)) return picp_set_err(PICP_ERR_ARG, "%s: null points", what);
  return PICP_OK;
}

// the packed inputs of a stateless call on the device: the offsets, wa and wb floats per item
struct RansacUpload {
  DevBuf<int64_t> offs;
  DevBuf<float> a, b;
};
inline int ransac_upload(RansacUpload* U, int n_problems, const int64_t* offs, const float* a, int wa, const float* b,
                         int wb) {
  const int64_t total = offs[n_problems];
  int rc;
  if ((rc = U->offs.grow(n_problems + 1)) || (rc = U->a.grow(wa * total)) || (rc = U->b.grow(wb * total))) return rc;
  HIP_TRY(hipMemcpy(U->offs, offs, (size_t)(n_problems + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  if (total) {
    HIP_TRY(hipMemcpy(U->a, a, (size_t)total * wa * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(U->b, b, (size_t)total * wb * sizeof(float), hipMemcpyHostToDevice));
  }
  return PICP_OK;
}

// One untimed run (first-launch costs), then `reps` timed ones of enqueue(spans, rep): us[s] the
// mean microseconds of stage s of n.
template <class Enqueue>
int ransac_time_stages(int n, int reps, float* us, Enqueue enqueue) {
  std::vector<TimedSpans> spans;
  for (int s = 0; s < n; ++s) spans.emplace_back(reps);  // moved as the vector grows, never copied
  for (TimedSpans& s : spans) HIP_TRY(s.create());
  HIP_TRY(enqueue(nullptr, 0));
  for (int r = 0; r < reps; ++r) HIP_TRY(enqueue(spans.data(), r));
  for (int s = 0; s < n; ++s) {
    double ms = 0.0;
    HIP_TRY(spans[(size_t)s].sum_ms(nullptr, &ms));
    us[s] = (float)(1000.0 * ms / reps);
  }
  return PICP_OK;
}

#pragma GCC visibility pop
