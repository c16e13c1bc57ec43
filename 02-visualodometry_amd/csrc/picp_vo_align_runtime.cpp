// picp_vo_align_runtime.cpp -- consecutive segments of a VO run aligned through their shared
// landmarks (picp_vo_align_segments): segment s + 1's map descriptors matched against segment
// s's on the rows resident on the device, the accepted matches compacted in order into 3D-3D pairs,
// and the Sim(3) RANSAC of picp_sim3.hip over them.  Everything it writes is its own: the run's
// maps, poses and step records are only read.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "picp_c.h"
#include "picp_host.h"
#include "picp_launch.h"
#include "picp_sim3_host.h"
#include "picp_vo_host.h"

#define VO_MATCH_DIST 0.2f   // DISTANCE_THRESHOLD, src/my_utilities.h:44 (the sequence's own)
#define VO_MATCH_RATIO 0.8f  // RATIO_THRESHOLD, src/my_utilities.h:46

extern "C" int picp_vo_align_segments(picp_vo_t* h, const picp_sim3_params* prm, float* S_out, float* scale,
                                      int32_t* inliers, int32_t* found, int64_t* n_pairs) {
  CHECK_ARG(h && h->plan.n_seg > 0, "picp_vo_align_segments: bad argument");
  const int np = h->plan.n_seg - 1;
  Sim3Run R;
  int rc = sim3_args(&R.A, prm, np);
  if (rc) return rc;
  if (np == 0) return PICP_OK;
  CHECK_ARG(S_out && inliers && found, "picp_vo_align_segments: null output");
  CHECK_ARG(np <= 65535, "picp_vo_align_segments: too many segments");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  const VoArgs& V = h->vargs;
  hipStream_t st = h->stream;
  // a segment's map never outgrows its slots: the bound of the match grid and of the buffers
  int64_t max_nq = 0;
  for (int s = 1; s <= np; ++s) {
    const int64_t end = (s + 1 < h->plan.n_seg) ? h->plan.segs[s + 1].map_off : h->plan.map_slots;
    max_nq = std::max(max_nq, end - h->plan.segs[s].map_off);
  }
  const int64_t slots = h->plan.map_slots;
  DevBuf<MatchProblem> probs;
  DevBuf<int32_t> bi, acc;
  DevBuf<float> bd, sd, src, dst;
  DevBuf<int64_t> cnt, offs_d;
  if ((rc = probs.grow(np)) || (rc = bi.grow(slots)) || (rc = acc.grow(slots)) || (rc = bd.grow(slots)) ||
      (rc = sd.grow(slots)) || (rc = cnt.grow(np)) || (rc = offs_d.grow(np + 1)))
    return rc;
  HIP_TRY(picp_launch_vo_align_probs(st, V.segs, V.map_n, np, probs));
  // the matcher's full form on the map's own rows and prepped rows, queries and references alike
  HIP_TRY(picp_launch_match_mfma(st, np, max_nq, V.map_desc, V.map_desc, V.map_h, V.map_n1, V.map_h, V.map_n1,
                                 V.map_n2, probs, h->dim, VO_MATCH_DIST, VO_MATCH_RATIO, bi, bd, sd, acc,
                                 PICP_MATCH_FORM_FULL, 1, nullptr, 0));
  HIP_TRY(picp_launch_vo_align_count(st, probs, np, acc, cnt));
  // the one read-back: the layout needs the pair counts
  std::vector<int64_t> offs((size_t)np + 1, 0);
  HIP_TRY(hipMemcpyAsync(offs.data() + 1, cnt, (size_t)np * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int s = 0; s < np; ++s) {
    if (n_pairs) n_pairs[s] = offs[s + 1];
    CHECK_ARG(offs[s + 1] >= 0 && offs[s + 1] <= max_nq, "picp_vo_align_segments: bad pair count");
    offs[s + 1] += offs[s];
  }
  const int64_t total = offs[np];
  if ((rc = src.grow(3 * total)) || (rc = dst.grow(3 * total))) return rc;
  HIP_TRY(hipMemcpyAsync(offs_d, offs.data(), (size_t)(np + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  HIP_TRY(picp_launch_vo_align_pairs(st, probs, np, acc, bi, V.map_xyz, offs_d, src, dst));
  R.I = Sim3Items{src, src + 1, src + 2, dst, dst + 1, dst + 2, 3, 3, offs_d, offs_d};
  if ((rc = sim3_prepare(&R, st, offs.data(), false, false))) return rc;
  HIP_TRY(sim3_enqueue(&R, st, nullptr, 0));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipMemcpy(S_out, R.S, (size_t)np * 16 * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(inliers, R.inliers, (size_t)np * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(found, R.found, (size_t)np * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (scale) HIP_TRY(hipMemcpy(scale, R.scale, (size_t)np * sizeof(float), hipMemcpyDeviceToHost));
  return PICP_OK;
}
