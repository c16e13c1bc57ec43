// pr/sim3.h -- 3D-3D alignment: "here are matched 3D points of two sets, which scale, rotation and
// translation map one onto the other?" (picp_sim3_batch, include/picp_c.h: Umeyama's closed form
// inside RANSAC on the GPU, then least-squares refits of the inliers).
#pragma once
#include <vector>

#include "picp_c.h"
#include "pr/defs.h"

namespace pr {

struct Sim3Params : picp_sim3_params {
  Sim3Params() { picp_sim3_params_default(this); }
};

// dst[k] ~ c R src[k] + t.  true: S (16 floats, column-major 4x4 [[c R, t], [0, 1]]) is the
// similarity with the most inliers, `scale` its c and `inliers` their number; false: nothing
// found or an error (picp_last_error()), S is the identity and scale 1.
inline bool alignPoints(const Vector3fVector& src, const Vector3fVector& dst, const Sim3Params& params, float S[16],
                        float& scale, int& inliers, int device = 0) {
  for (int k = 0; k < 16; ++k) S[k] = (k % 5 == 0) ? 1.0f : 0.0f;
  scale = 1.0f;
  inliers = 0;
  if (src.size() != dst.size()) return false;
  std::vector<float> p(3 * src.size()), q(3 * src.size());
  for (size_t k = 0; k < src.size(); ++k)
    for (int c = 0; c < 3; ++c) {
      p[3 * k + c] = src[k][c];
      q[3 * k + c] = dst[k][c];
    }
  const int64_t offs[2] = {0, (int64_t)src.size()};
  int32_t n_in = 0, found = 0;
  if (picp_sim3_batch(device, 1, offs, p.data(), q.data(), &params, S, &scale, &n_in, &found, nullptr, nullptr) !=
      PICP_OK)
    return false;
  inliers = n_in;
  return found != 0;
}

}  // namespace pr
