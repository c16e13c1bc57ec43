// pr/pnp.h -- absolute pose without a prior: "here are 2D-3D matches against a map, where is the
// camera?" (picp_pnp_batch, include/picp_c.h: P3P inside RANSAC on the GPU, scored with the
// solver's gate).  For a frame a PICPSolver already holds, PICPSolver::relocalize does the same on
// its device copies.
#pragma once
#include <vector>

#include "picp_c.h"
#include "pr/camera.h"
#include "pr/defs.h"
#include "pr/picp_solver.h"  // PnpParams

namespace pr {

// correspondences: (image index, world index) pairs, as for PICPSolver::oneRound.  true: T is the
// world-in-camera pose with the most inliers (their number in `inliers`), to be polished by PICP
// from there; false: nothing found or an error (picp_last_error()), T is the identity.  The
// camera's own pose is not read: no prior is needed.
inline bool localize(const Camera& camera, const Vector3fVector& world_points, const Vector2fVector& image_points,
                     const IntPairVector& correspondences, const PnpParams& params, Isometry3f& T, int& inliers,
                     int device = 0) {
  T = Isometry3f::Identity();
  inliers = 0;
  std::vector<float> xyz(3 * correspondences.size()), uv(2 * correspondences.size());
  for (size_t k = 0; k < correspondences.size(); ++k) {
    const int ii = correspondences[k].first, wi = correspondences[k].second;
    if (ii < 0 || (size_t)ii >= image_points.size() || wi < 0 || (size_t)wi >= world_points.size()) return false;
    for (int c = 0; c < 3; ++c) xyz[3 * k + c] = world_points[(size_t)wi][c];
    for (int c = 0; c < 2; ++c) uv[2 * k + c] = image_points[(size_t)ii][c];
  }
  const int64_t offs[2] = {0, (int64_t)correspondences.size()};
  float T16[16];
  int32_t n_in = 0, found = 0;
  if (picp_pnp_batch(device, 1, offs, xyz.data(), uv.data(), data9(camera.cameraMatrix()), camera.rows(),
                     camera.cols(), &params, T16, &n_in, &found, nullptr) != PICP_OK)
    return false;
  inliers = n_in;
  if (!found) return false;
  T = iso_from16(T16);
  return true;
}

}  // namespace pr
