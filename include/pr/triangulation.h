// pr/triangulation.h -- Cam::triangulatePoints' arithmetic (reference src/cam.cpp:94-140:
// P_k = K * inverse(T_k)(0:3,0:4), cv::triangulatePoints + convertPointsFromHomogeneous) on the
// GPU through the C-ABI.  T1/T2 are camera-in-world poses, as in the reference.
#pragma once
#include <vector>

#include "picp_c.h"
#include "pr/defs.h"

namespace pr {

// Returns a PICP_* status; out receives one point per input pair (no cheirality check, as
// in the reference).
inline int triangulatePoints(const Matrix3f& K, const Isometry3f& T1, const Isometry3f& T2,
                             const Vector2fVector& points1, const Vector2fVector& points2,
                             Vector3fVector& out, int device = 0) {
  if (points1.size() != points2.size()) return PICP_ERR_ARG;
  float P1[12], P2[12];
  int rc = picp_projection_matrix(data9(K), data16(T1), P1);
  if (rc) return rc;
  rc = picp_projection_matrix(data9(K), data16(T2), P2);
  if (rc) return rc;
  out.resize(points1.size());
  if (points1.empty()) return PICP_OK;
  return picp_triangulate(device, P1, P2, reinterpret_cast<const float*>(points1.data()),
                          reinterpret_cast<const float*>(points2.data()), (int64_t)points1.size(),
                          reinterpret_cast<float*>(out.data()));
}

// N-view refinement of points against all of their observations with the poses held fixed
// (picp_refine_*, include/picp_c.h: structure-only damped Gauss-Newton with the solver's gate).
// poses: world-in-camera, as Camera::worldInCameraPose.  Point i owns observations
// [track_off[i], track_off[i+1]) of obs_pose (indices into poses) and obs_uv; track_off has
// points.size() + 1 entries.  points is refined in place; stats (nullable) receives one record per
// point.  Returns a PICP_* status.
typedef std::vector<Isometry3f> Isometry3fVector;

inline int refinePoints(const Matrix3f& K, int rows, int cols, const Isometry3fVector& poses,
                        const std::vector<int64_t>& track_off, const std::vector<int32_t>& obs_pose,
                        const Vector2fVector& obs_uv, Vector3fVector& points, const picp_refine_params& params,
                        std::vector<picp_stats>* stats = nullptr, int device = 0) {
  if (track_off.size() != points.size() + 1 || obs_pose.size() != obs_uv.size()) return PICP_ERR_ARG;
  if (track_off.back() != (int64_t)obs_pose.size()) return PICP_ERR_ARG;
  std::vector<float> T(16 * poses.size());
  for (size_t k = 0; k < poses.size(); ++k) std::memcpy(&T[16 * k], data16(poses[k]), 16 * sizeof(float));
  picp_refine_t* h = nullptr;
  int rc = picp_refine_create(&h, device, rows, cols, data9(K));
  if (rc) return rc;
  rc = picp_refine_set_poses(h, T.data(), (int)poses.size());
  if (!rc)
    rc = picp_refine_set_tracks(h, (int64_t)points.size(), track_off.data(), obs_pose.data(),
                                reinterpret_cast<const float*>(obs_uv.data()));
  if (!rc) rc = picp_refine_set_points(h, reinterpret_cast<const float*>(points.data()));
  if (!rc) rc = picp_refine_run(h, &params);
  if (!rc) rc = picp_refine_get_points(h, reinterpret_cast<float*>(points.data()));
  if (!rc && stats) {
    stats->resize(points.size());
    rc = picp_refine_get_stats(h, stats->data());
  }
  picp_refine_destroy(h);
  return rc;
}

}  // namespace pr
