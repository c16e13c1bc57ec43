// refine_main -- pr::refinePoints (include/pr/triangulation.h) driven from plain host C++.
//
//   refine_main problem.txt
//
// problem.txt (whitespace separated; written by tests/test_gpu_refine.py):
//   rows cols
//   K (9, row-major)
//   threshold damping min_inliers keep_outliers max_rounds conv_eps
//   n_poses n_points n_obs
//   n_poses x T_wc (16, row-major, world-in-camera)
//   n_points + 1 track offsets | n_obs x (pose index, u, v) | n_points x (x y z)
// Prints one line per point: point <i> <x y z as hex float bits> <n_in> <n_projected> <rounds>
// <ok> <converged>.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <vector>

#include "pr/triangulation.h"

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: refine_main problem.txt" << std::endl;
    return 2;
  }
  std::ifstream f(argv[1]);
  if (!f) {
    std::cerr << "cannot open " << argv[1] << std::endl;
    return 2;
  }
  int rows = 0, cols = 0;
  f >> rows >> cols;
  pr::Matrix3f K;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) f >> K(r, c);
  picp_refine_params prm;
  picp_refine_params_default(&prm);
  f >> prm.threshold >> prm.damping >> prm.min_inliers >> prm.keep_outliers >> prm.max_rounds >> prm.conv_eps;
  size_t n_poses = 0, n_points = 0, n_obs = 0;
  f >> n_poses >> n_points >> n_obs;
  pr::Isometry3fVector poses;
  for (size_t k = 0; k < n_poses; ++k) {
    float T[16];  // column-major, the Isometry3f memory
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) f >> T[c * 4 + r];
    poses.push_back(pr::iso_from16(T));
  }
  std::vector<int64_t> off(n_points + 1);
  for (auto& o : off) f >> o;
  std::vector<int32_t> obs_pose(n_obs);
  pr::Vector2fVector obs_uv(n_obs);
  for (size_t k = 0; k < n_obs; ++k) f >> obs_pose[k] >> obs_uv[k].x() >> obs_uv[k].y();
  pr::Vector3fVector points(n_points);
  for (auto& p : points) f >> p.x() >> p.y() >> p.z();
  if (!f) {
    std::cerr << "malformed problem file" << std::endl;
    return 2;
  }
  std::vector<picp_stats> stats;
  const int rc = pr::refinePoints(K, rows, cols, poses, off, obs_pose, obs_uv, points, prm, &stats);
  if (rc) {
    std::cerr << "refinePoints: " << rc << " " << picp_last_error() << std::endl;
    return 1;
  }
  for (size_t i = 0; i < n_points; ++i) {
    uint32_t b[3];
    const float v[3] = {points[i].x(), points[i].y(), points[i].z()};
    std::memcpy(b, v, sizeof(b));
    std::printf("point %zu %08x %08x %08x %d %d %d %d %d\n", i, b[0], b[1], b[2], stats[i].n_in,
                stats[i].n_projected, stats[i].rounds, stats[i].ok, stats[i].converged);
  }
  return 0;
}
