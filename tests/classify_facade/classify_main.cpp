// classify_main -- pr::PICPSolver::classify / inliers (include/pr/picp_solver.h, extensions)
// driven from plain host C++, the way a front end would prune its matches.
//
//   classify_main problem.txt
//
// problem.txt (whitespace separated; written by tests/test_gpu_classify.py):
//   rows cols threshold
//   K (9, row-major)   T_wc (16, row-major, world-in-camera)
//   n_world n_image m
//   n_world x y z | n_image u v | m (image index, world index)
// Prints: counts <skipped> <inlier> <outlier>, inliers <n> <checksum of the inlier pairs>,
// consistent <0|1> (inliers() == the pairs classify() marks as inliers, in order; chi2 is -1
// exactly where skipped), pose_unchanged <0|1>.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <vector>

#include "pr/picp_solver.h"

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: classify_main problem.txt" << std::endl;
    return 2;
  }
  std::ifstream f(argv[1]);
  if (!f) {
    std::cerr << "cannot open " << argv[1] << std::endl;
    return 2;
  }
  int rows = 0, cols = 0;
  float thr = 0;
  f >> rows >> cols >> thr;
  pr::Matrix3f K;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) f >> K(r, c);
  float T[16];  // column-major, the Isometry3f memory
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) f >> T[c * 4 + r];
  size_t n_world = 0, n_image = 0, m = 0;
  f >> n_world >> n_image >> m;
  pr::Vector3fVector world(n_world);
  pr::Vector2fVector image(n_image);
  pr::IntPairVector pairs(m);
  for (auto& p : world) f >> p.x() >> p.y() >> p.z();
  for (auto& p : image) f >> p.x() >> p.y();
  for (auto& p : pairs) f >> p.first >> p.second;
  if (!f) {
    std::cerr << "malformed problem file" << std::endl;
    return 2;
  }
  pr::Camera cam(rows, cols, K, pr::iso_from16(T));
  pr::PICPSolver solver;
  solver.init(cam, world, image);
  solver.setKernelThreshold(thr);

  std::vector<uint8_t> state;
  std::vector<float> chi2;
  if (!solver.classify(pairs, state, &chi2)) return 1;
  long counts[3] = {0, 0, 0};
  for (uint8_t s : state) counts[s < 3 ? s : 0]++;
  pr::IntPairVector in;
  const int n_in = solver.inliers(pairs, in);
  if (n_in < 0) return 1;
  bool consistent = (size_t)n_in == in.size() && n_in == counts[PICP_CORR_INLIER];
  size_t q = 0;
  long long checksum = 0;
  for (size_t k = 0; k < pairs.size(); ++k) {
    if ((state[k] == PICP_CORR_SKIPPED) != (chi2[k] == -1.0f)) consistent = false;
    if (state[k] != PICP_CORR_INLIER) continue;
    if (q >= in.size() || in[q] != pairs[k]) consistent = false;
    checksum += (long long)(q + 1) * (pairs[k].first + 3LL * pairs[k].second);
    ++q;
  }
  const bool pose_unchanged = std::memcmp(pr::data16(solver.camera().worldInCameraPose()), T, sizeof(T)) == 0;
  std::printf("counts %ld %ld %ld\n", counts[0], counts[1], counts[2]);
  std::printf("inliers %d %lld\n", n_in, checksum);
  std::printf("consistent %d\n", consistent ? 1 : 0);
  std::printf("pose_unchanged %d\n", pose_unchanged ? 1 : 0);
  return 0;
}
