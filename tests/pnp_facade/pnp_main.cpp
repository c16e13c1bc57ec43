// pnp_main -- pr::localize and pr::PICPSolver::relocalize (include/pr/pnp.h) driven from plain
// host C++: find the camera without a prior, then polish with the oneRound loop.
//
//   pnp_main problem.txt
//
// problem.txt (whitespace separated; written by tests/test_gpu_pnp.py):
//   rows cols
//   K (9, row-major)
//   pnp threshold, hypotheses, min_inliers, seed
//   kernel threshold of the rounds, number of rounds
//   n_world n_image n_pairs
//   T_wc (16, row-major): the prior the solver is initialised with (never read by the RANSAC)
//   n_world x (x y z) | n_image x (u v) | n_pairs x (image index, world index)
// Prints, poses as the hex float bits of the column-major 4x4:
//   localize <found> <inliers> <pose>     pr::localize
//   relocalize <found> <inliers> <pose>   PICPSolver::relocalize
//   final <rounds that returned true> <pose>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "pr/pnp.h"

static void print_pose(const pr::Isometry3f& T) {
  uint32_t b[16];
  std::memcpy(b, pr::data16(T), sizeof(b));
  for (int k = 0; k < 16; ++k) std::printf(" %08x", b[k]);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: pnp_main problem.txt" << std::endl;
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
  pr::PnpParams prm;
  f >> prm.threshold >> prm.hypotheses >> prm.min_inliers >> prm.seed;
  float kernel_threshold = 0.f;
  int rounds = 0;
  f >> kernel_threshold >> rounds;
  size_t n_world = 0, n_image = 0, n_pairs = 0;
  f >> n_world >> n_image >> n_pairs;
  float T16[16];  // column-major, the Isometry3f memory
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) f >> T16[c * 4 + r];
  pr::Vector3fVector world(n_world);
  for (auto& p : world) f >> p.x() >> p.y() >> p.z();
  pr::Vector2fVector image(n_image);
  for (auto& p : image) f >> p.x() >> p.y();
  pr::IntPairVector pairs(n_pairs);
  for (auto& p : pairs) f >> p.first >> p.second;
  if (!f) {
    std::cerr << "malformed problem file" << std::endl;
    return 2;
  }
  const pr::Camera cam(rows, cols, K, pr::iso_from16(T16));

  pr::Isometry3f T;
  int inliers = 0;
  const bool found = pr::localize(cam, world, image, pairs, prm, T, inliers);
  std::printf("localize %d %d", found ? 1 : 0, inliers);
  print_pose(T);

  pr::PICPSolver solver;
  solver.init(cam, world, image);
  solver.setKernelThreshold(kernel_threshold);
  const bool ok = solver.relocalize(pairs, prm);
  if (!ok && solver.lastStatus() != PICP_TOO_FEW_INLIERS) return 1;
  std::printf("relocalize %d %d", ok ? 1 : 0, solver.lastRelocalizeInliers());
  print_pose(solver.camera().worldInCameraPose());
  int good = 0;
  for (int i = 0; i < rounds; ++i) good += solver.oneRound(pairs, false) ? 1 : 0;
  std::printf("final %d", good);
  print_pose(solver.camera().worldInCameraPose());
  return 0;
}
