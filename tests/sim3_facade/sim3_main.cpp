// sim3_main -- pr::alignPoints (include/pr/sim3.h) driven from plain host C++.
//
//   sim3_main problem.txt
//
// problem.txt (whitespace separated; written by tests/test_gpu_sim3.py):
//   threshold (hex float) hypotheses min_inliers with_scale refits seed
//   n
//   n x (src x y z, dst x y z), hex floats
// Prints `align <found> <inliers> <scale bits>` and the hex float bits of the column-major 4x4.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

#include "pr/sim3.h"

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: sim3_main problem.txt" << std::endl;
    return 2;
  }
  std::ifstream f(argv[1]);
  if (!f) {
    std::cerr << "cannot open " << argv[1] << std::endl;
    return 2;
  }
  pr::Sim3Params prm;
  size_t n = 0;
  std::string tok;
  f >> tok;
  prm.threshold = std::strtof(tok.c_str(), nullptr);
  f >> prm.hypotheses >> prm.min_inliers >> prm.with_scale >> prm.refits >> prm.seed >> n;
  pr::Vector3fVector src(n), dst(n);
  for (size_t k = 0; k < n; ++k)
    for (int c = 0; c < 6; ++c) {
      f >> tok;
      (c < 3 ? src[k] : dst[k])[c % 3] = std::strtof(tok.c_str(), nullptr);
    }
  if (!f) {
    std::cerr << "malformed problem file" << std::endl;
    return 2;
  }
  float S[16], scale = 0.f;
  int inliers = 0;
  const bool found = pr::alignPoints(src, dst, prm, S, scale, inliers);
  uint32_t b[17];
  std::memcpy(b, S, 16 * sizeof(float));
  std::memcpy(b + 16, &scale, sizeof(float));
  std::printf("align %d %d %08x", found ? 1 : 0, inliers, b[16]);
  for (int k = 0; k < 16; ++k) std::printf(" %08x", b[k]);
  std::printf("\n");
  return 0;
}
