// pgo_main -- pr::optimizePoseGraph (include/pr/pose_graph.h) driven from plain host C++.
//
//   pgo_main batch.txt
//
// batch.txt: the format of tests/pgo_check/pgo_main.cpp with one graph that has weights (written by
// tests/test_gpu_pgo.py).  Prints `pgo <ok> <status> <steps>`, the bits of the four figures (cost
// and gradient norm, initial and final) and the bits of every node's column-major 4x4.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

#include "pr/pose_graph.h"

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: pgo_main batch.txt" << std::endl;
    return 2;
  }
  std::ifstream f(argv[1]);
  if (!f) {
    std::cerr << "cannot open " << argv[1] << std::endl;
    return 2;
  }
  auto tok = [&]() {
    std::string t;
    f >> t;
    return t;
  };
  pr::PoseGraphParams prm;
  prm.with_scale = std::atoi(tok().c_str());
  prm.iterations = std::atoi(tok().c_str());
  prm.damping = std::strtod(tok().c_str(), nullptr);
  prm.eps = std::strtod(tok().c_str(), nullptr);
  const int ng = std::atoi(tok().c_str());
  const int n = std::atoi(tok().c_str()), m = std::atoi(tok().c_str()), hw = std::atoi(tok().c_str());
  if (!f || ng != 1 || n < 0 || m < 0) {
    std::cerr << "malformed batch file" << std::endl;
    return 2;
  }
  std::vector<pr::Similarity> nodes((size_t)n);
  std::vector<uint8_t> fixed((size_t)n);
  std::vector<pr::PoseGraphEdge> edges((size_t)m);
  for (int k = 0; k < n; ++k) {
    fixed[(size_t)k] = (uint8_t)std::atoi(tok().c_str());
    for (int q = 0; q < 16; ++q) nodes[(size_t)k][(size_t)q] = std::strtof(tok().c_str(), nullptr);
  }
  for (int e = 0; e < m; ++e) {
    pr::PoseGraphEdge& E = edges[(size_t)e];
    E.i = std::atoi(tok().c_str());
    E.j = std::atoi(tok().c_str());
    if (hw) E.weight = std::strtof(tok().c_str(), nullptr);
    for (int q = 0; q < 16; ++q) E.Z[(size_t)q] = std::strtof(tok().c_str(), nullptr);
  }
  if (!f) {
    std::cerr << "malformed batch file" << std::endl;
    return 2;
  }
  pr::PoseGraphResult res;
  const bool ok = pr::optimizePoseGraph(nodes, fixed, edges, prm, &res);
  std::printf("pgo %d %d %d", ok ? 1 : 0, res.status, res.steps);
  const double fig[4] = {res.cost_initial, res.cost_final, res.grad_initial, res.grad_final};
  for (int k = 0; k < 4; ++k) {
    uint64_t b;
    std::memcpy(&b, &fig[k], 8);
    std::printf(" %016llx", (unsigned long long)b);
  }
  for (int k = 0; k < n; ++k)
    for (int q = 0; q < 16; ++q) {
      uint32_t b;
      std::memcpy(&b, &nodes[(size_t)k][(size_t)q], 4);
      std::printf(" %08x", b);
    }
  std::printf("\n");
  return 0;
}
