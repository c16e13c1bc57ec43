// pgo_main.cpp -- the pose-graph solve on the host: csrc/picp_pgo_plan.cpp and the headers the
// kernel is made of (csrc/picp_pgo_solve.h, csrc/picp_sim3_lie.h) with one worker and no device.
// bin/pgo_check is this file with ASan/UBSan (tests/test_pgo_cpu.py runs it), bin/pgo_ref the same
// at -O3 (the single-thread figure of tools/pgo_bench.py).
//
//   pgo_check plan  batch.txt          the plan as JSON
//   pgo_check solve batch.txt [reps]   the outputs of picp_pgo_batch as JSON (floats as their bits);
//                                      with reps, the solve is repeated and "ms" is its mean time
//
// batch.txt (whitespace separated; floats in any form strtof reads, hex included):
//   with_scale iterations damping eps n_graphs
//   per graph: n m has_weight, then n x (fixed, 16 floats), then m x (i, j, [w,] 16 floats)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "picp_pgo_plan.h"
#include "picp_pgo_solve.h"

namespace {

template <class T>
void ints(const char* name, const std::vector<T>& v, size_t lo, size_t hi, const char* sep) {
  printf("\"%s\": [", name);
  for (size_t i = lo; i < hi; ++i) printf("%s%lld", i > lo ? ", " : "", (long long)v[i]);
  printf("]%s", sep);
}

void doubles(const char* name, const std::vector<double>& v, const char* sep) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) {
    if (v[i] == v[i] && fabs(v[i]) < INFINITY)
      printf("%s%.17g", i ? ", " : "", v[i]);
    else
      printf("%snull", i ? ", " : "");
  }
  printf("]%s", sep);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3 || (strcmp(argv[1], "plan") && strcmp(argv[1], "solve"))) {
    fprintf(stderr, "usage: %s plan|solve batch.txt [reps]\n", argv[0]);
    return 2;
  }
  std::ifstream f(argv[2]);
  if (!f) {
    fprintf(stderr, "cannot open %s\n", argv[2]);
    return 2;
  }
  auto num = [&]() {
    std::string tok;
    f >> tok;
    return tok;
  };
  PgoArgs args;
  args.with_scale = atoi(num().c_str());
  args.iterations = atoi(num().c_str());
  args.damping = strtod(num().c_str(), nullptr);
  args.eps = strtod(num().c_str(), nullptr);
  const int ng = atoi(num().c_str());
  std::vector<int64_t> node_off(1, 0), edge_off(1, 0);
  std::vector<float> S, Z, weight;
  std::vector<uint8_t> fixed;
  std::vector<int32_t> idx;
  bool any_weight = false;
  for (int g = 0; g < ng; ++g) {
    const int n = atoi(num().c_str()), m = atoi(num().c_str()), hw = atoi(num().c_str());
    any_weight = any_weight || hw;
    for (int k = 0; k < n; ++k) {
      fixed.push_back((uint8_t)atoi(num().c_str()));
      for (int q = 0; q < 16; ++q) S.push_back(strtof(num().c_str(), nullptr));
    }
    for (int e = 0; e < m; ++e) {
      idx.push_back(atoi(num().c_str()));
      idx.push_back(atoi(num().c_str()));
      weight.push_back(hw ? strtof(num().c_str(), nullptr) : 1.0f);
      for (int q = 0; q < 16; ++q) Z.push_back(strtof(num().c_str(), nullptr));
    }
    node_off.push_back(node_off.back() + n);
    edge_off.push_back(edge_off.back() + m);
  }
  if (!f) {
    fprintf(stderr, "malformed batch file\n");
    return 2;
  }
  PgoPlan P;
  if (const char* msg = picp_pgo_plan(ng, node_off.data(), edge_off.data(), S.data(), fixed.data(), idx.data(),
                                      Z.data(), any_weight ? weight.data() : nullptr, &P)) {
    printf("{\"error\": \"%s\"}\n", msg);
    return 0;
  }
  if (!strcmp(argv[1], "plan")) {
    printf("{");
    ints("status", P.status, 0, P.status.size(), ", ");
    ints("fidx", P.fidx, 0, P.fidx.size(), ", ");
    printf("\"scratch\": %lld, \"graphs\": [", (long long)P.scratch);
    for (size_t k = 0; k < P.graphs.size(); ++k) {
      const PgoGraph& G = P.graphs[k];
      printf("%s{\"batch_index\": %d, \"n\": %d, \"m\": %d, \"nf\": %d, \"n_blocks\": %d, \"n_tasks\": %d, "
             "\"scratch0\": %lld, ",
             k ? ", " : "", G.batch_index, G.n, G.m, G.nf, G.n_blocks, G.n_tasks, (long long)G.scratch0);
      ints("first", P.first, (size_t)G.free0, (size_t)(G.free0 + G.nf), ", ");
      ints("row_off", P.row_off, (size_t)G.row0, (size_t)(G.row0 + G.nf + 1), ", ");
      ints("task_slot", P.task_slot, (size_t)G.task0, (size_t)(G.task0 + G.n_tasks), ", ");
      ints("task_off", P.task_off, (size_t)G.toff0, (size_t)(G.toff0 + G.n_tasks + 1), ", ");
      ints("entries", P.entries, (size_t)G.entry0,
           (size_t)(G.entry0 + P.task_off[(size_t)(G.toff0 + G.n_tasks)]), "}");
    }
    printf("]}\n");
    return 0;
  }
  const int reps = argc > 3 ? atoi(argv[3]) : 0;
  const size_t nn = (size_t)node_off.back();
  std::vector<float> S_out(S);
  std::vector<double> cost0((size_t)ng, 0.0), cost1(cost0), grad0(cost0), grad1(cost0);
  std::vector<int32_t> steps((size_t)ng, 0), status(P.status);
  std::vector<double> scratch((size_t)P.scratch + 1);
  PgoArrays A;
  A.S = S.data(), A.edge_idx = idx.data(), A.Z = Z.data(), A.weight = any_weight ? weight.data() : nullptr;
  A.fidx = P.fidx.data(), A.first = P.first.data(), A.row_off = P.row_off.data(), A.task_slot = P.task_slot.data();
  A.task_off = P.task_off.data(), A.entries = P.entries.data(), A.scratch = scratch.data(), A.S_out = S_out.data();
  A.cost0 = cost0.data(), A.cost1 = cost1.data(), A.grad0 = grad0.data(), A.grad1 = grad1.data();
  A.steps = steps.data(), A.status = status.data();
  double ms = 0.0;
  for (int rep = 0; rep < (reps > 0 ? reps : 1); ++rep) {
    const auto t0 = std::chrono::steady_clock::now();
    for (const PgoGraph& G : P.graphs) {
      PgoShared sh;
      pgo_solve_graph(G, A, args, &sh, 0, 1);
    }
    ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  printf("{");
  ints("status", status, 0, status.size(), ", ");
  ints("steps", steps, 0, steps.size(), ", ");
  doubles("cost_initial", cost0, ", ");
  doubles("cost_final", cost1, ", ");
  doubles("grad_initial", grad0, ", ");
  doubles("grad_final", grad1, ", ");
  if (reps > 0) printf("\"ms\": %.6f, ", ms / reps);
  printf("\"S_bits\": [");
  for (size_t k = 0; k < 16 * nn; ++k) {
    uint32_t b;
    memcpy(&b, &S_out[k], 4);
    printf("%s%u", k ? ", " : "", b);
  }
  printf("]}\n");
  return 0;
}
