// ransac_main.cpp -- what the batched RANSAC solvers share, on the CPU: the sampling function of
// csrc/picp_ransac.h and the score grid of csrc/picp_ransac_plan.h, compiled as plain host C++
// (tests/test_ransac_cpu.py).
//   ransac_check samples SEED PROBLEM H N          H lines "a b c": the triples of hypotheses 0..H-1
//   ransac_check plan SCORE_TILE HYP_TILE HYP SIZE[xCOUNT]...
//                                                  one JSON object: nb, hsplit, blk [[problem, first]...],
//                                                  or error (the message of the rejected batch)
#define PICP_RANSAC_HOST
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "picp_ransac.h"
#include "picp_ransac_plan.h"

static int usage() {
  fprintf(stderr, "usage: ransac_check samples SEED PROBLEM H N | plan SCORE_TILE HYP_TILE HYP SIZE[xCOUNT]...\n");
  return 2;
}

int main(int argc, char** argv) {
  if (argc == 6 && !strcmp(argv[1], "samples")) {
    const uint64_t seed = strtoull(argv[2], nullptr, 0);
    const uint32_t i = (uint32_t)strtoull(argv[3], nullptr, 0), H = (uint32_t)strtoull(argv[4], nullptr, 0);
    const uint32_t n = (uint32_t)strtoull(argv[5], nullptr, 0);
    if (n < 3) return usage();
    for (uint32_t h = 0; h < H; ++h) {
      int32_t id[3];
      picp::sample_triple(seed, i, h, n, id);
      printf("%d %d %d\n", id[0], id[1], id[2]);
    }
    return 0;
  }
  if (argc >= 5 && !strcmp(argv[1], "plan")) {
    const int score_tile = atoi(argv[2]), hyp_tile = atoi(argv[3]), hyp = atoi(argv[4]);
    if (score_tile < 1 || hyp_tile < 1 || hyp < 1) return usage();
    std::vector<int64_t> offs(1, 0);
    for (int a = 5; a < argc; ++a) {
      char* end = nullptr;
      const int64_t size = strtoll(argv[a], &end, 10);
      const int64_t count = (*end == 'x') ? strtoll(end + 1, nullptr, 10) : 1;
      if (size < 0 || count < 0) return usage();
      for (int64_t k = 0; k < count; ++k) offs.push_back(offs.back() + size);
    }
    int nb = 0, hsplit = 1;
    std::vector<RansacBlock> blk;
    const char* err = picp_ransac_plan(offs.data(), (int)offs.size() - 1, hyp, score_tile, hyp_tile, &nb, &hsplit, &blk);
    if (err) {
      char msg[128];
      snprintf(msg, sizeof(msg), err, "check", "items");
      printf("{\"error\": \"%s\"}\n", msg);
      return 0;
    }
    printf("{\"nb\": %d, \"hsplit\": %d, \"blk\": [", nb, hsplit);
    for (size_t k = 0; k < blk.size(); ++k) printf("%s[%d, %d]", k ? ", " : "", (int)blk[k].problem, (int)blk[k].first);
    printf("]}\n");
    return 0;
  }
  return usage();
}
