// sim3_check -- csrc/picp_umeyama.h built for the host: the closed form of the Sim(3) RANSAC, one
// call of sim3_from_pivot_moments per case, without a GPU.
//
//   sim3_check FILE
//
// FILE holds numbers (decimal or hex floats), one case after another: with_scale, n, then n pairs of
// six coordinates (src x y z, dst x y z), each read as a float32 as the device reads them.  The
// moments are summed in double in the file's order about the first pair, as the hypothesis kernel
// of csrc/picp_sim3.hip sums its three.  Per case one output line: 1 and 13 hex floats (M = c R
// column-major, t, c), or 0 when the pairs give no transform.
#define PICP_UMEYAMA_HOST
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "picp_umeyama.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: sim3_check FILE\n");
    return 2;
  }
  std::FILE* fp = std::fopen(argv[1], "r");
  if (!fp) {
    std::fprintf(stderr, "sim3_check: cannot open %s\n", argv[1]);
    return 2;
  }
  std::vector<double> val;
  char tok[128];
  while (std::fscanf(fp, "%127s", tok) == 1) {
    char* end = nullptr;
    const double d = std::strtod(tok, &end);
    if (end == tok || *end != '\0') {
      std::fprintf(stderr, "sim3_check: not a number: %s\n", tok);
      std::fclose(fp);
      return 2;
    }
    val.push_back(d);
  }
  std::fclose(fp);
  size_t at = 0;
  while (at < val.size()) {
    if (at + 2 > val.size() || !(val[at + 1] >= 0.0 && val[at + 1] <= 1e8)) {
      std::fprintf(stderr, "sim3_check: bad case header at number %zu\n", at);
      return 2;
    }
    const int with_scale = val[at] != 0.0;
    const size_t n = (size_t)val[at + 1];
    at += 2;
    if (at + 6 * n > val.size()) {
      std::fprintf(stderr, "sim3_check: case of %zu pairs runs past the end\n", n);
      return 2;
    }
    double m[SIM3_MOMENTS] = {0.0}, pp[3] = {0.0, 0.0, 0.0}, pq[3] = {0.0, 0.0, 0.0};
    for (size_t j = 0; j < n; ++j) {
      double p[3], q[3];
      for (int k = 0; k < 3; ++k) {
        p[k] = (double)(float)val[at + 6 * j + k];
        q[k] = (double)(float)val[at + 6 * j + 3 + k];
      }
      if (j == 0)
        for (int k = 0; k < 3; ++k) pp[k] = p[k], pq[k] = q[k];
      for (int k = 0; k < 3; ++k) p[k] -= pp[k], q[k] -= pq[k];
      sim3_accumulate(m, p, q);
    }
    at += 6 * n;
    float out[13];
    const bool ok = sim3_from_pivot_moments((double)n, m, pp, pq, with_scale, out);
    std::printf("%d", ok ? 1 : 0);
    if (ok)
      for (int k = 0; k < 13; ++k) std::printf(" %a", (double)out[k]);
    std::printf("\n");
  }
  return 0;
}
