// p3p_check -- csrc/picp_p3p.h built for the host: the solve stage of the P3P RANSAC, one call of
// p3p_grunert per case, without a GPU.
//
//   p3p_check FILE
//
// FILE holds one case per line, 24 numbers (decimal or hex floats, each read as a float32 as the
// device reads them): K column-major (9), the three world points (9), their pixels (6).  K^-1 is
// taken as csrc/picp_pnp_runtime.cpp takes it (the adjugate, in double).  Per case one output
// line: the number of poses, then 12 hex floats per pose (R column-major, then t).
#define PICP_POLY_HOST
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "picp_p3p.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: p3p_check FILE\n");
    return 2;
  }
  std::FILE* fp = std::fopen(argv[1], "r");
  if (!fp) {
    std::fprintf(stderr, "p3p_check: cannot open %s\n", argv[1]);
    return 2;
  }
  std::vector<float> val;
  char tok[128];
  while (std::fscanf(fp, "%127s", tok) == 1) {
    char* end = nullptr;
    const double d = std::strtod(tok, &end);
    if (end == tok || *end != '\0') {
      std::fprintf(stderr, "p3p_check: not a number: %s\n", tok);
      std::fclose(fp);
      return 2;
    }
    val.push_back((float)d);
  }
  std::fclose(fp);
  if (val.size() % 24 != 0) {
    std::fprintf(stderr, "p3p_check: %zu numbers, not a multiple of 24\n", val.size());
    return 2;
  }
  for (size_t c = 0; c < val.size() / 24; ++c) {
    const float* K = val.data() + 24 * c;
    auto m = [&](int r, int col) { return (double)K[col * 3 + r]; };
    const double det = m(0, 0) * (m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1)) - m(0, 1) * (m(1, 0) * m(2, 2) - m(1, 2) * m(2, 0)) +
                       m(0, 2) * (m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0));
    double Kinv[9];
    for (int r = 0; r < 3; ++r)
      for (int col = 0; col < 3; ++col) {
        const int r1 = (col + 1) % 3, r2 = (col + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
        Kinv[3 * r + col] = (m(r1, c1) * m(r2, c2) - m(r1, c2) * m(r2, c1)) / det;
      }
    double P[3][3], px[3][2];
    for (int i = 0; i < 3; ++i) {
      for (int k = 0; k < 3; ++k) P[i][k] = (double)K[9 + 3 * i + k];
      for (int k = 0; k < 2; ++k) px[i][k] = (double)K[18 + 2 * i + k];
    }
    float out[4 * PNP_POSE];
    for (float& v : out) v = 0.0f;
    const int n = p3p_grunert(P, px, Kinv, K, out);
    std::printf("%d", n);
    for (int k = 0; k < n * PNP_POSE; ++k) std::printf(" %a", (double)out[k]);
    std::printf("\n");
  }
  return 0;
}
