// poly_check -- csrc/picp_poly.h built for the host: real_roots_t<4> (the P3P's quartic, a copy of
// the loop with the level's coefficients in registers) must return the bits of real_roots (the
// essential unit's) for every polynomial of degree <= 4.  Random coefficients over many scales,
// polynomials built from chosen roots (repeated, close, zero), vanishing leading coefficients and
// non-finite entries.  Prints the number of cases and of mismatches; exit status 1 on a mismatch.
//
//   poly_check --roots FILE
//
// reads one polynomial per line of FILE (coefficients ascending, degree <= 10, decimal or hex
// floats) and prints per line "d n r_1 .. r_n" for real_roots, where d <= 4 "| n r_1 .. r_n" for
// real_roots_t<4>, and for a quartic a third such group for p3p_quartic_roots (picp_p3p.h: a copy
// of the loop's last level between critical points it takes from real_roots_t<4> on the
// derivative; those come from a call with its own root bound, so its roots are not held to the
// other two's bits), roots as hex floats: tests/test_pnp_cpu.py compares them with known roots.
#define PICP_POLY_HOST
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "picp_p3p.h"
#include "picp_poly.h"

static uint64_t g_state = 0x243F6A8885A308D3ull;
static uint64_t next64() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static double unit() { return (double)(next64() >> 11) / 9007199254740992.0 * 2.0 - 1.0; }  // [-1, 1)

static long g_cases = 0, g_bad = 0;

static void check(const double* p, int d) {
  double a[10], b[4];
  for (double& v : a) v = -7.0;
  for (double& v : b) v = -7.0;
  const int na = real_roots(p, d, a), nb = real_roots_t<4>(p, d, b);
  ++g_cases;
  if (na != nb || na < 0 || na > 4 || std::memcmp(a, b, sizeof(double) * (size_t)(na > 0 ? na : 0)) != 0) {
    ++g_bad;
    std::printf("mismatch: degree %d, %d and %d roots, p = %a %a %a %a %a\n", d, na, nb, p[0], p[1], p[2], p[3],
                d == 4 ? p[4] : 0.0);
  }
}

// the coefficients (ascending) of lead * prod (x - r_k)
static void from_roots(const double* r, int n, double lead, double* p) {
  p[0] = lead;
  for (int k = 1; k <= 4; ++k) p[k] = 0.0;
  for (int k = 0; k < n; ++k) {
    for (int j = k + 1; j >= 1; --j) p[j] = p[j - 1] - r[k] * p[j];
    p[0] = -r[k] * p[0];
  }
}

static int print_roots(const char* path) {
  std::FILE* fp = std::fopen(path, "r");
  if (!fp) {
    std::fprintf(stderr, "poly_check: cannot open %s\n", path);
    return 2;
  }
  char line[4096];
  while (std::fgets(line, sizeof line, fp)) {
    std::istringstream in(line);
    std::vector<double> c;
    std::string tok;
    while (in >> tok) c.push_back(std::strtod(tok.c_str(), nullptr));
    if (c.empty()) continue;
    if (c.size() > 11) {
      std::fprintf(stderr, "poly_check: degree above 10\n");
      std::fclose(fp);
      return 2;
    }
    const int d = (int)c.size() - 1;
    double a[10], b[4];
    const int na = real_roots(c.data(), d, a);
    std::printf("%d %d", d, na);
    for (int k = 0; k < na; ++k) std::printf(" %a", a[k]);
    if (d <= 4) {
      const int nb = real_roots_t<4>(c.data(), d, b);
      std::printf(" | %d", nb);
      for (int k = 0; k < nb; ++k) std::printf(" %a", b[k]);
    }
    if (d == 4 && c[4] != 0.0) {
      double crit[4];
      int nc = 0;
      const int nq = p3p_quartic_roots(c.data(), b, crit, &nc);
      std::printf(" | %d", nq);
      for (int k = 0; k < nq; ++k) std::printf(" %a", b[k]);
    }
    std::printf("\n");
  }
  std::fclose(fp);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && std::strcmp(argv[1], "--roots") == 0) return print_roots(argv[2]);
  if (argc != 1) {
    std::fprintf(stderr, "usage: poly_check [--roots FILE]\n");
    return 2;
  }
  double p[5];
  for (int it = 0; it < 200000; ++it) {
    const int d = 1 + (int)(next64() % 4);
    for (int k = 0; k <= 4; ++k) {
      const int e = (int)(next64() % 41) - 20;  // scales 2^-20 .. 2^20
      p[k] = (k <= d) ? std::ldexp(unit(), e) : 0.0;
    }
    if (next64() % 8 == 0) p[next64() % (uint64_t)(d + 1)] = 0.0;
    if (next64() % 16 == 0) p[d] *= 1e-16;  // a leading coefficient the finder drops
    check(p, d);
  }
  for (int it = 0; it < 100000; ++it) {
    double r[4];
    const int n = 1 + (int)(next64() % 4);
    for (int k = 0; k < n; ++k) r[k] = 4.0 * unit();
    const uint64_t kind = next64() % 4;
    if (kind == 0 && n >= 2) r[1] = r[0];                      // a double root
    if (kind == 1 && n >= 3) r[2] = r[1] = r[0];               // a triple root
    if (kind == 2 && n >= 2) r[1] = r[0] * (1.0 + 1e-9);       // two close roots
    if (kind == 3) r[0] = 0.0;
    from_roots(r, n, 1.0 + unit() * 0.5, p);
    check(p, n);
  }
  const double special[][5] = {{0, 0, 0, 0, 0}, {1, 0, 0, 0, 0}, {0, 0, 0, 0, 1}, {1, 0, 2, 0, 1}, {-1, 0, 0, 0, 1},
                               {1, -4, 6, -4, 1}, {NAN, 1, 1, 1, 1}, {1, 1, INFINITY, 1, 1}, {1e300, 1, 1, 1, 1e-300}};
  for (const auto& s : special) check(s, 4);
  std::printf("%ld cases, %ld mismatches\n", g_cases, g_bad);
  return g_bad ? 1 : 0;
}
