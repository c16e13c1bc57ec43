// picp_poly.h -- real polynomials in double for the one-lane-per-hypothesis solvers
// (picp_essential.hip: Nister's degree-10 polynomial; picp_p3p.h: Grunert's quartic).
#pragma once
// PICP_POLY_HOST: a plain host build (bin/poly_check compares the two root finders on the CPU,
// bin/p3p_check runs the P3P; compile with -ffp-contract=off)
#ifdef PICP_POLY_HOST
#define PICP_POLY_FN
#else
#include <hip/hip_runtime.h>
#define PICP_POLY_FN __device__
#endif

#include <math.h>

#pragma clang fp contract(off)

namespace {

PICP_POLY_FN double ueval(const double* a, int d, double z) {
  double s = a[d];
  for (int k = d - 1; k >= 0; --k) s = s * z + a[k];
  return s;
}

// real roots (ascending) of a degree-d polynomial, d <= 10: bottom-up through the derivatives,
// one bisection per monotone interval between consecutive critical points (oracle: real_roots)
PICP_POLY_FN int real_roots(const double* p_in, int d, double* roots) {
  double p[11];
  for (int k = 0; k <= d; ++k) p[k] = p_in[k];
  double amax = 0.0;
  for (int k = 0; k <= d; ++k) amax = fmax(amax, fabs(p[k]));
  if (amax == 0.0) return 0;
  while (d > 0 && fabs(p[d]) <= 1e-14 * amax) --d;
  if (d == 0) return 0;
  double bound = 0.0;
  for (int k = 0; k < d; ++k) bound = fmax(bound, fabs(p[k] / p[d]));
  bound += 1.0;
  double der[11][11];
  for (int k = 0; k <= d; ++k) der[d][k] = p[k];
  for (int deg = d - 1; deg >= 1; --deg)
    for (int k = 0; k <= deg; ++k) der[deg][k] = der[deg + 1][k + 1] * (double)(k + 1);
  double crit[11], cur[11];
  int nc = 0, nr = 0;
  for (int deg = 1; deg <= d; ++deg) {
    double ends[12];
    int ne = 0;
    ends[ne++] = -bound;
    for (int i = 0; i < nc; ++i) ends[ne++] = crit[i];
    ends[ne++] = bound;
    nr = 0;
    for (int i = 0; i + 1 < ne; ++i) {
      double lo = ends[i], hi = ends[i + 1];
      double flo = ueval(der[deg], deg, lo), fhi = ueval(der[deg], deg, hi);
      if (flo == 0.0) {
        if (nr == 0 || cur[nr - 1] != lo) cur[nr++] = lo;
        continue;
      }
      if ((flo < 0.0) == (fhi < 0.0)) continue;
      for (int it = 0; it < 200 && hi - lo > 0.0; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (mid <= lo || mid >= hi) break;
        const double fm = ueval(der[deg], deg, mid);
        if (fm == 0.0) {
          lo = hi = mid;
          break;
        }
        if ((fm < 0.0) == (flo < 0.0)) {
          lo = mid;
          flo = fm;
        } else {
          hi = mid;
        }
      }
      cur[nr++] = 0.5 * (lo + hi);
    }
    for (int i = 0; i < nr; ++i) crit[i] = cur[i];
    nc = nr;
  }
  for (int i = 0; i < nr; ++i) roots[i] = cur[i];
  return nr;
}

// real_roots for d <= NR (NR small), the same roots bit for bit: a level's coefficients are held
// in NR + 1 registers while its intervals are bisected, the missing ones as zeros (0 * z + c == c),
// instead of being read from the derivative table in every Horner step.  A copy of the loop above
// rather than a parameter of it: as one template the essential unit's code object changed.
// tests/poly_check/poly_main.cpp (bin/poly_check) holds the two to the same bits: change both.
// A third copy of the loop's last level is p3p_quartic_roots (picp_p3p.h): it bisects the quartic
// between critical points it keeps for its caller.  Not held to these bits (its critical points come
// from a call of real_roots_t<4> on the derivative, with that polynomial's own root bound);
// tests/test_pnp_cpu.py holds it to known roots through bin/poly_check --roots.  Change it too.
template <int NR>
PICP_POLY_FN int real_roots_t(const double* p_in, int d, double* roots) {
  double p[NR + 1];
  for (int k = 0; k <= d; ++k) p[k] = p_in[k];
  double amax = 0.0;
  for (int k = 0; k <= d; ++k) amax = fmax(amax, fabs(p[k]));
  if (amax == 0.0) return 0;
  while (d > 0 && fabs(p[d]) <= 1e-14 * amax) --d;
  if (d == 0) return 0;
  double bound = 0.0;
  for (int k = 0; k < d; ++k) bound = fmax(bound, fabs(p[k] / p[d]));
  bound += 1.0;
  double der[NR + 1][NR + 1];
  for (int k = 0; k <= d; ++k) der[d][k] = p[k];
  for (int deg = d - 1; deg >= 1; --deg)
    for (int k = 0; k <= deg; ++k) der[deg][k] = der[deg + 1][k + 1] * (double)(k + 1);
  double crit[NR + 1], cur[NR + 1];
  int nc = 0, nr = 0;
  for (int deg = 1; deg <= d; ++deg) {
    double ends[NR + 2];
    int ne = 0;
    ends[ne++] = -bound;
    for (int i = 0; i < nc; ++i) ends[ne++] = crit[i];
    ends[ne++] = bound;
    nr = 0;
    double c[NR + 1];
#pragma unroll
    for (int k = 0; k <= NR; ++k) c[k] = (k <= deg) ? der[deg][k] : 0.0;
    auto eval = [&](double z) {
      double s = c[NR];
#pragma unroll
      for (int k = NR - 1; k >= 0; --k) s = s * z + c[k];
      return s;
    };
    for (int i = 0; i + 1 < ne; ++i) {
      double lo = ends[i], hi = ends[i + 1];
      double flo = eval(lo), fhi = eval(hi);
      if (flo == 0.0) {
        if (nr == 0 || cur[nr - 1] != lo) cur[nr++] = lo;
        continue;
      }
      if ((flo < 0.0) == (fhi < 0.0)) continue;
      for (int it = 0; it < 200 && hi - lo > 0.0; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (mid <= lo || mid >= hi) break;
        const double fm = eval(mid);
        if (fm == 0.0) {
          lo = hi = mid;
          break;
        }
        if ((fm < 0.0) == (flo < 0.0)) {
          lo = mid;
          flo = fm;
        } else {
          hi = mid;
        }
      }
      cur[nr++] = 0.5 * (lo + hi);
    }
    for (int i = 0; i < nr; ++i) crit[i] = cur[i];
    nc = nr;
  }
  for (int i = 0; i < nr; ++i) roots[i] = cur[i];
  return nr;
}

}  // namespace
