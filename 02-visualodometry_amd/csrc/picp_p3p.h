// picp_p3p.h -- the minimal absolute-pose solver of picp_pnp.hip (Grunert's P3P),
// one hypothesis per call, in double.  Under PICP_POLY_HOST (picp_poly.h) it is plain host C++:
// bin/p3p_check (tests/p3p_check/p3p_main.cpp) runs this source on the CPU, compiled with
// -ffp-contract=off, and tests/test_p3p_cpu.py compares it with tests/p3p_ref.py.
#pragma once
#include "picp_poly.h"

#include <math.h>

#pragma clang fp contract(off)

#define PNP_POSE 12  // floats of a stored pose: R column-major, then t

#ifdef PICP_POLY_HOST
#define PICP_P3P_INL inline
#else
#define PICP_P3P_INL __device__ __forceinline__
#endif

namespace {

PICP_P3P_INL double dot3(const double* a, const double* b) {
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

PICP_P3P_INL void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// the orthonormal triad of a triangle as the columns e1 | e2 | e3 of M (row-major 3x3):
// e1 along AB, e3 the normal, e2 = e3 x e1.  false when the triangle has no area.
PICP_POLY_FN bool triad(const double* A, const double* B, const double* C, double M[9]) {
  double e1[3], ac[3], e2[3], e3[3];
  for (int k = 0; k < 3; ++k) {
    e1[k] = B[k] - A[k];
    ac[k] = C[k] - A[k];
  }
  const double n1 = sqrt(dot3(e1, e1));
  if (!(n1 > 0.0)) return false;
  for (int k = 0; k < 3; ++k) e1[k] /= n1;
  cross3(e1, ac, e3);
  const double n3 = sqrt(dot3(e3, e3));
  if (!(n3 > 0.0)) return false;
  for (int k = 0; k < 3; ++k) e3[k] /= n3;
  cross3(e3, e1, e2);
  for (int k = 0; k < 3; ++k) {
    M[3 * k + 0] = e1[k];
    M[3 * k + 1] = e2[k];
    M[3 * k + 2] = e3[k];
  }
  return true;
}

// The two conics in x = s2/s1 - 1, y = s3/s1 - 1 (s_i the distance of point i), divided by b^2.
// With ma = 1 - cos(alpha), mb = 1 - cos(beta), mg = 1 - cos(gamma) taken from the bearings'
// differences, 1 + u^2 - 2 u cos = (u - 1)^2 + 2 u (1 - cos) is a sum of small terms and not the
// difference of large ones: a triangle that spans a hundredth of a radian has x, y and the m's
// near 1e-4, and in u, v every quantity below would be rounding noise.
//   F0 = (x^2 + 2 (1 + x) mg) - (c^2/b^2) (y^2 + 2 (1 + y) mb)
//   F1 = (a^2/b^2) (y^2 + 2 (1 + y) mb) - ((x - y)^2 + 2 (1 + x) (1 + y) ma)
struct P3pConics {
  double ma, mb, mg, cb2, ab2;
};

// F at (x, y); returns |F0| + |F1| and in *size the sum of the magnitudes of F's terms
PICP_P3P_INL double p3p_residual(const P3pConics& g, double x, double y, double F[2], double* size) {
  const double t0 = x * x + 2.0 * (1.0 + x) * g.mg, t1 = y * y + 2.0 * (1.0 + y) * g.mb;
  const double t2 = (x - y) * (x - y) + 2.0 * ((1.0 + x) * (1.0 + y)) * g.ma;
  F[0] = t0 - g.cb2 * t1;
  F[1] = g.ab2 * t1 - t2;
  *size = (fabs(t0) + g.cb2 * fabs(t1)) + (g.ab2 * fabs(t1) + fabs(t2));
  return fabs(F[0]) + fabs(F[1]);
}

// Up to six Newton steps on both conics from (x, y); a step is taken only while it lowers
// |F0| + |F1|, so a point is never made worse (a NaN step ends the loop).  true when the point
// ends on both conics to rounding: |F0| + |F1| <= 1e-12 of the magnitudes of F's terms (each F is
// a dozen operations on them, 1e-15; Newton reaches that from a start near a simple intersection
// and never where the conics only come close).
PICP_POLY_FN bool p3p_polish(const P3pConics& g, double* x, double* y) {
  double F[2], size, cx = *x, cy = *y;
  double best = p3p_residual(g, cx, cy, F, &size);
  bool on = best <= 1e-12 * size;
  for (int it = 0; it < 6; ++it) {
    const double j00 = 2.0 * (cx + g.mg), j01 = -2.0 * g.cb2 * (cy + g.mb);
    const double j10 = -2.0 * ((cx - cy) + (1.0 + cy) * g.ma);
    const double j11 = 2.0 * g.ab2 * (cy + g.mb) - 2.0 * ((cy - cx) + (1.0 + cx) * g.ma);
    const double det = j00 * j11 - j01 * j10;
    if (!(fabs(det) > 0.0)) break;
    cx -= (F[0] * j11 - F[1] * j01) / det;
    cy -= (F[1] * j00 - F[0] * j10) / det;
    const double r = p3p_residual(g, cx, cy, F, &size);
    if (!(r < best)) break;
    best = r;
    on = best <= 1e-12 * size;
    *x = cx;
    *y = cy;
  }
  return on;
}

// The real roots (ascending) of the quartic p, p[4] != 0, and its critical points crit[0..*nc):
// real_roots_t<4> on the derivative, then the last level of real_roots_t on p itself, one
// bisection per monotone interval between consecutive critical points.  The work of
// real_roots_t<4>(p, 4, .), which finds the same critical points on its way and keeps them.
// A copy of that loop's last level (picp_poly.h: change all three together); interior ends are the
// critical points inside the root bound, in ascending order.  bin/poly_check --roots prints its
// roots and tests/test_pnp_cpu.py compares them with known ones.
PICP_POLY_FN int p3p_quartic_roots(const double* p, double* roots, double* crit, int* nc) {
  double bound = 0.0;
  for (int k = 0; k < 4; ++k) bound = fmax(bound, fabs(p[k] / p[4]));
  bound += 1.0;
  double dp[4];
  for (int k = 0; k < 4; ++k) dp[k] = p[k + 1] * (double)(k + 1);
  *nc = real_roots_t<4>(dp, 3, crit);
  const double c0 = p[0], c1 = p[1], c2 = p[2], c3 = p[3], c4 = p[4];
  auto eval = [&](double z) { return (((c4 * z + c3) * z + c2) * z + c1) * z + c0; };
  double ends[5];
  int ne = 0, nr = 0;
  ends[ne++] = -bound;
  for (int i = 0; i < *nc; ++i)
    if (crit[i] > ends[ne - 1] && crit[i] < bound) ends[ne++] = crit[i];
  ends[ne++] = bound;
  for (int i = 0; i + 1 < ne; ++i) {
    double lo = ends[i], hi = ends[i + 1];
    double flo = eval(lo);
    const double fhi = eval(hi);
    if (flo == 0.0) {
      if (nr == 0 || roots[nr - 1] != lo) roots[nr++] = lo;
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
    roots[nr++] = 0.5 * (lo + hi);
  }
  return nr;
}

// Grunert's P3P.  P: the three world points, px: their pixels, Kinv / K: the camera (K
// column-major float).  Writes up to four poses (PNP_POSE floats each) and returns their number.
//
// F0 + F1 is linear in x: 2 x D(y) + N(y) = 0, and F0 at x = -N / (2 D) is the quartic
// N^2 - 4 mg N D + 4 D^2 c0 in y (Grunert's, moved to y = v - 1 so that its coefficients are
// built from the small quantities themselves).  Candidates for y are its real roots and, when
// fewer than four were found, its critical points where it all but vanishes: a root of even
// multiplicity, which the bisection of real_roots_t cannot see (an equilateral triangle seen
// along its axis has the true pose there).  Each y gives x by the quotient; where D is small
// against its terms, x is instead either root of F0 at that y (two triangles then share one y).
// Every (x, y) is polished by Newton on both conics, so a y the quartic gives badly (close
// roots) still yields its pose, and is kept only if it ends on both conics (p3p_polish), its three
// depths are positive, it is not a copy of a kept one, its pose is finite in float32 and, in
// double, it reprojects its own three points within 1e-3 px: what does not solve the triangle is
// dropped, so degenerate samples give no pose rather than a wrong one.
PICP_POLY_FN int p3p_grunert(const double P[3][3], const double px[3][2], const double* Kinv, const float* K,
                             float* out) {
  double f[3][3];
  for (int i = 0; i < 3; ++i) {
    double nn = 0.0;
    for (int r = 0; r < 3; ++r) {
      f[i][r] = (Kinv[3 * r + 0] * px[i][0] + Kinv[3 * r + 1] * px[i][1]) + Kinv[3 * r + 2];
      nn += f[i][r] * f[i][r];
    }
    nn = sqrt(nn);
    if (!(nn > 0.0) || !(nn < INFINITY)) return 0;  // NaN or infinite pixel
    for (int r = 0; r < 3; ++r) f[i][r] /= nn;
  }
  double d12[3], d13[3], d23[3], nrm[3];
  for (int k = 0; k < 3; ++k) {
    d12[k] = P[1][k] - P[0][k];
    d13[k] = P[2][k] - P[0][k];
    d23[k] = P[2][k] - P[1][k];
  }
  const double a2 = dot3(d23, d23), b2 = dot3(d13, d13), c2 = dot3(d12, d12);
  cross3(d12, d13, nrm);
  // coincident, collinear (sin^2 of the angle at P1 under 1e-10: float32 points on a line) or non-finite points
  if (!(a2 > 0.0 && b2 > 0.0 && c2 > 0.0 && a2 < INFINITY && b2 < INFINITY && c2 < INFINITY &&
        dot3(nrm, nrm) > 1e-10 * b2 * c2))
    return 0;
  double ma = 0.0, mb = 0.0, mg = 0.0;
  for (int k = 0; k < 3; ++k) {
    ma += (f[1][k] - f[2][k]) * (f[1][k] - f[2][k]);
    mb += (f[0][k] - f[2][k]) * (f[0][k] - f[2][k]);
    mg += (f[0][k] - f[1][k]) * (f[0][k] - f[1][k]);
  }
  ma *= 0.5;
  mb *= 0.5;
  mg *= 0.5;
  const double cb2 = c2 / b2, ab2 = a2 / b2, q = (a2 - c2) / b2;
  const P3pConics G = {ma, mb, mg, cb2, ab2};
  // ascending in y
  const double D[2] = {mg - ma, 1.0 - ma};
  const double N[3] = {2.0 * ((mg - ma) + q * mb), 2.0 * (q * mb - ma), q - 1.0};
  const double c0[3] = {2.0 * (mg - cb2 * mb), -2.0 * cb2 * mb, -cb2};
  const double DD[3] = {D[0] * D[0], 2.0 * D[0] * D[1], D[1] * D[1]};
  const double ND[4] = {N[0] * D[0], N[0] * D[1] + N[1] * D[0], N[1] * D[1] + N[2] * D[0], N[2] * D[1]};
  double poly[5];
  poly[0] = (N[0] * N[0] - 4.0 * mg * ND[0]) + 4.0 * DD[0] * c0[0];
  poly[1] = (2.0 * N[0] * N[1] - 4.0 * mg * ND[1]) + 4.0 * (DD[0] * c0[1] + DD[1] * c0[0]);
  poly[2] = ((2.0 * N[0] * N[2] + N[1] * N[1]) - 4.0 * mg * ND[2]) + 4.0 * ((DD[0] * c0[2] + DD[1] * c0[1]) + DD[2] * c0[0]);
  poly[3] = (2.0 * N[1] * N[2] - 4.0 * mg * ND[3]) + 4.0 * (DD[1] * c0[2] + DD[2] * c0[1]);
  poly[4] = N[2] * N[2] + 4.0 * DD[2] * c0[2];
  for (int k = 0; k < 5; ++k)
    if (!(fabs(poly[k]) < INFINITY)) return 0;
  double ys[7], amax = 0.0;
  for (int k = 0; k < 5; ++k) amax = fmax(amax, fabs(poly[k]));
  int ny;
  if (fabs(poly[4]) <= 1e-14 * amax) {
    ny = real_roots_t<4>(poly, 4, ys);  // not a quartic: the degree real_roots_t takes it for
  } else {
    double cs[4];
    int nc;
    ny = p3p_quartic_roots(poly, ys, cs, &nc);
    for (int i = 0; i < nc && ny < 4; ++i) {
      const double z = fabs(cs[i]);
      const double size = (((fabs(poly[4]) * z + fabs(poly[3])) * z + fabs(poly[2])) * z + fabs(poly[1])) * z + fabs(poly[0]);
      if (fabs(ueval(poly, 4, cs[i])) <= 1e-12 * size) ys[ny++] = cs[i];
    }
  }
  double W[9], pc[3] = {0.0, 0.0, 0.0};
  if (!triad(P[0], P[1], P[2], W)) return 0;
  for (int k = 0; k < 3; ++k) pc[k] = ((P[0][k] + P[1][k]) + P[2][k]) / 3.0;
  int ns = 0;
  double kx[4], ky[4];  // the kept (x, y)
  for (int s = 0; s < ny; ++s) {
    const double y0 = ys[s];
    if (!(y0 > -1.0)) continue;
    const double den = D[0] + D[1] * y0;
    double xs[2];
    int nx = 0;
    if (fabs(den) >= 1e-4 * (fabs(D[0]) + fabs(D[1] * y0))) {
      xs[nx++] = -((N[2] * y0 + N[1]) * y0 + N[0]) / (2.0 * den);
    } else {
      const double cy = (c0[2] * y0 + c0[1]) * y0 + c0[0], disc = mg * mg - cy;
      if (disc >= -1e-9 * (mg * mg + fabs(cy))) {  // a tangency rounded below zero included
        const double sq = sqrt(fmax(disc, 0.0));
        xs[nx++] = -mg + sq;
        if (sq > 0.0) xs[nx++] = -mg - sq;
      }
    }
    for (int c = 0; c < nx && ns < 4; ++c) {
      double x = xs[c], y = y0;
      if (!p3p_polish(G, &x, &y)) continue;
      const double u = 1.0 + x, v = 1.0 + y;
      const double d1 = y * y + 2.0 * v * mb;
      if (!(u > 0.0 && v > 0.0 && d1 > 0.0)) continue;
      bool copy = false;
      for (int k = 0; k < ns; ++k) copy = copy || (fabs(x - kx[k]) + fabs(y - ky[k]) <= 1e-6 * ((fabs(x) + fabs(y)) + ((ma + mb) + mg)));
      if (copy) continue;
      const double s1 = sqrt(b2 / d1);
      const double sc[3] = {s1, u * s1, v * s1};
      double Q[3][3], qc[3];
      for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) Q[i][k] = sc[i] * f[i][k];
      double C[9], R[9], t[3];
      if (!triad(Q[0], Q[1], Q[2], C)) continue;
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (C[3 * i] * W[3 * j] + C[3 * i + 1] * W[3 * j + 1]) + C[3 * i + 2] * W[3 * j + 2];
      for (int k = 0; k < 3; ++k) qc[k] = ((Q[0][k] + Q[1][k]) + Q[2][k]) / 3.0;
      for (int i = 0; i < 3; ++i) t[i] = qc[i] - dot3(R + 3 * i, pc);
      bool ok = true;
      for (int i = 0; i < 3; ++i) {
        double c3[3], ph[3];
        for (int k = 0; k < 3; ++k) c3[k] = dot3(R + 3 * k, P[i]) + t[k];
        for (int k = 0; k < 3; ++k) ph[k] = ((double)K[k] * c3[0] + (double)K[3 + k] * c3[1]) + (double)K[6 + k] * c3[2];
        const double eu = ph[0] / ph[2] - px[i][0], ev = ph[1] / ph[2] - px[i][1];
        ok = ok && (eu * eu + ev * ev <= 1e-6);  // false for NaN
      }
      float* o = out + PNP_POSE * ns;
      for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) o[3 * j + i] = (float)R[3 * i + j];
      for (int i = 0; i < 3; ++i) o[9 + i] = (float)t[i];
      for (int k = 0; k < PNP_POSE; ++k) ok = ok && (fabsf(o[k]) < INFINITY);
      if (ok) {
        kx[ns] = x;
        ky[ns] = y;
        ++ns;
      }
    }
  }
  // the kernel's caller zeroes the slots: a rejected candidate's floats must not stay behind
  for (int k = PNP_POSE * ns; k < PNP_POSE * 4; ++k) out[k] = 0.0f;
  return ns;
}

}  // namespace
