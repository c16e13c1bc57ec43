// picp_sim3_lie.h -- the arithmetic of the pose-graph solver (picp_pgo.hip) on
// Sim(3), in double: Exp, Log, Ad, the right Jacobian's inverse, the canonical form of an input
// matrix, and the small dense Cholesky and triangular solves.  Under PICP_LIE_HOST it is plain host
// C++ (bin/pgo_check, bin/pgo_ref), compiled with -ffp-contract=off like picp_umeyama.h.
//
// An element is S = (c, R, t), the matrix [[c R, t], [0, 1]]; R is row-major.  A tangent vector is
// x = (upsilon, omega, sigma), the matrix [[omega^ + sigma I, upsilon], [0, 0]].
#pragma once
#ifdef PICP_LIE_HOST
#define PICP_LIE_FN inline
#else
#include <hip/hip_runtime.h>
#define PICP_LIE_FN __device__ __forceinline__
#endif

#include <math.h>

#pragma clang fp contract(off)

// doubles of a stored element: c, R row-major (9), t (3), 3 unused
#define LIE_SIM3 16
// the step of the central differences of lie_jr_inv: 2^-17
#define LIE_FD_STEP 7.62939453125e-06

namespace {

struct LieSim3 {
  double c, R[9], t[3];
};

PICP_LIE_FN void lie_load(LieSim3* S, const double* p) {
  S->c = p[0];
  for (int k = 0; k < 9; ++k) S->R[k] = p[1 + k];
  for (int k = 0; k < 3; ++k) S->t[k] = p[10 + k];
}

PICP_LIE_FN void lie_store(double* p, const LieSim3& S) {
  p[0] = S.c;
  for (int k = 0; k < 9; ++k) p[1 + k] = S.R[k];
  for (int k = 0; k < 3; ++k) p[10 + k] = S.t[k];
}

// A B
PICP_LIE_FN void lie_mul(LieSim3* out, const LieSim3& A, const LieSim3& B) {
  LieSim3 o;
  o.c = A.c * B.c;
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k)
      o.R[3 * r + k] = (A.R[3 * r] * B.R[k] + A.R[3 * r + 1] * B.R[3 + k]) + A.R[3 * r + 2] * B.R[6 + k];
    o.t[r] = A.c * ((A.R[3 * r] * B.t[0] + A.R[3 * r + 1] * B.t[1]) + A.R[3 * r + 2] * B.t[2]) + A.t[r];
  }
  *out = o;
}

// A^-1 = (1 / c, R^T, -R^T t / c)
PICP_LIE_FN void lie_inv(LieSim3* out, const LieSim3& A) {
  LieSim3 o;
  o.c = 1.0 / A.c;
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) o.R[3 * r + k] = A.R[3 * k + r];
    o.t[r] = -(((A.R[r] * A.t[0] + A.R[3 + r] * A.t[1]) + A.R[6 + r] * A.t[2]) / A.c);
  }
  *out = o;
}

// Functions of M = sigma I + W, W = omega^, are a I + b W + c W^2, because W^3 = -theta^2 W: the
// product of two of them in that basis.
struct LieAbc {
  double a, b, c;
};

PICP_LIE_FN LieAbc lie_abc_mul(const LieAbc& x, const LieAbc& y, double th2) {
  LieAbc o;
  o.a = x.a * y.a;
  o.b = (x.a * y.b + x.b * y.a) - th2 * (x.b * y.c + x.c * y.b);
  o.c = ((x.a * y.c + x.c * y.a) + x.b * y.b) - th2 * (x.c * y.c);
  return o;
}

// E = exp(M) and P = phi(M) = sum M^k / (k + 1)! (the integral of exp(s M) over [0, 1], the V of
// the translation part), M = sigma I + W, from the Taylor series of M / 2^k with |M / 2^k| <= 1/2
// and k doublings phi(2 M) = phi(M) (exp(M) + I) / 2, exp(2 M) = exp(M)^2.  No division by theta
// or sigma: every (sigma, theta) is computed the same way, zero included.
PICP_LIE_FN void lie_exp_phi(double sigma, double th2, LieAbc* E, LieAbc* P) {
  double norm = fabs(sigma) + sqrt(th2), s = 1.0;
  int k = 0;
  while (norm > 0.5 && k < 16) {
    norm *= 0.5;
    s *= 0.5;
    ++k;
  }
  const LieAbc m = {sigma * s, s, 0.0};
  LieAbc term = {1.0, 0.0, 0.0}, e = term, p = term;
  for (int n = 1; n <= 16; ++n) {
    term = lie_abc_mul(term, m, th2);
    term.a /= n, term.b /= n, term.c /= n;
    e.a += term.a, e.b += term.b, e.c += term.c;
    p.a += term.a / (n + 1), p.b += term.b / (n + 1), p.c += term.c / (n + 1);
  }
  for (int i = 0; i < k; ++i) {
    const LieAbc h = {0.5 * (e.a + 1.0), 0.5 * e.b, 0.5 * e.c};
    p = lie_abc_mul(p, h, th2);
    e = lie_abc_mul(e, e, th2);
  }
  *E = e;
  *P = p;
}

// out = a I + b w^ + c (w^)^2, row-major
PICP_LIE_FN void lie_abc_matrix(double* out, const LieAbc& f, const double* w) {
  const double W[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) {
      const double w2 = (W[3 * r] * W[k] + W[3 * r + 1] * W[3 + k]) + W[3 * r + 2] * W[6 + k];
      out[3 * r + k] = ((r == k ? f.a : 0.0) + f.b * W[3 * r + k]) + f.c * w2;
    }
}

// Exp(x), x = (upsilon, omega, sigma): c = e^sigma, R = exp(omega^), t = V upsilon.  sigma == 0
// gives c == 1 exactly.
PICP_LIE_FN void lie_exp(LieSim3* S, const double* x) {
  const double* w = x + 3;
  const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  LieAbc E, P;
  lie_exp_phi(x[6], th2, &E, &P);
  S->c = E.a;
  const LieAbc rot = {1.0, E.b / E.a, E.c / E.a};
  lie_abc_matrix(S->R, rot, w);
  double V[9];
  lie_abc_matrix(V, P, w);
  for (int r = 0; r < 3; ++r) S->t[r] = (V[3 * r] * x[0] + V[3 * r + 1] * x[1]) + V[3 * r + 2] * x[2];
}

// the rotation vector of R (angle in [0, pi])
PICP_LIE_FN void lie_rot_log(double* w, const double* R) {
  const double s[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};  // sin(theta) axis
  const double sn = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
  const double cs = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
  const double th = atan2(sn, cs);
  if (cs > -0.9) {
    const double f = sn > 0.0 ? th / sn : 1.0;
    for (int k = 0; k < 3; ++k) w[k] = f * s[k];
    return;
  }
  // near pi, sin(theta) has no digits: the axis from the symmetric part cos I + (1 - cos) a a^T
  int i = 0;
  if (R[4] > R[0]) i = 1;
  if (R[8] > R[4 * i]) i = 2;
  const double d = 1.0 - cs;
  double a[3];
  a[i] = sqrt(fmax((R[4 * i] - cs) / d, 0.0));
  for (int k = 0; k < 3; ++k)
    if (k != i) a[k] = a[i] > 0.0 ? 0.5 * (R[3 * i + k] + R[3 * k + i]) / (d * a[i]) : 0.0;
  const double dot = (a[0] * s[0] + a[1] * s[1]) + a[2] * s[2];
  const double len = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
  const double f = len > 0.0 ? (dot < 0.0 ? -th : th) / len : 0.0;
  for (int k = 0; k < 3; ++k) w[k] = f * a[k];
}

// y = V^-1 t by the adjugate of the row-major 3x3 V
PICP_LIE_FN void lie_solve3(double* y, const double* V, const double* t) {
  double C[9];
  C[0] = V[4] * V[8] - V[5] * V[7];
  C[1] = V[2] * V[7] - V[1] * V[8];
  C[2] = V[1] * V[5] - V[2] * V[4];
  C[3] = V[5] * V[6] - V[3] * V[8];
  C[4] = V[0] * V[8] - V[2] * V[6];
  C[5] = V[2] * V[3] - V[0] * V[5];
  C[6] = V[3] * V[7] - V[4] * V[6];
  C[7] = V[1] * V[6] - V[0] * V[7];
  C[8] = V[0] * V[4] - V[1] * V[3];
  const double det = (V[0] * C[0] + V[1] * C[3]) + V[2] * C[6];
  for (int r = 0; r < 3; ++r) y[r] = ((C[3 * r] * t[0] + C[3 * r + 1] * t[1]) + C[3 * r + 2] * t[2]) / det;
}

// x = Log(S) = (V^-1 t, log R, log c).  c == 1 gives sigma == 0 exactly.
PICP_LIE_FN void lie_log(double* x, const LieSim3& S) {
  double* w = x + 3;
  lie_rot_log(w, S.R);
  x[6] = log(S.c);
  const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  LieAbc E, P;
  lie_exp_phi(x[6], th2, &E, &P);
  double V[9];
  lie_abc_matrix(V, P, w);
  lie_solve3(x, V, S.t);
}

// Ad(S) = [[c R, t^ R, -t], [0, R, 0], [0, 0, 1]], row-major 7x7: S Exp(x) S^-1 = Exp(Ad(S) x)
PICP_LIE_FN void lie_adjoint(double* A, const LieSim3& S) {
  for (int k = 0; k < 49; ++k) A[k] = 0.0;
  const double* t = S.t;
  const double T[9] = {0.0, -t[2], t[1], t[2], 0.0, -t[0], -t[1], t[0], 0.0};
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) {
      A[7 * r + k] = S.c * S.R[3 * r + k];
      A[7 * r + 3 + k] = (T[3 * r] * S.R[k] + T[3 * r + 1] * S.R[3 + k]) + T[3 * r + 2] * S.R[6 + k];
      A[7 * (3 + r) + 3 + k] = S.R[3 * r + k];
    }
    A[7 * r + 6] = -t[r];
  }
  A[48] = 1.0;
}

// J (row-major 7x7, rows and columns below dim only) = d Log(E Exp(d)) / d d at d = 0, which is
// the inverse of the right Jacobian at Log(E), by central differences with the step LIE_FD_STEP:
// truncation and rounding are both near 1e-11 of an entry.  dim = 6 leaves sigma out (SE(3)).
PICP_LIE_FN void lie_jr_inv(double* J, const LieSim3& E, int dim) {
#pragma nounroll
  for (int c = 0; c < dim; ++c) {
    double d[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, lo[7], hi[7];
    LieSim3 X, Y;
    d[c] = LIE_FD_STEP;
    lie_exp(&X, d);
    lie_mul(&Y, E, X);
    lie_log(hi, Y);
    d[c] = -LIE_FD_STEP;
    lie_exp(&X, d);
    lie_mul(&Y, E, X);
    lie_log(lo, Y);
    for (int r = 0; r < dim; ++r) J[7 * r + c] = (hi[r] - lo[r]) / (2.0 * LIE_FD_STEP);
  }
}

// The canonical form of an input: m is a column-major 4x4 in float32.  With M its upper 3x3,
// c = cbrt(det M) and R is the orthogonal polar factor of M / c, by Newton's iteration
// X <- (X + X^-T) / 2; t is the fourth column.  with_scale == 0: c = 1.  false (S untouched) when
// one of the 16 entries is not finite, det M <= 0 or the result is not finite.
PICP_LIE_FN bool lie_canonical(LieSim3* S, const float* m, int with_scale) {
  bool finite = true;
  for (int k = 0; k < 16; ++k) finite = finite && fabsf(m[k]) < INFINITY;
  if (!finite) return false;
  double X[9];
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) X[3 * r + k] = (double)m[4 * k + r];
  const double det = (X[0] * (X[4] * X[8] - X[5] * X[7]) - X[1] * (X[3] * X[8] - X[5] * X[6])) +
                     X[2] * (X[3] * X[7] - X[4] * X[6]);
  if (!(det > 0.0) || !(det < INFINITY)) return false;
  const double c = cbrt(det);
  for (int k = 0; k < 9; ++k) X[k] /= c;
  for (int it = 0; it < 60; ++it) {
    double C[9];  // cofactors: X^-T = C / det X
    C[0] = X[4] * X[8] - X[5] * X[7];
    C[1] = X[5] * X[6] - X[3] * X[8];
    C[2] = X[3] * X[7] - X[4] * X[6];
    C[3] = X[2] * X[7] - X[1] * X[8];
    C[4] = X[0] * X[8] - X[2] * X[6];
    C[5] = X[1] * X[6] - X[0] * X[7];
    C[6] = X[1] * X[5] - X[2] * X[4];
    C[7] = X[2] * X[3] - X[0] * X[5];
    C[8] = X[0] * X[4] - X[1] * X[3];
    const double dx = (X[0] * C[0] + X[1] * C[1]) + X[2] * C[2];
    double step = 0.0;
    for (int k = 0; k < 9; ++k) {
      const double nx = 0.5 * (X[k] + C[k] / dx);
      step = fmax(step, fabs(nx - X[k]));
      X[k] = nx;
    }
    if (!(step > 1e-15)) break;  // converged, or NaN
  }
  LieSim3 o;
  o.c = with_scale ? c : 1.0;
  finite = fabs(o.c) < INFINITY && o.c > 0.0;
  for (int k = 0; k < 9; ++k) {
    o.R[k] = X[k];
    finite = finite && fabs(X[k]) < INFINITY;
  }
  for (int k = 0; k < 3; ++k) o.t[k] = (double)m[12 + k];
  if (!finite) return false;
  *S = o;
  return true;
}

// the float32 column-major 4x4 [[c R, t], [0, 1]] of S
PICP_LIE_FN void lie_to_float(float* m, const LieSim3& S) {
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) m[4 * k + r] = (float)(S.c * S.R[3 * r + k]);
    m[12 + r] = (float)S.t[r];
    m[4 * r + 3] = 0.0f;
  }
  m[15] = 1.0f;
}

// In-place Cholesky A = L L^T of the leading dim x dim part of a row-major 7x7 (lower triangle
// read and written, the strict upper triangle zeroed).  false at the first pivot that is not
// positive (a NaN included); A is then partly overwritten.
PICP_LIE_FN bool lie_chol(double* A, int dim) {
  for (int j = 0; j < dim; ++j) {
    double d = A[7 * j + j];
    for (int q = 0; q < j; ++q) d -= A[7 * j + q] * A[7 * j + q];
    if (!(d > 0.0) || !(d < INFINITY)) return false;
    d = sqrt(d);
    A[7 * j + j] = d;
    for (int i = j + 1; i < dim; ++i) {
      double v = A[7 * i + j];
      for (int q = 0; q < j; ++q) v -= A[7 * i + q] * A[7 * j + q];
      A[7 * i + j] = v / d;
    }
    for (int i = 0; i < j; ++i) A[7 * i + j] = 0.0;
  }
  return true;
}

// x <- L^-1 x
PICP_LIE_FN void lie_forward(const double* L, double* x, int dim) {
  for (int r = 0; r < dim; ++r) {
    double v = x[r];
    for (int q = 0; q < r; ++q) v -= L[7 * r + q] * x[q];
    x[r] = v / L[7 * r + r];
  }
}

// x <- L^-T x
PICP_LIE_FN void lie_backward(const double* L, double* x, int dim) {
  for (int r = dim - 1; r >= 0; --r) {
    double v = x[r];
    for (int q = r + 1; q < dim; ++q) v -= L[7 * q + r] * x[q];
    x[r] = v / L[7 * r + r];
  }
}

}  // namespace
