// picp_triangulate.h -- two-view linear (DLT) triangulation of one point (src/cam.cpp:94-140).
#pragma once
#include <hip/hip_runtime.h>

#include <float.h>

#include "picp_recip.h"

namespace picp {

// Right singular vector of the smallest singular value of the 4x4 DLT system A, by one-sided
// (Hestenes) Jacobi, at most 10 sweeps, stopping after the first sweep that rotates nothing
// (every later sweep would be a no-op); all indices compile-time so A and V stay in registers.
// A is consumed.
// A with a non-finite entry gives four NaNs.  Left alone it would give a finite vector: a column
// with a NaN or Inf entry keeps one through every rotation (c x - s y of a non-finite x is
// non-finite), its products gamma are NaN or Inf and fail the rotation test (NaN compares false,
// Inf > Inf is false), its norm never compares below `best`, and so the result would be another
// column of V, or column 0 of the identity when every column is affected (a NaN pixel: the finite
// point (1, 0, 0)).  A finite A keeps finite norms (entries below 2^257), so the sum of the four
// norms is finite exactly then.
__device__ __forceinline__ void tri_null_jacobi(double A[4][4], double v[4]) {
  double Vm[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) Vm[r][c] = (r == c) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 10; ++sweep) {
    bool rotated = false;  // a sweep that rotates nothing leaves A and V unchanged: stop there
#pragma unroll
    for (int pq = 0; pq < 6; ++pq) {
      const int p = (pq < 3) ? 0 : ((pq < 5) ? 1 : 2);
      const int qq = (pq < 3) ? pq + 1 : ((pq < 5) ? pq - 1 : 3);
      double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        alpha += A[k][p] * A[k][p];
        beta += A[k][qq] * A[k][qq];
        gamma += A[k][p] * A[k][qq];
      }
      // Rotate unless the pair is orthogonal to 1e-12 relative (gamma^2 <= 1e-24 alpha beta): the
      // smaller rotations move the result below float precision.
      if (fabs(gamma) > 1e-300 && gamma * gamma > 1e-24 * (alpha * beta)) {
        rotated = true;
        const double zeta = (beta - alpha) * rcp_f64(2.0 * gamma);
        const double q = fma(zeta, zeta, 1.0);
        const double t = ((zeta >= 0.0) ? 1.0 : -1.0) * rcp_f64(fabs(zeta) + q * rsq_f64(q));  // 1/(|z| + sqrt(1+z^2))
        const double c = rsq_f64(fma(t, t, 1.0));
        const double s = c * t;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double akp = A[k][p], akq = A[k][qq];
          A[k][p] = c * akp - s * akq;
          A[k][qq] = s * akp + c * akq;
          const double vkp = Vm[k][p], vkq = Vm[k][qq];
          Vm[k][p] = c * vkp - s * vkq;
          Vm[k][qq] = s * vkp + c * vkq;
        }
      }
    }
    if (!rotated) break;  // identical result to running all 10 sweeps
  }
  double nrm[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) nrm[c] = A[0][c] * A[0][c] + A[1][c] * A[1][c] + A[2][c] * A[2][c] + A[3][c] * A[3][c];
  double best = nrm[0];
  v[0] = Vm[0][0]; v[1] = Vm[1][0]; v[2] = Vm[2][0]; v[3] = Vm[3][0];
#pragma unroll
  for (int c = 1; c < 4; ++c) {
    const bool take = nrm[c] < best;
    best = take ? nrm[c] : best;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = take ? Vm[r][c] : v[r];
  }
  const bool finite = (nrm[0] + nrm[1]) + (nrm[2] + nrm[3]) <= DBL_MAX;  // false for NaN and Inf
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = finite ? v[r] : __builtin_nan("");
}

// Two-view linear (DLT) triangulation of one point, cv::triangulatePoints as called from
// src/cam.cpp:115 then convertPointsFromHomogeneous :118.  P1, P2: 3x4 ROW-major float.
// A (4x4) in double; X_h = the right singular vector of A's smallest singular value, by the
// one-sided Jacobi above (tri_null_jacobi).  (Inverse iteration on A^T A was slower: DESIGN.md
// Appendix A, "inverse-iteration triangulation".)
// A non-finite pixel or P entry gives (NaN, NaN, NaN), as OpenCV's SVD does (tri_null_jacobi's
// rule: every input reaches an entry of A, a product of floats in double cannot overflow and
// 0 * Inf is NaN, so A is finite exactly when the inputs are; a NaN W4 selects scale 1).
__device__ inline void triangulate_dlt(const float* P1, const float* P2, float2 a, float2 b,
                                       float out[3]) {
  double A[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    A[0][k] = (double)a.x * (double)P1[8 + k] - (double)P1[0 + k];
    A[1][k] = (double)a.y * (double)P1[8 + k] - (double)P1[4 + k];
    A[2][k] = (double)b.x * (double)P2[8 + k] - (double)P2[0 + k];
    A[3][k] = (double)b.y * (double)P2[8 + k] - (double)P2[4 + k];
  }
  double v[4];
  tri_null_jacobi(A, v);
  // points4D is float; convertPointsFromHomogeneous in float, scale 1 when |w| <= FLT_EPSILON
  const float X4 = (float)v[0], Y4 = (float)v[1], Z4 = (float)v[2], W4 = (float)v[3];
  const float scale = (fabsf(W4) > FLT_EPSILON) ? 1.0f / W4 : 1.0f;
  out[0] = X4 * scale;
  out[1] = Y4 * scale;
  out[2] = Z4 * scale;
}

}  // namespace picp
