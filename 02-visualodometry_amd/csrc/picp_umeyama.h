// picp_umeyama.h -- the closed form of picp_sim3.hip: Umeyama's least-squares
// similarity dst ~ c R src + t from the moments of matched 3D points, in double.  Under
// PICP_UMEYAMA_HOST it is plain host C++: bin/sim3_check (tests/sim3_check/sim3_main.cpp) runs this
// source on the CPU, compiled with -ffp-contract=off, and tests/test_sim3_cpu.py compares it with
// tests/sim3_ref.py.
#pragma once
#ifdef PICP_UMEYAMA_HOST
#define PICP_UME_FN inline
#else
#include <hip/hip_runtime.h>
#define PICP_UME_FN __device__ __forceinline__
#endif

#include <math.h>

#pragma clang fp contract(off)

// The moments of a set of pairs (p, q) about a pivot pair, in one array:
//   [0..3) sum of p, [3..6) sum of q, [6..15) sum of q_r p_c (row r of dst, column c of src),
//   [15] sum of |p|^2, [16] sum of |q|^2
#define SIM3_MOMENTS 17
// floats of a stored transform: M = c R column-major (9), t (3), c, 3 unused
#define SIM3_XF 16

namespace {

// adds the pair (p - pivot_p, q - pivot_q) to the moments m
PICP_UME_FN void sim3_accumulate(double* m, const double* p, const double* q) {
  for (int k = 0; k < 3; ++k) {
    m[k] += p[k];
    m[3 + k] += q[k];
  }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) m[6 + 3 * r + c] += q[r] * p[c];
  m[15] += (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
  m[16] += (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
}

// Umeyama's (c, R, t) of n pairs with first moments ms (src) and md (dst), cross sums C (row-major,
// C[3 r + c] = sum dst_r src_c) and source square sum vs; none of them centred or divided by n.
// R is row-major.  with_scale == 0: the rigid (Kabsch) form, c = 1.  Returns false, and writes
// nothing, when the pairs give no transform: n < 3, a non-finite moment, no source variance, or a
// covariance of rank < 2 (sigma_2 <= 1e-10 sigma_1: coincident or collinear points).
//
// The 3x3 SVD is a one-sided Jacobi on the covariance scaled to unit size: rotations from the
// right make its columns orthogonal, their lengths are the singular values and the accumulated
// rotations the right vectors.  Only the two largest are used: the third pair of singular vectors
// is the cross product of the first two on each side, which is Umeyama's diag(1, 1, det U det V)
// without ever forming a third vector from a column that may have no length (three points: rank 2),
// so det R = +1 always, and the third singular value enters the scale with its sign,
// (u1 x u2)^T Sigma (v1 x v2).
PICP_UME_FN bool sim3_from_moments(double n, const double* ms, const double* md, const double* C, double vs,
                                   int with_scale, double* c_out, double* R, double* t) {
  if (!(n >= 3.0)) return false;
  bool finite = fabs(vs) < INFINITY;
  for (int k = 0; k < 3; ++k) finite = finite && fabs(ms[k]) < INFINITY && fabs(md[k]) < INFINITY;
  for (int k = 0; k < 9; ++k) finite = finite && fabs(C[k]) < INFINITY;
  if (!finite) return false;
  const double var = vs - ((ms[0] * ms[0] + ms[1] * ms[1]) + ms[2] * ms[2]) / n;
  if (!(var > 0.0)) return false;
  double S[9], A[9], V[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  double big = 0.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      S[3 * r + c] = C[3 * r + c] - md[r] * ms[c] / n;
      big = fmax(big, fabs(S[3 * r + c]));
    }
  if (!(big > 0.0) || !(big < INFINITY)) return false;
  for (int k = 0; k < 9; ++k) A[k] = S[k] = S[k] / big;
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool turned = false;
    for (int i = 0; i < 2; ++i)
      for (int j = i + 1; j < 3; ++j) {
        double al = 0.0, be = 0.0, ga = 0.0;
        for (int r = 0; r < 3; ++r) {
          al += A[3 * r + i] * A[3 * r + i];
          be += A[3 * r + j] * A[3 * r + j];
          ga += A[3 * r + i] * A[3 * r + j];
        }
        if (!(ga * ga > 1e-30 * (al * be))) continue;  // orthogonal to rounding, or a column without length
        turned = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double tn = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
        for (int r = 0; r < 3; ++r) {
          const double ai = A[3 * r + i], aj = A[3 * r + j], vi = V[3 * r + i], vj = V[3 * r + j];
          A[3 * r + i] = cs * ai - sn * aj;
          A[3 * r + j] = sn * ai + cs * aj;
          V[3 * r + i] = cs * vi - sn * vj;
          V[3 * r + j] = sn * vi + cs * vj;
        }
      }
    if (!turned) break;
  }
  double len[3];
  for (int k = 0; k < 3; ++k) len[k] = sqrt((A[k] * A[k] + A[3 + k] * A[3 + k]) + A[6 + k] * A[6 + k]);
  // the two longest columns, the earlier one on a tie
  int i1 = 0;
  for (int k = 1; k < 3; ++k)
    if (len[k] > len[i1]) i1 = k;
  int i2 = i1 == 0 ? 1 : 0;
  for (int k = 0; k < 3; ++k)
    if (k != i1 && len[k] > len[i2]) i2 = k;
  const double s1 = len[i1], s2 = len[i2];
  if (!(s1 > 0.0) || !(s2 > 1e-10 * s1)) return false;
  double u1[3], u2[3], u3[3], v1[3], v2[3], v3[3];
  for (int r = 0; r < 3; ++r) {
    u1[r] = A[3 * r + i1] / s1;
    u2[r] = A[3 * r + i2] / s2;
    v1[r] = V[3 * r + i1];
    v2[r] = V[3 * r + i2];
  }
  u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
  u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
  u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
  v3[0] = v1[1] * v2[2] - v1[2] * v2[1];
  v3[1] = v1[2] * v2[0] - v1[0] * v2[2];
  v3[2] = v1[0] * v2[1] - v1[1] * v2[0];
  double s3 = 0.0;  // signed: negative where dst mirrors src
  for (int r = 0; r < 3; ++r) s3 += u3[r] * ((S[3 * r] * v3[0] + S[3 * r + 1] * v3[1]) + S[3 * r + 2] * v3[2]);
  const double c = with_scale ? big * ((s1 + s2) + s3) / var : 1.0;
  if (!(c > 0.0) || !(c < INFINITY)) return false;
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) R[3 * r + k] = (u1[r] * v1[k] + u2[r] * v2[k]) + u3[r] * v3[k];
  for (int r = 0; r < 3; ++r)
    t[r] = md[r] / n - c * ((R[3 * r] * (ms[0] / n) + R[3 * r + 1] * (ms[1] / n)) + R[3 * r + 2] * (ms[2] / n));
  *c_out = c;
  return true;
}

// The float32 transform of the moments m of n pairs about the pivot pair (pp, pq): out[0..9) M = c R
// column-major, out[9..12) t, out[12] c; the translation is moved back from the pivot,
// t = pq + t' - M pp.  false (out zeroed) when there is no transform or a float is not finite.
PICP_UME_FN bool sim3_from_pivot_moments(double n, const double* m, const double* pp, const double* pq,
                                         int with_scale, float* out) {
  double c, R[9], t[3];
  bool ok = sim3_from_moments(n, m, m + 3, m + 6, m[15], with_scale, &c, R, t);
  if (ok) {
    for (int r = 0; r < 3; ++r) {
      const double Mp = (c * R[3 * r] * pp[0] + c * R[3 * r + 1] * pp[1]) + c * R[3 * r + 2] * pp[2];
      out[9 + r] = (float)((pq[r] + t[r]) - Mp);
      for (int k = 0; k < 3; ++k) out[3 * k + r] = (float)(c * R[3 * r + k]);
    }
    out[12] = (float)c;
    for (int k = 0; k < 13; ++k) ok = ok && fabsf(out[k]) < INFINITY;
  }
  if (!ok)
    for (int k = 0; k < 13; ++k) out[k] = 0.0f;
  return ok;
}

}  // namespace
