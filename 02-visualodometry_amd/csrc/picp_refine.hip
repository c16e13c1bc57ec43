// picp_refine.hip -- structure-only Gauss-Newton: refine map points against all of their
// observations with the poses held fixed (include/picp_c.h picp_refine_*).  The counterpart of the
// PICP solve: the same projection, bounds test, chi2 gate and robust weight (classify_item,
// picp_item.h, bit-identical to the solve kernels' decisions at the same point and pose), a 3x3
// damped system per point instead of a 6x6 per frame.
//
//   picp_refine_kernel : every round of every point in ONE launch.  A 16-lane DPP row owns a point
//                        (4 points per wave, 16 per block); the point, its loop state and its
//                        statistics live in registers from the first round to the last.
//     round : the row's lanes stride over the point's track (CSR: track_off, obs_pose, obs_uv; 12 B
//             per observation) and gather the observation's pose from the 48-B [R|t] table
//             (RefinePose, built at upload).  The DECISION of an observation (projectable, inlier,
//             outlier) is classify_item's, in FP32; its TERMS -- projection, error, the 2x3
//             Jacobian, the 6 + 3 normal-equation sums -- are formed in FP64 from the same float
//             inputs.  (FP32 terms are 1.2-1.75x faster and miss the position tolerance; a point
//             seen with little parallax loses centimetres to them: DESIGN.md 4.9.)
//     reduce: an all-reduce inside the row by the four DPP steps of wave_reduce32's tail
//             (row_mirror, row_half_mirror, quad_perm xor 2, xor 1): every lane ends with the same
//             bits of every total, in a fixed order, without LDS or atomics.
//     solve : every lane of the row solves the damped 3x3 system by LDL^T in FP64 (a dozen
//             operations) and applies the update; the picp_solve convergence rule ends the point.
// A row whose point has finished (or that has no point: n_points not a multiple of 16) keeps
// running with an empty track, so EXEC is full at every DPP step; the wave leaves the round loop
// when none of its rows is active.
#include "picp_c.h"
#include "picp_item.h"
#include "picp_launch.h"
#include "picp_pose.h"
#include "picp_recip.h"
#include "picp_variant.h"
#include "picp_wave.h"

using namespace picp;

#define RF_BLOCK 256
#define RF_ROW 16                      // lanes per point
#define RF_PPB (RF_BLOCK / RF_ROW)     // points per block

// The sums of one linearisation of a point: the upper triangle of H, b, chi_in, chi_out, counts.
struct RfAcc {
  double h00, h01, h02, h11, h12, h22, b0, b1, b2, chi_in, chi_out;
  int n_in, n_proj;
};

// One observation z of the point (X0, X1, X2) from pose T into the sums.  PH: the pinhole K
// [fx 0 cx; 0 fy cy; 0 0 1] (is_pinhole): the terms K's zeros and its one make trivial are dropped.
template <bool PH>
__device__ __forceinline__ void refine_item(const Pose& T, const Cam& C, float thr, bool keep,
                                            float X0, float X1, float X2, float2 z, RfAcc& A) {
  // the decision: classify_item, the bits of the solve kernels' gate at this point and pose
  float chi, iu, iv;
  const int st = classify_item(T, C, thr, PH, X0, X1, X2, z.x, z.y, &chi, &iu, &iv);
  const bool valid = st != 0, inl = st == 1;
  const bool use = inl | (valid & keep);
  A.chi_in += inl ? (double)chi : 0.0;
  A.chi_out += (valid & !inl) ? (double)chi : 0.0;
  A.n_in += inl ? 1 : 0;
  A.n_proj += valid ? 1 : 0;
  // the terms: projection, error and J = Jp K R (2x3) in double from the same float inputs
  // (src/picp_solver.cpp:38-52 with the pose columns dropped and R_k applied)
  const double x0 = X0, x1 = X1, x2 = X2;
  const double pc0 = ((double)T.r00 * x0 + (double)T.r01 * x1 + (double)T.r02 * x2) + (double)T.t0;
  const double pc1 = ((double)T.r10 * x0 + (double)T.r11 * x1 + (double)T.r12 * x2) + (double)T.t1;
  const double pc2 = ((double)T.r20 * x0 + (double)T.r21 * x1 + (double)T.r22 * x2) + (double)T.t2;
  double ph0, ph1, ph2;
  if constexpr (PH) {
    ph0 = (double)C.k00 * pc0 + (double)C.k02 * pc2;
    ph1 = (double)C.k11 * pc1 + (double)C.k12 * pc2;
    ph2 = pc2;
  } else {
    ph0 = (double)C.k00 * pc0 + (double)C.k01 * pc1 + (double)C.k02 * pc2;
    ph1 = (double)C.k10 * pc0 + (double)C.k11 * pc1 + (double)C.k12 * pc2;
    ph2 = (double)C.k20 * pc0 + (double)C.k21 * pc1 + (double)C.k22 * pc2;
  }
  // an unused observation (possibly with an infinite 1/z) contributes exact zeros
  const double iz = use ? rcp_f64(ph2) : 0.0;
  const double ix = use ? ph0 * iz : 0.0, iy = use ? ph1 * iz : 0.0;
  const double e0 = use ? ix - (double)z.x : 0.0, e1 = use ? iy - (double)z.y : 0.0;
  // src/picp_solver.cpp:75-89: sqrt kernel weight, outliers only with keep
  double w = use ? 1.0 : 0.0;
  if (keep) {  // uniform
    const double ch = e0 * e0 + e1 * e1;
    w = (use & !inl) ? sqrt((double)thr / ch) : w;
  }
  const double jp0 = -(ix * iz), jp1 = -(iy * iz);  // -ph0 iz^2, -ph1 iz^2
  double J00, J01, J02, J10, J11, J12;
  if constexpr (PH) {
    const double a00 = iz * (double)C.k00, a02 = iz * (double)C.k02 + jp0;
    const double a11 = iz * (double)C.k11, a12 = iz * (double)C.k12 + jp1;
    J00 = a00 * (double)T.r00 + a02 * (double)T.r20;
    J01 = a00 * (double)T.r01 + a02 * (double)T.r21;
    J02 = a00 * (double)T.r02 + a02 * (double)T.r22;
    J10 = a11 * (double)T.r10 + a12 * (double)T.r20;
    J11 = a11 * (double)T.r11 + a12 * (double)T.r21;
    J12 = a11 * (double)T.r12 + a12 * (double)T.r22;
  } else {
    const double a00 = iz * (double)C.k00 + jp0 * (double)C.k20, a01 = iz * (double)C.k01 + jp0 * (double)C.k21,
               a02 = iz * (double)C.k02 + jp0 * (double)C.k22;
    const double a10 = iz * (double)C.k10 + jp1 * (double)C.k20, a11 = iz * (double)C.k11 + jp1 * (double)C.k21,
               a12 = iz * (double)C.k12 + jp1 * (double)C.k22;
    J00 = a00 * (double)T.r00 + a01 * (double)T.r10 + a02 * (double)T.r20;
    J01 = a00 * (double)T.r01 + a01 * (double)T.r11 + a02 * (double)T.r21;
    J02 = a00 * (double)T.r02 + a01 * (double)T.r12 + a02 * (double)T.r22;
    J10 = a10 * (double)T.r00 + a11 * (double)T.r10 + a12 * (double)T.r20;
    J11 = a10 * (double)T.r01 + a11 * (double)T.r11 + a12 * (double)T.r21;
    J12 = a10 * (double)T.r02 + a11 * (double)T.r12 + a12 * (double)T.r22;
  }
  const double W00 = w * J00, W01 = w * J01, W02 = w * J02;
  const double W10 = w * J10, W11 = w * J11, W12 = w * J12;
  A.h00 += W00 * J00 + W10 * J10;
  A.h01 += W00 * J01 + W10 * J11;
  A.h02 += W00 * J02 + W10 * J12;
  A.h11 += W01 * J01 + W11 * J11;
  A.h12 += W01 * J02 + W11 * J12;
  A.h22 += W02 * J02 + W12 * J12;
  A.b0 += W00 * e0 + W10 * e1;
  A.b1 += W01 * e0 + W11 * e1;
  A.b2 += W02 * e0 + W12 * e1;
}

// Damped 3x3 normal equations -> dx by LDL^T without pivoting, in double (pivot reciprocals: rcp_f64,
// the hardware estimate and two Newton steps).  h: upper triangle
// row-major (00 01 02 11 12 22) with the damping already on the diagonal; solves H dx = -b.
// Returns false when H is not positive definite (a pivot <= 0 or NaN) or dx is not finite.
__device__ __forceinline__ bool ldl3_solve(const double h[6], const double b[3], double dx[3]) {
  const double d0 = h[0];
  const double i0 = rcp_f64(d0);
  const double l10 = h[1] * i0, l20 = h[2] * i0;
  const double d1 = h[3] - l10 * h[1];
  const double i1 = rcp_f64(d1);
  const double l21 = (h[4] - l20 * h[1]) * i1;
  const double d2 = h[5] - l20 * h[2] - l21 * (l21 * d1);
  const double i2 = rcp_f64(d2);
  const double y0 = -b[0];
  const double y1 = -b[1] - l10 * y0;
  const double y2 = -b[2] - l20 * y0 - l21 * y1;
  const double x2 = y2 * i2;
  const double x1 = y1 * i1 - l21 * x2;
  const double x0 = y0 * i0 - l10 * x1 - l20 * x2;
  dx[0] = x0;
  dx[1] = x1;
  dx[2] = x2;
  const bool pd = (d0 > 0.0) & (d1 > 0.0) & (d2 > 0.0);
  const bool fin = (fabs(x0) <= DBL_MAX) & (fabs(x1) <= DBL_MAX) & (fabs(x2) <= DBL_MAX);
  return pd & fin;
}

// The loop state of a point between its rounds, and what it reports.
struct RfState {
  float X0, X1, X2;
  float chi_prev;  // picp_solve's rule (exec/icp_test.cpp:89)
  float chi_in, chi_out;
  int n_in, n_proj, ok, rounds, conv;
  bool active;
};

// Finish a round of an active point from the totals of its linearisation: record the stats (those
// of this linearisation, before the update, as in PICP), the min-inlier check, the damped solve,
// the update and the picp_solve convergence rule.
__device__ __forceinline__ void rf_finish_round(const RefineArgs& a, const RfAcc& t, RfState& S) {
  S.chi_in = (float)t.chi_in;
  S.chi_out = (float)t.chi_out;
  S.n_in = t.n_in;
  S.n_proj = t.n_proj;
  if (t.n_in < a.min_inliers) {  // src/picp_solver.cpp:97-100: the point keeps its value
    S.ok = 0;
    S.active = false;
    return;
  }
  const double d = (double)a.damping;
  const double H[6] = {(double)t.h00 + d, (double)t.h01, (double)t.h02, (double)t.h11 + d, (double)t.h12,
                       (double)t.h22 + d};
  const double B[3] = {(double)t.b0, (double)t.b1, (double)t.b2};
  double dx[3];
  if (!ldl3_solve(H, B, dx)) {
    S.ok = 0;
    S.active = false;
    return;
  }
  S.X0 = (float)((double)S.X0 + dx[0]);
  S.X1 = (float)((double)S.X1 + dx[1]);
  S.X2 = (float)((double)S.X2 + dx[2]);
  S.ok = 1;
  S.rounds += 1;
  // exec/icp_test.cpp:99-106, as finish_round_pose
  const float rel = (S.chi_prev > 1e-10f) ? fabsf(S.chi_prev - S.chi_in) / S.chi_prev : 0.0f;
  if (rel < a.conv_eps) {
    S.conv = 1;
    S.active = false;
  } else {
    S.chi_prev = S.chi_in;
  }
}

__device__ __forceinline__ void rf_store(const RfState& S, int64_t p, float* __restrict__ xyz,
                                         picp_stats* __restrict__ stats) {
  xyz[3 * p + 0] = S.X0;
  xyz[3 * p + 1] = S.X1;
  xyz[3 * p + 2] = S.X2;
  picp_stats s;
  s.chi_in = S.chi_in;
  s.chi_out = S.chi_out;
  s.n_in = S.n_in;
  s.ok = S.ok;
  s.rounds = S.rounds;
  s.converged = S.conv;
  s.n_projected = S.n_proj;
  s.reserved = 0;
  stats[p] = s;
}

template <bool PH>
__global__ __launch_bounds__(RF_BLOCK) void picp_refine_kernel(const RefineArgs a,
                                                              const RefinePose* __restrict__ poses,
                                                              const int64_t* __restrict__ track_off,
                                                              const int32_t* __restrict__ obs_pose,
                                                              const float2* __restrict__ obs_uv,
                                                              float* __restrict__ xyz,
                                                              picp_stats* __restrict__ stats) {
  const int sub = threadIdx.x & (RF_ROW - 1);
  const int64_t p = (int64_t)blockIdx.x * RF_PPB + (threadIdx.x / RF_ROW);
  const bool has_point = p < a.n_points;
  Cam C;
  cam_load(a.K, a.maxx, a.maxy, C);
  const bool keep = a.keep_outliers != 0;

  int64_t o0 = 0;
  int len = 0;
  RfState S = {};  // the same in the 16 lanes of the point's row
  S.chi_prev = FLT_MAX;
  if (has_point) {
    o0 = track_off[p];
    len = (int)(track_off[p + 1] - o0);
    S.X0 = xyz[3 * p + 0];
    S.X1 = xyz[3 * p + 1];
    S.X2 = xyz[3 * p + 2];
  }
  S.active = has_point && a.max_rounds > 0;

  for (int round = 0; round < a.max_rounds; ++round) {
    if (__builtin_amdgcn_ballot_w64(S.active) == 0) break;  // wave-uniform: every row has finished
    RfAcc A = {};
    const int n = S.active ? len : 0;  // a finished row idles with an empty track
    for (int i = sub; i < n; i += RF_ROW) {
      Pose T;
      pose_load(poses[obs_pose[o0 + i]], T);
      refine_item<PH>(T, C, a.threshold, keep, S.X0, S.X1, S.X2, obs_uv[o0 + i], A);
    }
    // all 64 lanes are here (no lane leaves the kernel early): EXEC is full for the DPP steps
    RfAcc t;
    t.h00 = row_sum(A.h00); t.h01 = row_sum(A.h01); t.h02 = row_sum(A.h02);
    t.h11 = row_sum(A.h11); t.h12 = row_sum(A.h12); t.h22 = row_sum(A.h22);
    t.b0 = row_sum(A.b0); t.b1 = row_sum(A.b1); t.b2 = row_sum(A.b2);
    t.chi_in = row_sum(A.chi_in);
    t.chi_out = row_sum(A.chi_out);
    t.n_in = row_sum(A.n_in);
    t.n_proj = row_sum(A.n_proj);
    if (S.active) rf_finish_round(a, t, S);
  }
  if (has_point && sub == 0) rf_store(S, p, xyz, stats);
}

// one launch: every round of every point.  n_points == 0 launches nothing.
extern "C" hipError_t picp_launch_refine(hipStream_t stream, const RefineArgs* a, const RefinePose* poses,
                                         const int64_t* track_off, const int32_t* obs_pose, const float2* obs_uv,
                                         float* xyz, picp_stats* stats) {
  if (!a || a->n_points < 0) return hipErrorInvalidValue;
  if (a->n_points == 0) return hipSuccess;
  if (!poses || !track_off || !xyz || !stats) return hipErrorInvalidValue;
  const int64_t grid = (a->n_points + RF_PPB - 1) / RF_PPB;
  if (grid > INT32_MAX) return hipErrorInvalidValue;
  RefineArgs ra = *a;
  ra.pinhole = picp_use_pinhole(ra.K) ? 1 : 0;  // the camera path the solve kernels take
  if (ra.pinhole)
    hipLaunchKernelGGL(picp_refine_kernel<true>, dim3((unsigned)grid), dim3(RF_BLOCK), 0, stream, ra, poses, track_off,
                       obs_pose, obs_uv, xyz, stats);
  else
    hipLaunchKernelGGL(picp_refine_kernel<false>, dim3((unsigned)grid), dim3(RF_BLOCK), 0, stream, ra, poses, track_off,
                       obs_pose, obs_uv, xyz, stats);
  return hipGetLastError();
}
