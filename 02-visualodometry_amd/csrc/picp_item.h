// picp_item.h -- the per-correspondence math of the PICP solve: projection, Jacobian and chi2 gate
// (src/camera.h:24-36, src/picp_solver.cpp:26-91) in every accumulation form the kernels use, and
// the observers' restatement of the gate (classify_item).
#pragma once
#include <hip/hip_runtime.h>

#include <float.h>

#include <type_traits>

#include "picp_internal.h"
#include "picp_pose.h"
#include "picp_recip.h"
#include "picp_variant.h"

namespace picp {

struct Acc {
  float h[21];  // upper triangle of H, row-major (i<=j)
  float b[6];
  float chi_in, chi_out;
};

// n_in / n_proj of a wave, counted on the SCALAR unit: each item's inlier and projectable
// predicates are already lane masks (v_cmp results), so a count is s_bcnt1 + s_add per mask,
// issued beside the VALU work instead of as selects and adds in it.  Inside a divergent loop the
// compiler keeps the counter per lane; a lane's copy then counts the items of every iteration
// that lane ran, and lane 0 of a wave runs every iteration any lane of it runs (its items come
// first), so wave_counts reads lane 0.
struct Cnt {
  unsigned n_in, n_proj;
};

__device__ __forceinline__ void cnt_add(Cnt& c, bool inl, bool valid) {
  c.n_in += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(inl));
  c.n_proj += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(valid));
}

// After wave_reduce32 (lane l holds the wave total of value l >> 1): the wave's counts, as the
// float words of PICP_P_N_IN / PICP_P_N_PROJ (exact: a wave counts far fewer than 2^24 items).
__device__ __forceinline__ float wave_counts(float wsum, int lane, const Cnt& c) {
  const unsigned n_in = __builtin_amdgcn_readlane(c.n_in, 0);
  const unsigned n_proj = __builtin_amdgcn_readlane(c.n_proj, 0);
  wsum = ((lane >> 1) == PICP_P_N_IN) ? (float)n_in : wsum;
  return ((lane >> 1) == PICP_P_N_PROJ) ? (float)n_proj : wsum;
}

typedef float f2 __attribute__((ext_vector_type(2)));

// Two accumulation slots per lane: correspondences are processed in PAIRS, item A in .x and
// item B in .y of every value (written as float2 math: packed-FP32 instructions until the device
// code was built without them, picp_internal.h; now two scalar chains); the slots are folded
// once per thread at the end.
struct Acc2 {
  f2 h[21];
  f2 b[6];
  f2 chi_in, chi_out;
};

__device__ __forceinline__ void acc2_zero(Acc2& a) {
#pragma unroll
  for (int i = 0; i < 21; ++i) a.h[i] = (f2){0.0f, 0.0f};
#pragma unroll
  for (int i = 0; i < 6; ++i) a.b[i] = (f2){0.0f, 0.0f};
  a.chi_in = a.chi_out = (f2){0.0f, 0.0f};
}

// fold the two slots into the 32-term partial layout (picp_internal.h PICP_P_*); the counts
// are wave-level (Cnt, wave_counts)
__device__ __forceinline__ void acc2_fold(const Acc2& a, float v[PICP_NPART]) {
#pragma unroll
  for (int i = 0; i < 21; ++i) v[PICP_P_H + i] = a.h[i].x + a.h[i].y;
#pragma unroll
  for (int i = 0; i < 6; ++i) v[PICP_P_B + i] = a.b[i].x + a.b[i].y;
  v[PICP_P_CHI_IN] = a.chi_in.x + a.chi_in.y;
  v[PICP_P_CHI_OUT] = a.chi_out.x + a.chi_out.y;
  v[PICP_P_N_IN] = 0.0f;
  v[PICP_P_N_PROJ] = 0.0f;
  v[31] = 0.0f;
}

// ---------------------------------------------------------------------------------------
// Per-correspondence math.  The block that decides projectability and the chi2 gate is
// compiled with FP contraction OFF and evaluates every sum left to right, exactly like the
// CPU oracle (oracle/picp_oracle.c), so inlier/outlier/skip decisions are bit-identical to
// the oracle at the same pose.  The Jacobian and accumulation are free to use FMA.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void accumulate_one(const Pose& T, const Cam& C, float thr,
                                               bool keep, float x, float y, float z, float u,
                                               float v, bool in_range, Acc& a, Cnt& n) {
  float pc0, pc1, pc2, ph0, ph1, ph2, iz, e0, e1, chi;
  bool valid;
  {
#pragma clang fp contract(off)
    // src/camera.h:26  pc = R*p + t
    pc0 = ((T.r00 * x + T.r01 * y) + T.r02 * z) + T.t0;
    pc1 = ((T.r10 * x + T.r11 * y) + T.r12 * z) + T.t1;
    pc2 = ((T.r20 * x + T.r21 * y) + T.r22 * z) + T.t2;
    // src/camera.h:29  ph = K*pc
    ph0 = (C.k00 * pc0 + C.k01 * pc1) + C.k02 * pc2;
    ph1 = (C.k10 * pc0 + C.k11 * pc1) + C.k12 * pc2;
    ph2 = (C.k20 * pc0 + C.k21 * pc1) + C.k22 * pc2;
    // src/camera.h:30 / picp_solver.cpp:44: (float)(1.0/(double)z) == correctly rounded
    // 1.0f/z (double rounding is innocuous for division at 53 >= 2*24+2); hipcc's default
    // fp32 division is correctly rounded.
    iz = 1.0f / ph2;
    const float ix = ph0 * iz;
    const float iy = ph1 * iz;
    // src/camera.h:27-28 (z<=0 rejects; NaN passes as in the reference) and :31-34
    // bitwise, not short-circuit: the same predicate without per-item exec-mask branches
    valid = in_range & !(pc2 <= 0.0f) & !((ix < 0.0f) | (ix > C.maxx) | (iy < 0.0f) | (iy > C.maxy));
    e0 = ix - u;  // src/picp_solver.cpp:34
    e1 = iy - v;
    chi = e0 * e0 + e1 * e1;  // src/picp_solver.cpp:74
  }
  // src/picp_solver.cpp:75-89: strict gate, sqrt kernel weight, outliers only with keep
  const bool outlier = chi > thr;
  const bool inl = valid & !outlier;
  const bool use = inl | (valid & keep);
  const float lambda = outlier ? sqrtf(thr / chi) : 1.0f;
  const float w = inl ? 1.0f : lambda;
  a.chi_in += inl ? chi : 0.0f;
  a.chi_out += (valid && outlier) ? chi : 0.0f;
  cnt_add(n, inl, valid);
  // unused terms are zeroed by select before the Jacobian, so a skipped point (possibly
  // with an infinite iz) can never inject inf/NaN into H or b
  iz = use ? iz : 0.0f;
  pc0 = use ? pc0 : 0.0f;
  pc1 = use ? pc1 : 0.0f;
  pc2 = use ? pc2 : 0.0f;
  ph0 = use ? ph0 : 0.0f;
  ph1 = use ? ph1 : 0.0f;
  e0 = use ? e0 : 0.0f;
  e1 = use ? e1 : 0.0f;
  // src/picp_solver.cpp:38-52: J = Jp * K * [I | skew(-pc)]
  const float iz2 = iz * iz;
  const float jp02 = -ph0 * iz2, jp12 = -ph1 * iz2;
  const float a00 = iz * C.k00 + jp02 * C.k20;  // (Jp*K)(0,c)
  const float a01 = iz * C.k01 + jp02 * C.k21;
  const float a02 = iz * C.k02 + jp02 * C.k22;
  const float a10 = iz * C.k10 + jp12 * C.k20;  // (Jp*K)(1,c)
  const float a11 = iz * C.k11 + jp12 * C.k21;
  const float a12 = iz * C.k12 + jp12 * C.k22;
  float J0[6], J1[6];
  J0[0] = a00; J0[1] = a01; J0[2] = a02;
  J0[3] = a02 * pc1 - a01 * pc2;
  J0[4] = a00 * pc2 - a02 * pc0;
  J0[5] = a01 * pc0 - a00 * pc1;
  J1[0] = a10; J1[1] = a11; J1[2] = a12;
  J1[3] = a12 * pc1 - a11 * pc2;
  J1[4] = a10 * pc2 - a12 * pc0;
  J1[5] = a11 * pc0 - a10 * pc1;
  float W0[6], W1[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    W0[i] = w * J0[i];
    W1[i] = w * J1[i];
  }
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) {
      a.h[k] = fmaf(W0[i], J0[j], fmaf(W1[i], J1[j], a.h[k]));
      ++k;
    }
    a.b[i] = fmaf(W0[i], e0, fmaf(W1[i], e1, a.b[i]));
  }
}

// The reciprocal of the depth (ph2 == pc2 exactly): RCP_CHECK decides per pair by a wave vote;
// RCP_FAST: the caller's vote found every depth of the section inside rcp_safe's range (rcp_rn,
// exhaustively verified); RCP_DIV: the IEEE division.
#define RCP_CHECK 0
#define RCP_FAST 1
#define RCP_DIV 2

// Pinhole camera K = [fx 0 cx; 0 fy cy; 0 0 1] (the reference's K, src/cam.cpp:11-16; the
// runtime selects this path only when K has exactly that structure).  Every term the general
// form multiplies by one of K's zeros is an exact +-0 and K(2,2) = 1 makes ph2 == pc2, so with
// those terms dropped the projection, bounds test, error and chi -- the gate -- AND the
// Jacobian, evaluated in the oracle's operation order with contraction off
// (oracle/picp_oracle.c or_error_and_jacobian: (Jp*K)*[I | skew(-pc)]), are bit-identical to
// the reference arithmetic for finite inputs (a sign of zero can differ only where pc2 == 0,
// which is rejected):
//   a00 = fx/z, a02 = cx/z - ph0/z^2, a11 = fy/z, a12 = cy/z - ph1/z^2
//   J0 = [a00, 0, a02, a02 pc1, a00 pc2 - a02 pc0, -a00 pc1]
//   J1 = [0, a11, a12, a12 pc1 - a11 pc2, -a12 pc0, a11 pc0]
// For a used item whose Jacobian is not finite (a NaN point passes the gate as in the reference)
// the reference's products with K's zeros are NaN, not 0.  Every entry of H and b but H(0,1) keeps
// a term that carries the NaN; H(0,1) consists of dropped terms only.  The pair form adds them
// back in the waves that take the division (pinhole2_h01_dropped), so picp_linearize returns the
// reference's all-NaN H; the one-slot form leaves H(0,1) = 0 there (the solve of such an H gives a
// NaN pose either way).
// The structural zeros drop 12 of the 54 multiply-adds of H and b, and lambda = sqrt(thr/chi)
// comes from v_rsq (it only weighs kept outliers, within the H/b tolerance): ~1/3 fewer VALU
// instructions per correspondence than the general path.  KEEP (keep_outliers, compile time):
// without it every used item has weight 1 and every other item has J = e = 0 (zeroed inputs),
// so H and b take J itself -- bit-identical to multiplying by w in {0, 1}, 10 multiplies fewer.
// The camera-frame depth of one item in accumulate_pinhole's exact operation order (so the
// compiler shares it with the item's projection).
__device__ __forceinline__ float item_depth(const Pose& T, float x, float y, float z) {
#pragma clang fp contract(off)
  return ((T.r20 * x + T.r21 * y) + T.r22 * z) + T.t2;  // src/camera.h:26, row 2
}

// RCP: RCP_DIV (the IEEE division) or RCP_FAST (rcp_rn: the caller's wave vote found the depth
// inside rcp_safe's range; the same bits).
template <bool KEEP, int RCP = RCP_DIV>
__device__ __forceinline__ void accumulate_pinhole(const Pose& T, const Cam& C, float thr,
                                                   float inv_thr, float x, float y,
                                                   float z, float u, float v, bool in_range,
                                                   Acc& a, Cnt& n) {
  float pc0, pc1, pc2, ph0, ph1, iz, e0, e1, chi;
  bool valid, proj;
  {
#pragma clang fp contract(off)
    pc0 = ((T.r00 * x + T.r01 * y) + T.r02 * z) + T.t0;  // src/camera.h:26
    pc1 = ((T.r10 * x + T.r11 * y) + T.r12 * z) + T.t1;
    pc2 = ((T.r20 * x + T.r21 * y) + T.r22 * z) + T.t2;
    ph0 = C.k00 * pc0 + C.k02 * pc2;  // src/camera.h:29 without the zero terms
    ph1 = C.k11 * pc1 + C.k12 * pc2;
    iz = (RCP == RCP_FAST) ? rcp_rn(pc2) : 1.0f / pc2;  // ph2 == pc2 exactly
    const float ix = ph0 * iz;
    const float iy = ph1 * iz;
    // bitwise, not short-circuit: the same predicate without per-item exec-mask branches
    proj = !(pc2 <= 0.0f) & !((ix < 0.0f) | (ix > C.maxx) | (iy < 0.0f) | (iy > C.maxy));
    valid = in_range & proj;
    e0 = ix - u;
    e1 = iy - v;
    chi = e0 * e0 + e1 * e1;
  }
  const bool outlier = chi > thr;
  const bool inl = valid & !outlier;
  const bool use = inl | (valid & KEEP);
  // the robust weight only when outliers are kept
  const float w = KEEP ? (use ? (inl ? 1.0f : __builtin_amdgcn_rsqf(chi * inv_thr)) : 0.0f) : 1.0f;
  a.chi_in += inl ? chi : 0.0f;
  a.chi_out += (valid && outlier) ? chi : 0.0f;
  cnt_add(n, inl, valid);
  // A skipped point gets weight 0 and zeroed inputs, so it can never inject 0 * inf.  The
  // zeroing only matters for points whose J could be non-finite: ones that do not project, or
  // project from a depth under 1e-12.  A skipped point that projects from a larger depth
  // (an outlier, a padding lane's copy) has finite pc, ph and, with a finite chi, finite e: its
  // J is exactly 0 once iz alone is zeroed, and fma(+-0, finite, h) == h exactly (the sums start
  // at +0 and never become -0), so waves without a dangerous skipped point zero only iz, with
  // bit-identical H and b.
  if (__all(use | (proj & (pc2 >= 1e-12f) & (chi <= FLT_MAX)))) {
    iz = use ? iz : 0.0f;
  } else {
    iz = use ? iz : 0.0f;
    pc0 = use ? pc0 : 0.0f;
    pc1 = use ? pc1 : 0.0f;
    pc2 = use ? pc2 : 0.0f;
    ph0 = use ? ph0 : 0.0f;
    ph1 = use ? ph1 : 0.0f;
    e0 = use ? e0 : 0.0f;
    e1 = use ? e1 : 0.0f;
  }
  float J0[6], J1[6];
  {
#pragma clang fp contract(off)
    const float iz2 = iz * iz;  // src/picp_solver.cpp:45-50
    const float jp0 = -(ph0 * iz2), jp1 = -(ph1 * iz2);
    const float a00 = iz * C.k00, a02 = iz * C.k02 + jp0;
    const float a11 = iz * C.k11, a12 = iz * C.k12 + jp1;
    J0[0] = a00; J0[1] = 0.0f; J0[2] = a02;
    J0[3] = a02 * pc1;
    J0[4] = a00 * pc2 - a02 * pc0;
    J0[5] = -(a00 * pc1);
    J1[0] = 0.0f; J1[1] = a11; J1[2] = a12;
    J1[3] = -(a11 * pc2) + a12 * pc1;
    J1[4] = -(a12 * pc0);
    J1[5] = a11 * pc0;
  }
  float W0[6], W1[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    W0[i] = KEEP ? w * J0[i] : J0[i];
    W1[i] = KEEP ? w * J1[i] : J1[i];
  }
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) {
      float h = a.h[k];
      if (i != 0 && j != 0) h = fmaf(W1[i], J1[j], h);  // J1[0] == 0
      if (i != 1 && j != 1) h = fmaf(W0[i], J0[j], h);  // J0[1] == 0
      a.h[k] = h;
      ++k;
    }
    float bb = a.b[i];
    if (i != 0) bb = fmaf(W1[i], e1, bb);
    if (i != 1) bb = fmaf(W0[i], e0, bb);
    a.b[i] = bb;
  }
}

// The state of one correspondence at a pose (include/picp_c.h PICP_CORR_*: 0 skipped, 1 inlier,
// 2 outlier) with its chi2 and projection (-1 where skipped): the projection, bounds test, error
// and chi2 of accumulate_one (general K) or accumulate_pinhole (pinhole K: the zero terms of K
// dropped, ph2 == pc2) restated with contraction off, in their operation order and with the
// IEEE division, so all three are bit-identical to the oracle's or_error_and_jacobian /
// or_project_point at the same pose -- and so to what the solve kernels decide.  The accumulate
// functions are deliberately not rewritten on top of this one: their code stays as measured.
__device__ __forceinline__ int classify_item(const Pose& T, const Cam& C, float thr, bool pinhole,
                                             float x, float y, float z, float u, float v,
                                             float* chi_out, float* iu, float* iv) {
#pragma clang fp contract(off)
  const float pc0 = ((T.r00 * x + T.r01 * y) + T.r02 * z) + T.t0;  // src/camera.h:26
  const float pc1 = ((T.r10 * x + T.r11 * y) + T.r12 * z) + T.t1;
  const float pc2 = ((T.r20 * x + T.r21 * y) + T.r22 * z) + T.t2;
  float ph0, ph1, ph2;
  if (pinhole) {  // uniform
    ph0 = C.k00 * pc0 + C.k02 * pc2;  // src/camera.h:29 without the zero terms
    ph1 = C.k11 * pc1 + C.k12 * pc2;
    ph2 = pc2;
  } else {
    ph0 = (C.k00 * pc0 + C.k01 * pc1) + C.k02 * pc2;
    ph1 = (C.k10 * pc0 + C.k11 * pc1) + C.k12 * pc2;
    ph2 = (C.k20 * pc0 + C.k21 * pc1) + C.k22 * pc2;
  }
  const float iz = 1.0f / ph2;  // src/camera.h:30, correctly rounded
  const float ix = ph0 * iz;
  const float iy = ph1 * iz;
  // src/camera.h:27-28 (z <= 0 rejects; NaN passes as in the reference) and :31-34
  const bool valid = !(pc2 <= 0.0f) & !((ix < 0.0f) | (ix > C.maxx) | (iy < 0.0f) | (iy > C.maxy));
  const float e0 = ix - u;  // src/picp_solver.cpp:34
  const float e1 = iy - v;
  const float chi = e0 * e0 + e1 * e1;  // src/picp_solver.cpp:74
  *chi_out = valid ? chi : -1.0f;
  *iu = valid ? ix : -1.0f;
  *iv = valid ? iy : -1.0f;
  return valid ? ((chi > thr) ? 2 : 1) : 0;  // src/picp_solver.cpp:77, strict gate
}

// The general-K per-item math of accumulate_one up to the weighted Jacobian (for the packed
// pair accumulation): outputs are zeroed for an unused item, w is its kernel weight.
struct Item {
  float J0[6], J1[6], e0, e1, w, chi;
  bool inl, valid;
};

__device__ __forceinline__ void item_general(const Pose& T, const Cam& C, float thr, bool keep,
                                             float x, float y, float z, float u, float v,
                                             bool in_range, Item& o) {
  float pc0, pc1, pc2, ph0, ph1, ph2, iz, e0, e1, chi;
  bool valid;
  {
#pragma clang fp contract(off)
    pc0 = ((T.r00 * x + T.r01 * y) + T.r02 * z) + T.t0;
    pc1 = ((T.r10 * x + T.r11 * y) + T.r12 * z) + T.t1;
    pc2 = ((T.r20 * x + T.r21 * y) + T.r22 * z) + T.t2;
    ph0 = (C.k00 * pc0 + C.k01 * pc1) + C.k02 * pc2;
    ph1 = (C.k10 * pc0 + C.k11 * pc1) + C.k12 * pc2;
    ph2 = (C.k20 * pc0 + C.k21 * pc1) + C.k22 * pc2;
    iz = 1.0f / ph2;
    const float ix = ph0 * iz;
    const float iy = ph1 * iz;
    // bitwise, not short-circuit: the same predicate without per-item exec-mask branches
    valid = in_range & !(pc2 <= 0.0f) & !((ix < 0.0f) | (ix > C.maxx) | (iy < 0.0f) | (iy > C.maxy));
    e0 = ix - u;
    e1 = iy - v;
    chi = e0 * e0 + e1 * e1;
  }
  const bool outlier = chi > thr;
  const bool inl = valid & !outlier;
  const bool use = inl | (valid & keep);
  const float lambda = outlier ? sqrtf(thr / chi) : 1.0f;
  o.w = use ? (inl ? 1.0f : lambda) : 0.0f;
  o.chi = chi;
  o.inl = inl;
  o.valid = valid;
  iz = use ? iz : 0.0f;
  pc0 = use ? pc0 : 0.0f;
  pc1 = use ? pc1 : 0.0f;
  pc2 = use ? pc2 : 0.0f;
  ph0 = use ? ph0 : 0.0f;
  ph1 = use ? ph1 : 0.0f;
  o.e0 = use ? e0 : 0.0f;
  o.e1 = use ? e1 : 0.0f;
  const float iz2 = iz * iz;
  const float jp02 = -ph0 * iz2, jp12 = -ph1 * iz2;
  const float a00 = iz * C.k00 + jp02 * C.k20;
  const float a01 = iz * C.k01 + jp02 * C.k21;
  const float a02 = iz * C.k02 + jp02 * C.k22;
  const float a10 = iz * C.k10 + jp12 * C.k20;
  const float a11 = iz * C.k11 + jp12 * C.k21;
  const float a12 = iz * C.k12 + jp12 * C.k22;
  o.J0[0] = a00; o.J0[1] = a01; o.J0[2] = a02;
  o.J0[3] = a02 * pc1 - a01 * pc2;
  o.J0[4] = a00 * pc2 - a02 * pc0;
  o.J0[5] = a01 * pc0 - a00 * pc1;
  o.J1[0] = a10; o.J1[1] = a11; o.J1[2] = a12;
  o.J1[3] = a12 * pc1 - a11 * pc2;
  o.J1[4] = a10 * pc2 - a12 * pc0;
  o.J1[5] = a11 * pc0 - a10 * pc1;
}

// H += w (J0^T J0 + J1^T J1), b += w (J0^T e0 + J1^T e1) for both slots; SPARSE skips the
// pinhole Jacobian's structural zeros J0[1] = J1[0] = 0; !WEIGHTED: w is 1 for every item whose
// J is not zero (outliers rejected), so w is not applied
template <bool SPARSE, bool WEIGHTED>
__device__ __forceinline__ void acc2_normal(const f2 J0[6], const f2 J1[6], f2 e0, f2 e1, f2 w,
                                            Acc2& a) {
  f2 W0[6], W1[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    W0[i] = WEIGHTED ? w * J0[i] : J0[i];
    W1[i] = WEIGHTED ? w * J1[i] : J1[i];
  }
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) {
      f2 h = a.h[k];
      if (!SPARSE || (i != 0 && j != 0)) h = __builtin_elementwise_fma(W1[i], J1[j], h);
      if (!SPARSE || (i != 1 && j != 1)) h = __builtin_elementwise_fma(W0[i], J0[j], h);
      a.h[k] = h;
      ++k;
    }
    f2 bb = a.b[i];
    if (!SPARSE || i != 0) bb = __builtin_elementwise_fma(W1[i], e1, bb);
    if (!SPARSE || i != 1) bb = __builtin_elementwise_fma(W0[i], e0, bb);
    a.b[i] = bb;
  }
}

__device__ __forceinline__ void acc2_stats(f2 chi, bool inlA, bool inlB, bool validA, bool validB,
                                           Acc2& a, Cnt& n) {
  a.chi_in += (f2){inlA ? chi.x : 0.0f, inlB ? chi.y : 0.0f};
  a.chi_out += (f2){(validA & !inlA) ? chi.x : 0.0f, (validB & !inlB) ? chi.y : 0.0f};
  cnt_add(n, inlA, validA);
  cnt_add(n, inlB, validB);
}

// A pair of correspondences, pinhole K: accumulate_pinhole's exact arithmetic with every
// elementwise step written on float2 (A in .x, B in .y).  Only the correctly rounded reciprocal, the
// compares and the selects stay per item.  Contraction is off exactly where the oracle has it
// off (gate and Jacobian), so both items are bit-identical to the scalar path.
// The camera-frame depth of a pair, in the exact operation order of accumulate_pinhole2 (so the
// compiler shares it): callers check a whole section of pairs for the fast reciprocal at once.
__device__ __forceinline__ f2 pair_depth(const Pose& T, f2 x, f2 y, f2 z) {
#pragma clang fp contract(off)
  return ((T.r20 * x + T.r21 * y) + T.r22 * z) + T.t2;  // src/camera.h:26, row 2
}

__device__ __forceinline__ bool pair_rcp_safe(const Pose& T, f2 x, f2 y, f2 z) {
  const f2 d = pair_depth(T, x, y, z);
  return rcp_safe(d.x) & rcp_safe(d.y);
}

// What the sparse pinhole form drops from H(0,1), for the waves that take the division (a lane
// holds an extreme depth): w (J(0,0) J(0,1) + J(1,0) J(1,1)) of a used item with the reference's
// J(0,1) = iz*0 + jp0*0 and J(1,0) = iz*0 + jp1*0 (src/picp_solver.cpp:47-52, the products with
// K's zeros): +-0 while iz and jp are finite -- H(0,1) keeps its bits -- and NaN otherwise, so an
// item that passes the gate with a NaN or infinite Jacobian (NaN passes as in the reference)
// makes H(0,1) NaN as it makes every other entry.  The gate is restated here, inside the rare
// branch, so that the common path keeps its instruction stream: this is a SECOND COPY of the
// bounds test, chi, inlier / use flags and robust weight of accumulate_pinhole2 below and has to
// change with them.
template <bool KEEP>
__device__ __forceinline__ f2 pinhole2_h01_dropped(const Cam& C, float thr, float inv_thr, f2 ph0, f2 ph1,
                                                   f2 pc2, f2 iz, f2 u, f2 v, bool inA, bool inB) {
#pragma clang fp contract(off)
  const f2 ix = ph0 * iz, iy = ph1 * iz;
  const bool validA = inA & !(pc2.x <= 0.0f) & !((ix.x < 0.0f) | (ix.x > C.maxx) | (iy.x < 0.0f) | (iy.x > C.maxy));
  const bool validB = inB & !(pc2.y <= 0.0f) & !((ix.y < 0.0f) | (ix.y > C.maxx) | (iy.y < 0.0f) | (iy.y > C.maxy));
  const f2 e0 = ix - u, e1 = iy - v;
  const f2 chi = e0 * e0 + e1 * e1;
  const bool inlA = validA & !(chi.x > thr), inlB = validB & !(chi.y > thr);
  const bool useA = inlA | (validA & KEEP), useB = inlB | (validB & KEEP);
  const f2 iz2 = iz * iz;
  const f2 j01 = iz * 0.0f + -(ph0 * iz2) * 0.0f, j10 = iz * 0.0f + -(ph1 * iz2) * 0.0f;
  f2 t = (iz * C.k00) * j01 + j10 * (iz * C.k11);
  if constexpr (KEEP) {
    const f2 q = chi * inv_thr;
    t = (f2){(inlA ? 1.0f : __builtin_amdgcn_rsqf(q.x)) * t.x, (inlB ? 1.0f : __builtin_amdgcn_rsqf(q.y)) * t.y};
  }
  return (f2){useA ? t.x : 0.0f, useB ? t.y : 0.0f};
}

template <bool KEEP, int RCP = RCP_CHECK>
__device__ __forceinline__ void accumulate_pinhole2(const Pose& T, const Cam& C, float thr,
                                                    float inv_thr, f2 x, f2 y, f2 z,
                                                    f2 u, f2 v, bool inA, bool inB, Acc2& a, Cnt& n) {
  f2 pc0, pc1, pc2, ph0, ph1, iz, e0, e1, chi;
  bool validA, validB;
  {
#pragma clang fp contract(off)
    pc0 = ((T.r00 * x + T.r01 * y) + T.r02 * z) + T.t0;  // src/camera.h:26
    pc1 = ((T.r10 * x + T.r11 * y) + T.r12 * z) + T.t1;
    pc2 = pair_depth(T, x, y, z);
    ph0 = C.k00 * pc0 + C.k02 * pc2;  // src/camera.h:29 without the zero terms
    ph1 = C.k11 * pc1 + C.k12 * pc2;
    // ph2 == pc2 exactly; the correctly rounded reciprocal per item (rcp_rn, exhaustively
    // verified), the IEEE division only when a lane of the wave holds an extreme value
    if (RCP == RCP_FAST || (RCP == RCP_CHECK && __all(rcp_safe(pc2.x) & rcp_safe(pc2.y)))) {
      iz.x = rcp_rn(pc2.x);
      iz.y = rcp_rn(pc2.y);
    } else {
      iz.x = 1.0f / pc2.x;
      iz.y = 1.0f / pc2.y;
      a.h[1] += pinhole2_h01_dropped<KEEP>(C, thr, inv_thr, ph0, ph1, pc2, iz, u, v, inA, inB);
    }
    const f2 ix = ph0 * iz;
    const f2 iy = ph1 * iz;
    // bitwise, not short-circuit: the same predicate without per-item exec-mask branches
    // (this gate, down to the weight, has a second copy in pinhole2_h01_dropped: keep them in step)
    validA = inA & !(pc2.x <= 0.0f) &
             !((ix.x < 0.0f) | (ix.x > C.maxx) | (iy.x < 0.0f) | (iy.x > C.maxy));
    validB = inB & !(pc2.y <= 0.0f) &
             !((ix.y < 0.0f) | (ix.y > C.maxx) | (iy.y < 0.0f) | (iy.y > C.maxy));
    e0 = ix - u;
    e1 = iy - v;
    chi = e0 * e0 + e1 * e1;
  }
  const bool outA = chi.x > thr, outB = chi.y > thr;
  const bool inlA = validA & !outA, inlB = validB & !outB;
  const bool useA = inlA | (validA & KEEP), useB = inlB | (validB & KEEP);
  f2 w = {1.0f, 1.0f};
  if constexpr (KEEP) {  // the robust weight only when outliers are kept
    const f2 q = chi * inv_thr;
    w = (f2){useA ? (inlA ? 1.0f : __builtin_amdgcn_rsqf(q.x)) : 0.0f,
             useB ? (inlB ? 1.0f : __builtin_amdgcn_rsqf(q.y)) : 0.0f};
  }
  acc2_stats(chi, inlA, inlB, validA, validB, a, n);
  // a skipped item gets weight 0 and zeroed inputs, so it can never inject inf/NaN.  (Skipping
  // these selects for waves of projectable items, as accumulate_pinhole does, measured 1-4 %
  // slower here: the branches split the unrolled pairs' straight-line schedule.)
#define PICP_Z2(val) val = (f2){useA ? val.x : 0.0f, useB ? val.y : 0.0f}
  PICP_Z2(iz); PICP_Z2(pc0); PICP_Z2(pc1); PICP_Z2(pc2); PICP_Z2(ph0); PICP_Z2(ph1); PICP_Z2(e0); PICP_Z2(e1);
#undef PICP_Z2
  f2 J0[6], J1[6];
  {
#pragma clang fp contract(off)
    const f2 iz2 = iz * iz;  // src/picp_solver.cpp:45-52, the oracle's operation order
    const f2 jp0 = -(ph0 * iz2), jp1 = -(ph1 * iz2);
    const f2 a00 = iz * C.k00, a02 = iz * C.k02 + jp0;
    const f2 a11 = iz * C.k11, a12 = iz * C.k12 + jp1;
    const f2 zero = {0.0f, 0.0f};
    J0[0] = a00; J0[1] = zero; J0[2] = a02;
    J0[3] = a02 * pc1;
    J0[4] = a00 * pc2 - a02 * pc0;
    J0[5] = -(a00 * pc1);
    J1[0] = zero; J1[1] = a11; J1[2] = a12;
    J1[3] = -(a11 * pc2) + a12 * pc1;
    J1[4] = -(a12 * pc0);
    J1[5] = a11 * pc0;
  }
  acc2_normal<true, KEEP>(J0, J1, e0, e1, w, a);
}

// A pair of correspondences, general K: per-item math (item_general), paired accumulation.
__device__ __forceinline__ void accumulate_general2(const Pose& T, const Cam& C, float thr, bool keep,
                                                    f2 x, f2 y, f2 z, f2 u, f2 v, bool inA,
                                                    bool inB, Acc2& a, Cnt& n) {
  Item A, B;
  item_general(T, C, thr, keep, x.x, y.x, z.x, u.x, v.x, inA, A);
  item_general(T, C, thr, keep, x.y, y.y, z.y, u.y, v.y, inB, B);
  acc2_stats((f2){A.chi, B.chi}, A.inl, B.inl, A.valid, B.valid, a, n);
  f2 J0[6], J1[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    J0[i] = (f2){A.J0[i], B.J0[i]};
    J1[i] = (f2){A.J1[i], B.J1[i]};
  }
  acc2_normal<false, true>(J0, J1, (f2){A.e0, B.e0}, (f2){A.e1, B.e1}, (f2){A.w, B.w}, a);
}

// PH: the per-item variant (PICP_V_*); keep is read only by the general variant; RCP: how the
// pinhole variants take the reciprocal (RCP_*)
template <int PH, int RCP = RCP_CHECK>
__device__ __forceinline__ void accumulate2(const Pose& T, const Cam& C, float thr, float inv_thr,
                                            bool keep, f2 x, f2 y, f2 z, f2 u, f2 v, bool inA,
                                            bool inB, Acc2& a, Cnt& n) {
  if constexpr (PH == PICP_V_GENERAL)
    accumulate_general2(T, C, thr, keep, x, y, z, u, v, inA, inB, a, n);
  else
    accumulate_pinhole2<PH == PICP_V_PINHOLE_KEEP, RCP>(T, C, thr, inv_thr, x, y, z, u, v, inA, inB, a, n);
}

// NPT register-resident items per lane (item k at lane + k * stride) as pairs (k, k + 1) (NPT == 1:
// slot B repeats item 0, masked), with ONE wave vote on the fast reciprocal for the whole set
// instead of one per pair: the pairs then run as one straight-line block (a vote per pair split
// them into blocks, so every per-item predicate crossing the block edge was kept as a 0/1 VGPR and
// compared again, and the masks' scalar registers spilled).
template <int PH, int NPT>
__device__ __forceinline__ void accumulate_regs(const Pose& T, const Cam& C, float thr, float inv_thr,
                                                bool keep, const float* xs, const float* ys,
                                                const float* zs, const float* us, const float* vs,
                                                int first, int stride, int n, Acc2& a, Cnt& cnt) {
  bool fast = true;
  if constexpr (PH != PICP_V_GENERAL) {
#pragma unroll
    for (int k = 0; k < NPT; k += 2) {
      const int k1 = (k + 1 < NPT) ? k + 1 : k;
      fast &= pair_rcp_safe(T, (f2){xs[k], xs[k1]}, (f2){ys[k], ys[k1]}, (f2){zs[k], zs[k1]});
    }
  }
  auto run = [&](auto rcp) {
#pragma unroll
    for (int k = 0; k < NPT; k += 2) {
      const int k1 = (k + 1 < NPT) ? k + 1 : k;
      accumulate2<PH, decltype(rcp)::value>(T, C, thr, inv_thr, keep, (f2){xs[k], xs[k1]}, (f2){ys[k], ys[k1]},
                                            (f2){zs[k], zs[k1]}, (f2){us[k], us[k1]}, (f2){vs[k], vs[k1]},
                                            first + k * stride < n, k + 1 < NPT && first + (k + 1) * stride < n,
                                            a, cnt);
    }
  };
  if (PH == PICP_V_GENERAL || __all(fast))
    run(std::integral_constant<int, RCP_FAST>());
  else
    run(std::integral_constant<int, RCP_DIV>());
}

// Which accumulation form a kernel with NPT register-resident items per lane uses.  Measured on
// MI355X with the unpacked build (profiles/r03/acc/): one slot is faster at small NPT (C5, NPT 4:
// +2.7 %), the two-slot pair form at NPT 8 (C3 +5-9 %, C4 +17 %: its two independent
// accumulation chains and its paired LDS/stream loops).  (One slot with the per-item math in
// pairs gave the same bits and no gain: DESIGN.md Appendix A, "paired one-slot".)
__host__ __device__ constexpr bool acc_pairs(int npt) { return npt >= 8; }

// accumulate_regs with ONE accumulator slot, item by item (the default since the device code is
// built without packed FP32, hipcc_nopk.sh): the pair form's two slots only paid for themselves
// as packed instructions; unpacked, they double the accumulator registers (58 instead of 29 per
// lane) and every per-pair select.  The fast-reciprocal vote is taken once for the whole set.
// The sum runs over the items in order k = 0 .. NPT-1 (the pair form summed even and odd items in
// separate slots): the bits differ from it in the last place, within the H/b tolerance.
template <int PH, int NPT>
__device__ __forceinline__ void accumulate_regs1(const Pose& T, const Cam& C, float thr, float inv_thr,
                                                 bool keep, const float* xs, const float* ys,
                                                 const float* zs, const float* us, const float* vs,
                                                 int first, int stride, int n, Acc& a, Cnt& cnt) {
  if constexpr (PH == PICP_V_GENERAL) {
#pragma unroll
    for (int k = 0; k < NPT; ++k)
      accumulate_one(T, C, thr, keep, xs[k], ys[k], zs[k], us[k], vs[k], first + k * stride < n, a, cnt);
  } else {
    bool fast = true;
#pragma unroll
    for (int k = 0; k < NPT; ++k) fast &= rcp_safe(item_depth(T, xs[k], ys[k], zs[k]));
    auto run = [&](auto rcp) {
      constexpr bool KP = PH == PICP_V_PINHOLE_KEEP;
      constexpr int R = decltype(rcp)::value;
#pragma unroll
      for (int k = 0; k < NPT; ++k)
        // the last slot only in waves that hold an item there (a wave-uniform branch): a frame
        // that fills 3.5 of 4 slots leaves whole waves empty in it, and with waves dealt to the
        // SIMDs in turn every SIMD then issues one slot less when n <= (NPT - 1/2) x BS (C5's
        // ~1,750 correspondences on 2,048 slots).  A skipped item adds exact zeros: same bits.
        if (NPT < 2 || k + 1 < NPT || __any(first + k * stride < n))
          accumulate_pinhole<KP, R>(T, C, thr, inv_thr, xs[k], ys[k], zs[k], us[k], vs[k], first + k * stride < n, a,
                                    cnt);
    };
    if (__all(fast))
      run(std::integral_constant<int, RCP_FAST>());
    else
      run(std::integral_constant<int, RCP_DIV>());
  }
}

// One streamed (LDS or HBM) item, pinhole or general, the fast reciprocal by a vote of the lanes
// that run this item (the loops that call it are divergent).
template <int PH>
__device__ __forceinline__ void accumulate_item(const Pose& T, const Cam& C, float thr, float inv_thr,
                                                bool keep, float x, float y, float z, float u, float v,
                                                bool in_range, Acc& a, Cnt& n) {
  if constexpr (PH == PICP_V_GENERAL) {
    accumulate_one(T, C, thr, keep, x, y, z, u, v, in_range, a, n);
  } else {
    if (__all(rcp_safe(item_depth(T, x, y, z))))
      accumulate_pinhole<PH == PICP_V_PINHOLE_KEEP, RCP_FAST>(T, C, thr, inv_thr, x, y, z, u, v, in_range, a, n);
    else
      accumulate_pinhole<PH == PICP_V_PINHOLE_KEEP, RCP_DIV>(T, C, thr, inv_thr, x, y, z, u, v, in_range, a, n);
  }
}

// Streamed (LDS or HBM) items i, i + stride, i + 2 stride, ... (i = first) of one lane into one
// slot, in that order, item by item (accumulate_item).  get(i, x, y, z, u, v) loads item i.
template <int PH, typename Get>
__device__ __forceinline__ void accumulate_stream1(const Pose& T, const Cam& C, float thr, float inv_thr, bool keep,
                                                   int first, int stride, int count, Get get, Acc& a, Cnt& n) {
  for (int i = first; i < count; i += stride) {
    float x, y, z, u, v;
    get(i, x, y, z, u, v);
    accumulate_item<PH>(T, C, thr, inv_thr, keep, x, y, z, u, v, true, a, n);
  }
}

__device__ __forceinline__ void acc_zero(Acc& a) {
#pragma unroll
  for (int i = 0; i < 21; ++i) a.h[i] = 0.0f;
#pragma unroll
  for (int i = 0; i < 6; ++i) a.b[i] = 0.0f;
  a.chi_in = a.chi_out = 0.0f;
}

__device__ __forceinline__ void acc_fold(const Acc& a, float v[PICP_NPART]) {
#pragma unroll
  for (int i = 0; i < 21; ++i) v[PICP_P_H + i] = a.h[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) v[PICP_P_B + i] = a.b[i];
  v[PICP_P_CHI_IN] = a.chi_in;
  v[PICP_P_CHI_OUT] = a.chi_out;
  v[PICP_P_N_IN] = 0.0f;
  v[PICP_P_N_PROJ] = 0.0f;
  v[31] = 0.0f;
}

// one correspondence with the variant chosen at compile time
template <int PH>
__device__ __forceinline__ void accumulate(const Pose& T, const Cam& C, float thr, float inv_thr,
                                           bool keep, float x, float y, float z, float u,
                                           float v, bool in_range, Acc& a, Cnt& n) {
  if constexpr (PH == PICP_V_GENERAL)
    accumulate_one(T, C, thr, keep, x, y, z, u, v, in_range, a, n);
  else
    accumulate_pinhole<PH == PICP_V_PINHOLE_KEEP>(T, C, thr, inv_thr, x, y, z, u, v, in_range, a, n);
}

}  // namespace picp
