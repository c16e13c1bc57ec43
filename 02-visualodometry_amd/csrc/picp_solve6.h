// picp_solve6.h -- the finish of a PICP round from its totals: the damped 6x6 LDL^T solve and the
// v2tEuler left update (src/picp_solver.cpp:93-105, src/defs.h:100-136), the icp_test convergence
// rule (exec/icp_test.cpp:99-106), uniform or spread over the lanes of the finishing wave, and
// the stores of the resulting state.
#pragma once
#include <hip/hip_runtime.h>

#include <float.h>
#include <stdint.h>

#include "picp_internal.h"

namespace picp {

// Damped normal equations -> dx, in float32, the precision the reference solves in
// (Matrix6f::ldlt, src/picp_solver.cpp:102); H and b arrive as exact double sums.  LDL^T without
// pivoting, by Gaussian elimination on the LOWER triangle (H + damping*I is SPD: Eigen's diagonal
// pivoting only changes rounding): step j scales column j by 1/d_j and updates the trailing
// lower triangle; the back substitution reads U = D L^T from the lower entries (symmetry).  Pivot
// reciprocals are the hardware v_rcp_f32 (<= 1 ulp).  A pivot with |d| <= FLT_MIN gives 1/d = 0,
// Eigen's zero-pivot rule for float; that test is kept off the pivot chain (a flag, and the rare
// flagged system is solved again with the guard in the chain).  One lane, registers only, every
// index compile-time: the per-round critical path of every kernel (tools/ubench/parts_ubench).
// Row r of the system is read from the converted totals tw (total_word: damping folded into the
// diagonal, -b), upper triangle row-major.
__device__ __forceinline__ int tri_index(int r, int c) {  // upper-triangle slot of (min, max)
  const int lo = r < c ? r : c, hi = r < c ? c : r;
  return PICP_P_H + lo * (11 - lo) / 2 + hi;
}

template <bool GUARD>
__device__ __forceinline__ bool ldl6_solve(const float* tw, float dx[6]) {
  float a[6][6], rhs[6], id[6];
  bool bad = false;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int c = 0; c <= i; ++c) a[i][c] = tw[tri_index(c, i)];
    rhs[i] = tw[PICP_P_B + i];
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const float d = a[j][j];
    float inv = __builtin_amdgcn_rcpf(d);
    if (GUARD) inv = (fabsf(d) > FLT_MIN) ? inv : 0.0f;
    else bad |= !(fabsf(d) > FLT_MIN);
    id[j] = inv;
    float f[6];
#pragma unroll
    for (int i = j + 1; i < 6; ++i) f[i] = a[i][j] * inv;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
#pragma unroll
      for (int c = j + 1; c <= i; ++c) a[i][c] = fmaf(-f[i], a[c][j], a[i][c]);
      rhs[i] = fmaf(-f[i], rhs[j], rhs[i]);
    }
  }
#pragma unroll
  for (int k = 5; k >= 0; --k) {
    const float x = rhs[k] * id[k];
    dx[k] = x;
#pragma unroll
    for (int i = 0; i < k; ++i) rhs[i] = fmaf(-a[k][i], x, rhs[i]);
  }
  return bad;
}

__device__ __forceinline__ void ldl6_solve(const float* tw, float dx[6]) {
  if (ldl6_solve<false>(tw, dx)) ldl6_solve<true>(tw, dx);  // a (near-)zero pivot: rare
}

// sin/cos of GN increment angles.  Increments are small, so the float Taylor series (exact to
// float rounding for |a| <= 1/16: next term a^9/9! < 1e-16) avoids sincosf's range reduction
// on the critical path; ONE test for the three angles keeps the common case straight-line (three
// independent polynomial chains); larger angles take the libm path.
__device__ __forceinline__ void taylor_sincos(float a, float* s, float* c) {
  const float a2 = a * a;
  *s = a * fmaf(a2, fmaf(a2, fmaf(a2, -1.0f / 5040.0f, 1.0f / 120.0f), -1.0f / 6.0f), 1.0f);
  *c = fmaf(a2, fmaf(a2, fmaf(a2, fmaf(a2, 1.0f / 40320.0f, -1.0f / 720.0f), 1.0f / 24.0f), -0.5f), 1.0f);
}

// src/defs.h:100-136 v2tEuler's rotation: Rd = Rx(a)*Ry(b)*Rz(c) (float) of dx[3..5].
// ONE_CMP: the range test as one compare, the unsigned maximum of the three |angle| bit patterns
// against the bits of 0.0625 (positive floats order as their bits; a NaN's bits lie above every
// finite value's, so it takes the libm path as it does with the three float compares), and the
// Taylor path as the fall-through.  The same path for every input, so the same bits.
template <bool ONE_CMP = false>
__device__ __forceinline__ void update_rotation(const float dx[6], float Rd[3][3]) {
  float sa, ca, sb, cb, sc, cc;
  bool small;
  if constexpr (ONE_CMP) {
    const unsigned a = __float_as_uint(dx[3]) & 0x7fffffffu, b = __float_as_uint(dx[4]) & 0x7fffffffu,
                   c = __float_as_uint(dx[5]) & 0x7fffffffu;
    const unsigned ab = a > b ? a : b;
    small = __builtin_expect((ab > c ? ab : c) <= 0x3d800000u, 1);  // 0x3d800000: 0.0625f
  } else {
    small = fabsf(dx[3]) <= 0.0625f && fabsf(dx[4]) <= 0.0625f && fabsf(dx[5]) <= 0.0625f;
  }
  if (small) {
    taylor_sincos(dx[3], &sa, &ca);
    taylor_sincos(dx[4], &sb, &cb);
    taylor_sincos(dx[5], &sc, &cc);
  } else {
    sincosf(dx[3], &sa, &ca);
    sincosf(dx[4], &sb, &cb);
    sincosf(dx[5], &sc, &cc);
  }
  // Rd = Rx(a)*Ry(b)*Rz(c) in closed form: the same products and sums as the 3x3 products
  // of src/defs.h:133 with their structural zeros and ones folded away (x*1 = x, x+0 = x).
  const float sasb = sa * sb, casb = ca * sb;
  Rd[0][0] = cb * cc;
  Rd[0][1] = -(cb * sc);
  Rd[0][2] = sb;
  Rd[1][0] = sasb * cc + ca * sc;
  Rd[1][1] = ca * cc - sasb * sc;
  Rd[1][2] = -(sa * cb);
  Rd[2][0] = sa * sc - casb * cc;
  Rd[2][1] = casb * sc + sa * cc;
  Rd[2][2] = ca * cb;
}

// src/defs.h:100-136 v2tEuler: R = Rx(a)*Ry(b)*Rz(c) (float), t = v[0:3]; then
// src/picp_solver.cpp:103 T <- v2tEuler(dx) * T.
__device__ __forceinline__ void apply_update(const float dx[6], float R[9], float t[3]) {
  // (round 4 pinned the contractions here with fp contract(off) for a fused append that is gone;
  // it cost C2/C3 1-2 % -- profiles/r05/ab_regress/ -- and parity does not depend on it)
  float Rd[3][3];
  update_rotation(dx, Rd);
  float Rn[9], tn[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      float s = Rd[i][0] * R[j * 3 + 0];
      s = s + Rd[i][1] * R[j * 3 + 1];
      s = s + Rd[i][2] * R[j * 3 + 2];
      Rn[j * 3 + i] = s;
    }
    float s = Rd[i][0] * t[0];
    s = s + Rd[i][1] * t[1];
    s = s + Rd[i][2] * t[2];
    tn[i] = s + dx[i];
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = Rn[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = tn[i];
}

// The 32 block-partial totals (double) -> the float words finish_round_f consumes, one word per
// total so lane e of a wave can convert total e: H entries with the damping added on the
// diagonal (src/picp_solver.cpp:96), -b, chi_in, chi_out as float, n_in and n_proj as int bits.
__device__ __forceinline__ float total_word(const PicpArgs& A, int e, double t) {
  const bool diag = (e == 0) | (e == 6) | (e == 11) | (e == 15) | (e == 18) | (e == 20);
  // straight-line selects (lane e converts total e: branches would serialise the wave)
  const double h = t + (diag ? (double)A.damping : 0.0);
  const double d = (e < PICP_P_B) ? h : ((e < PICP_P_CHI_IN) ? -t : t);
  const float f = (float)d;
  const float c = __int_as_float((int32_t)t);
  return (e < PICP_P_N_IN) ? f : ((e < 31) ? c : 0.0f);
}

// total_word for a lane that converts the same total e every round (the finishing wave of the
// persistent and block kernels): what depends on e only, computed once per launch (the
// persistent kernel keeps it in VGPRs, the block kernel in LDS), so the round pays one add, the
// two converts and four bit operations instead of the classification of e (compares, lane masks
// in SGPR pairs).  20 bytes, 24 with the double's alignment.
//   add   : (double)damping on the diagonal of H, +0.0 on the rest of H (total_word's t + 0.0),
//           -0.0 elsewhere (t + -0.0 is t for every t, -0.0 included)
//   sign  : the sign bit for -b.  Negating the float after the conversion gives the bits of
//           converting -t: round-to-nearest is symmetric
//   fmask / imask : all ones where the word is the float / the int conversion (both zero: word 31)
struct TotalLane {
  double add;
  unsigned sign, fmask, imask;
};

__device__ __forceinline__ TotalLane total_lane(const PicpArgs& A, int e) {
  const bool diag = (e == 0) | (e == 6) | (e == 11) | (e == 15) | (e == 18) | (e == 20);
  TotalLane k;
  k.add = diag ? (double)A.damping : ((e < PICP_P_B) ? 0.0 : -0.0);
  k.sign = (e >= PICP_P_B && e < PICP_P_CHI_IN) ? 0x80000000u : 0u;
  k.fmask = (e < PICP_P_N_IN) ? ~0u : 0u;
  k.imask = (e >= PICP_P_N_IN && e < 31) ? ~0u : 0u;
  // opaque from here: as plain selects of e the compiler turns the masks back into compares whose
  // lane masks it hoists into (spilled) SGPR pairs
  asm volatile("" : "+v"(k.add), "+v"(k.sign), "+v"(k.fmask), "+v"(k.imask));
  return k;
}

__device__ __forceinline__ float total_word(const TotalLane& k, double t) {
  const unsigned f = __float_as_uint((float)(t + k.add)) ^ k.sign;
  const unsigned c = (unsigned)(int32_t)t;
  return __uint_as_float((f & k.fmask) | (c & k.imask));
}

// What a round leaves besides the pose: the state fields no later round reads.
struct RoundOut {
  float chi_in, chi_out;
  int32_t n_in, n_proj, ok, done, converged;
};

// Finish round j of a problem from its converted totals (total_word: damping already in): the
// min-inlier check, the 6x6 solve, the update and the icp_test loop rule.  The loop state a round
// reads -- the pose R (column-major) / t and chi_prev -- is carried in registers by the finishing
// wave (every lane computes the same values; no LDS state round trip on the critical path).
// tw may be LDS.  (The elimination spread over a 16-lane row of the finishing wave was not
// faster: DESIGN.md Appendix A, "DPP-row solve".)
__device__ __forceinline__ void finish_round_pose(const PicpArgs& A, const float* tw, int j, float R[9],
                                                  float t[3], float& chi_prev, RoundOut& o) {
  o.chi_in = tw[PICP_P_CHI_IN];
  o.chi_out = tw[PICP_P_CHI_OUT];
  o.n_in = __float_as_int(tw[PICP_P_N_IN]);
  o.n_proj = __float_as_int(tw[PICP_P_N_PROJ]);
  o.converged = 0;  // a converged loop is done: no round runs after it
  if (o.n_in < A.min_inliers) {  // src/picp_solver.cpp:97-100
    o.ok = 0;
    o.done = 1;
    return;
  }
  float dx[6];
  ldl6_solve(tw, dx);  // :96 (damping folded in by total_word), :102
  apply_update(dx, R, t);  // :103
  o.ok = 1;
  o.done = 0;
  // exec/icp_test.cpp:99-106
  const float prev = chi_prev, cur = o.chi_in;
  const float rel = (prev > 1e-10f) ? fabsf(prev - cur) / prev : 0.0f;
  if (rel < A.conv_eps) {
    o.converged = 1;
    o.done = 1;
  } else {
    chi_prev = cur;
  }
  if (j >= A.max_rounds) o.done = 1;
}

// ---- the finish with the pose update spread over the lanes of the finishing wave ----
// Only word l of the new pose is needed in lane l (the publish and the control row are "lane l
// owns word l"), so after the uniform solve and rotation lane l < 12 computes word l alone instead
// of every lane computing all twelve.  With i = l % 3 and base = 3 (l / 3), words 0-8 being R
// column-major and 9-11 t, word l is row i of Rd times old[base .. base+2], plus dx[i] for t:
// one formula for both.  FinishLanes holds what depends on the lane only, made once per launch:
// the row masks (all ones where l % 3 == i, l < 12), the t mask (9 <= l < 12) and the word-12
// mask, as opaque VGPR values (as TotalLane: plain selects of the lane become compares whose lane
// masks are hoisted into SGPR pairs and spilled), and the LDS word index of old[0].
struct FinishLanes {
  unsigned row[3], tmask, m12;
  int base;
};

__device__ __forceinline__ FinishLanes finish_lanes(int lane) {
  FinishLanes k;
  const bool pose = lane < 12;
#pragma unroll
  for (int i = 0; i < 3; ++i) k.row[i] = (pose && lane % 3 == i) ? ~0u : 0u;
  k.tmask = (lane >= 9 && lane < 12) ? ~0u : 0u;
  k.m12 = (lane == 12) ? ~0u : 0u;
  k.base = pose ? 3 * (lane / 3) : 0;
  asm volatile("" : "+v"(k.row[0]), "+v"(k.row[1]), "+v"(k.row[2]), "+v"(k.tmask), "+v"(k.m12), "+v"(k.base));
  return k;
}

__device__ __forceinline__ float lanes_pick(const FinishLanes& k, float a0, float a1, float a2) {
  return __uint_as_float((__float_as_uint(a0) & k.row[0]) | (__float_as_uint(a1) & k.row[1]) |
                         (__float_as_uint(a2) & k.row[2]));
}

// finish_round_pose for a whole wave: the same RoundOut and chi_prev in every lane, and the
// return value is word l of the new pose in lane l < 12 (unspecified in the other lanes).  pose:
// the twelve words of the old pose (LDS or global), read per lane before the solve.  The
// convergence quotient (an IEEE division that feeds only the done word) is computed ahead of the
// solve, unconditionally: prev <= 1e-10 selects 0 whatever the quotient is, so the same bits as
// the branch of finish_round_pose.
// The three products of a word are summed as apply_update's are where the pose is live in
// registers (the round kernel, the persistent kernel with one item per lane), a contraction that
// was the compiler's choice and is not the same for every row of Rd: rows 1 and 2 are
// fma(Rdi2, o2, fma(Rdi0, o0, Rdi1 * o1)), and row 0, whose Rd01 is a negated product, is
// fma(Rd02, o2, fma(Rd01, o1, Rd00 * o0)); t adds dx separately.  Here it is written out (fp
// contract off) and no longer rests on the compiler: each lane multiplies its "first" pair, then
// fuses the "second" and the third.  (Where the pose is re-read from LDS, the persistent kernel
// with two or more items per lane, the compiler sums row 0 as the other rows; those kernels keep
// the uniform form and their bits.)  t's add is selected, not masked to an add of zero, which
// would turn a -0 word of R into +0.
__device__ __forceinline__ float finish_round_lanes(const PicpArgs& A, const float* tw, const float* pose, int j,
                                                    const FinishLanes& k, float& chi_prev, RoundOut& o) {
#pragma clang fp contract(off)
  const float old0 = pose[k.base], old1 = pose[k.base + 1], old2 = pose[k.base + 2];
  o.chi_in = tw[PICP_P_CHI_IN];
  o.chi_out = tw[PICP_P_CHI_OUT];
  o.n_in = __float_as_int(tw[PICP_P_N_IN]);
  o.n_proj = __float_as_int(tw[PICP_P_N_PROJ]);
  o.converged = 0;
  if (o.n_in < A.min_inliers) {  // the pose stays: lane l's own old word
    o.ok = 0;
    o.done = 1;
    return lanes_pick(k, old0, old1, old2);
  }
  // exec/icp_test.cpp:99-106, the quotient first
  const float prev = chi_prev, cur = o.chi_in;
  float quot = fabsf(prev - cur) / prev;
  asm volatile("" : "+v"(quot));  // computed here, not sunk under a branch behind the solve
  const float rel = (prev > 1e-10f) ? quot : 0.0f;
  const bool conv = rel < A.conv_eps;
  float dx[6];
  ldl6_solve(tw, dx);
  float Rd[3][3];
  update_rotation<true>(dx, Rd);
  // rows 1, 2: (Rdi1, old1) first, (Rdi0, old0) second; row 0 the other way round
  const unsigned u0 = __float_as_uint(old0), u1 = __float_as_uint(old1), r0 = k.row[0];
  const float of = __uint_as_float((u0 & r0) | (u1 & ~r0)), os = __uint_as_float((u1 & r0) | (u0 & ~r0));
  float s = lanes_pick(k, Rd[0][0], Rd[1][1], Rd[2][1]) * of;
  s = fmaf(lanes_pick(k, Rd[0][1], Rd[1][0], Rd[2][0]), os, s);
  s = fmaf(lanes_pick(k, Rd[0][2], Rd[1][2], Rd[2][2]), old2, s);
  // t: dx + s with dx as the first operand, as the uniform form compiles: where both are NaN the
  // add returns the first one's sign, and the compiler commutes a plain + (inline assembly: the
  // operand order is part of the result here)
  float st;
  asm("v_add_f32_e32 %0, %1, %2" : "=v"(st) : "v"(lanes_pick(k, dx[0], dx[1], dx[2])), "v"(s));
  const float w = __uint_as_float((__float_as_uint(st) & k.tmask) | (__float_as_uint(s) & ~k.tmask));
  o.ok = 1;
  o.converged = conv ? 1 : 0;
  o.done = (conv || j >= A.max_rounds) ? 1 : 0;
  chi_prev = conv ? prev : cur;
  return w;
}

// The 128-byte state after round j, written field by field (padding zeroed): a whole-struct copy
// from a local goes through a scratch alloca (SROA cannot split the memcpy).  dst: LDS or global.
// store_state_rest: everything but the pose (finish_round_lanes has the pose one word per lane).
template <typename S>
__device__ __forceinline__ void store_state_rest(S* dst, float chi_prev, const RoundOut& o, int j) {
  dst->chi_prev = chi_prev;
  dst->chi_in = o.chi_in;
  dst->chi_out = o.chi_out;
  dst->n_in = o.n_in;
  dst->n_proj = o.n_proj;
  dst->rounds = j;
  dst->done = o.done;
  dst->ok = o.ok;
  dst->converged = o.converged;
#pragma unroll
  for (int i = 0; i < 11; ++i) dst->pad[i] = 0;
}

template <typename S>
__device__ __forceinline__ void store_state(S* dst, const float R[9], const float t[3], float chi_prev,
                                            const RoundOut& o, int j) {
#pragma unroll
  for (int i = 0; i < 9; ++i) dst->R[i] = R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) dst->t[i] = t[i];
  store_state_rest(dst, chi_prev, o, j);
}

// finish_round_pose on a stored state (the multi-launch round kernel: one lane).
__device__ __forceinline__ void finish_round_f(const PicpArgs& A, const PicpState& s,
                                               const float* tw, int j, PicpState& ns) {
  float R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = s.R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = s.t[i];
  float chi_prev = s.chi_prev;
  RoundOut o;
  finish_round_pose(A, tw, j, R, t, chi_prev, o);
  store_state(&ns, R, t, chi_prev, o, j);
}

// Finish round (j-1) of a problem from its block-partial totals (double): H, b, stats -> new
// state.  One lane.
__device__ __forceinline__ void finish_round(const PicpArgs& A, const PicpState& s,
                                             const double* tot, int j, PicpState& ns) {
  float tw[PICP_NPART];
#pragma unroll
  for (int e = 0; e < PICP_NPART; ++e) tw[e] = total_word(A, e, tot[e]);
  finish_round_f(A, s, tw, j, ns);
}

}  // namespace picp
