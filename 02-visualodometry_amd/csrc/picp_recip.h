// picp_recip.h -- refined hardware reciprocals: the correctly rounded float 1/x of the projection
// (rcp_rn, rcp_safe), the LDL^T pivot reciprocal (rcp32), and the double reciprocal and reciprocal
// square root of the triangulation and the point refiner (rcp_f64, rsq_f64).
#pragma once
#include <hip/hip_runtime.h>

#include <float.h>

namespace picp {

// Correctly rounded 1/x in 3 instructions: v_rcp_f32 (about 1 ulp) and one FMA Newton step.
// Verified bit-identical to the IEEE division 1.0f/x for EVERY float x in [2^-8, 2^8) by
// picp_selftest_rcp (tests/test_gpu_parity.py); both operations are exact under power-of-two
// scaling inside the normal range, so that covers every x with 2^-100 <= |x| <= 2^100
// (rcp_safe).  Outside it (and for 0, inf, NaN) callers use the IEEE division.
__device__ __forceinline__ float rcp_rn(float x) {
  const float r = __builtin_amdgcn_rcpf(x);
  const float e = fmaf(-x, r, 1.0f);
  return fmaf(e, r, r);
}

__device__ __forceinline__ bool rcp_safe(float x) {
  const float a = fabsf(x);
  return (a >= 7.8886091e-31f) & (a <= 1.2676506e30f);  // [2^-100, 2^100]; NaN -> false
}

// 1/d in float: hardware v_rcp_f32 estimate refined by one Newton step (<= 1 ulp for normal
// d); |d| <= FLT_MIN -> 0 (Eigen's LDLT zero-pivot rule for float, src/picp_solver.cpp:102).
__device__ __forceinline__ float rcp32(float d) {
  float r = __builtin_amdgcn_rcpf(d);
  r = fmaf(r, fmaf(-d, r, 1.0f), r);
  return (fabsf(d) > FLT_MIN) ? r : 0.0f;
}

// Refined hardware reciprocal and reciprocal square root in double: the v_rcp_f64 / v_rsq_f64
// estimate and two Newton steps (full double precision), half the dependency chain of the IEEE
// division / sqrt sequences.
__device__ __forceinline__ double rcp_f64(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(r, fma(-x, r, 1.0), r);
  return fma(r, fma(-x, r, 1.0), r);
}
__device__ __forceinline__ double rsq_f64(double x) {
  double y = __builtin_amdgcn_rsq(x);
  y = fma(0.5 * y, fma(-x * y, y, 1.0), y);
  return fma(0.5 * y, fma(-x * y, y, 1.0), y);
}

}  // namespace picp
