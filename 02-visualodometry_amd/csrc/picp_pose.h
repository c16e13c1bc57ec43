// picp_pose.h -- the layouts of a pose and of the camera matrix, and every conversion between
// them, written once.  A world-in-camera pose (R, t) is kept in five layouts:
//   PicpState      : R[9] column-major, then t[3] (picp_internal.h; the solvers' state)
//   4x4            : column-major float[16], (R | t) over (0 0 0 1) (the C-ABI's poses)
//   RefinePose     : three float4 rows of [R | t] (picp_internal.h; the refiner's 48-B table)
//   Pose           : the per-item math's register struct, below
//   s_pose         : 12 floats of LDS, R[9] column-major then t[3] (persistent and block kernels)
// K is column-major float[9] everywhere but in Cam.  Host code includes this header too.
#pragma once
#include <hip/hip_runtime.h>

#include "picp_internal.h"

#pragma GCC visibility push(hidden)  // the host's out-of-line copies are not exports of the library

namespace picp {

struct Pose {
  float r00, r01, r02, r10, r11, r12, r20, r21, r22;
  float t0, t1, t2;
};

struct Cam {
  float k00, k01, k02, k10, k11, k12, k20, k21, k22;
  float maxx, maxy;  // cols-1, rows-1 (src/camera.h:31,33)
};

// PicpState <-> column-major 4x4 (the state's other fields are left alone)
__host__ __device__ inline void pose_to_state(const float T[16], PicpState& s) {
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i) s.R[j * 3 + i] = T[j * 4 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) s.t[i] = T[12 + i];
}

__host__ __device__ inline void state_to_pose(const PicpState& s, float T[16]) {
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i) T[j * 4 + i] = s.R[j * 3 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) T[12 + i] = s.t[i];
  T[3] = T[7] = T[11] = 0.0f;
  T[15] = 1.0f;
}

// PicpState <-> RefinePose rows
__host__ __device__ inline RefinePose state_to_rows(const PicpState& s) {
  RefinePose P;
  P.r0 = make_float4(s.R[0], s.R[3], s.R[6], s.t[0]);
  P.r1 = make_float4(s.R[1], s.R[4], s.R[7], s.t[1]);
  P.r2 = make_float4(s.R[2], s.R[5], s.R[8], s.t[2]);
  return P;
}

__host__ __device__ inline void rows_to_state(const RefinePose& P, PicpState& s) {
  s.R[0] = P.r0.x; s.R[3] = P.r0.y; s.R[6] = P.r0.z; s.t[0] = P.r0.w;
  s.R[1] = P.r1.x; s.R[4] = P.r1.y; s.R[7] = P.r1.z; s.t[1] = P.r1.w;
  s.R[2] = P.r2.x; s.R[5] = P.r2.y; s.R[8] = P.r2.z; s.t[2] = P.r2.w;
}

// column-major 4x4 -> RefinePose rows
__host__ __device__ inline RefinePose pose_to_rows(const float T[16]) {
  RefinePose P;
  P.r0 = make_float4(T[0], T[4], T[8], T[12]);
  P.r1 = make_float4(T[1], T[5], T[9], T[13]);
  P.r2 = make_float4(T[2], T[6], T[10], T[14]);
  return P;
}

// Pose from R (column-major) and t: a PicpState's fields, or s_pose and s_pose + 9
__device__ __forceinline__ void pose_load(const float* R, const float* t, Pose& T) {
  T.r00 = R[0]; T.r10 = R[1]; T.r20 = R[2];
  T.r01 = R[3]; T.r11 = R[4]; T.r21 = R[5];
  T.r02 = R[6]; T.r12 = R[7]; T.r22 = R[8];
  T.t0 = t[0]; T.t1 = t[1]; T.t2 = t[2];
}

__device__ __forceinline__ void pose_load(const RefinePose& P, Pose& T) {
  T.r00 = P.r0.x; T.r01 = P.r0.y; T.r02 = P.r0.z; T.t0 = P.r0.w;
  T.r10 = P.r1.x; T.r11 = P.r1.y; T.r12 = P.r1.z; T.t1 = P.r1.w;
  T.r20 = P.r2.x; T.r21 = P.r2.y; T.r22 = P.r2.z; T.t2 = P.r2.w;
}

// Cam from the column-major K and the image bounds (cols-1, rows-1)
__device__ __forceinline__ void cam_load(const float K[9], float maxx, float maxy, Cam& C) {
  C.k00 = K[0]; C.k10 = K[1]; C.k20 = K[2];
  C.k01 = K[3]; C.k11 = K[4]; C.k21 = K[5];
  C.k02 = K[6]; C.k12 = K[7]; C.k22 = K[8];
  C.maxx = maxx;
  C.maxy = maxy;
}

// Eigen::Isometry3f::inverse() of a column-major 4x4 (oracle/picp_oracle.c or_iso_inverse order)
__device__ __forceinline__ void vo_iso_inverse(const float* T, float* Ti) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Ti[j * 4 + i] = T[i * 4 + j];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float s = Ti[0 * 4 + i] * T[12 + 0];
    s = s + Ti[1 * 4 + i] * T[12 + 1];
    s = s + Ti[2 * 4 + i] * T[12 + 2];
    Ti[12 + i] = -s;
  }
  Ti[3] = Ti[7] = Ti[11] = 0.0f;
  Ti[15] = 1.0f;
}

// P = K * inverse(T_cw)(0:3, 0:4), row-major 3x4 (src/cam.cpp:109-112)
__device__ __forceinline__ void vo_projection(const float* K, const float* Tcw, float* P) {
#pragma clang fp contract(off)
  float Ti[16];
  vo_iso_inverse(Tcw, Ti);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float s = K[0 * 3 + i] * Ti[j * 4 + 0];
      s = s + K[1 * 3 + i] * Ti[j * 4 + 1];
      s = s + K[2 * 3 + i] * Ti[j * 4 + 2];
      P[i * 4 + j] = s;
    }
}

}  // namespace picp

#pragma GCC visibility pop
