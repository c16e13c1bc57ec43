// picp_pnp.hip -- absolute pose without a prior: P3P inside RANSAC for a ragged batch of 2D-3D
// problems, scored with PICP's own gate (classify_item) and meant to be polished by PICP itself
// (DESIGN.md §4.12).  Four launches; what the Sim(3) solver has too is in picp_ransac.h:
//   1. picp_ransac_samples_kernel (picp_ransac.hip): three distinct indices per (problem, hypothesis);
//   2. picp_pnp_solve_kernel    one lane per (problem, hypothesis), in double with contraction off:
//                               Grunert's quartic (picp_p3p.h), up to four float32 world-in-camera poses;
//   3. picp_pnp_score_kernel    the hot path: a block keeps up to PNP_TILE correspondences of one
//                               problem in registers and loops over the problem's poses (each one
//                               wave-uniform: scalar loads); counts are ballots and scalar popcounts,
//                               gathered per 64 hypotheses in LDS and added to the [hyp x root]
//                               table with integer atomics (order-free);
//   4. picp_pnp_select_kernel   one block per problem: the largest count, then the lowest
//                               hypothesis, then the lowest root; the mask at the winner.
// No block waits for another.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "picp_internal.h"
#include "picp_item.h"
#include "picp_launch.h"
#include "picp_p3p.h"
#include "picp_pose.h"
#include "picp_ransac.h"
#include "picp_variant.h"

#pragma clang fp contract(off)

#define PNP_BS 256
#define PNP_NPT 4
#define PNP_TILE (PNP_BS * PNP_NPT)  // correspondences a score block keeps in registers
#define PNP_HT 64                    // hypotheses per LDS count tile: PNP_HT * 4 roots == PNP_BS

namespace {

using picp::Cam;
using picp::Pose;

// whether correspondence j (< n) of the problem at element b is an inlier of pose T
template <bool PIN>
__device__ __forceinline__ bool pnp_inlier(const Pose& T, const Cam& C, float thr, float x, float y, float z, float u,
                                           float v) {
  float chi, iu, iv;
  return picp::classify_item(T, C, thr, PIN, x, y, z, u, v, &chi, &iu, &iv) == PICP_CORR_INLIER;
}

}  // namespace

// 2. the poses of (problem, hypothesis) g
extern "C" __global__ __launch_bounds__(64) void picp_pnp_solve_kernel(PnpArgs A, PnpItems I,
                                                                       const int32_t* __restrict__ samples,
                                                                       int32_t* __restrict__ n_roots,
                                                                       float* __restrict__ hyp_T) {
  const int64_t g = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (g >= (int64_t)A.n_problems * A.hyp) return;
  const int p = (int)(g / A.hyp);
  const int64_t n = I.offs[p + 1] - I.offs[p], b = I.base[p];
  float* out = hyp_T + (size_t)g * 4 * PNP_POSE;
  for (int k = 0; k < 4 * PNP_POSE; ++k) out[k] = 0.0f;
  if (n < 4) {
    n_roots[g] = 0;
    return;
  }
  double P[3][3], px[3][2];
  for (int k = 0; k < 3; ++k) {
    const int64_t j = b + samples[3 * g + k];
    P[k][0] = (double)I.x[j * I.sx];
    P[k][1] = (double)I.y[j * I.sx];
    P[k][2] = (double)I.z[j * I.sx];
    px[k][0] = (double)I.u[j * I.su];
    px[k][1] = (double)I.v[j * I.su];
  }
  n_roots[g] = p3p_grunert(P, px, A.Kinv, A.K, out);
}

// 3. the inlier counts.  Block blockIdx.x holds correspondences [first, first + PNP_TILE) of
// problem blk[blockIdx.x].x; slice blockIdx.y of gridDim.y takes every gridDim.y-th tile of
// PNP_HT hypotheses.  cnt ([hyp x 4] per problem) is zeroed by the caller.
template <bool PIN>
__device__ __forceinline__ void pnp_score(const PnpArgs& A, const PnpItems& I, const int2* __restrict__ blk,
                                          const int32_t* __restrict__ n_roots, const float* __restrict__ hyp_T,
                                          int32_t* __restrict__ cnt, int* s_cnt) {
  const int tid = threadIdx.x;
  const int2 bi = blk[blockIdx.x];
  const int p = bi.x, first = bi.y;
  const int n = (int)(I.offs[p + 1] - I.offs[p]);
  const int64_t b = I.base[p];
  Cam C;
  picp::cam_load(A.K, A.maxx, A.maxy, C);
  float x[PNP_NPT], y[PNP_NPT], z[PNP_NPT], u[PNP_NPT], v[PNP_NPT];
  bool in[PNP_NPT];
#pragma unroll
  for (int k = 0; k < PNP_NPT; ++k) {
    const int64_t j = (int64_t)first + k * PNP_BS + tid;  // n may be INT32_MAX
    in[k] = j < n;
    const int64_t e = b + (in[k] ? j : first);  // a lane past the end re-reads a valid item, masked below
    x[k] = I.x[e * I.sx];
    y[k] = I.y[e * I.sx];
    z[k] = I.z[e * I.sx];
    u[k] = I.u[e * I.su];
    v[k] = I.v[e * I.su];
  }
  const size_t ph0 = (size_t)p * A.hyp;
  for (int h0 = blockIdx.y * PNP_HT; h0 < A.hyp; h0 += gridDim.y * PNP_HT) {
    s_cnt[tid] = 0;
    __syncthreads();
    const int h1 = (h0 + PNP_HT < A.hyp) ? h0 + PNP_HT : A.hyp;
    for (int h = h0; h < h1; ++h) {
      const int nr = n_roots[ph0 + h];  // wave-uniform: scalar loads, as the pose below
      for (int r = 0; r < nr; ++r) {
        const float* Tp = hyp_T + ((ph0 + h) * 4 + r) * PNP_POSE;
        Pose T;
        picp::pose_load(Tp, Tp + 9, T);
        unsigned c = 0;
#pragma unroll
        for (int k = 0; k < PNP_NPT; ++k) {
          const bool inl = in[k] & pnp_inlier<PIN>(T, C, A.threshold, x[k], y[k], z[k], u[k], v[k]);
          c += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(inl));
        }
        if ((tid & 63) == 0 && c) atomicAdd(&s_cnt[(h - h0) * 4 + r], (int)c);
      }
    }
    __syncthreads();
    const int mine = s_cnt[tid];  // entry (h0 + tid / 4, root tid % 4)
    if (mine) atomicAdd(&cnt[(ph0 + h0) * 4 + tid], mine);
    __syncthreads();
  }
}

extern "C" __global__ __launch_bounds__(PNP_BS) void picp_pnp_score_kernel(PnpArgs A, PnpItems I,
                                                                           const int2* __restrict__ blk,
                                                                           const int32_t* __restrict__ n_roots,
                                                                           const float* __restrict__ hyp_T,
                                                                           int32_t* __restrict__ cnt) {
  __shared__ int s_cnt[PNP_HT * 4];  // counts of one tile of hypotheses, entry 4 (h - h0) + root
  if (A.pinhole)
    pnp_score<true>(A, I, blk, n_roots, hyp_T, cnt, s_cnt);
  else
    pnp_score<false>(A, I, blk, n_roots, hyp_T, cnt, s_cnt);
}

// 4. the winner of problem blockIdx.x and the mask at it
extern "C" __global__ __launch_bounds__(PNP_BS) void picp_pnp_select_kernel(
    PnpArgs A, PnpItems I, const int32_t* __restrict__ n_roots, const float* __restrict__ hyp_T,
    const int32_t* __restrict__ cnt, float* __restrict__ T_out, int32_t* __restrict__ inliers,
    int32_t* __restrict__ found, uint8_t* __restrict__ mask) {
  __shared__ unsigned long long s_key[PNP_BS / 64];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n = (int)(I.offs[p + 1] - I.offs[p]);
  const size_t ph0 = (size_t)p * A.hyp;
  // entry e = 4 h + r is valid when r < n_roots[h]
  const unsigned long long key = picp::block_winner<PNP_BS>(A.hyp * 4, cnt + ph0 * 4, s_key, [&](int e) {
    return (e & 3) < n_roots[ph0 + (e >> 2)];
  });
  const int best = picp::winner_count(key);
  const bool ok = key != 0 && n >= 4 && best >= A.min_inliers;
  const float* Tp = hyp_T + (ph0 * 4 + picp::winner_entry(key)) * PNP_POSE;  // read only when ok
  if (tid < 16) {
    float val = (tid % 5 == 0) ? 1.0f : 0.0f;  // the identity, and the bottom row of a pose
    const int r = tid & 3, c = tid >> 2;
    if (ok && r < 3) val = (c < 3) ? Tp[3 * c + r] : Tp[9 + r];
    T_out[16 * (size_t)p + tid] = val;
  }
  if (tid == 0) {
    inliers[p] = best;
    found[p] = ok ? 1 : 0;
  }
  if (!mask) return;
  const int64_t b = I.base[p], o = I.offs[p];
  if (!ok) {
    for (int j = tid; j < n; j += PNP_BS) mask[o + j] = 0;
    return;
  }
  Pose T;
  picp::pose_load(Tp, Tp + 9, T);
  Cam C;
  picp::cam_load(A.K, A.maxx, A.maxy, C);
  for (int j = tid; j < n; j += PNP_BS) {
    const int64_t e = b + j;
    const float x = I.x[e * I.sx], y = I.y[e * I.sx], z = I.z[e * I.sx], u = I.u[e * I.su], v = I.v[e * I.su];
    const bool inl = A.pinhole ? pnp_inlier<true>(T, C, A.threshold, x, y, z, u, v)
                               : pnp_inlier<false>(T, C, A.threshold, x, y, z, u, v);
    mask[o + j] = inl ? 1 : 0;
  }
}

// ------------------------------- host launch wrappers -------------------------------
// Every per-(problem, hypothesis) array is indexed p * hyp + h; problems sit on grid x.
extern "C" int picp_pnp_score_tile(void) { return PNP_TILE; }
extern "C" int picp_pnp_hyp_tile(void) { return PNP_HT; }

extern "C" hipError_t picp_launch_pnp_solve(hipStream_t stream, const PnpArgs* A, const PnpItems* I,
                                            const int32_t* samples, int32_t* n_roots, float* hyp_T) {
  const int64_t g = (int64_t)A->n_problems * A->hyp;
  hipLaunchKernelGGL(picp_pnp_solve_kernel, dim3((unsigned)((g + 63) / 64)), dim3(64), 0, stream, *A, *I, samples,
                     n_roots, hyp_T);
  return hipGetLastError();
}

extern "C" hipError_t picp_launch_pnp_score(hipStream_t stream, const PnpArgs* A, const PnpItems* I, int nb,
                                            const int2* blk, int hsplit, const int32_t* n_roots, const float* hyp_T,
                                            int32_t* cnt) {
  if (nb <= 0) return hipSuccess;  // no problem has a correspondence
  PnpArgs a = *A;
  a.pinhole = picp_use_pinhole(a.K) ? 1 : 0;  // the camera path the classify pass takes
  hipLaunchKernelGGL(picp_pnp_score_kernel, dim3((unsigned)nb, (unsigned)hsplit), dim3(PNP_BS), 0, stream, a, *I, blk,
                     n_roots, hyp_T, cnt);
  return hipGetLastError();
}

extern "C" hipError_t picp_launch_pnp_select(hipStream_t stream, const PnpArgs* A, const PnpItems* I,
                                             const int32_t* n_roots, const float* hyp_T, const int32_t* cnt,
                                             float* T_out, int32_t* inliers, int32_t* found, uint8_t* mask) {
  PnpArgs a = *A;
  a.pinhole = picp_use_pinhole(a.K) ? 1 : 0;
  hipLaunchKernelGGL(picp_pnp_select_kernel, dim3((unsigned)A->n_problems), dim3(PNP_BS), 0, stream, a, *I, n_roots,
                     hyp_T, cnt, T_out, inliers, found, mask);
  return hipGetLastError();
}
