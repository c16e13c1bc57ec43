// picp_adjust.hip -- what connects the point refiner (picp_refine.hip) and the PICP batch solve on
// the device for the alternating adjustment (include/picp_c.h picp_refine_run_poses,
// picp_refine_adjust).  Neither solver's kernels are here: these kernels only move
// data between them.
//
// The pose-major view of the point-major tracks (built once per track set):
//   adj_count_kernel  : thread per point: its observations counted per pose (integer atomics: no order).
//   adj_scan_kernel   : one block: exclusive scan of the counts -> pose_off (int64).
//   adj_fill_kernel   : thread per point: (source position, point) of every observation, at atomic
//                       cursors inside its pose's list ...
//   adj_rank_kernel   : ... and a block per pose ranks every entry by counting the smaller source
//                       positions of its list (staged through LDS in tiles of AJ_TILE, any length) and
//                       scatters it to base + rank.  Positions are distinct, so the ranks are a
//                       permutation and the order the atomics gave does not survive: pose k's list is
//                       ascending in source position (ascending point, then place in the track).
// The pose step around the batch's solve:
//   adj_gather_kernel : block per problem (movable pose): X, Y, Z of the list's current points (and,
//                       once per view, U, V) straight into the batch's SoA planes at plane_off[p];
//                       thread 0 writes the problem's initial state from the refiner's pose row.
//   adj_writeback_kernel : thread per problem: the solved pose into the refiner's 48-B row and the
//                       4x4 table unless an entry is not finite; the pose's picp_stats.
// The sweep record:
//   adj_sums_kernel   : one block, a fixed strided order per thread and a fixed LDS tree: the sums of
//                       chi_in (double), n_in and ok (int64) of the point and the pose stats.
#include <float.h>

#include "picp_c.h"
#include "picp_launch.h"
#include "picp_pose.h"
#include "picp_wave.h"

using namespace picp;

#define AJ_BLOCK 256
#define AJ_SCAN 1024
#define AJ_SCAN_WAVES (AJ_SCAN / 64)
#define AJ_TILE 1024                   // source positions staged per LDS tile of the rank kernel
#define AJ_EPT (AJ_TILE / AJ_BLOCK)    // entries a thread ranks at once

extern "C" int picp_adjust_rank_tile(void) { return AJ_TILE; }

__global__ __launch_bounds__(AJ_BLOCK) void adj_count_kernel(const AdjView v) {
  const int64_t p = (int64_t)blockIdx.x * AJ_BLOCK + threadIdx.x;
  if (p >= v.n_points) return;
  const int64_t b = v.track_off[p], e = v.track_off[p + 1];
  for (int64_t k = b; k < e; ++k) atomicAdd(v.cnt + v.obs_pose[k], 1);
}

__global__ __launch_bounds__(AJ_SCAN) void adj_scan_kernel(const AdjView v) {
  __shared__ int s_w[AJ_SCAN_WAVES];
  int64_t carry = 0;
  for (int64_t c0 = 0; c0 < v.n_poses; c0 += AJ_SCAN) {  // uniform
    const int64_t j = c0 + threadIdx.x;
    const int c = j < v.n_poses ? v.cnt[j] : 0;
    int tot;
    const int excl = block_scan<AJ_SCAN_WAVES>(c, s_w, &tot);
    if (j < v.n_poses) {
      v.pose_off[j] = carry + excl;
      v.cnt[j] = 0;  // the fill's cursor
    }
    carry += tot;
    __syncthreads();  // s_w is reused by the next chunk
  }
  if (threadIdx.x == 0) v.pose_off[v.n_poses] = carry;
}

__global__ __launch_bounds__(AJ_BLOCK) void adj_fill_kernel(const AdjView v) {
  const int64_t p = (int64_t)blockIdx.x * AJ_BLOCK + threadIdx.x;
  if (p >= v.n_points) return;
  const int64_t b = v.track_off[p], e = v.track_off[p + 1];
  for (int64_t k = b; k < e; ++k) {
    const int32_t q = v.obs_pose[k];
    const int64_t o = v.pose_off[q] + atomicAdd(v.cnt + q, 1);
    v.tmp[o] = make_int2((int)k, (int)p);
  }
}

__global__ __launch_bounds__(AJ_BLOCK) void adj_rank_kernel(const AdjView v) {
  __shared__ int s_key[AJ_TILE];
  const int64_t base = v.pose_off[blockIdx.x];
  const int64_t len = v.pose_off[blockIdx.x + 1] - base;
  for (int64_t i0 = 0; i0 < len; i0 += AJ_TILE) {  // uniform: AJ_TILE entries ranked per pass
    int2 mine[AJ_EPT];
    int rank[AJ_EPT];
#pragma unroll
    for (int q = 0; q < AJ_EPT; ++q) {
      const int64_t i = i0 + q * AJ_BLOCK + threadIdx.x;
      mine[q] = i < len ? v.tmp[base + i] : make_int2(0, 0);
      rank[q] = 0;
    }
    for (int64_t t0 = 0; t0 < len; t0 += AJ_TILE) {  // uniform
      const int nt = (int)min((int64_t)AJ_TILE, len - t0);
      __syncthreads();  // the previous tile has been read
      for (int j = threadIdx.x; j < nt; j += AJ_BLOCK) s_key[j] = v.tmp[base + t0 + j].x;
      __syncthreads();
      for (int j = 0; j < nt; ++j) {
        const int key = s_key[j];  // the same address in every lane: a broadcast
#pragma unroll
        for (int q = 0; q < AJ_EPT; ++q) rank[q] += key < mine[q].x ? 1 : 0;
      }
    }
#pragma unroll
    for (int q = 0; q < AJ_EPT; ++q) {
      const int64_t i = i0 + q * AJ_BLOCK + threadIdx.x;
      if (i < len) {  // rank < len: fewer than len positions are smaller
        v.view_point[base + rank[q]] = mine[q].y;
        v.view_uv[base + rank[q]] = v.obs_uv[mine[q].x];
      }
    }
  }
}

__global__ __launch_bounds__(AJ_BLOCK) void adj_gather_kernel(const AdjPose g, int write_uv) {
  const int p = (int)blockIdx.x;
  const int32_t k = g.movable[p];
  const int64_t base = g.pose_off[k], len = g.pose_off[k + 1] - base;
  const int64_t dst = g.plane_off[p];
  for (int64_t i = threadIdx.x; i < len; i += AJ_BLOCK) {
    const int64_t j = g.view_point[base + i];
    g.X[dst + i] = g.xyz[3 * j + 0];
    g.Y[dst + i] = g.xyz[3 * j + 1];
    g.Z[dst + i] = g.xyz[3 * j + 2];
    if (write_uv) {
      const float2 z = g.view_uv[base + i];
      g.U[dst + i] = z.x;
      g.V[dst + i] = z.y;
    }
  }
  if (threadIdx.x == 0) {
    // the state picp_batch_set_poses leaves: the pose, and the loop state at entry
    PicpState s = {};
    rows_to_state(g.rposes[k], s);
    s.chi_prev = FLT_MAX;
    s.ok = 1;
    g.init[p] = s;
  }
}

__global__ __launch_bounds__(AJ_BLOCK) void adj_writeback_kernel(const AdjPose g, const PicpState* __restrict__ st) {
  const int p = (int)(blockIdx.x * AJ_BLOCK + threadIdx.x);
  if (p >= g.n_problems) return;
  const int32_t k = g.movable[p];
  const PicpState s = st[p];
  bool finite = true;
#pragma unroll
  for (int q = 0; q < 9; ++q) finite &= isfinite(s.R[q]);
#pragma unroll
  for (int q = 0; q < 3; ++q) finite &= isfinite(s.t[q]);
  picp_stats o;
  o.chi_in = s.chi_in;
  o.chi_out = s.chi_out;
  o.n_in = s.n_in;
  o.ok = finite ? s.ok : 0;
  o.rounds = s.rounds;
  o.converged = s.converged;
  o.n_projected = s.n_proj;
  o.reserved = 0;
  g.pose_stats[k] = o;
  if (!finite) return;  // the pose keeps its value
  g.rposes[k] = state_to_rows(s);
  state_to_pose(s, g.T + 16 * (int64_t)k);
}

// thread t adds items t, t + AJ_SCAN, ... in that order; then a fixed binary tree over the threads
__device__ __forceinline__ void adj_sum3(const picp_stats* __restrict__ st, int64_t n, double* s_d, long long* s_n,
                                         long long* s_k, double* chi, int64_t* n_in, int64_t* ok) {
  double c = 0.0;
  long long ni = 0, nk = 0;
  for (int64_t i = threadIdx.x; i < n; i += AJ_SCAN) {
    const picp_stats s = st[i];
    c += (double)s.chi_in;
    ni += s.n_in;
    nk += s.ok;
  }
  s_d[threadIdx.x] = c;
  s_n[threadIdx.x] = ni;
  s_k[threadIdx.x] = nk;
  __syncthreads();
  for (int h = AJ_SCAN / 2; h >= 1; h /= 2) {  // uniform
    if ((int)threadIdx.x < h) {
      s_d[threadIdx.x] += s_d[threadIdx.x + h];
      s_n[threadIdx.x] += s_n[threadIdx.x + h];
      s_k[threadIdx.x] += s_k[threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *chi = s_d[0];
    *n_in = s_n[0];
    *ok = s_k[0];
  }
  __syncthreads();  // the arrays are reused by the next call
}

__global__ __launch_bounds__(AJ_SCAN) void adj_sums_kernel(const picp_stats* __restrict__ pt, int64_t n_points,
                                                           const picp_stats* __restrict__ ps, int64_t n_poses,
                                                           picp_adjust_sweep* out) {
  __shared__ double s_d[AJ_SCAN];
  __shared__ long long s_n[AJ_SCAN];
  __shared__ long long s_k[AJ_SCAN];
  adj_sum3(pt, n_points, s_d, s_n, s_k, &out->chi_in_points, &out->n_in_points, &out->ok_points);
  adj_sum3(ps, n_poses, s_d, s_n, s_k, &out->chi_in_poses, &out->n_in_poses, &out->ok_poses);
}

static bool adj_view_ok(const AdjView* v) {
  return v && v->n_points >= 0 && v->n_points <= INT32_MAX && v->n_poses >= 0 && v->n_obs >= 0 &&
         v->n_obs <= INT32_MAX && v->track_off && v->cnt && v->pose_off &&
         (v->n_obs == 0 || (v->obs_pose && v->obs_uv && v->tmp && v->view_point && v->view_uv));
}

// the whole view build (cnt zeroed by the caller); n_poses == 0 writes pose_off[0] = 0 only
extern "C" hipError_t picp_launch_adjust_view(hipStream_t stream, const AdjView* v) {
  if (!adj_view_ok(v)) return hipErrorInvalidValue;
  const unsigned gp = (unsigned)((v->n_points + AJ_BLOCK - 1) / AJ_BLOCK);
  if (v->n_obs > 0) hipLaunchKernelGGL(adj_count_kernel, dim3(gp), dim3(AJ_BLOCK), 0, stream, *v);
  hipLaunchKernelGGL(adj_scan_kernel, dim3(1), dim3(AJ_SCAN), 0, stream, *v);
  if (v->n_obs > 0) {
    hipLaunchKernelGGL(adj_fill_kernel, dim3(gp), dim3(AJ_BLOCK), 0, stream, *v);
    hipLaunchKernelGGL(adj_rank_kernel, dim3((unsigned)v->n_poses), dim3(AJ_BLOCK), 0, stream, *v);
  }
  return hipGetLastError();
}

static bool adj_pose_ok(const AdjPose* g) {
  return g && g->n_problems >= 0 && (g->n_problems == 0 || (g->movable && g->pose_off && g->plane_off &&
         g->view_point && g->view_uv && g->xyz && g->X && g->Y && g->Z && g->U && g->V && g->init && g->rposes &&
         g->T && g->pose_stats));
}

extern "C" hipError_t picp_launch_adjust_gather(hipStream_t stream, const AdjPose* g, int write_uv) {
  if (!adj_pose_ok(g)) return hipErrorInvalidValue;
  if (g->n_problems == 0) return hipSuccess;
  hipLaunchKernelGGL(adj_gather_kernel, dim3((unsigned)g->n_problems), dim3(AJ_BLOCK), 0, stream, *g, write_uv);
  return hipGetLastError();
}

extern "C" hipError_t picp_launch_adjust_writeback(hipStream_t stream, const AdjPose* g, const PicpState* st) {
  if (!adj_pose_ok(g) || (g->n_problems > 0 && !st)) return hipErrorInvalidValue;
  if (g->n_problems == 0) return hipSuccess;
  hipLaunchKernelGGL(adj_writeback_kernel, dim3((unsigned)((g->n_problems + AJ_BLOCK - 1) / AJ_BLOCK)),
                     dim3(AJ_BLOCK), 0, stream, *g, st);
  return hipGetLastError();
}

extern "C" hipError_t picp_launch_adjust_sums(hipStream_t stream, const picp_stats* point_stats, int64_t n_points,
                                              const picp_stats* pose_stats, int64_t n_poses,
                                              picp_adjust_sweep* out) {
  if (!out || n_points < 0 || n_poses < 0 || (n_points > 0 && !point_stats) || (n_poses > 0 && !pose_stats))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(adj_sums_kernel, dim3(1), dim3(AJ_SCAN), 0, stream, point_stats, n_points, pose_stats, n_poses,
                     out);
  return hipGetLastError();
}
