// picp_vo_tracks.hip -- the VO sequence's observation tracks (include/picp_c.h picp_vo_set_track_log,
// picp_vo_get_tracks, picp_vo_refine_map).
//
// The track of map point j of a segment: the two observations (x, y) that created it and every
// accepted frame->map match whose best index is j, except the match of y itself; ascending by
// global observation index.
//
//   vo_tracklog_kernel     : in the step chain, after every append (t = -1: the bootstrap), one
//                            block per segment.  Copies the step's accepted best indices (wm_*, still
//                            this segment's) into the segment's own dense log and the append's
//                            pairs into the new points' creation records.  No compaction, no atomics.
//   after the run, on the handle's stream (the host reads the segments' totals in between):
//   vo_tracks_count_kernel : block (step, segment): matches per point (integer atomics: no order).
//   vo_tracks_scan_kernel  : block per segment: exclusive scan of the track lengths (count + 2).
//   vo_tracks_place_kernel : thread per point: its offset, x and y, the fill cursor, the packed map.
//   vo_tracks_fill_kernel  : block (step, segment): the matches, at atomic cursors ...
//   vo_tracks_sort_kernel  : ... and a thread per point sorts its track by observation index (the
//                            keys are distinct, so the order the atomics gave does not survive),
//                            then gathers obs_pose and obs_uv.
//   vo_tracks_pose_kernel  : thread per slot: vo_iso_inverse of the run's pose, as 4x4 and as the
//                            refiner's [R | t] rows.
#include <algorithm>

#include "picp_launch.h"
#include "picp_pose.h"
#include "picp_wave.h"

using namespace picp;

#define VT_BLOCK 256
#define VT_SCAN 1024
#define VT_SCAN_WAVES (VT_SCAN / 64)

__global__ __launch_bounds__(VT_BLOCK) void vo_tracklog_kernel(const VoArgs a, int t, const VoTrackLog L) {
  const int s = a.seg0 + (int)blockIdx.x;
  const VoSegment G = a.segs[s];
  const bool boot = t < 0;
  if (!boot && t >= G.steps) return;  // uniform: segment finished
  // the append that just ran: its record, its pairs, and the map size it left
  const int64_t rec = G.slot0 + (boot ? 0 : t + 1);
  const int64_t cnt = a.steps[rec].n_new;
  const int64_t m0 = G.map_off + a.map_n[s] - cnt;
  const int2* pairs = a.pairs + (int64_t)s * a.cap_c;
  const int c = boot ? 0 : t;
  for (int64_t k = threadIdx.x; k < cnt; k += VT_BLOCK) {
    const int2 pr = pairs[k];
    L.cre_c[m0 + k] = c;
    L.cre_x[m0 + k] = pr.x;
    L.cre_y[m0 + k] = pr.y;
  }
  if (boot) return;
  const int64_t nf = G.f0 + t + 1;
  const int64_t on = a.frame_off[nf], nn = a.frame_off[nf + 1] - on;
  int32_t* log = L.mlog + L.log_off[s] + (on - a.frame_off[G.f0 + 1]);
  for (int64_t i = threadIdx.x; i < nn; i += VT_BLOCK) log[i] = a.wm_acc[on + i] != 0 ? a.wm_bi[on + i] : -1;
}

// the logged matches of step t of segment s that belong to a track: f(i, j) for observation i of
// frame f0+t+1 matching map point j, the match of the point's own y left out
template <typename F>
__device__ __forceinline__ void vt_for_matches(const VoTrackCsr& B, int s, int t, const VoSegment& G, F f) {
  const int64_t nf = G.f0 + t + 1;
  const int64_t on = B.frame_off[nf], nn = B.frame_off[nf + 1] - on;
  const int32_t* log = B.L.mlog + B.L.log_off[s] + (on - B.frame_off[G.f0 + 1]);
  const int64_t n = B.pt_base[s + 1] - B.pt_base[s];
  for (int64_t i = threadIdx.x; i < nn; i += VT_BLOCK) {
    const int64_t j = log[i];
    if (j < 0 || j >= n) continue;
    const int64_t m = G.map_off + j;
    if (B.L.cre_c[m] == t && B.L.cre_y[m] == i) continue;  // y itself: already in the track
    f(i, j, on);
  }
}

__global__ __launch_bounds__(VT_BLOCK) void vo_tracks_count_kernel(const VoTrackCsr B) {
  const int s = (int)blockIdx.y, t = (int)blockIdx.x;
  const VoSegment G = B.segs[s];
  if (t >= G.steps) return;  // uniform
  int32_t* cnt = B.cnt + B.pt_base[s];
  vt_for_matches(B, s, t, G, [&](int64_t, int64_t j, int64_t) { atomicAdd(cnt + j, 1); });
}

__global__ __launch_bounds__(VT_SCAN) void vo_tracks_scan_kernel(const VoTrackCsr B) {
  const int s = (int)blockIdx.x;
  const int64_t pb = B.pt_base[s], n = B.pt_base[s + 1] - pb;
  __shared__ int s_w[VT_SCAN_WAVES];
  int64_t carry = 0;
  for (int64_t c0 = 0; c0 < n; c0 += VT_SCAN) {  // uniform
    const int64_t j = c0 + threadIdx.x;
    const int v = j < n ? B.cnt[pb + j] + 2 : 0;  // the matches, x and y
    int tot;
    const int excl = block_scan<VT_SCAN_WAVES>(v, s_w, &tot);
    if (j < n) B.rel[pb + j] = carry + excl;
    carry += tot;
    __syncthreads();  // s_w is reused by the next chunk
  }
  if (threadIdx.x == 0) B.seg_tot[s] = carry;
}

__global__ __launch_bounds__(VT_BLOCK) void vo_tracks_place_kernel(const VoTrackCsr B) {
  const int s = (int)blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * VT_BLOCK + threadIdx.x;
  if (s == 0 && j == 0) B.track_off[B.n_points] = B.n_obs;
  const int64_t pb = B.pt_base[s];
  if (j >= B.pt_base[s + 1] - pb) return;
  const VoSegment G = B.segs[s];
  const int64_t p = pb + j, m = G.map_off + j;
  const int64_t o = B.seg_base[s] + B.rel[p];
  const int c = B.L.cre_c[m];
  const int64_t fx = G.f0 + c;
  B.track_off[p] = o;
  B.obs_index[o] = B.frame_off[fx] + B.L.cre_x[m];
  B.obs_slot[o] = c;
  B.obs_index[o + 1] = B.frame_off[fx + 1] + B.L.cre_y[m];
  B.obs_slot[o + 1] = c + 1;
  B.cnt[p] = 2;  // the fill's cursor
  B.xyz0[3 * p + 0] = B.map_xyz[3 * m + 0];
  B.xyz0[3 * p + 1] = B.map_xyz[3 * m + 1];
  B.xyz0[3 * p + 2] = B.map_xyz[3 * m + 2];
}

__global__ __launch_bounds__(VT_BLOCK) void vo_tracks_fill_kernel(const VoTrackCsr B) {
  const int s = (int)blockIdx.y, t = (int)blockIdx.x;
  const VoSegment G = B.segs[s];
  if (t >= G.steps) return;  // uniform
  const int64_t pb = B.pt_base[s];
  vt_for_matches(B, s, t, G, [&](int64_t i, int64_t j, int64_t on) {
    const int64_t o = B.track_off[pb + j] + atomicAdd(B.cnt + pb + j, 1);
    B.obs_index[o] = on + i;
    B.obs_slot[o] = t + 1;
  });
}

__global__ __launch_bounds__(VT_BLOCK) void vo_tracks_sort_kernel(const VoTrackCsr B) {
  const int s = (int)blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * VT_BLOCK + threadIdx.x;
  const int64_t pb = B.pt_base[s];
  if (j >= B.pt_base[s + 1] - pb) return;
  const int64_t b = B.track_off[pb + j], e = B.track_off[pb + j + 1];
  // insertion sort (tracks are short and the cursors hand out nearly ascending places)
  for (int64_t k = b + 1; k < e; ++k) {
    const int64_t key = B.obs_index[k];
    const int32_t sl = B.obs_slot[k];
    int64_t q = k;
    while (q > b && B.obs_index[q - 1] > key) {
      B.obs_index[q] = B.obs_index[q - 1];
      B.obs_slot[q] = B.obs_slot[q - 1];
      --q;
    }
    B.obs_index[q] = key;
    B.obs_slot[q] = sl;
  }
  const int32_t slot0 = (int32_t)B.segs[s].slot0;
  for (int64_t k = b; k < e; ++k) {
    B.obs_pose[k] = slot0 + B.obs_slot[k];
    B.obs_uv[k] = B.uv[B.obs_index[k]];
  }
}

__global__ __launch_bounds__(VT_BLOCK) void vo_tracks_pose_kernel(const VoTrackCsr B) {
  const int64_t k = (int64_t)blockIdx.x * VT_BLOCK + threadIdx.x;
  if (k >= B.n_slots) return;
  float T[16], Ti[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) T[q] = B.poses[16 * k + q];
  vo_iso_inverse(T, Ti);
#pragma unroll
  for (int q = 0; q < 16; ++q) B.pose_wc[16 * k + q] = Ti[q];
  B.rposes[k] = pose_to_rows(Ti);  // as picp_refine_set_poses
}

extern "C" hipError_t picp_launch_vo_tracklog(hipStream_t stream, const VoArgs* a, int t, const VoTrackLog* L) {
  if (!a || !L || a->n_seg <= 0 || !L->mlog || !L->log_off || !L->cre_c || !L->cre_x || !L->cre_y)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(vo_tracklog_kernel, dim3(a->n_seg), dim3(VT_BLOCK), 0, stream, *a, t, *L);
  return hipGetLastError();
}

static bool vt_grid_ok(const VoTrackCsr* B) {
  return B && B->n_seg >= 1 && B->n_seg <= 65535 && B->max_steps >= 1 && B->n_points >= 0 && B->n_slots >= 0 &&
         (B->max_pts + VT_BLOCK - 1) / VT_BLOCK <= INT32_MAX;
}

extern "C" hipError_t picp_launch_vo_tracks_count(hipStream_t stream, const VoTrackCsr* B) {
  if (!vt_grid_ok(B)) return hipErrorInvalidValue;
  if (B->n_points > 0)
    hipLaunchKernelGGL(vo_tracks_count_kernel, dim3(B->max_steps, B->n_seg), dim3(VT_BLOCK), 0, stream, *B);
  hipLaunchKernelGGL(vo_tracks_scan_kernel, dim3(B->n_seg), dim3(VT_SCAN), 0, stream, *B);
  return hipGetLastError();
}

extern "C" hipError_t picp_launch_vo_tracks_fill(hipStream_t stream, const VoTrackCsr* B) {
  if (!vt_grid_ok(B) || B->n_obs < 0 || B->n_obs > INT32_MAX) return hipErrorInvalidValue;
  const unsigned gp = (unsigned)std::max<int64_t>((B->max_pts + VT_BLOCK - 1) / VT_BLOCK, 1);
  hipLaunchKernelGGL(vo_tracks_place_kernel, dim3(gp, B->n_seg), dim3(VT_BLOCK), 0, stream, *B);
  if (B->n_points > 0) {
    hipLaunchKernelGGL(vo_tracks_fill_kernel, dim3(B->max_steps, B->n_seg), dim3(VT_BLOCK), 0, stream, *B);
    hipLaunchKernelGGL(vo_tracks_sort_kernel, dim3(gp, B->n_seg), dim3(VT_BLOCK), 0, stream, *B);
  }
  if (B->n_slots > 0)
    hipLaunchKernelGGL(vo_tracks_pose_kernel, dim3((unsigned)((B->n_slots + VT_BLOCK - 1) / VT_BLOCK)),
                       dim3(VT_BLOCK), 0, stream, *B);
  return hipGetLastError();
}
