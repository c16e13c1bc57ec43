// picp_refine_host.h -- the point refiner's handle, shared by the runtime translation units that
// drive it: picp_refine_runtime.cpp (the point step), picp_adjust_runtime.cpp (the pose step and the
// sweeps) and picp_vo_tracks_runtime.cpp (picp_vo_adjust runs one on the run's tracks).  Not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <vector>

#include "picp_c.h"
#include "picp_host.h"
#include "picp_internal.h"

struct picp_batch;

#pragma GCC visibility push(hidden)

// What the alternating adjustment adds to the refiner (picp_adjust_runtime.cpp).
// Everything here is built lazily by the first call that needs it and costs nothing before.
struct RefineAdjust {
  DevBuf<float> T_d;            // the poses as 4x4, 16 floats each (picp_refine_get_poses)
  std::vector<uint8_t> fixed;      // n_poses flags; empty: none fixed
  // the pose-major view of the tracks
  bool view_built = false;
  DevBuf<int32_t> cnt_d;        // per pose: the count, then the fill's cursor
  DevBuf<int64_t> pose_off_d;   // n_poses + 1
  DevBuf<int2> tmp_d;           // per entry, in the order the cursors gave: (source position, point)
  DevBuf<int32_t> view_point_d; // per entry, canonical order: the owning point
  DevBuf<float2> view_uv_d;     // per entry, canonical order: the pixel
  std::vector<int64_t> pose_off;   // the host's copy (the batch's layout needs the sizes)
  // the pose batch: one problem per movable pose, ascending
  bool batch_ready = false;        // the batch below is laid out for the view and the fixed mask
  bool uv_written = false;         // U and V planes hold the view's pixels
  picp_batch* batch = nullptr;
  std::vector<int32_t> movable;    // problem -> pose
  DevBuf<int32_t> movable_d;
  DevBuf<int64_t> plane_off_d;  // problem -> offset into the batch's planes
  hipEvent_t ev = nullptr;         // orders the batch's stream after the refiner's
  DevBuf<picp_stats> pose_stats_d;  // n_poses
  bool have_pose_stats = false;
  // sweep records of the last picp_refine_adjust
  DevBuf<picp_adjust_sweep> sweeps_d;
  int n_sweeps = 0;
  // picp_refine_adjust_time: the poses the call found
  DevBuf<RefinePose> poses0_d;
  DevBuf<float> T0_d;
};

struct picp_refine {
  int device = 0, rows = 0, cols = 0;
  float K[9];
  hipStream_t stream = nullptr;
  DevBuf<RefinePose> poses_d;
  int n_poses = -1;              // -1: not set
  DevBuf<int64_t> off_d;
  DevBuf<int32_t> obs_pose_d;
  DevBuf<float2> obs_uv_d;
  int64_t n_points = -1, n_obs = 0;  // -1: tracks not set
  int32_t max_pose_idx = -1;     // largest pose index of the tracks (-1: no observation)
  DevBuf<float> xyz_d;        // the current points
  DevBuf<float> xyz0_d;       // picp_refine_time: the points the call found
  DevBuf<picp_stats> stats_d;
  bool have_points = false, have_stats = false;
  RefineAdjust adj;
};

// The by-value arguments of a point-step launch over n_points points (the parameters checked by the
// caller, with its own messages).
inline void refine_fill_args(const float K[9], int rows, int cols, const picp_refine_params* prm, int64_t n_points,
                             RefineArgs* a) {
  memcpy(a->K, K, sizeof(a->K));
  a->maxx = (float)(cols - 1);
  a->maxy = (float)(rows - 1);
  a->threshold = prm->threshold;
  a->damping = prm->damping;
  a->conv_eps = prm->conv_eps;
  a->min_inliers = prm->min_inliers;
  a->keep_outliers = prm->keep_outliers;
  a->max_rounds = prm->max_rounds;
  a->pinhole = 0;
  a->n_points = n_points;
}

// picp_refine_runtime.cpp: everything a point-step launch needs is set and consistent; fills the
// by-value arguments.  refine_enqueue launches it on the handle's stream without waiting.
int refine_prepare(picp_refine* h, const picp_refine_params* prm, RefineArgs* a);
hipError_t refine_enqueue(picp_refine* h, const RefineArgs* a);

// picp_adjust_runtime.cpp
void adjust_poses_changed(picp_refine* h);   // picp_refine_set_poses: mask and sweep records reset
void adjust_tracks_changed(picp_refine* h);  // picp_refine_set_tracks: the view is stale
void adjust_free(picp_refine* h);
// Poses, tracks and points from device memory (copied on the handle's stream; the sources must be
// complete).  tracks == false keeps the tracks of the last call (and the view built from them).
int refine_load_device(picp_refine* h, int n_poses, const RefinePose* rposes, const float* T_wc, bool tracks,
                       int64_t n_points, int64_t n_obs, const int64_t* track_off, const int32_t* obs_pose,
                       const float2* obs_uv, const float* xyz);

#pragma GCC visibility pop
