// picp_refine_host.h -- the point refiner's handle, shared by the runtime translation units that
// drive it: picp_refine_runtime.cpp (the point step), picp_adjust_runtime.cpp (the pose step and the
// sweeps) and picp_vo_runtime.cpp (picp_vo_adjust runs one on the run's tracks).  Not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <vector>

#include "picp_c.h"
#include "picp_internal.h"

struct picp_batch;

#pragma GCC visibility push(hidden)

// What the alternating adjustment adds to the refiner (picp_adjust_runtime.cpp).
// Everything here is built lazily by the first call that needs it and costs nothing before.
struct RefineAdjust {
  float* T_d = nullptr;            // the poses as 4x4, 16 floats each (picp_refine_get_poses)
  int64_t cap_T = 0;
  std::vector<uint8_t> fixed;      // n_poses flags; empty: none fixed
  // the pose-major view of the tracks
  bool view_built = false;
  int32_t* cnt_d = nullptr;        // per pose: the count, then the fill's cursor
  int64_t cap_cnt = 0;
  int64_t* pose_off_d = nullptr;   // n_poses + 1
  int64_t cap_pose_off = 0;
  int2* tmp_d = nullptr;           // per entry, in the order the cursors gave: (source position, point)
  int64_t cap_tmp = 0;
  int32_t* view_point_d = nullptr; // per entry, canonical order: the owning point
  int64_t cap_view_point = 0;
  float2* view_uv_d = nullptr;     // per entry, canonical order: the pixel
  int64_t cap_view_uv = 0;
  std::vector<int64_t> pose_off;   // the host's copy (the batch's layout needs the sizes)
  // the pose batch: one problem per movable pose, ascending
  bool batch_ready = false;        // the batch below is laid out for the view and the fixed mask
  bool uv_written = false;         // U and V planes hold the view's pixels
  picp_batch* batch = nullptr;
  std::vector<int32_t> movable;    // problem -> pose
  int32_t* movable_d = nullptr;
  int64_t cap_movable = 0;
  int64_t* plane_off_d = nullptr;  // problem -> offset into the batch's planes
  int64_t cap_plane_off = 0;
  hipEvent_t ev = nullptr;         // orders the batch's stream after the refiner's
  picp_stats* pose_stats_d = nullptr;  // n_poses
  int64_t cap_pose_stats = 0;
  bool have_pose_stats = false;
  // sweep records of the last picp_refine_adjust
  picp_adjust_sweep* sweeps_d = nullptr;
  int64_t cap_sweeps = 0;
  int n_sweeps = 0;
  // picp_refine_adjust_time: the poses the call found
  RefinePose* poses0_d = nullptr;
  int64_t cap_poses0 = 0;
  float* T0_d = nullptr;
  int64_t cap_T0 = 0;
};

struct picp_refine {
  int device = 0, rows = 0, cols = 0;
  float K[9];
  hipStream_t stream = nullptr;
  RefinePose* poses_d = nullptr;
  int64_t cap_poses = 0;
  int n_poses = -1;              // -1: not set
  int64_t* off_d = nullptr;
  int64_t cap_off = 0;
  int32_t* obs_pose_d = nullptr;
  int64_t cap_obs_pose = 0;
  float2* obs_uv_d = nullptr;
  int64_t cap_obs_uv = 0;
  int64_t n_points = -1, n_obs = 0;  // -1: tracks not set
  int32_t max_pose_idx = -1;     // largest pose index of the tracks (-1: no observation)
  float* xyz_d = nullptr;        // the current points
  int64_t cap_xyz = 0;
  float* xyz0_d = nullptr;       // picp_refine_time: the points the call found
  int64_t cap_xyz0 = 0;
  picp_stats* stats_d = nullptr;
  int64_t cap_stats = 0;
  bool have_points = false, have_stats = false;
  RefineAdjust adj;
};

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
