// picp_refine_runtime.cpp -- host side of the point refiner (picp_refine.hip), C-ABI in
// include/picp_c.h (picp_refine_*): device-resident poses, tracks and points; one launch per run.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "picp_c.h"
#include "picp_host.h"
#include "picp_launch.h"
#include "picp_refine_host.h"

#define set_err picp_set_err

extern "C" void picp_refine_params_default(picp_refine_params* p) {
  if (!p) return;
  p->threshold = 3000.0f;  // exec/icp_test.cpp:86
  p->damping = 1.0f;
  p->min_inliers = 2;
  p->keep_outliers = 0;
  p->max_rounds = 10;
  p->conv_eps = 1e-5f;
}

extern "C" int picp_refine_create(picp_refine_t** out, int device, int rows, int cols, const float K[9]) {
  CHECK_ARG(out && K, "picp_refine_create: null argument");
  CHECK_ARG(rows > 0 && cols > 0, "picp_refine_create: rows/cols must be positive");
  if (int rc = select_device("picp_refine_create", device)) return rc;
  picp_refine* h = new picp_refine();
  h->device = device;
  h->rows = rows;
  h->cols = cols;
  memcpy(h->K, K, sizeof(h->K));
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete h;
    return set_err(PICP_ERR_DEVICE, "picp_refine_create: stream create: %s", hipGetErrorString(e));
  }
  *out = h;
  return PICP_OK;
}

extern "C" int picp_refine_destroy(picp_refine_t* h) {
  if (!h) return PICP_OK;
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  adjust_free(h);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;  // the device buffers free themselves
  return PICP_OK;
}

extern "C" int picp_refine_set_poses(picp_refine_t* h, const float* T_wc, int n_poses) {
  CHECK_ARG(h, "picp_refine_set_poses: null handle");
  CHECK_ARG(n_poses >= 0 && (n_poses == 0 || T_wc), "picp_refine_set_poses: bad array");
  HIP_TRY(hipSetDevice(h->device));
  // the 48-B table the kernel gathers from: the rows of [R | t] of every pose
  std::vector<RefinePose> tab((size_t)n_poses);
  for (int k = 0; k < n_poses; ++k) tab[k] = picp::pose_to_rows(T_wc + 16 * (size_t)k);
  int rc = h->poses_d.grow(n_poses);
  if (!rc) rc = h->adj.T_d.grow(16 * (int64_t)n_poses);
  if (rc) return rc;
  if (n_poses) {
    HIP_TRY(hipMemcpyAsync(h->poses_d, tab.data(), (size_t)n_poses * sizeof(RefinePose), hipMemcpyHostToDevice, h->stream));
    // the same poses as given: picp_refine_get_poses returns a pose that never moved with these bits
    HIP_TRY(hipMemcpyAsync(h->adj.T_d, T_wc, (size_t)n_poses * 16 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  h->n_poses = n_poses;
  adjust_poses_changed(h);
  return PICP_OK;
}

extern "C" int picp_refine_set_tracks(picp_refine_t* h, int64_t n_points, const int64_t* track_off,
                                      const int32_t* obs_pose, const float* obs_uv) {
  CHECK_ARG(h, "picp_refine_set_tracks: null handle");
  CHECK_ARG(n_points >= 0 && track_off, "picp_refine_set_tracks: bad offsets");
  CHECK_ARG(n_points <= (int64_t)INT32_MAX * 8, "picp_refine_set_tracks: too many points");
  CHECK_ARG(track_off[0] == 0, "picp_refine_set_tracks: track_off[0] must be 0");
  for (int64_t i = 0; i < n_points; ++i)
    CHECK_ARG(track_off[i + 1] >= track_off[i], "picp_refine_set_tracks: offsets decrease");
  const int64_t n_obs = track_off[n_points];
  CHECK_ARG(n_obs <= INT32_MAX, "picp_refine_set_tracks: more observations than an int32 addresses");
  CHECK_ARG(n_obs == 0 || (obs_pose && obs_uv), "picp_refine_set_tracks: null observation array");
  int32_t max_idx = -1;
  for (int64_t k = 0; k < n_obs; ++k) {
    if (obs_pose[k] < 0 || (h->n_poses >= 0 && obs_pose[k] >= h->n_poses))
      return set_err(PICP_ERR_RANGE, "observation %lld: pose index %d out of range (%d poses)", (long long)k,
                     obs_pose[k], h->n_poses);
    max_idx = std::max(max_idx, obs_pose[k]);
  }
  HIP_TRY(hipSetDevice(h->device));
  int rc = h->off_d.grow(n_points + 1);
  if (!rc) rc = h->obs_pose_d.grow(n_obs);
  if (!rc) rc = h->obs_uv_d.grow(n_obs);
  if (rc) {
    h->n_points = -1;
    return rc;
  }
  const int64_t old_points = h->n_points;
  h->n_points = -1;  // a failed upload leaves no half-set tracks
  HIP_TRY(hipMemcpyAsync(h->off_d, track_off, (size_t)(n_points + 1) * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  if (n_obs) {
    HIP_TRY(hipMemcpyAsync(h->obs_pose_d, obs_pose, (size_t)n_obs * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->obs_uv_d, obs_uv, (size_t)n_obs * sizeof(float2), hipMemcpyHostToDevice, h->stream));
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->n_points = n_points;
  h->n_obs = n_obs;
  h->max_pose_idx = max_idx;
  if (old_points != n_points) h->have_points = false;
  h->have_stats = false;
  adjust_tracks_changed(h);
  return PICP_OK;
}

extern "C" int picp_refine_set_points(picp_refine_t* h, const float* xyz) {
  CHECK_ARG(h, "picp_refine_set_points: null handle");
  if (h->n_points < 0) return set_err(PICP_ERR_STATE, "picp_refine_set_points: tracks not set (they give n_points)");
  CHECK_ARG(h->n_points == 0 || xyz, "picp_refine_set_points: null array");
  HIP_TRY(hipSetDevice(h->device));
  int rc = h->xyz_d.grow(3 * h->n_points);
  if (rc) return rc;
  if (h->n_points) {
    HIP_TRY(hipMemcpyAsync(h->xyz_d, xyz, (size_t)h->n_points * 3 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  h->have_points = true;
  h->have_stats = false;
  return PICP_OK;
}

// everything a launch needs is set and consistent; fills the by-value arguments
int refine_prepare(picp_refine* h, const picp_refine_params* prm, RefineArgs* a) {
  CHECK_ARG(!(prm->threshold != prm->threshold) && !(prm->damping != prm->damping), "refine: NaN parameter");
  CHECK_ARG(prm->max_rounds >= 0, "refine: max_rounds must not be negative");
  if (h->n_poses < 0) return set_err(PICP_ERR_STATE, "refine: poses not set");
  if (h->n_points < 0) return set_err(PICP_ERR_STATE, "refine: tracks not set");
  if (!h->have_points) return set_err(PICP_ERR_STATE, "refine: points not set");
  if (h->max_pose_idx >= h->n_poses)
    return set_err(PICP_ERR_RANGE, "refine: the tracks use pose index %d but %d poses are set", h->max_pose_idx,
                   h->n_poses);
  HIP_TRY(hipSetDevice(h->device));
  int rc = h->stats_d.grow(h->n_points);
  if (rc) return rc;
  refine_fill_args(h->K, h->rows, h->cols, prm, h->n_points, a);
  return PICP_OK;
}

hipError_t refine_enqueue(picp_refine* h, const RefineArgs* a) {
  return picp_launch_refine(h->stream, a, h->poses_d, h->off_d, h->obs_pose_d, h->obs_uv_d, h->xyz_d, h->stats_d);
}

extern "C" int picp_refine_run(picp_refine_t* h, const picp_refine_params* prm) {
  CHECK_ARG(h && prm, "picp_refine_run: null argument");
  RefineArgs a;
  int rc = refine_prepare(h, prm, &a);
  if (rc) return rc;
  HIP_TRY(refine_enqueue(h, &a));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->have_stats = true;
  return PICP_OK;
}

extern "C" int picp_refine_get_points(picp_refine_t* h, float* xyz) {
  CHECK_ARG(h, "picp_refine_get_points: null handle");
  if (h->n_points < 0 || !h->have_points) return set_err(PICP_ERR_STATE, "picp_refine_get_points: points not set");
  CHECK_ARG(h->n_points == 0 || xyz, "picp_refine_get_points: null array");
  if (h->n_points == 0) return PICP_OK;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpyAsync(xyz, h->xyz_d, (size_t)h->n_points * 3 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return PICP_OK;
}

extern "C" int picp_refine_get_stats(picp_refine_t* h, picp_stats* stats) {
  CHECK_ARG(h, "picp_refine_get_stats: null handle");
  if (!h->have_stats) return set_err(PICP_ERR_STATE, "picp_refine_get_stats: no run since the inputs were set");
  CHECK_ARG(h->n_points == 0 || stats, "picp_refine_get_stats: null array");
  if (h->n_points == 0) return PICP_OK;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpyAsync(stats, h->stats_d, (size_t)h->n_points * sizeof(picp_stats), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return PICP_OK;
}

extern "C" int picp_refine_time(picp_refine_t* h, const picp_refine_params* prm, int reps, float* us_per_run) {
  CHECK_ARG(h && prm && us_per_run && reps > 0 && reps <= 4096, "picp_refine_time: bad argument");
  RefineArgs a;
  int rc = refine_prepare(h, prm, &a);
  if (rc) return rc;
  *us_per_run = 0.0f;
  if (h->n_points == 0) {
    h->have_stats = true;
    return PICP_OK;
  }
  rc = h->xyz0_d.grow(3 * h->n_points);
  if (rc) return rc;
  const size_t bytes = (size_t)h->n_points * 3 * sizeof(float);
  HIP_TRY(hipMemcpyAsync(h->xyz0_d, h->xyz_d, bytes, hipMemcpyDeviceToDevice, h->stream));
  // every repetition: restore (untimed), event, launch, event; one wait at the end
  TimedSpans ev(reps);
  HIP_TRY(ev.create());
  for (int r = 0; r < reps; ++r) {
    HIP_TRY(hipMemcpyAsync(h->xyz_d, h->xyz0_d, bytes, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(ev.begin(r, h->stream));
    HIP_TRY(refine_enqueue(h, &a));
    HIP_TRY(ev.end(r, h->stream));
  }
  double total_ms = 0.0;
  HIP_TRY(ev.sum_ms(h->stream, &total_ms));
  *us_per_run = (float)(1000.0 * total_ms / reps);
  h->have_stats = true;
  return PICP_OK;
}
