// picp_adjust_runtime.cpp -- host side of the alternating adjustment (picp_adjust.hip), C-ABI in
// include/picp_c.h (picp_refine_run_poses, picp_refine_adjust, ...): the pose-major view of the
// refiner's tracks, a pose step as one solve of an internal picp_batch, and the sweep driver.
//
// Streams: the refiner's kernels (point step, view build, gather, write-back, sums) run on the
// refiner's stream; the solve runs on the batch's own stream, ordered after the gather by an event,
// and ends in the batch's blocking read-back -- the one host wait of a pose step.  The write-back
// is enqueued after that wait, so it needs no event; the getters wait for the refiner's stream.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "picp_batch.h"
#include "picp_c.h"
#include "picp_host.h"
#include "picp_launch.h"
#include "picp_refine_host.h"

#define set_err picp_set_err

extern "C" void picp_adjust_params_default(picp_adjust_params* p) {
  if (!p) return;
  picp_refine_params_default(&p->points);
  picp_params_default(&p->poses);
  p->poses.threshold = p->points.threshold;  // one gate for both steps (exec/icp_test.cpp:86)
  p->sweeps = 3;
  p->reserved = 0;
}

static void drop_batch(picp_refine* h) {
  RefineAdjust& A = h->adj;
  if (A.batch) picp_batch_destroy(A.batch);
  A.batch = nullptr;
  A.batch_ready = A.uv_written = false;
  A.movable.clear();
}

void adjust_poses_changed(picp_refine* h) {
  RefineAdjust& A = h->adj;
  A.fixed.clear();
  A.n_sweeps = 0;
  A.have_pose_stats = false;
  drop_batch(h);
  if ((int64_t)A.pose_off.size() != (int64_t)h->n_poses + 1) A.view_built = false;
}

void adjust_tracks_changed(picp_refine* h) {
  h->adj.view_built = false;
  h->adj.have_pose_stats = false;
  drop_batch(h);
}

void adjust_free(picp_refine* h) {
  RefineAdjust& A = h->adj;
  drop_batch(h);
  if (A.ev) hipEventDestroy(A.ev);
  A = RefineAdjust{};  // the device buffers free themselves
}

extern "C" int picp_refine_set_fixed_poses(picp_refine_t* h, const uint8_t* fixed) {
  CHECK_ARG(h, "picp_refine_set_fixed_poses: null handle");
  CHECK_ARG(h->n_poses >= 0, "picp_refine_set_fixed_poses: the poses are not set (they give the mask's length)");
  std::vector<uint8_t> m;
  if (fixed) {
    m.assign(fixed, fixed + h->n_poses);
    for (auto& f : m) f = f != 0;
    if (std::find(m.begin(), m.end(), 1) == m.end()) m.clear();
  }
  if (m == h->adj.fixed) return PICP_OK;
  h->adj.fixed = std::move(m);
  drop_batch(h);
  return PICP_OK;
}

// the state rules of the refiner's run, for calls that take no picp_refine_params
static int adjust_state(picp_refine* h, const char* who) {
  if (h->n_poses < 0) return set_err(PICP_ERR_STATE, "%s: poses not set", who);
  if (h->n_points < 0) return set_err(PICP_ERR_STATE, "%s: tracks not set", who);
  if (h->max_pose_idx >= h->n_poses)
    return set_err(PICP_ERR_RANGE, "%s: the tracks use pose index %d but %d poses are set", who, h->max_pose_idx,
                   h->n_poses);
  return PICP_OK;
}

static AdjView view_args(picp_refine* h) {
  RefineAdjust& A = h->adj;
  AdjView v = {};
  v.track_off = h->off_d;
  v.obs_pose = h->obs_pose_d;
  v.obs_uv = h->obs_uv_d;
  v.cnt = A.cnt_d;
  v.pose_off = A.pose_off_d;
  v.tmp = A.tmp_d;
  v.view_point = A.view_point_d;
  v.view_uv = A.view_uv_d;
  v.n_points = h->n_points;
  v.n_obs = h->n_obs;
  v.n_poses = h->n_poses;
  return v;
}

// the timed part of the build: the counters' memset and the four kernels
static hipError_t view_enqueue(picp_refine* h) {
  const AdjView v = view_args(h);
  hipError_t e = hipMemsetAsync(v.cnt, 0, (size_t)std::max(h->n_poses, 1) * sizeof(int32_t), h->stream);
  return e == hipSuccess ? picp_launch_adjust_view(h->stream, &v) : e;
}

// The pose-major view, built once per track set; the host reads back pose_off only.
static int view_build(picp_refine* h) {
  RefineAdjust& A = h->adj;
  if (A.view_built) return PICP_OK;
  CHECK_ARG(h->n_points <= INT32_MAX, "adjust: more points than the view's int32 point index addresses");
  HIP_TRY(hipSetDevice(h->device));
  const int64_t no = h->n_obs;
  int rc = A.cnt_d.grow(std::max(h->n_poses, 1));
  if (!rc) rc = A.pose_off_d.grow((int64_t)h->n_poses + 1);
  if (!rc) rc = A.tmp_d.grow(no);
  if (!rc) rc = A.view_point_d.grow(no);
  if (!rc) rc = A.view_uv_d.grow(no);
  if (rc) return rc;
  HIP_TRY(view_enqueue(h));
  A.pose_off.assign((size_t)h->n_poses + 1, 0);
  HIP_TRY(hipMemcpyAsync(A.pose_off.data(), A.pose_off_d, A.pose_off.size() * sizeof(int64_t), hipMemcpyDeviceToHost,
                         h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (A.pose_off[h->n_poses] != no)
    return set_err(PICP_ERR_DEVICE, "adjust: the view holds %lld entries for %lld observations",
                   (long long)A.pose_off[h->n_poses], (long long)no);
  A.view_built = true;
  drop_batch(h);
  return PICP_OK;
}

// The internal batch: one problem per movable pose, ascending, laid out as a user's batch of those
// sizes is.  No movable pose: no batch.
static int batch_build(picp_refine* h) {
  RefineAdjust& A = h->adj;
  if (A.batch_ready) return PICP_OK;
  drop_batch(h);
  std::vector<int64_t> offs(1, 0);
  for (int k = 0; k < h->n_poses; ++k) {
    const int64_t n = A.pose_off[k + 1] - A.pose_off[k];
    if (n == 0 || (!A.fixed.empty() && A.fixed[k])) continue;
    A.movable.push_back(k);
    offs.push_back(offs.back() + n);
  }
  const int np = (int)A.movable.size();
  if (np > 0) {
    int rc = batch_create(&A.batch, h->device, np, offs.data(), h->rows, h->cols, h->K);
    if (rc) {
      A.batch = nullptr;
      return rc;
    }
    rc = A.movable_d.grow(np);
    if (!rc) rc = A.plane_off_d.grow(np);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(A.movable_d, A.movable.data(), (size_t)np * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(A.plane_off_d, A.batch->plane_off.data(), (size_t)np * sizeof(int64_t), hipMemcpyHostToDevice,
                           h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));  // the vectors may change before an async copy reads them
    if (!A.ev) HIP_TRY(hipEventCreateWithFlags(&A.ev, hipEventDisableTiming));
  }
  A.batch_ready = true;
  return PICP_OK;
}

static int check_pose_params(const picp_params* p) {
  CHECK_ARG(!(p->threshold != p->threshold) && !(p->damping != p->damping) && !(p->conv_eps != p->conv_eps),
            "adjust: NaN pose parameter");
  CHECK_ARG(p->max_rounds >= 0 && p->max_rounds <= 100000, "adjust: poses.max_rounds out of range");
  return PICP_OK;
}

// everything a pose step needs, checked and built before anything of it is launched
static int poses_prepare(picp_refine* h, const picp_params* prm, const char* who) {
  int rc = check_pose_params(prm);
  if (!rc) rc = adjust_state(h, who);
  if (rc) return rc;
  if (!h->have_points) return set_err(PICP_ERR_STATE, "%s: points not set", who);
  HIP_TRY(hipSetDevice(h->device));
  rc = view_build(h);
  if (!rc) rc = batch_build(h);
  if (!rc) rc = h->adj.pose_stats_d.grow(std::max(h->n_poses, 1));
  return rc;
}

static AdjPose pose_args(picp_refine* h) {
  RefineAdjust& A = h->adj;
  AdjPose g = {};
  g.n_problems = (int32_t)A.movable.size();
  if (!A.batch) return g;
  picp_batch* b = A.batch;
  g.movable = A.movable_d;
  g.pose_off = A.pose_off_d;
  g.plane_off = A.plane_off_d;
  g.view_point = A.view_point_d;
  g.view_uv = A.view_uv_d;
  g.xyz = h->xyz_d;
  g.X = b->X();
  g.Y = b->Y();
  g.Z = b->Z();
  g.U = b->U();
  g.V = b->V();
  g.init = b->init_d;
  g.rposes = h->poses_d;
  g.T = A.T_d;
  g.pose_stats = A.pose_stats_d;
  return g;
}

// optional event pairs around the parts of a pose step (picp_refine_adjust_time)
struct PoseTimers {
  EventPair *gather = nullptr, *solve = nullptr, *writeback = nullptr;
};

static hipError_t gather_enqueue(picp_refine* h) {
  RefineAdjust& A = h->adj;
  const AdjPose g = pose_args(h);
  hipError_t e = picp_launch_adjust_gather(h->stream, &g, A.uv_written ? 0 : 1);
  if (e != hipSuccess) return e;
  A.uv_written = true;
  e = hipEventRecord(A.ev, h->stream);
  return e == hipSuccess ? hipStreamWaitEvent(A.batch->stream, A.ev, 0) : e;
}

// One pose step after poses_prepare: gather, the batch's blocking solve, write-back (enqueued).
static int poses_step(picp_refine* h, const picp_params* prm, const PoseTimers* tm) {
  RefineAdjust& A = h->adj;
  HIP_TRY(hipMemsetAsync(A.pose_stats_d, 0, (size_t)std::max(h->n_poses, 1) * sizeof(picp_stats), h->stream));
  A.have_pose_stats = true;
  if (!A.batch) return PICP_OK;
  picp_batch* b = A.batch;
  if (tm) HIP_TRY(hipEventRecord(tm->gather->a, h->stream));
  HIP_TRY(gather_enqueue(h));
  if (tm) HIP_TRY(hipEventRecord(tm->gather->b, h->stream));
  if (tm) HIP_TRY(hipEventRecord(tm->solve->a, b->stream));
  const int fb0 = b->fallbacks;
  int rc = picp_batch_solve(b, prm);
  if (rc) return rc;
  if (b->fallbacks != fb0) {
    // A hand-off wait timed out and the batch laid itself out again without hand-offs, re-running
    // from its host copy of the initial states, which this handle never fills: solve once more from
    // the states the gather writes.  The plane offsets depend on the sizes alone, the data stayed.
    HIP_TRY(gather_enqueue(h));
    rc = picp_batch_solve(b, prm);
    if (rc) return rc;
  }
  if (tm) HIP_TRY(hipEventRecord(tm->solve->b, b->stream));
  const AdjPose g = pose_args(h);
  if (tm) HIP_TRY(hipEventRecord(tm->writeback->a, h->stream));
  HIP_TRY(picp_launch_adjust_writeback(h->stream, &g, b->st_d[b->result_idx]));
  if (tm) HIP_TRY(hipEventRecord(tm->writeback->b, h->stream));
  return PICP_OK;
}

extern "C" int picp_refine_run_poses(picp_refine_t* h, const picp_params* prm) {
  CHECK_ARG(h && prm, "picp_refine_run_poses: null argument");
  int rc = poses_prepare(h, prm, "picp_refine_run_poses");
  if (rc) return rc;
  rc = poses_step(h, prm, nullptr);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return PICP_OK;
}

static int adjust_prepare(picp_refine* h, const picp_adjust_params* prm, RefineArgs* a, const char* who) {
  CHECK_ARG(prm->sweeps >= 0 && prm->sweeps <= 100000, "adjust: sweeps out of range");
  CHECK_ARG(!(prm->points.conv_eps != prm->points.conv_eps), "adjust: NaN point parameter");
  int rc = check_pose_params(&prm->poses);
  if (!rc) rc = refine_prepare(h, &prm->points, a);
  if (!rc && prm->sweeps > 0) rc = poses_prepare(h, &prm->poses, who);
  if (!rc) rc = h->adj.sweeps_d.grow(std::max(prm->sweeps, 1));
  return rc;
}

// the sweeps after adjust_prepare; tm (nullable): per sweep the point step's and the pose step's event pairs
static int adjust_sweeps(picp_refine* h, const picp_adjust_params* prm, const RefineArgs* a, EventPair* point_ev,
                         EventPair* gather_ev, EventPair* solve_ev, EventPair* wb_ev) {
  RefineAdjust& A = h->adj;
  A.n_sweeps = 0;
  for (int s = 0; s < prm->sweeps; ++s) {
    if (point_ev) HIP_TRY(hipEventRecord(point_ev[s].a, h->stream));
    HIP_TRY(refine_enqueue(h, a));
    if (point_ev) HIP_TRY(hipEventRecord(point_ev[s].b, h->stream));
    h->have_stats = true;
    PoseTimers tm = {gather_ev ? gather_ev + s : nullptr, solve_ev ? solve_ev + s : nullptr, wb_ev ? wb_ev + s : nullptr};
    int rc = poses_step(h, &prm->poses, point_ev ? &tm : nullptr);
    if (rc) return rc;
    HIP_TRY(picp_launch_adjust_sums(h->stream, h->stats_d, h->n_points, A.pose_stats_d, h->n_poses, A.sweeps_d + s));
    A.n_sweeps = s + 1;
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  return PICP_OK;
}

extern "C" int picp_refine_adjust(picp_refine_t* h, const picp_adjust_params* prm) {
  CHECK_ARG(h && prm, "picp_refine_adjust: null argument");
  RefineArgs a;
  int rc = adjust_prepare(h, prm, &a, "picp_refine_adjust");
  if (rc) return rc;
  return adjust_sweeps(h, prm, &a, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int picp_refine_get_poses(picp_refine_t* h, float* T_wc) {
  CHECK_ARG(h, "picp_refine_get_poses: null handle");
  if (h->n_poses < 0) return set_err(PICP_ERR_STATE, "picp_refine_get_poses: poses not set");
  CHECK_ARG(h->n_poses == 0 || T_wc, "picp_refine_get_poses: null array");
  if (h->n_poses == 0) return PICP_OK;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpyAsync(T_wc, h->adj.T_d, (size_t)h->n_poses * 16 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return PICP_OK;
}

extern "C" int picp_refine_get_pose_stats(picp_refine_t* h, picp_stats* stats) {
  CHECK_ARG(h, "picp_refine_get_pose_stats: null handle");
  if (!h->adj.have_pose_stats)
    return set_err(PICP_ERR_STATE, "picp_refine_get_pose_stats: no pose step since the inputs were set");
  CHECK_ARG(h->n_poses == 0 || stats, "picp_refine_get_pose_stats: null array");
  if (h->n_poses == 0) return PICP_OK;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpyAsync(stats, h->adj.pose_stats_d, (size_t)h->n_poses * sizeof(picp_stats), hipMemcpyDeviceToHost,
                         h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return PICP_OK;
}

extern "C" int picp_refine_get_pose_view(picp_refine_t* h, int64_t* pose_off, int32_t* obs_point, float* obs_uv) {
  CHECK_ARG(h, "picp_refine_get_pose_view: null handle");
  int rc = adjust_state(h, "picp_refine_get_pose_view");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  rc = view_build(h);
  if (rc) return rc;
  if (pose_off) memcpy(pose_off, h->adj.pose_off.data(), h->adj.pose_off.size() * sizeof(int64_t));
  if (obs_point && h->n_obs)
    HIP_TRY(hipMemcpyAsync(obs_point, h->adj.view_point_d, (size_t)h->n_obs * sizeof(int32_t), hipMemcpyDeviceToHost,
                           h->stream));
  if (obs_uv && h->n_obs)
    HIP_TRY(hipMemcpyAsync(obs_uv, h->adj.view_uv_d, (size_t)h->n_obs * sizeof(float2), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return PICP_OK;
}

extern "C" int picp_refine_get_sweeps(picp_refine_t* h, picp_adjust_sweep* out, int cap, int* n) {
  CHECK_ARG(h && n, "picp_refine_get_sweeps: null argument");
  *n = h->adj.n_sweeps;
  const int k = std::min(h->adj.n_sweeps, std::max(cap, 0));
  if (k == 0) return PICP_OK;
  CHECK_ARG(out, "picp_refine_get_sweeps: null array");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpyAsync(out, h->adj.sweeps_d, (size_t)k * sizeof(picp_adjust_sweep), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return PICP_OK;
}

extern "C" int picp_refine_adjust_time(picp_refine_t* h, const picp_adjust_params* prm, int reps, float* build_us,
                                       float* gather_us, float* pose_us, float* point_us) {
  CHECK_ARG(h && prm && build_us && gather_us && pose_us && point_us, "picp_refine_adjust_time: null argument");
  CHECK_ARG(reps >= 1 && reps <= 4096, "picp_refine_adjust_time: reps must be in [1, 4096]");
  RefineArgs a;
  int rc = adjust_prepare(h, prm, &a, "picp_refine_adjust_time");
  if (rc) return rc;
  *build_us = *gather_us = *pose_us = *point_us = 0.0f;
  RefineAdjust& A = h->adj;
  const int S = prm->sweeps;
  if (S == 0) {
    A.n_sweeps = 0;
    return PICP_OK;
  }
  // the view again into the same buffers, reps times (the same entries in the same places)
  {
    TimedSpans ev(reps);
    HIP_TRY(ev.create());
    for (int r = 0; r < reps; ++r) {
      HIP_TRY(ev.begin(r, h->stream));
      HIP_TRY(view_enqueue(h));
      HIP_TRY(ev.end(r, h->stream));
    }
    double t = 0.0;
    HIP_TRY(ev.sum_ms(h->stream, &t));
    *build_us = (float)(1000.0 * t / reps);
  }
  // what the call found, restored before every repetition outside the timed spans
  const size_t xb = (size_t)h->n_points * 3 * sizeof(float), pb = (size_t)h->n_poses * sizeof(RefinePose),
               tb = (size_t)h->n_poses * 16 * sizeof(float);
  rc = h->xyz0_d.grow(3 * h->n_points);
  if (!rc) rc = A.poses0_d.grow(h->n_poses);
  if (!rc) rc = A.T0_d.grow(16 * (int64_t)h->n_poses);
  if (rc) return rc;
  if (xb) HIP_TRY(hipMemcpyAsync(h->xyz0_d, h->xyz_d, xb, hipMemcpyDeviceToDevice, h->stream));
  if (pb) HIP_TRY(hipMemcpyAsync(A.poses0_d, h->poses_d, pb, hipMemcpyDeviceToDevice, h->stream));
  if (tb) HIP_TRY(hipMemcpyAsync(A.T0_d, A.T_d, tb, hipMemcpyDeviceToDevice, h->stream));
  double tg = 0.0, tp = 0.0, tx = 0.0;
  for (int r = 0; r < reps; ++r) {
    if (xb) HIP_TRY(hipMemcpyAsync(h->xyz_d, h->xyz0_d, xb, hipMemcpyDeviceToDevice, h->stream));
    if (pb) HIP_TRY(hipMemcpyAsync(h->poses_d, A.poses0_d, pb, hipMemcpyDeviceToDevice, h->stream));
    if (tb) HIP_TRY(hipMemcpyAsync(A.T_d, A.T0_d, tb, hipMemcpyDeviceToDevice, h->stream));
    TimedSpans ep(S), eg(S), es(S), ew(S);
    HIP_TRY(ep.create());
    HIP_TRY(eg.create());
    HIP_TRY(es.create());
    HIP_TRY(ew.create());
    rc = adjust_sweeps(h, prm, &a, ep.ev.data(), eg.ev.data(), es.ev.data(), ew.ev.data());
    if (rc) return rc;
    double t = 0.0;
    HIP_TRY(ep.sum_ms(h->stream, &t));
    tx += t;
    if (!A.batch) continue;
    HIP_TRY(eg.sum_ms(A.batch->stream, &t));
    tg += t;
    HIP_TRY(ew.sum_ms(A.batch->stream, &t));
    tg += t;
    HIP_TRY(es.sum_ms(A.batch->stream, &t));
    tp += t;
  }
  const double per = 1000.0 / ((double)reps * S);
  *gather_us = (float)(tg * per);
  *pose_us = (float)(tp * per);
  *point_us = (float)(tx * per);
  return PICP_OK;
}

int refine_load_device(picp_refine* h, int n_poses, const RefinePose* rposes, const float* T_wc, bool tracks,
                       int64_t n_points, int64_t n_obs, const int64_t* track_off, const int32_t* obs_pose,
                       const float2* obs_uv, const float* xyz) {
  HIP_TRY(hipSetDevice(h->device));
  int rc = h->poses_d.grow(n_poses);
  if (!rc) rc = h->adj.T_d.grow(16 * (int64_t)n_poses);
  if (rc) return rc;
  if (n_poses) {
    HIP_TRY(hipMemcpyAsync(h->poses_d, rposes, (size_t)n_poses * sizeof(RefinePose), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->adj.T_d, T_wc, (size_t)n_poses * 16 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  }
  const bool same_poses = h->n_poses == n_poses;
  h->n_poses = n_poses;
  if (tracks || !same_poses) {
    adjust_poses_changed(h);
  } else {  // the same table again: the mask, the view and the batch stay
    h->adj.n_sweeps = 0;
    h->adj.have_pose_stats = false;
  }
  if (tracks) {
    rc = h->off_d.grow(n_points + 1);
    if (!rc) rc = h->obs_pose_d.grow(n_obs);
    if (!rc) rc = h->obs_uv_d.grow(n_obs);
    if (rc) {
      h->n_points = -1;
      return rc;
    }
    h->n_points = -1;
    HIP_TRY(hipMemcpyAsync(h->off_d, track_off, (size_t)(n_points + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, h->stream));
    if (n_obs) {
      HIP_TRY(hipMemcpyAsync(h->obs_pose_d, obs_pose, (size_t)n_obs * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
      HIP_TRY(hipMemcpyAsync(h->obs_uv_d, obs_uv, (size_t)n_obs * sizeof(float2), hipMemcpyDeviceToDevice, h->stream));
    }
    h->n_points = n_points;
    h->n_obs = n_obs;
    h->max_pose_idx = n_obs > 0 ? n_poses - 1 : -1;  // the caller's indices are in range by construction
    adjust_tracks_changed(h);
  }
  rc = h->xyz_d.grow(3 * h->n_points);
  if (rc) return rc;
  if (h->n_points)
    HIP_TRY(hipMemcpyAsync(h->xyz_d, xyz, (size_t)h->n_points * 3 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->have_points = true;
  h->have_stats = false;
  return PICP_OK;
}
