// picp_vo_tracks_runtime.cpp -- what the VO sequence does with a run's observation tracks
// (picp_vo_tracks.hip), C-ABI in include/picp_c.h.  Owns the track log's
// buffers (picp_vo_set_track_log), the CSR build after a run (picp_vo_get_tracks,
// picp_vo_get_poses_wc), map refinement with the poses fixed (picp_vo_refine_*) and the
// alternating adjustment of poses and maps (picp_vo_adjust, picp_vo_get_adjusted_*).  The handle
// and the run itself: picp_vo_host.h, picp_vo_runtime.cpp.
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>
#include <vector>

#include "picp_c.h"
#include "picp_host.h"
#include "picp_internal.h"
#include "picp_launch.h"
#include "picp_refine_host.h"
#include "picp_vo_host.h"

// the CSR build of the last run (release = true: and the log's segment-sized buffers)
void vo_tlog_free(picp_vo* h, bool release) {
  if (h->csr_a) vo_dfree(h, h->csr_a);
  if (h->csr_b) vo_dfree(h, h->csr_b);
  h->csr_a = h->csr_b = nullptr;
  h->csr_built = h->refined = false;
  h->adj_tracks = h->adjusted = false;
  h->xyz_ref = nullptr;
  h->stats_ref = nullptr;
  if (!release) return;
  if (h->tlog_mem) vo_dfree(h, h->tlog_mem);
  h->tlog_mem = nullptr;
  h->tl = VoTrackLog{};
  h->tlog_ran = false;
}

// the track log's buffers for the current segments (log on, segments set)
int vo_tlog_alloc(picp_vo* h) {
  if (!h->tlog || h->plan.n_seg <= 0 || h->tlog_mem) return PICP_OK;
  HIP_TRY(hipSetDevice(h->device));
  // frames f0+1 .. f0+steps, the segment's query frames, are contiguous observations
  std::vector<int64_t> log_off((size_t)h->plan.n_seg);
  int64_t log_slots = 0;
  for (int s = 0; s < h->plan.n_seg; ++s) {
    const VoSegment& G = h->plan.segs[s];
    log_off[s] = log_slots;
    log_slots += h->frame_off[G.f0 + G.steps + 1] - h->frame_off[G.f0 + 1];
  }
  VoParts P;
  const size_t o_log = P.add((size_t)std::max<int64_t>(log_slots, 1) * sizeof(int32_t)).off;
  const size_t o_off = P.add((size_t)h->plan.n_seg * sizeof(int64_t)).off;
  const size_t o_c = P.add((size_t)h->plan.map_slots * sizeof(int32_t)).off;
  const size_t o_x = P.add((size_t)h->plan.map_slots * sizeof(int32_t)).off;
  const size_t o_y = P.add((size_t)h->plan.map_slots * sizeof(int32_t)).off;
  HIP_TRY(vo_malloc(h, &h->tlog_mem, P.total, "track log"));
  char* m = (char*)h->tlog_mem;
  HIP_TRY(hipMemset(m, 0, P.total));
  HIP_TRY(hipMemcpy(m + o_off, log_off.data(), (size_t)h->plan.n_seg * sizeof(int64_t), hipMemcpyHostToDevice));
  h->tl.mlog = (int32_t*)(m + o_log);
  h->tl.log_off = (const int64_t*)(m + o_off);
  h->tl.cre_c = (int32_t*)(m + o_c);
  h->tl.cre_x = (int32_t*)(m + o_x);
  h->tl.cre_y = (int32_t*)(m + o_y);
  return PICP_OK;
}

// ---- observation tracks and map refinement (picp_vo_tracks.hip)

extern "C" int picp_vo_set_track_log(picp_vo_t* h, int enable) {
  CHECK_ARG(h, "picp_vo_set_track_log: null handle");
  const bool on = enable != 0;
  if (on == h->tlog) return PICP_OK;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->tlog = on;
  vo_drop_graph(h);  // the captured sequence has (or lacks) the log launches
  vo_tlog_free(h, true);
  return vo_tlog_alloc(h);
}

static int vo_tracks_ready(picp_vo* h, const char* who) {
  if (!h->tlog || !h->tlog_mem)
    return picp_set_err(PICP_ERR_STATE, "%s: the track log is off (picp_vo_set_track_log)", who);
  if (!h->tlog_ran)
    return picp_set_err(PICP_ERR_STATE, "%s: no run since the track log was switched on or the segments were set", who);
  return PICP_OK;
}

// the timed part of the build: everything but the allocations and the host's look at the totals
static hipError_t vo_tracks_enqueue_count(picp_vo* h) {
  hipError_t e = hipSuccess;
  if (h->csr.n_points > 0)
    e = hipMemsetAsync(h->csr.cnt, 0, (size_t)h->csr.n_points * sizeof(int32_t), h->stream);
  return e == hipSuccess ? picp_launch_vo_tracks_count(h->stream, &h->csr) : e;
}

// the last run's tracks in CSR form, the refiner's pose table and the packed map, on the device
static int vo_tracks_build(picp_vo* h) {
  if (h->csr_built) return PICP_OK;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  vo_tlog_free(h, false);
  CHECK_ARG(h->plan.n_slots <= INT32_MAX, "picp_vo tracks: more pose slots than an int32 addresses");
  const int ns = h->plan.n_seg;
  std::vector<int64_t> mn((size_t)ns);
  HIP_TRY(hipMemcpy(mn.data(), h->vargs.map_n, (size_t)ns * sizeof(int64_t), hipMemcpyDeviceToHost));
  h->pt_base.assign((size_t)ns + 1, 0);
  int64_t max_pts = 0;
  for (int s = 0; s < ns; ++s) {
    h->pt_base[s + 1] = h->pt_base[s] + mn[s];
    max_pts = std::max(max_pts, mn[s]);
  }
  const int64_t np = h->pt_base[ns];
  const size_t np1 = (size_t)std::max<int64_t>(np, 1);
  VoTrackCsr& B = h->csr;
  B = VoTrackCsr{};
  B.L = h->tl;
  B.frame_off = h->frame_off_d;
  B.uv = h->uv_d;
  B.segs = h->vargs.segs;
  B.map_xyz = h->vargs.map_xyz;
  B.poses = h->vargs.poses;
  B.n_points = np;
  B.n_slots = h->plan.n_slots;
  B.n_seg = ns;
  B.max_steps = h->plan.max_steps;
  B.max_pts = max_pts;
  {
    VoParts P;
    const size_t o_pb = P.add(((size_t)ns + 1) * sizeof(int64_t)).off;
    const size_t o_tot = P.add((size_t)ns * sizeof(int64_t)).off;
    const size_t o_base = P.add((size_t)ns * sizeof(int64_t)).off;
    const size_t o_cnt = P.add(np1 * sizeof(int32_t)).off;
    const size_t o_rel = P.add(np1 * sizeof(int64_t)).off;
    HIP_TRY(vo_malloc(h, &h->csr_a, P.total, "track counts"));
    char* m = (char*)h->csr_a;
    B.pt_base = (const int64_t*)(m + o_pb);
    B.seg_tot = (int64_t*)(m + o_tot);
    B.seg_base = (const int64_t*)(m + o_base);
    B.cnt = (int32_t*)(m + o_cnt);
    B.rel = (int64_t*)(m + o_rel);
    HIP_TRY(hipMemcpy(m + o_pb, h->pt_base.data(), ((size_t)ns + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  }
  HIP_TRY(vo_tracks_enqueue_count(h));
  std::vector<int64_t> tot((size_t)ns);
  HIP_TRY(hipMemcpyAsync(tot.data(), B.seg_tot, (size_t)ns * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->obs_base.assign((size_t)ns + 1, 0);
  for (int s = 0; s < ns; ++s) h->obs_base[s + 1] = h->obs_base[s] + tot[s];
  const int64_t no = h->obs_base[ns];
  // picp_refine_set_tracks' limit: the refine kernel addresses observations with an int32
  CHECK_ARG(no <= INT32_MAX, "picp_vo tracks: more observations than an int32 addresses");
  B.n_obs = no;
  const size_t no1 = (size_t)std::max<int64_t>(no, 1);
  {
    VoParts P;
    const size_t o_off = P.add(((size_t)np + 1) * sizeof(int64_t)).off;
    const size_t o_idx = P.add(no1 * sizeof(int64_t)).off;
    const size_t o_slot = P.add(no1 * sizeof(int32_t)).off;
    const size_t o_pose = P.add(no1 * sizeof(int32_t)).off;
    const size_t o_uv = P.add(no1 * sizeof(float2)).off;
    const size_t o_xyz0 = P.add(np1 * 3 * sizeof(float)).off;
    const size_t o_wc = P.add((size_t)h->plan.n_slots * 16 * sizeof(float)).off;
    const size_t o_rp = P.add((size_t)h->plan.n_slots * sizeof(RefinePose)).off;
    const size_t o_xyz = P.add(np1 * 3 * sizeof(float)).off;
    const size_t o_st = P.add(np1 * sizeof(picp_stats)).off;
    HIP_TRY(vo_malloc(h, &h->csr_b, P.total, "tracks"));
    char* m = (char*)h->csr_b;
    B.track_off = (int64_t*)(m + o_off);
    B.obs_index = (int64_t*)(m + o_idx);
    B.obs_slot = (int32_t*)(m + o_slot);
    B.obs_pose = (int32_t*)(m + o_pose);
    B.obs_uv = (float2*)(m + o_uv);
    B.xyz0 = (float*)(m + o_xyz0);
    B.pose_wc = (float*)(m + o_wc);
    B.rposes = (RefinePose*)(m + o_rp);
    h->xyz_ref = (float*)(m + o_xyz);
    h->stats_ref = (picp_stats*)(m + o_st);
  }
  HIP_TRY(hipMemcpyAsync((void*)B.seg_base, h->obs_base.data(), (size_t)ns * sizeof(int64_t), hipMemcpyHostToDevice,
                         h->stream));
  HIP_TRY(picp_launch_vo_tracks_fill(h->stream, &B));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->csr_built = true;
  return PICP_OK;
}

extern "C" int picp_vo_get_tracks(picp_vo_t* h, int seg, int64_t* track_off, int32_t* obs_slot, int64_t* obs_index,
                                  int64_t* n_points, int64_t* n_obs) {
  CHECK_ARG(h, "picp_vo_get_tracks: null handle");
  int rc = vo_tracks_ready(h, "picp_vo_get_tracks");
  if (rc != PICP_OK) return rc;
  CHECK_ARG(seg >= 0 && seg < h->plan.n_seg, "picp_vo_get_tracks: segment out of range");
  rc = vo_tracks_build(h);
  if (rc != PICP_OK) return rc;
  const int64_t p0 = h->pt_base[seg], np = h->pt_base[seg + 1] - p0;
  const int64_t o0 = h->obs_base[seg], no = h->obs_base[seg + 1] - o0;
  if (n_points) *n_points = np;
  if (n_obs) *n_obs = no;
  if (track_off) {
    HIP_TRY(hipMemcpy(track_off, h->csr.track_off + p0, (size_t)(np + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    for (int64_t j = 0; j <= np; ++j) track_off[j] -= o0;
  }
  if (obs_slot && no)
    HIP_TRY(hipMemcpy(obs_slot, h->csr.obs_slot + o0, (size_t)no * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (obs_index && no)
    HIP_TRY(hipMemcpy(obs_index, h->csr.obs_index + o0, (size_t)no * sizeof(int64_t), hipMemcpyDeviceToHost));
  return PICP_OK;
}

extern "C" int picp_vo_get_poses_wc(picp_vo_t* h, float* T_wc) {
  CHECK_ARG(h && T_wc, "picp_vo_get_poses_wc: null argument");
  int rc = vo_tracks_ready(h, "picp_vo_get_poses_wc");
  if (rc == PICP_OK) rc = vo_tracks_build(h);
  if (rc != PICP_OK) return rc;
  HIP_TRY(hipMemcpy(T_wc, h->csr.pose_wc, (size_t)h->plan.n_slots * 16 * sizeof(float), hipMemcpyDeviceToHost));
  return PICP_OK;
}

// the refine launch's by-value arguments, the parameters checked
static int vo_refine_args(picp_vo* h, const picp_refine_params* prm, RefineArgs* a) {
  picp_refine_params def;
  if (!prm) {
    picp_refine_params_default(&def);
    prm = &def;
  }
  CHECK_ARG(!(prm->threshold != prm->threshold) && !(prm->damping != prm->damping), "picp_vo refine: NaN parameter");
  CHECK_ARG(prm->max_rounds >= 0, "picp_vo refine: max_rounds must not be negative");
  refine_fill_args(h->K, h->rows, h->cols, prm, h->csr.n_points, a);
  return PICP_OK;
}

// the run's packed map into the result buffer (untimed), then the refine kernel on it
static hipError_t vo_refine_restore(picp_vo* h) {
  if (h->csr.n_points == 0) return hipSuccess;
  return hipMemcpyAsync(h->xyz_ref, h->csr.xyz0, (size_t)h->csr.n_points * 3 * sizeof(float),
                        hipMemcpyDeviceToDevice, h->stream);
}
static hipError_t vo_refine_enqueue(picp_vo* h, const RefineArgs* a) {
  const VoTrackCsr& B = h->csr;
  return picp_launch_refine(h->stream, a, B.rposes, B.track_off, B.obs_pose, B.obs_uv, h->xyz_ref, h->stats_ref);
}

extern "C" int picp_vo_refine_map(picp_vo_t* h, const picp_refine_params* prm) {
  CHECK_ARG(h, "picp_vo_refine_map: null handle");
  int rc = vo_tracks_ready(h, "picp_vo_refine_map");
  if (rc == PICP_OK) rc = vo_tracks_build(h);
  RefineArgs a;
  if (rc == PICP_OK) rc = vo_refine_args(h, prm, &a);
  if (rc != PICP_OK) return rc;
  HIP_TRY(vo_refine_restore(h));
  HIP_TRY(vo_refine_enqueue(h, &a));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->refined = true;
  return PICP_OK;
}

extern "C" int picp_vo_get_refined_map(picp_vo_t* h, int seg, int64_t cap, float* xyz, picp_stats* stats,
                                       int64_t* n) {
  CHECK_ARG(h && n, "picp_vo_get_refined_map: null argument");
  if (!h->refined || !h->csr_built)
    return picp_set_err(PICP_ERR_STATE, "picp_vo_get_refined_map: no picp_vo_refine_map since the last run");
  CHECK_ARG(seg >= 0 && seg < h->plan.n_seg, "picp_vo_get_refined_map: segment out of range");
  HIP_TRY(hipSetDevice(h->device));
  const int64_t p0 = h->pt_base[seg], np = h->pt_base[seg + 1] - p0;
  return vo_copy_prefix(np, cap, n, {{xyz, h->xyz_ref + 3 * p0, 3 * sizeof(float)},
                                     {stats, h->stats_ref + p0, sizeof(picp_stats)}});
}

extern "C" int picp_vo_refine_time(picp_vo_t* h, const picp_refine_params* prm, int reps, float* build_us,
                                   float* refine_us) {
  CHECK_ARG(h && build_us && refine_us, "picp_vo_refine_time: null argument");
  CHECK_ARG(reps >= 1 && reps <= 4096, "picp_vo_refine_time: reps must be in [1, 4096]");
  int rc = vo_tracks_ready(h, "picp_vo_refine_time");
  if (rc == PICP_OK) rc = vo_tracks_build(h);  // the allocations and the totals, untimed
  RefineArgs a;
  if (rc == PICP_OK) rc = vo_refine_args(h, prm, &a);
  if (rc != PICP_OK) return rc;
  // every repetition rebuilds the same CSR into the same buffers, then refines the restored map
  TimedSpans evb(reps), evr(reps);
  HIP_TRY(evb.create());
  HIP_TRY(evr.create());
  for (int r = 0; r < reps; ++r) {
    HIP_TRY(evb.begin(r, h->stream));
    HIP_TRY(vo_tracks_enqueue_count(h));
    HIP_TRY(picp_launch_vo_tracks_fill(h->stream, &h->csr));
    HIP_TRY(evb.end(r, h->stream));
  }
  for (int r = 0; r < reps; ++r) {
    HIP_TRY(vo_refine_restore(h));
    HIP_TRY(evr.begin(r, h->stream));
    HIP_TRY(vo_refine_enqueue(h, &a));
    HIP_TRY(evr.end(r, h->stream));
  }
  double tb = 0.0, tr = 0.0;
  HIP_TRY(evb.sum_ms(h->stream, &tb));
  HIP_TRY(evr.sum_ms(h->stream, &tr));
  *build_us = (float)(1000.0 * tb / reps);
  *refine_us = (float)(1000.0 * tr / reps);
  h->refined = true;
  return PICP_OK;
}

// ---- alternating adjustment of the run's poses and maps (picp_adjust_runtime.cpp)

extern "C" int picp_vo_adjust(picp_vo_t* h, const picp_adjust_params* prm) {
  CHECK_ARG(h, "picp_vo_adjust: null handle");
  int rc = vo_tracks_ready(h, "picp_vo_adjust");
  if (rc == PICP_OK) rc = vo_tracks_build(h);
  if (rc != PICP_OK) return rc;
  picp_adjust_params def;
  if (!prm) {
    picp_adjust_params_default(&def);
    prm = &def;
  }
  CHECK_ARG(prm->sweeps >= 0, "picp_vo_adjust: sweeps must not be negative");  // before anything is copied
  if (!h->adj) {
    rc = picp_refine_create(&h->adj, h->device, h->rows, h->cols, h->K);
    if (rc != PICP_OK) return rc;
  }
  h->adjusted = false;
  // from the run's map and poses every time; the tracks once per build
  const VoTrackCsr& B = h->csr;
  rc = refine_load_device(h->adj, (int)h->plan.n_slots, B.rposes, B.pose_wc, !h->adj_tracks, B.n_points, B.n_obs,
                          B.track_off, B.obs_pose, B.obs_uv, B.xyz0);
  if (rc != PICP_OK) return rc;
  h->adj_tracks = true;
  // slot 0 of every segment is its world frame
  std::vector<uint8_t> fixed((size_t)h->plan.n_slots, 0);
  for (int s = 0; s < h->plan.n_seg; ++s) fixed[(size_t)h->plan.segs[(size_t)s].slot0] = 1;
  rc = picp_refine_set_fixed_poses(h->adj, fixed.data());
  if (rc == PICP_OK) rc = picp_refine_adjust(h->adj, prm);
  if (rc != PICP_OK) return rc;
  h->adjusted = true;
  return PICP_OK;
}

extern "C" int picp_vo_get_adjusted_poses_wc(picp_vo_t* h, float* T_wc) {
  CHECK_ARG(h && T_wc, "picp_vo_get_adjusted_poses_wc: null argument");
  if (!h->adjusted || !h->csr_built)
    return picp_set_err(PICP_ERR_STATE, "picp_vo_get_adjusted_poses_wc: no picp_vo_adjust since the last run");
  return picp_refine_get_poses(h->adj, T_wc);
}

extern "C" int picp_vo_get_adjusted_map(picp_vo_t* h, int seg, int64_t cap, float* xyz, picp_stats* stats,
                                        int64_t* n) {
  CHECK_ARG(h && n, "picp_vo_get_adjusted_map: null argument");
  if (!h->adjusted || !h->csr_built)
    return picp_set_err(PICP_ERR_STATE, "picp_vo_get_adjusted_map: no picp_vo_adjust since the last run");
  CHECK_ARG(seg >= 0 && seg < h->plan.n_seg, "picp_vo_get_adjusted_map: segment out of range");
  HIP_TRY(hipSetDevice(h->device));
  const int64_t p0 = h->pt_base[seg], np = h->pt_base[seg + 1] - p0;
  if (stats && !h->adj->have_stats) {  // sweeps == 0: no point step
    memset(stats, 0, (size_t)std::min(np, std::max<int64_t>(cap, 0)) * sizeof(picp_stats));
    stats = nullptr;
  }
  // picp_refine_adjust returned: the refiner's stream is idle
  return vo_copy_prefix(np, cap, n, {{xyz, h->adj->xyz_d + 3 * p0, 3 * sizeof(float)},
                                     {stats, h->adj->stats_d + p0, sizeof(picp_stats)}});
}
