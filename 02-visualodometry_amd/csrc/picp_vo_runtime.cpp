// picp_vo_runtime.cpp -- host side of the device-resident VO sequence (picp_vo.hip), C-ABI in
// include/picp_c.h (picp_vo_*).  Owns create and destroy, applying the segment plan
// (picp_vo_plan.h) to device memory, the run's enqueue, launch and timing, the plain getters, the
// per-map-point track counters and the guard and diagnostic calls.
//
// A handle owns one packed observation sequence in HBM (frame offsets, uv, descriptors) and,
// after picp_vo_set_segments, everything a run needs: per-segment maps, the PICP SoA planes,
// problem tables and states, match outputs, poses and step records.  A run is
//   1 (or ceil(frames/65535)) launch(es) matching every frame f against f+1,
//   1 bootstrap append, then per step: world match, gather, picp_block_kernel, append,
// enqueued back to back on the handle's stream and captured once into a hipGraph that is
// replayed by every later run.  No host round trip inside a run; no host fallback.
// Opt-in and read-only beside it: the per-map-point track counters (picp_vo_set_track_stats) and
// the observation tracks (picp_vo_set_track_log: one more launch after every append records them,
// picp_vo_get_tracks / picp_vo_refine_map build and use them after the run:
// picp_vo_tracks_runtime.cpp).
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "picp_c.h"
#include "picp_host.h"
#include "picp_internal.h"
#include "picp_launch.h"
#include "picp_refine_host.h"
#include "picp_vo_host.h"

static_assert(sizeof(picp_vo_step) == sizeof(VoStep), "picp_vo_step must mirror VoStep");
// the sizes the plan carves with
static_assert(sizeof(PicpState) == VO_STATE_BYTES && sizeof(VoStep) == VO_STEP_BYTES && sizeof(int2) == VO_PAIR_BYTES &&
                  sizeof(_Float16) == VO_HALF_BYTES && sizeof(float4) == VO_FLOAT4_BYTES,
              "picp_vo_plan.h: a part's element size");

#define VO_MATCH_DIST 0.2f   // DISTANCE_THRESHOLD, src/my_utilities.h:44
#define VO_MATCH_RATIO 0.8f  // RATIO_THRESHOLD, src/my_utilities.h:46

hipError_t vo_malloc(picp_vo* h, void** p, size_t bytes, const char* name) {
  if (!h->guard) return hipMalloc(p, bytes);
  char* base = nullptr;
  hipError_t e = hipMalloc((void**)&base, bytes + 2 * (size_t)VO_GUARD);
  if (e != hipSuccess) return e;
  e = hipMemset(base, VO_GUARD_BYTE, bytes + 2 * (size_t)VO_GUARD);
  if (e != hipSuccess) return e;
  h->guards.push_back(VoGuarded{base, bytes, name});
  *p = base + VO_GUARD;
  return hipSuccess;
}

void vo_dfree(picp_vo* h, void* p) {
  if (!h->guard) {
    hipFree(p);
    return;
  }
  for (size_t i = 0; i < h->guards.size(); ++i)
    if (h->guards[i].base + VO_GUARD == (char*)p) {
      hipFree(h->guards[i].base);
      h->guards.erase(h->guards.begin() + (long)i);
      return;
    }
}

void vo_drop_graph(picp_vo* h) {
  if (h->exec) hipGraphExecDestroy(h->exec);
  if (h->graph) hipGraphDestroy(h->graph);
  h->exec = nullptr;
  h->graph = nullptr;
}

static void vo_free_segments(picp_vo* h) {
  vo_tlog_free(h, true);
  vo_drop_graph(h);
  for (hipEvent_t e : h->ev_chunk)
    if (e) hipEventDestroy(e);
  h->ev_chunk.clear();
  if (h->seg_mem) vo_dfree(h, h->seg_mem);
  h->seg_mem = nullptr;
  h->plan = VoPlan{};
}

extern "C" int picp_vo_destroy(picp_vo_t* h) {
  if (!h) return PICP_OK;
  if (h->stream) hipStreamSynchronize(h->stream);
  vo_free_segments(h);
  if (h->adj) picp_refine_destroy(h->adj);
  h->adj = nullptr;
  void* bufs[] = {h->frame_off_d, h->uv_d, h->desc_d, h->pm_bi, h->pm_acc, h->wm_bi, h->wm_acc,
                  h->pm_bd, h->pm_sd, h->wm_bd, h->wm_sd, h->obs_h, h->obs_n1, h->obs_n2, h->track_d};
  for (void* p : bufs)
    if (p) vo_dfree(h, p);
  if (h->ev0) hipEventDestroy(h->ev0);
  if (h->ev1) hipEventDestroy(h->ev1);
  if (h->ev_fork) hipEventDestroy(h->ev_fork);
  if (h->side) hipStreamDestroy(h->side);
  for (hipEvent_t e : h->ev_cj)
    if (e) hipEventDestroy(e);
  for (hipEvent_t e : h->ev_ph)
    if (e) hipEventDestroy(e);
  for (hipEvent_t e : h->ev_app)
    if (e) hipEventDestroy(e);
  for (hipEvent_t e : h->ev_early)
    if (e) hipEventDestroy(e);
  for (hipStream_t c : h->estream)
    if (c) hipStreamDestroy(c);
  for (hipStream_t c : h->cstream)
    if (c) hipStreamDestroy(c);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
  return PICP_OK;
}

extern "C" int picp_vo_create(picp_vo_t** out, int device, int rows, int cols, const float K[9],
                              int64_t n_frames, const int64_t* frame_off, const float* uv,
                              const float* desc, int dim) {
  CHECK_ARG(out, "picp_vo_create: null output");
  *out = nullptr;
  CHECK_ARG(K && frame_off && rows > 0 && cols > 0, "picp_vo_create: bad camera or frame table");
  CHECK_ARG(n_frames >= 2, "picp_vo_create: need at least two frames");
  CHECK_ARG(dim >= 1 && dim <= 32, "picp_vo_create: dim must be in [1, 32]");
  CHECK_ARG(frame_off[0] == 0, "picp_vo_create: frame_off[0] must be 0");
  int64_t mx = 0;
  for (int64_t f = 0; f < n_frames; ++f) {
    CHECK_ARG(frame_off[f + 1] >= frame_off[f], "picp_vo_create: frame_off must be non-decreasing");
    mx = std::max(mx, frame_off[f + 1] - frame_off[f]);
  }
  CHECK_ARG(mx <= (1 << 30), "picp_vo_create: frame too large");
  const int64_t n_obs = frame_off[n_frames];
  CHECK_ARG(n_obs == 0 || (uv && desc), "picp_vo_create: null observation arrays");
  if (int rc = select_device("picp_vo_create", device)) return rc;
  picp_vo* h = new picp_vo();
  h->device = device;
  h->rows = rows;
  h->cols = cols;
  h->dim = dim;
  memcpy(h->K, K, sizeof(h->K));
  h->n_frames = n_frames;
  h->n_obs = n_obs;
  h->max_obs = mx;
  h->frame_off.assign(frame_off, frame_off + n_frames + 1);
  if (const char* e = getenv("PICP_VO_GRAPH")) {
    h->use_graph = atoi(e) != 0;
    h->graph_env = true;
  }
  if (const char* e = getenv("PICP_VO_MATCH_FULL")) h->opt.accept_only = atoi(e) != 0 ? 0 : 1;
  if (const char* e = getenv("PICP_VO_OVERLAP")) h->opt.overlap = atoi(e) != 0;
  // at most two groups: three and four measured slower at the default shape (C5 592k / 404k vs
  // 597-600k frames/s with two, round 2), and so did four and eight at the
  // latency-bound shapes, where a step waits for its chain's slowest segment (round 6: 8e
  // 32.5k / 18.4k vs 42.0k frames/s, the N = 8 per-rank shape 90.2k / 50.0k vs 156.9k;
  // profiles/r06/t2/ab.log), also with 16 hardware queues (8e 30.1k / 28.5k, t6) and replayed
  // from a hipGraph (11.3k-25.8k, t7): the extra chains' world matches compete for the chip
  if (const char* e = getenv("PICP_VO_CHAINS")) h->opt.chains = std::max(1, std::min(2, atoi(e)));
  if (const char* e = getenv("PICP_VO_PHASE")) h->phase = atoi(e) != 0;
  if (const char* e = getenv("PICP_VO_FUSE")) h->fuse = atoi(e) != 0;
  if (const char* e = getenv("PICP_VO_SPLIT")) h->opt.split_env = atoi(e) < 0 ? -1 : (atoi(e) != 0 ? 1 : 0);
  if (!h->graph_env && (h->opt.overlap || h->opt.chains > 1)) h->use_graph = false;
  const size_t no = (size_t)std::max<int64_t>(n_obs, 1);
#define VO_TRY(expr)              \
  do {                            \
    int rc_ = (expr);             \
    if (rc_ != PICP_OK) {         \
      picp_vo_destroy(h);         \
      return rc_;                 \
    }                             \
  } while (0)
  if (const char* e = getenv("PICP_VO_GUARD")) h->guard = atoi(e) != 0;
  auto alloc = [&](void** p, size_t bytes) -> int {
    HIP_TRY(vo_malloc(h, p, bytes, "create"));
    return PICP_OK;
  };
  VO_TRY([&]() -> int {
    // the step chains' streams at the highest priority, the side stream at the lowest
    // (PICP_VO_PRIO=0: all at the default)
    int lo = 0;
    int hi = 0;
    const char* pe = getenv("PICP_VO_PRIO");
    if (!(pe && atoi(pe) == 0)) HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIP_TRY(hipStreamCreateWithPriority(&h->stream, hipStreamNonBlocking, hi));
    // (a CU-masked side stream leaving every 2nd / 4th / 8th CU to the step chains measured equal
    // at every C5 shape, round 6, profiles/r06/t3/ab.log: not kept)
    if (h->opt.overlap) HIP_TRY(hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, lo));
    HIP_TRY(hipEventCreate(&h->ev0));
    HIP_TRY(hipEventCreate(&h->ev1));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    h->cstream.assign((size_t)h->opt.chains, nullptr);
    h->ev_cj.assign((size_t)h->opt.chains, nullptr);
    h->ev_ph.assign((size_t)h->opt.chains, nullptr);
    for (int c = 0; c < h->opt.chains; ++c) {
      if (c > 0) HIP_TRY(hipStreamCreateWithPriority(&h->cstream[c], hipStreamNonBlocking, hi));
      HIP_TRY(hipEventCreateWithFlags(&h->ev_cj[c], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&h->ev_ph[c], hipEventDisableTiming));
    }
    // the early world-match parts: throughput work beside the chains, at the side stream's priority
    h->opt.early_streams = h->opt.split_env != 0;
    if (h->opt.early_streams) {
      h->estream.assign((size_t)h->opt.chains, nullptr);
      h->ev_app.assign((size_t)h->opt.chains, nullptr);
      h->ev_early.assign((size_t)2 * h->opt.chains, nullptr);
      for (int c = 0; c < h->opt.chains; ++c) {
        HIP_TRY(hipStreamCreateWithPriority(&h->estream[c], hipStreamNonBlocking, lo));
        HIP_TRY(hipEventCreateWithFlags(&h->ev_app[c], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&h->ev_early[2 * c], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&h->ev_early[2 * c + 1], hipEventDisableTiming));
      }
    }
    return PICP_OK;
  }());
  VO_TRY(alloc((void**)&h->frame_off_d, (size_t)(n_frames + 1) * sizeof(int64_t)));
  VO_TRY(alloc((void**)&h->uv_d, no * sizeof(float2)));
  VO_TRY(alloc((void**)&h->desc_d, no * dim * sizeof(float)));
  VO_TRY(alloc((void**)&h->pm_bi, no * 4));
  VO_TRY(alloc((void**)&h->pm_acc, no * 4));
  VO_TRY(alloc((void**)&h->wm_bi, no * 4));
  VO_TRY(alloc((void**)&h->wm_acc, no * 4));
  VO_TRY(alloc((void**)&h->pm_bd, no * 4));
  VO_TRY(alloc((void**)&h->pm_sd, no * 4));
  VO_TRY(alloc((void**)&h->wm_bd, no * 4));
  VO_TRY(alloc((void**)&h->wm_sd, no * 4));
  h->dp = 16 * picp_match_prep_kch(dim);
  VO_TRY(alloc((void**)&h->obs_h, no * h->dp * sizeof(_Float16)));
  VO_TRY(alloc((void**)&h->obs_n1, no * 4));
  VO_TRY(alloc((void**)&h->obs_n2, no * 4));
  VO_TRY([&]() -> int {
    HIP_TRY(hipMemcpy(h->frame_off_d, frame_off, (size_t)(n_frames + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    if (n_obs) {
      HIP_TRY(hipMemcpy(h->uv_d, uv, (size_t)n_obs * sizeof(float2), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(h->desc_d, desc, (size_t)n_obs * dim * sizeof(float), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemset(h->wm_acc, 0, no * 4));
    HIP_TRY(picp_launch_match_prep(nullptr, h->desc_d, n_obs, dim, h->obs_h, h->obs_n1, h->obs_n2));
    HIP_TRY(hipDeviceSynchronize());
    return PICP_OK;
  }());
#undef VO_TRY
  *out = h;
  return PICP_OK;
}

// the track counters for the current segments' map (tracking on, segments set)
static int vo_track_alloc(picp_vo* h) {
  if (!h->track || h->plan.n_seg <= 0 || h->track_slots >= h->plan.map_slots) return PICP_OK;
  HIP_TRY(hipSetDevice(h->device));
  if (h->track_d) vo_dfree(h, h->track_d);
  h->track_d = nullptr;
  h->track_slots = 0;
  HIP_TRY(vo_malloc(h, (void**)&h->track_d, 2 * (size_t)h->plan.map_slots * sizeof(int32_t), "track"));
  HIP_TRY(hipMemset(h->track_d, 0, 2 * (size_t)h->plan.map_slots * sizeof(int32_t)));
  h->track_slots = h->plan.map_slots;
  return PICP_OK;
}

// the PICP launch's and the VO kernels' by-value arguments over the plan's parts of seg_mem
static void vo_fill_args(picp_vo* h, const picp_params* prm) {
  const VoPlan& L = h->plan;
  char* m = (char*)h->seg_mem;
  PicpArgs& A = h->pargs;
  memset(&A, 0, sizeof(A));
  memcpy(A.K, h->K, sizeof(A.K));
  A.maxx = (float)(h->cols - 1);
  A.maxy = (float)(h->rows - 1);
  A.threshold = prm->threshold;
  A.damping = prm->damping;
  A.conv_eps = prm->conv_eps;
  A.min_inliers = prm->min_inliers;
  A.keep_outliers = prm->keep_outliers ? 1 : 0;
  A.max_rounds = prm->max_rounds;
  A.uniform = 0;

  VoArgs& V = h->vargs;
  memset(&V, 0, sizeof(V));
  memcpy(V.K, h->K, sizeof(V.K));
  V.dim = h->dim;
  V.n_seg = L.n_seg;
  V.seg0 = 0;
  V.frame_off = h->frame_off_d;
  V.uv = h->uv_d;
  V.desc = h->desc_d;
  V.segs = (const VoSegment*)(m + L.p_segs.off);
  V.boot = (const float*)(m + L.p_boot.off);
  V.pm_bi = h->pm_bi;
  V.pm_acc = h->pm_acc;
  V.wm_bi = h->wm_bi;
  V.wm_acc = h->wm_acc;
  V.map_xyz = (float*)(m + L.p_mxyz.off);
  V.map_desc = (float*)(m + L.p_mdesc.off);
  V.map_n = (int64_t*)(m + L.p_mn.off);
  float* planes = (float*)(m + L.p_planes.off);
  const size_t plane = (size_t)L.n_seg * L.cap_c;
  V.X = planes;
  V.Y = planes + plane;
  V.Z = planes + 2 * plane;
  V.U = planes + 3 * plane;
  V.V = planes + 4 * plane;
  V.cap_c = L.cap_c;
  V.probs = (PicpProblem*)(m + L.p_probs.off);
  V.st_in = (PicpState*)(m + L.p_stin.off);
  V.st_out = (const PicpState*)(m + L.p_stout.off);
  V.wprobs = (MatchProblem*)(m + L.p_wprobs.off);
  V.lprobs = (MatchProblem*)(m + L.p_lprobs.off);
  V.eprobs = (MatchProblem*)(m + L.p_eprobs.off);
  V.seg_all = L.n_seg;
  // the append writes the split tables when any chain splits (one launch covers one chain)
  V.split = 0;
  for (char s : L.split_c) V.split |= s ? 1 : 0;
  V.poses = (float*)(m + L.p_poses.off);
  V.steps = (VoStep*)(m + L.p_steps.off);
  V.pairs = (int2*)(m + L.p_pairs.off);
  V.dp = h->dp;
  V.obs_h = h->obs_h;
  V.obs_n1 = h->obs_n1;
  V.obs_n2 = h->obs_n2;
  V.map_h = (_Float16*)(m + L.p_mh.off);
  V.map_n1 = (float*)(m + L.p_mn1.off);
  V.map_n2 = (float*)(m + L.p_mn2.off);
  h->wprobs_d = V.wprobs;
  h->pprobs_d = (MatchProblem*)(m + L.p_pprobs.off);
}

extern "C" int picp_vo_set_segments(picp_vo_t* h, int n_seg, const int64_t* first,
                                    const int32_t* steps, const float* boot_poses,
                                    const picp_params* prm) {
  CHECK_ARG(h && first && steps && boot_poses && prm, "picp_vo_set_segments: null argument");
  CHECK_ARG(prm->max_rounds >= 0 && prm->max_rounds <= 100000, "params.max_rounds out of range");
  CHECK_ARG(!(prm->threshold != prm->threshold), "params.threshold is NaN");
  HIP_TRY(hipSetDevice(h->device));  // the split rule asks the current device for its CU count
  // every argument is validated before the handle's current segments are released: a rejected
  // call leaves the handle as it was
  VoPlanOptions opt = h->opt;
  opt.ks_force = picp_match_ksplit_env();  // PICP_MATCH_KSPLIT: read once per layout, here
  const VoPlanCaps caps{picp_match_ksplit_forced, picp_match_split_scratch};
  VoPlan P;
  if (const char* msg = picp_vo_plan(h->n_frames, h->frame_off.data(), h->max_obs, h->dim, h->dp, n_seg, first, steps,
                                     opt, caps, &P))
    return picp_set_err(PICP_ERR_ARG, "%s", msg);
  HIP_TRY(hipStreamSynchronize(h->stream));
  vo_free_segments(h);
  HIP_TRY(vo_malloc(h, &h->seg_mem, P.total, "segments"));
  HIP_TRY(hipMemset(h->seg_mem, 0, P.total));  // every table defined before the first run
  char* m = (char*)h->seg_mem;
  h->ev_chunk.assign((size_t)P.max_steps, nullptr);
  for (auto& e : h->ev_chunk) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  h->plan = std::move(P);
  const VoPlan& L = h->plan;
  const int C = L.chains_eff;
  h->part_w.assign((size_t)C, nullptr);
  h->part_e.assign((size_t)2 * C, nullptr);
  for (int c = 0; c < C; ++c) {
    if (L.p_partw[c].bytes) h->part_w[c] = (float4*)(m + L.p_partw[c].off);
    if (L.split_c[c]) {
      h->part_e[2 * c] = (float4*)(m + L.p_parte[c].off);
      h->part_e[2 * c + 1] = h->part_e[2 * c] + L.cap_e[c];
    }
  }
  h->part_p = L.p_partp.bytes ? (float4*)(m + L.p_partp.off) : nullptr;
  HIP_TRY(hipMemcpy(m + L.p_segs.off, L.segs.data(), L.p_segs.bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(m + L.p_boot.off, boot_poses, L.p_boot.bytes, hipMemcpyHostToDevice));
  if (!L.pprobs.empty())
    HIP_TRY(hipMemcpy(m + L.p_pprobs.off, L.pprobs.data(), L.p_pprobs.bytes, hipMemcpyHostToDevice));
  vo_fill_args(h, prm);
  const int rc = vo_track_alloc(h);
  return rc != PICP_OK ? rc : vo_tlog_alloc(h);
}

// frame->next match problems [p0, p1) on stream st, in launches of at most VO_MAX_GRID_Y problems
static hipError_t vo_frame_match(picp_vo* h, hipStream_t st, size_t p0, size_t p1) {
  hipError_t e = hipSuccess;
  for (; p0 < p1 && e == hipSuccess; p0 += VO_MAX_GRID_Y) {
    const int np = (int)std::min<size_t>(VO_MAX_GRID_Y, p1 - p0);
    // the split planned for this launch at set_segments (a launch it did not plan runs unsplit)
    auto it = std::lower_bound(h->plan.ks_p.begin(), h->plan.ks_p.end(), std::make_pair(p0, 0));
    const int ks = (it != h->plan.ks_p.end() && it->first == p0) ? it->second : 1;
    e = picp_launch_match_mfma(st, np, h->max_obs, h->desc_d, h->desc_d, h->obs_h, h->obs_n1, h->obs_h,
                               h->obs_n1, h->obs_n2, h->pprobs_d + p0, h->dim, VO_MATCH_DIST, VO_MATCH_RATIO,
                               h->pm_bi, h->pm_bd, h->pm_sd, h->pm_acc, h->opt.accept_only, ks, h->part_p, h->plan.cap_p);
  }
  return e;
}

#ifdef PICP_VO_DIAG
// Diagnostic build only (tools/vo_snap.py): after step t's PICP launch over segments [s0, s1),
// copy its problems, initial and final states and SoA planes into snapshot t (layout:
// picp_vo_debug_snap_bytes).  Copies run on the launch's stream, so they see exactly the block
// kernel's inputs and outputs.
static size_t vo_snap_step_bytes(const picp_vo* h) {
  return (size_t)h->plan.n_seg * (sizeof(PicpProblem) + 2 * sizeof(PicpState) + 5 * (size_t)h->plan.cap_c * sizeof(float));
}
static hipError_t vo_snap(picp_vo* h, hipStream_t st, int t, int s0, int s1) {
  if (!h->snap) return hipSuccess;
  const VoArgs& V = h->vargs;
  char* d = h->snap + (size_t)t * vo_snap_step_bytes(h);
  const size_t ns = (size_t)h->plan.n_seg, k = (size_t)(s1 - s0);
  hipError_t e = hipMemcpyAsync(d + s0 * sizeof(PicpProblem), V.probs + s0, k * sizeof(PicpProblem),
                                hipMemcpyDeviceToDevice, st);
  d += ns * sizeof(PicpProblem);
  if (e == hipSuccess)
    e = hipMemcpyAsync(d + s0 * sizeof(PicpState), V.st_in + s0, k * sizeof(PicpState), hipMemcpyDeviceToDevice, st);
  d += ns * sizeof(PicpState);
  if (e == hipSuccess)
    e = hipMemcpyAsync(d + s0 * sizeof(PicpState), V.st_out + s0, k * sizeof(PicpState), hipMemcpyDeviceToDevice, st);
  d += ns * sizeof(PicpState);
  const float* planes[5] = {V.X, V.Y, V.Z, V.U, V.V};
  for (int q = 0; q < 5 && e == hipSuccess; ++q)
    e = hipMemcpyAsync(d + ((size_t)q * ns + s0) * h->plan.cap_c * sizeof(float), planes[q] + (size_t)s0 * h->plan.cap_c,
                       k * h->plan.cap_c * sizeof(float), hipMemcpyDeviceToDevice, st);
  return e;
}
extern "C" int picp_vo_debug_snap_bytes(picp_vo_t* h, int64_t* per_step, int* n_steps) {
  CHECK_ARG(h && per_step && n_steps && h->plan.n_seg > 0, "picp_vo_debug_snap_bytes: bad argument");
  *per_step = (int64_t)vo_snap_step_bytes(h);
  *n_steps = h->plan.max_steps;
  return PICP_OK;
}
extern "C" int picp_vo_debug_snap_set(picp_vo_t* h, void* dev_buf) {
  CHECK_ARG(h, "picp_vo_debug_snap_set: bad argument");
  h->snap = (char*)dev_buf;
  vo_drop_graph(h);  // re-capture with (or without) the copies
  return PICP_OK;
}
#endif

// the whole sequence on the handle's stream.  With overlap on, the frame->next match chunks
// 1.. run on the side stream (forked after chunk 0, joined by each step's append, which waits
// for its own chunk): the step chain is a string of latency-bound one-block-per-segment
// kernels, and the throughput-bound match chunks fill the CUs it leaves idle.
static hipError_t vo_enqueue(picp_vo* h) {
#ifdef PICP_VO_DIAG
  // diagnostic build only (wrong results; never the shipped library): PICP_VO_DIAG_SKIP bit 1
  // gather, 2 append, 4 PICP, 8 world match launches left out of the sequence
  static const int skip = [] {
    const char* e = getenv("PICP_VO_DIAG_SKIP");
    return e ? atoi(e) : 0;
  }();
#else
  constexpr int skip = 0;
#endif
  const size_t nck = h->plan.chunk_off.size() - 1;
  const bool ov = h->opt.overlap && nck > 1;
  // track counters: zeroed before anything of the run (the chains' streams fork from this one)
  const bool track = h->track && h->track_d && h->track_slots >= h->plan.map_slots;
  ClsArgs targs;
  memset(&targs, 0, sizeof(targs));
  memcpy(targs.K, h->K, sizeof(targs.K));
  targs.maxx = h->pargs.maxx;
  targs.maxy = h->pargs.maxy;
  targs.threshold = h->pargs.threshold;
  if (track) {
    hipError_t ez = hipMemsetAsync(h->track_d, 0, 2 * (size_t)h->track_slots * sizeof(int32_t), h->stream);
    if (ez != hipSuccess) return ez;
  }
  hipError_t e = vo_frame_match(h, h->stream, 0, ov ? h->plan.chunk_off[1] : h->plan.chunk_off[nck]);
  if (e == hipSuccess && ov) {
    e = hipEventRecord(h->ev_fork, h->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(h->side, h->ev_fork, 0);
    for (size_t k = 1; k < nck && e == hipSuccess; ++k) {
      e = vo_frame_match(h, h->side, h->plan.chunk_off[k], h->plan.chunk_off[k + 1]);
      if (e == hipSuccess) e = hipEventRecord(h->ev_chunk[k], h->side);
    }
  }
  if (e == hipSuccess && !(skip & 2)) e = picp_launch_vo_append(h->stream, &h->vargs, -1);
  // the track log: after every append, while wm_* and pairs are still that step's
  const bool tlog = h->tlog && h->tlog_mem && !(skip & 2);
  if (e == hipSuccess && tlog) e = picp_launch_vo_tracklog(h->stream, &h->vargs, -1, &h->tl);
  const int C = std::min(h->plan.chains_eff, h->plan.n_seg);
  // step u's early world-match part of chain c (the map as step u-2's append left it) on the
  // chain's early stream; its ranges go to scratch slots 0.. of buffer u & 1
  auto early_part = [&](int c, const VoArgs& V, int u) {
    hipStream_t es = h->estream[c];
    const int p = u & 1;
    hipError_t r = hipSuccess;
    if (!(skip & 8))
      r = picp_launch_match_mfma_parts(es, V.n_seg, h->max_obs, h->desc_d, V.map_desc, h->obs_h, h->obs_n1,
                                       V.map_h, V.map_n1, V.map_n2, V.eprobs + (size_t)p * h->plan.n_seg + V.seg0,
                                       h->dim, VO_MATCH_DIST, VO_MATCH_RATIO, h->opt.accept_only, h->plan.ks_w[c], 0,
                                       h->part_e[2 * c + p], h->plan.cap_e[c]);
    if (r == hipSuccess) r = hipEventRecord(h->ev_early[2 * c + p], es);
    return r;
  };

  // one world-match launch over chain c's segments [s0, s0 + n): tables probs (+ s0)
  auto world_match = [&](hipStream_t st, const VoArgs& V, const MatchProblem* probs, int c) {
    return picp_launch_match_mfma(st, V.n_seg, h->max_obs, h->desc_d, V.map_desc, h->obs_h, h->obs_n1, V.map_h,
                                  V.map_n1, V.map_n2, probs + V.seg0, h->dim, VO_MATCH_DIST, VO_MATCH_RATIO,
                                  h->wm_bi, h->wm_bd, h->wm_sd, h->wm_acc, h->opt.accept_only,
                                  h->part_w[c] ? h->plan.ks_w[c] : 1, h->part_w[c], h->plan.cap_w[c]);
  };
#ifdef PICP_VO_DIAG
  const bool fused = false;  // vo_snap and PICP_VO_DIAG_SKIP need the gather's planes and launch
#else
  const bool fused = h->fuse && picp_vo_block_fusable(h->plan.npt, h->max_obs);
#endif
  if (e == hipSuccess && C > 1) e = hipEventRecord(h->ev_cj[0], h->stream);  // fork
  // the chains' launches are enqueued step by step, chain after chain within a step: enqueued
  // chain after chain, every later chain's first launch waited on the host for the earlier
  // chains' whole sequence (~120 launches each), which is how long the GPU ran without it at the
  // start of a timed region.  Each stream's own order, and so every result, is unchanged.
  std::vector<hipStream_t> cst((size_t)C);
  std::vector<VoArgs> cv((size_t)C, h->vargs);
  std::vector<int> csteps((size_t)C, 0);
  int max_steps = 0;
  for (int c = 0; c < C; ++c) {
    cst[c] = (c == 0) ? h->stream : h->cstream[c];
    const int s0 = (int)((int64_t)h->plan.n_seg * c / C), s1 = (int)((int64_t)h->plan.n_seg * (c + 1) / C);
    cv[c].seg0 = s0;
    cv[c].n_seg = s1 - s0;
    for (int s = s0; s < s1; ++s) csteps[c] = std::max(csteps[c], (int)h->plan.segs[s].steps);
    max_steps = std::max(max_steps, csteps[c]);
  }

  for (int t = 0; t < max_steps && e == hipSuccess; ++t) {
    for (int c = 0; c < C && e == hipSuccess; ++c) {
      if (t >= csteps[c]) continue;
      hipStream_t st = cst[c];
      const VoArgs& V = cv[c];
      const int s0 = V.seg0, s1 = V.seg0 + V.n_seg;
      (void)s1;
      // chain c starts after chain c-1's first world match (enqueued just before, at t = 0)
      if (t == 0 && c > 0) e = hipStreamWaitEvent(st, (h->phase ? h->ev_ph[c - 1] : h->ev_cj[0]), 0);
      const bool sp = h->plan.split_c[c] && t >= 1;
      if (sp) {
        // the late part into the slot after the early ranges, then the merge of both
        const int p = t & 1;
        e = hipStreamWaitEvent(st, h->ev_early[2 * c + p], 0);
        if (e == hipSuccess && !(skip & 8))
          e = picp_launch_match_mfma_parts(st, V.n_seg, h->max_obs, h->desc_d, V.map_desc, h->obs_h, h->obs_n1,
                                           V.map_h, V.map_n1, V.map_n2, V.lprobs + s0, h->dim, VO_MATCH_DIST,
                                           VO_MATCH_RATIO, h->opt.accept_only, 1, h->plan.ks_w[c], h->part_e[2 * c + p],
                                           h->plan.cap_e[c]);
        if (e == hipSuccess && !(skip & 8))
          e = picp_launch_match_merge(st, V.eprobs + (size_t)p * h->plan.n_seg + s0, V.n_seg, h->max_obs, h->plan.ks_w[c],
                                      h->plan.ks_w[c], h->part_e[2 * c + p], h->plan.cap_e[c], VO_MATCH_DIST, VO_MATCH_RATIO,
                                      h->wm_bi, h->wm_bd, h->wm_sd, h->wm_acc);
      } else if (e == hipSuccess && !(skip & 8)) {
        e = world_match(st, V, h->wprobs_d, c);
      }
      // step t+1's early part (the map as step t-1's append left it), started once this step's
      // match is merged: it runs beside this step's latency-bound PICP kernel and append rather
      // than beside the next step's late part and merge (round 6, profiles/r06/t15/)
      if (h->plan.split_c[c] && t + 1 < csteps[c] && e == hipSuccess) {
        e = hipEventRecord(h->ev_app[c], st);
        if (e == hipSuccess) e = hipStreamWaitEvent(h->estream[c], h->ev_app[c], 0);
        if (e == hipSuccess) e = early_part(c, V, t + 1);
      }
      if (e == hipSuccess && t == 0 && C > 1 && c + 1 < C) e = hipEventRecord(h->ev_ph[c], st);
      if (fused) {
        if (e == hipSuccess && !(skip & 4)) e = picp_launch_vo_block(st, &V, t, h->plan.npt, &h->pargs, h->max_obs);
      } else {
        if (e == hipSuccess && !(skip & 1)) e = picp_launch_vo_gather(st, &V, t);
        if (e == hipSuccess && !(skip & 4))
          e = picp_launch_block(st, V.n_seg, h->plan.npt, V.X, V.Y, V.Z, V.U, V.V, &h->pargs, V.probs + s0,
                                V.st_in + s0, (PicpState*)V.st_out + s0, (int)h->max_obs, 1, nullptr, nullptr,
                                nullptr, 0);
      }
#ifdef PICP_VO_DIAG
      if (e == hipSuccess) e = vo_snap(h, st, t, s0, s1);
#endif
      // wm_* and st_out are both this step's here (the append below writes the next step's)
      if (e == hipSuccess && track)
        e = picp_launch_vo_track(st, &V, t, &targs, h->track_d, h->track_d + h->track_slots);
      if (e == hipSuccess && ov && t >= 1) e = hipStreamWaitEvent(st, h->ev_chunk[t], 0);
      if (e == hipSuccess && !(skip & 2)) e = picp_launch_vo_append(st, &V, t);
      if (e == hipSuccess && tlog) e = picp_launch_vo_tracklog(st, &V, t, &h->tl);
    }
  }
  for (int c = 1; c < C && e == hipSuccess; ++c) e = hipEventRecord(h->ev_cj[c], cst[c]);
  for (int c = 1; c < C && e == hipSuccess; ++c) e = hipStreamWaitEvent(h->stream, h->ev_cj[c], 0);  // join
  return e;
}

static int vo_launch_seq(picp_vo* h);

static int vo_launch(picp_vo* h) {
  CHECK_ARG(h && h->plan.n_seg > 0, "picp_vo: no segments set");
  HIP_TRY(hipSetDevice(h->device));
  // a new run: the tracks built from the last one are stale
  if (h->tlog) vo_tlog_free(h, false);
  const int rc = vo_launch_seq(h);
  if (rc == PICP_OK && h->tlog && h->tlog_mem) h->tlog_ran = true;
  return rc;
}

static int vo_launch_seq(picp_vo* h) {
  if (!h->use_graph) {
    HIP_TRY(vo_enqueue(h));
    return PICP_OK;
  }
  if (!h->exec) {
    HIP_TRY(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    hipError_t e = vo_enqueue(h);
    hipGraph_t g = nullptr;
    hipError_t e2 = hipStreamEndCapture(h->stream, &g);
    if (e != hipSuccess || e2 != hipSuccess) {
      if (g) hipGraphDestroy(g);
      return picp_set_err(PICP_ERR_DEVICE, "picp_vo: graph capture failed: %s",
                          hipGetErrorString(e != hipSuccess ? e : e2));
    }
    h->graph = g;
    HIP_TRY(hipGraphInstantiate(&h->exec, g, nullptr, nullptr, 0));
  }
  HIP_TRY(hipGraphLaunch(h->exec, h->stream));
  return PICP_OK;
}

extern "C" int picp_vo_run_async(picp_vo_t* h) { return vo_launch(h); }

extern "C" int picp_vo_sync(picp_vo_t* h) {
  CHECK_ARG(h, "picp_vo_sync: null handle");
  HIP_TRY(hipStreamSynchronize(h->stream));
  return PICP_OK;
}

extern "C" int picp_vo_run(picp_vo_t* h) {
  int rc = vo_launch(h);
  if (rc != PICP_OK) return rc;
  return picp_vo_sync(h);
}

extern "C" int picp_vo_time(picp_vo_t* h, int reps, float* ms_per_run) {
  CHECK_ARG(h && ms_per_run && reps >= 1, "picp_vo_time: bad argument");
  int rc = PICP_OK;
  if (h->use_graph && !h->exec) {  // capture outside the timed events
    rc = vo_launch(h);
    if (rc != PICP_OK) return rc;
  }
  HIP_TRY(hipEventRecord(h->ev0, h->stream));
  for (int r = 0; r < reps; ++r) {
    rc = vo_launch(h);
    if (rc != PICP_OK) return rc;
  }
  HIP_TRY(hipEventRecord(h->ev1, h->stream));
  HIP_TRY(hipEventSynchronize(h->ev1));
  float ms = 0.0f;
  HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  *ms_per_run = ms / reps;
  return PICP_OK;
}

extern "C" int picp_vo_get_poses(picp_vo_t* h, float* poses) {
  CHECK_ARG(h && poses && h->plan.n_seg > 0, "picp_vo_get_poses: bad argument");
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(poses, h->vargs.poses, (size_t)h->plan.n_slots * 16 * sizeof(float), hipMemcpyDeviceToHost));
  return PICP_OK;
}

extern "C" int picp_vo_get_steps(picp_vo_t* h, picp_vo_step* steps) {
  CHECK_ARG(h && steps && h->plan.n_seg > 0, "picp_vo_get_steps: bad argument");
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(steps, h->vargs.steps, (size_t)h->plan.n_slots * sizeof(VoStep), hipMemcpyDeviceToHost));
  return PICP_OK;
}

// The first min(count, cap) rows of each device array to its host destination.
int vo_copy_prefix(int64_t count, int64_t cap, int64_t* n, std::initializer_list<VoRows> arrays) {
  *n = count;
  const int64_t k = std::min(count, std::max<int64_t>(cap, 0));
  for (const VoRows& r : arrays)
    if (r.dst && k) HIP_TRY(hipMemcpy(r.dst, r.src, (size_t)k * r.row_bytes, hipMemcpyDeviceToHost));
  return PICP_OK;
}

// segment seg's map count, once the run is complete
static int vo_map_count(picp_vo* h, int seg, int64_t* mn) {
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(mn, h->vargs.map_n + seg, sizeof(int64_t), hipMemcpyDeviceToHost));
  return PICP_OK;
}

extern "C" int picp_vo_get_map(picp_vo_t* h, int seg, int64_t cap, float* xyz, float* desc, int64_t* n) {
  CHECK_ARG(h && n && h->plan.n_seg > 0 && seg >= 0 && seg < h->plan.n_seg, "picp_vo_get_map: bad argument");
  int64_t mn = 0;
  const int rc = vo_map_count(h, seg, &mn);
  if (rc != PICP_OK) return rc;
  const int64_t off = h->plan.segs[seg].map_off;
  return vo_copy_prefix(mn, cap, n, {{xyz, h->vargs.map_xyz + 3 * off, 3 * sizeof(float)},
                                     {desc, h->vargs.map_desc + off * h->dim, h->dim * sizeof(float)}});
}

extern "C" int picp_vo_set_track_stats(picp_vo_t* h, int enable) {
  CHECK_ARG(h, "picp_vo_set_track_stats: null handle");
  const bool on = enable != 0;
  if (on == h->track) return PICP_OK;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->track = on;
  vo_drop_graph(h);  // the captured sequence has (or lacks) the track launches
  return vo_track_alloc(h);
}

extern "C" int picp_vo_get_map_stats(picp_vo_t* h, int seg, int64_t cap, int32_t* n_matched, int32_t* n_inlier,
                                     int64_t* n) {
  CHECK_ARG(h && n && h->plan.n_seg > 0 && seg >= 0 && seg < h->plan.n_seg, "picp_vo_get_map_stats: bad argument");
  if (!h->track || !h->track_d)
    return picp_set_err(PICP_ERR_STATE, "picp_vo_get_map_stats: tracking is off (picp_vo_set_track_stats)");
  HIP_TRY(hipSetDevice(h->device));
  int64_t mn = 0;
  const int rc = vo_map_count(h, seg, &mn);
  if (rc != PICP_OK) return rc;
  const int64_t off = h->plan.segs[seg].map_off;
  return vo_copy_prefix(mn, cap, n, {{n_matched, h->track_d + off, sizeof(int32_t)},
                                     {n_inlier, h->track_d + h->track_slots + off, sizeof(int32_t)}});
}

extern "C" int picp_vo_debug_matches(picp_vo_t* h, int which, int32_t* dst) {
  CHECK_ARG(h && dst && which >= 0 && which <= 3, "picp_vo_debug_matches: bad argument");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  const int32_t* src[4] = {h->pm_bi, h->pm_acc, h->wm_bi, h->wm_acc};
  if (h->n_obs) HIP_TRY(hipMemcpy(dst, src[which], (size_t)h->n_obs * 4, hipMemcpyDeviceToHost));
  return PICP_OK;
}

extern "C" int picp_vo_debug_guard(picp_vo_t* h, int64_t* bad_bytes, int* bad_buffer) {
  CHECK_ARG(h && bad_bytes && bad_buffer, "picp_vo_debug_guard: bad argument");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  *bad_bytes = 0;
  *bad_buffer = -1;
  std::vector<unsigned char> pad(VO_GUARD);
  for (size_t i = 0; i < h->guards.size(); ++i) {
    const VoGuarded& g = h->guards[i];
    for (int side = 0; side < 2; ++side) {
      const char* src = side ? g.base + VO_GUARD + g.bytes : g.base;
      HIP_TRY(hipMemcpy(pad.data(), src, VO_GUARD, hipMemcpyDeviceToHost));
      int64_t bad = 0;
      for (unsigned char c : pad) bad += (c != VO_GUARD_BYTE);
      if (bad && *bad_buffer < 0) *bad_buffer = (int)(2 * i + side);
      *bad_bytes += bad;
    }
  }
  return PICP_OK;
}

extern "C" int picp_vo_info(picp_vo_t* h, int64_t* n_obs, int64_t* n_slots, int64_t* map_slots, int* npt) {
  CHECK_ARG(h, "picp_vo_info: null handle");
  if (n_obs) *n_obs = h->n_obs;
  if (n_slots) *n_slots = h->plan.n_slots;
  if (map_slots) *map_slots = h->plan.map_slots;
  if (npt) *npt = h->plan.npt;
  return PICP_OK;
}
