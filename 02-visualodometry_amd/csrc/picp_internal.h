// picp_internal.h -- device-visible data layout shared by the HIP kernels and the host
// runtime of libpicp_amd.so.  Not part of the public C-ABI (include/picp_c.h).
//
// HBM layout of a PICP batch (DESIGN.md §Data layout):
//   planes X,Y,Z,U,V : float32 SoA, one plane each, problem p occupies
//                      [prob.offset, prob.offset + prob.n) of every plane; offsets are
//                      multiples of 4 floats so every block streams float4 (dwordx4) loads.
//   PicpArgs         : batch-wide camera/gate/loop parameters, by-value kernel argument.
//   PicpProblem[np]  : ragged batches only: per-problem partition.
//   int4 blkinfo[nb] : ragged batches only: block -> (problem, first item, item count).
//   PicpState[2][np] : ping-pong per-problem solver state (pose + icp_test loop state).
//   float part[2][nb][32] : ping-pong per-block partial sums of the normal equations.
#pragma once
#include <stdint.h>

#include "picp_c.h"        // picp_stats
#include "picp_problem.h"  // PICP_BLOCK, PICP_NPART, PICP_POSE_SETS, PicpProblem, MatchProblem, VoSegment

// partial slot layout
#define PICP_P_H 0                // 21 upper-triangle entries of H (row-major upper)
#define PICP_P_B 21               // 6 entries of b
#define PICP_P_CHI_IN 27
#define PICP_P_CHI_OUT 28
#define PICP_P_N_IN 29
#define PICP_P_N_PROJ 30

// Batch-wide launch arguments, passed BY VALUE (kernel-argument SGPRs: no memory hop).
struct PicpArgs {
  float K[9];            // camera matrix, column-major (src/camera.h:45)
  float maxx, maxy;      // cols-1, rows-1 (src/camera.h:31,33)
  float threshold;       // kernel threshold (src/picp_solver.h:72)
  float damping;         // src/picp_solver.h:73
  float conv_eps;        // exec/icp_test.cpp:91 (negative: never converge)
  int32_t min_inliers;   // src/picp_solver.h:74
  int32_t keep_outliers; // oneRound's keep_outliers
  int32_t max_rounds;    // exec/icp_test.cpp:88
  int32_t uniform;       // 1: problem p = block / nblk_u, items at p*stride_u (no tables)
  int32_t n_u;           // uniform: correspondences per problem
  int32_t nblk_u;        // uniform: blocks per problem
  int32_t ipb;           // items per linearize block
  int64_t stride_u;      // uniform: plane stride between problems (multiple of 4)
};

// 128-byte per-problem solver state
struct PicpState {
  float R[9];          // world-in-camera rotation, column-major
  float t[3];          // world-in-camera translation
  float chi_prev;      // icp_test's prevError (exec/icp_test.cpp:89,106)
  float chi_in;        // stats of the last linearization (chiInliers)
  float chi_out;       // chiOutliers
  int32_t n_in;        // numInliers
  int32_t n_proj;      // correspondences that passed projectPoint
  int32_t rounds;      // oneRound calls executed
  int32_t done;        // loop finished (converged, failed or max_rounds)
  int32_t ok;          // return value of the last oneRound
  int32_t converged;   // icp_test's convergenceReached
  int32_t pad[11];
};

// classify pass (picp_classify.hip): camera, gate and per-item path, by value
struct ClsArgs {
  float K[9];          // camera matrix, column-major
  float maxx, maxy;    // cols-1, rows-1
  float threshold;     // chi2 gate
  int32_t pinhole;     // 1: the pinhole-K operation order (accumulate_pinhole), 0: general K
};

// point refinement (picp_refine.hip): camera, gate and loop parameters, by value
struct RefineArgs {
  float K[9];            // camera matrix, column-major
  float maxx, maxy;      // cols-1, rows-1
  float threshold;       // chi2 gate
  float damping;
  float conv_eps;        // negative: never converge
  int32_t min_inliers;
  int32_t keep_outliers;
  int32_t max_rounds;
  int32_t pinhole;       // set by the launcher (classify_item's camera path)
  int64_t n_points;
};

// one world-in-camera pose of the refiner's table: the rows of [R | t], 48 B (three 16-B loads)
struct RefinePose {
  float4 r0, r1, r2;     // (r00 r01 r02 t0), (r10 r11 r12 t1), (r20 r21 r22 t2)
};

// alternating adjustment (picp_adjust.hip), by value; every pointer is device memory
// The build of the pose-major view of the refiner's point-major tracks.
struct AdjView {
  const int64_t* track_off;  // n_points + 1
  const int32_t* obs_pose;   // per observation (source position)
  const float2* obs_uv;
  int32_t* cnt;              // per pose: observations counted, then the fill's cursor
  int64_t* pose_off;         // n_poses + 1
  int2* tmp;                 // per entry, as the cursors placed it: (source position, point)
  int32_t* view_point;       // per entry, canonical order
  float2* view_uv;
  int64_t n_points, n_obs;
  int32_t n_poses, pad;
};

// One pose step: problem p of the batch is pose movable[p].
struct AdjPose {
  const int32_t* movable;    // n_problems
  const int64_t* pose_off;
  const int64_t* plane_off;  // n_problems: the batch's plane offsets
  const int32_t* view_point;
  const float2* view_uv;
  const float* xyz;          // the current points
  float* X;                  // the batch's SoA planes
  float* Y;
  float* Z;
  float* U;
  float* V;
  PicpState* init;           // the batch's initial states
  RefinePose* rposes;        // the refiner's pose rows
  float* T;                  // the poses as 4x4, 16 floats each
  picp_stats* pose_stats;    // n_poses
  int32_t n_problems, pad;
};

static_assert(sizeof(RefinePose) == 48, "RefinePose must be 48 B");
static_assert(sizeof(PicpState) == 128, "PicpState must be 128 B");

// ---------------------------------------------------------------------------------------
// descriptor matching (picp_match.hip; MatchProblem: picp_problem.h).
// Every PICP device translation unit is compiled WITHOUT packed-FP32 VALU instructions
// (v_pk_fma/mul/add_f32): hipcc_nopk.sh passes -target-feature -packed-fp32-ops to the whole
// device compile.  On MI355X (gfx950, ROCm 7.2) the compiler's packed code for apply_update gave
// lanes 48-63 of a wave results that differ from lanes 0-47 on identical inputs whenever an MFMA
// kernel ran on the same CU (tools/ubench/permlane_stress.hip victim 9 beside an MFMA kernel; none
// alone or beside LDS / FP32 / FP64 / transcendental / DPP / permlane load; the scalar build of the
// same function, victim 23, none).  In the VO sequence that made the PICP poses depend on whether
// the matcher ran beside the block kernel.  The flag is TU-wide on purpose: a
// per-kernel target("no-packed-fp32-ops") attribute stops HIP's header functions (__syncthreads,
// ...) from inlining into the kernel, and the calls cost C2 18 % and C5 80 % (round-3 pass).

// ---------------------------------------------------------------------------------------
// essential-matrix bootstrap (picp_essential.hip; src/cam.cpp:37-91), by value
struct EssArgs {
  int32_t n_problems;
  int32_t max_iters;   // findEssentialMat maxIters (RANSAC hypotheses scored per problem)
  double fx, fy, cx, cy;
  double prob;         // findEssentialMat prob
  double threshold;    // findEssentialMat threshold (pixels)
  double dist;         // recoverPose distanceThresh
};

// ---------------------------------------------------------------------------------------
// absolute pose by P3P RANSAC (picp_pnp.hip), by value
struct PnpArgs {
  float K[9];            // camera matrix, column-major
  float maxx, maxy;      // cols-1, rows-1
  float threshold;       // chi2 gate (squared pixels)
  int32_t pinhole;       // classify_item's camera path (set by the launcher)
  double Kinv[9];        // K^-1, row-major (the back-projection of the three sampled pixels)
  uint64_t seed;
  int32_t n_problems;
  int32_t hyp;           // hypotheses per problem
  int32_t min_inliers;
  int32_t prob0;         // batch position of problem 0 (the sampling function's problem index)
};

// The correspondences of a PnP batch, packed (xyz float3, uv float2: x = xyz, y = xyz + 1,
// z = xyz + 2, sx = 3, ...) or as the planes of a picp_batch (strides 1).  Correspondence j of
// problem i is element base[i] + j; offs (n_problems + 1) gives the sizes.
struct PnpItems {
  const float* x;
  const float* y;
  const float* z;
  const float* u;
  const float* v;
  int32_t sx, su;        // element strides of x/y/z and of u/v
  const int64_t* offs;
  const int64_t* base;
};

// 3D-3D alignment by Sim(3) RANSAC (picp_sim3.hip), by value
struct Sim3Args {
  float threshold;       // squared distance in dst units, strict
  int32_t with_scale;    // 0: rigid, c = 1
  uint64_t seed;
  int32_t n_problems;
  int32_t hyp;           // hypotheses per problem
  int32_t min_inliers;
  int32_t refits;
  int32_t prob0;         // batch position of problem 0 (the sampling function's problem index)
  int32_t fit_only;      // the refit kernel alone over a given set (picp_sim3_fit_batch)
};

// The pairs of a Sim(3) batch: packed float3 (x = src, y = src + 1, z = src + 2, stride 3) or any
// other element stride.  Pair j of problem i is element base[i] + j of both sets; offs
// (n_problems + 1) gives the sizes and the position of the problem's mask bytes.
struct Sim3Items {
  const float* px;
  const float* py;
  const float* pz;
  const float* qx;
  const float* qy;
  const float* qz;
  int32_t sp, sq;        // element strides of the src and of the dst coordinates
  const int64_t* offs;
  const int64_t* base;
};

// ---------------------------------------------------------------------------------------
// device-resident VO sequence (picp_vo.hip; VoSegment: picp_problem.h)
struct VoStep {     // per pose slot; slot 0 of a segment = the bootstrap
  int32_t n_corr;   // map correspondences of the frame (PICP input size)
  int32_t n_in;     // inliers of the last PICP round
  int32_t rounds;   // oneRound calls
  int32_t n_new;    // points triangulated and appended after this frame
  float chi_in;
  float chi_out;
  int32_t converged;
  int32_t n_proj;
};

struct VoArgs {     // by value; every pointer is device memory
  float K[9];
  int32_t dim;
  int32_t n_seg;             // segments of this launch: seg0 .. seg0 + n_seg - 1
  int32_t seg0;
  const int64_t* frame_off;  // n_frames + 1
  const float2* uv;          // per observation
  const float* desc;         // per observation, dim floats
  const VoSegment* segs;
  const float* boot;         // per segment: camera-in-world poses of f0 and f0+1 (2 x 16)
  const int32_t* pm_bi;      // frame f -> f+1 matches, indexed by f's observation
  const int32_t* pm_acc;
  const int32_t* wm_bi;      // next frame -> map matches, indexed by the frame's observation
  const int32_t* wm_acc;
  float* map_xyz;            // 3 per slot
  float* map_desc;           // dim per slot
  int64_t* map_n;            // per segment
  float* X;                  // PICP SoA planes, segment s at s * cap_c
  float* Y;
  float* Z;
  float* U;
  float* V;
  int64_t cap_c;
  PicpProblem* probs;
  PicpState* st_in;
  const PicpState* st_out;
  MatchProblem* wprobs;      // next step's world-match problem of each segment
  // the world match split by map age (split != 0; picp_vo_runtime.cpp): the append of step t
  // writes the LATE part of step t + 1 (the points it added) and the EARLY part of step t + 2
  // (the map as it leaves it), the latter double-buffered by step parity:
  // eprobs[(step & 1) * seg_all + s]
  MatchProblem* lprobs;
  MatchProblem* eprobs;
  int32_t split;
  int32_t seg_all;           // segments of the handle (eprobs' parity stride)
  float* poses;              // 16 per slot, camera-in-world, column-major
  VoStep* steps;
  int2* pairs;               // append scratch: segment s at s * cap_c
  // matcher prep (picp_match.hip): fp16 rows of dp = 16*kch halves + two guard norms
  int32_t dp;
  const _Float16* obs_h;
  const float* obs_n1;
  const float* obs_n2;
  _Float16* map_h;
  float* map_n1;
  float* map_n2;
};

// ---------------------------------------------------------------------------------------
// observation tracks of the VO sequence (picp_vo_tracks.hip), by value
// What a run records with the track log on: vo_tracklog_kernel after every append.
struct VoTrackLog {
  int32_t* mlog;           // per segment, dense: for observation i of frame f0+t+1 the accepted map
                           // index or -1, at log_off[s] + (frame_off[f0+t+1] - frame_off[f0+1]) + i
  const int64_t* log_off;  // per segment
  int32_t* cre_c;          // per map slot: the step that created the point (bootstrap: 0), ...
  int32_t* cre_x;          // ... its observation x in frame f0+c and ...
  int32_t* cre_y;          // ... y in frame f0+c+1 (indices in the frame)
};

// The CSR build after a run: points are packed segment-major (segment s at pt_base[s], its used
// map prefix only).
struct VoTrackCsr {
  VoTrackLog L;
  const int64_t* frame_off;
  const float2* uv;
  const VoSegment* segs;
  const float* map_xyz;
  const float* poses;       // 16 per slot, camera-in-world
  const int64_t* pt_base;   // n_seg + 1
  int32_t* cnt;             // per point: matches counted, then the fill's cursor
  int64_t* rel;             // per point: exclusive scan of the track lengths inside its segment
  int64_t* seg_tot;         // per segment: its observations
  const int64_t* seg_base;  // per segment: first observation (host prefix of seg_tot)
  int64_t* track_off;       // n_points + 1
  int64_t* obs_index;       // per observation: global observation index
  int32_t* obs_slot;        // pose slot inside the segment
  int32_t* obs_pose;        // slot0 + obs_slot
  float2* obs_uv;
  float* xyz0;              // the packed map, 3 per point
  float* pose_wc;           // 16 per slot, world-in-camera
  RefinePose* rposes;       // the refiner's table of the same poses
  int64_t n_points, n_obs, n_slots;
  int32_t n_seg, max_steps;
  int64_t max_pts;          // the largest segment map
};
