/*
 * picp_c.h -- C-ABI of libpicp_amd.so, the MI355X (gfx950) PICP hot path.
 *
 * This is the drop-in boundary for the reference's pr::PICPSolver / pr::Camera
 * (llepa/02-VisualOdometry; paths below are relative to the reference repo root).  Plain
 * pointers and sizes only; no C++ or framework types.  Every call returns an int status
 * (PICP_OK == 0); nothing throws across the ABI.  picp_last_error() returns a
 * thread-local description of the last failure.
 *
 * Memory layouts (identical to the reference's Eigen types):
 *   pose  T_wc[16] : 4x4 float COLUMN-major (Eigen::Isometry3f), the world-in-camera pose
 *                    (pr::Camera::worldInCameraPose, src/camera.h:51).
 *   K[9]           : 3x3 float column-major (Eigen::Matrix3f, src/camera.h:45).
 *   world xyz      : float[3*n] packed (Vector3fVector, src/defs.h:22).
 *   image uv       : float[2*n] packed (Vector2fVector, src/defs.h:23).
 *   pairs          : int32[2*m] (first = image index, second = world index)
 *                    (IntPairVector, src/defs.h:209-211; src/picp_solver.cpp:65-66).
 *   P[12]          : 3x4 float ROW-major projection matrix (cv::Mat, src/cam.cpp:111-112).
 *
 * Threading: a handle is bound to one HIP device and owns one HIP stream; a handle must
 * not be used from two threads at once (the reference solver is single-threaded too).
 */
#ifndef PICP_C_H
#define PICP_C_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PICP_ABI_VERSION 3

/* status codes */
#define PICP_OK 0
#define PICP_ERR_ARG -1      /* null pointer / bad size / bad parameter           */
#define PICP_ERR_DEVICE -2   /* HIP runtime error (see picp_last_error)           */
#define PICP_ERR_RANGE -3    /* a correspondence index is out of range            */
#define PICP_ERR_STATE -4    /* call order violated (e.g. round before set_points)*/
#define PICP_ERR_NOMEM -5    /* device allocation failed                          */
#define PICP_TOO_FEW_INLIERS 1 /* oneRound returned false: n_in < min_inliers
                                  (src/picp_solver.cpp:97-100); pose not updated   */

typedef struct picp_handle picp_t;
typedef struct picp_batch picp_batch_t;

/* Solver statistics, the reference's accessors plus the icp_test loop outcome. */
typedef struct picp_stats {
  float chi_in;       /* PICPSolver::chiInliers  (src/picp_solver.h:47)  */
  float chi_out;      /* PICPSolver::chiOutliers (src/picp_solver.h:50)  */
  int32_t n_in;       /* PICPSolver::numInliers  (src/picp_solver.h:53)  */
  int32_t ok;         /* return value of the last oneRound               */
  int32_t rounds;     /* oneRound calls executed                          */
  int32_t converged;  /* exec/icp_test.cpp:92 convergenceReached          */
  int32_t n_projected;/* correspondences that passed projectPoint         */
  int32_t reserved;
} picp_stats;

/* Solver parameters. picp_params_default() gives the reference's values. */
typedef struct picp_params {
  float threshold;      /* kernel threshold; PICPSolver ctor default 1000 (src/picp_solver.cpp:14),
                           icp_test uses 3000 (exec/icp_test.cpp:86)                          */
  float damping;        /* 1 (src/picp_solver.cpp:11)                                          */
  int32_t min_inliers;  /* 0 (src/picp_solver.cpp:12)                                          */
  int32_t keep_outliers;/* 0 in icp_test (exec/icp_test.cpp:95)                                */
  int32_t max_rounds;   /* 50 (exec/icp_test.cpp:88)                                           */
  float conv_eps;       /* 1e-5 relative chi_in change (exec/icp_test.cpp:91); < 0 disables   */
} picp_params;

void picp_params_default(picp_params* p);
int picp_abi_version(void);
const char* picp_last_error(void);
int picp_device_count(int* n);

/* ---------------- single-problem handle: the pr::PICPSolver drop-in ---------------- */

/* Replaces PICPSolver() + the Camera passed to init (src/picp_solver.cpp:8-15,17-20). */
int picp_create(picp_t** out, int device, int rows, int cols, const float K[9]);
int picp_destroy(picp_t* h);
int picp_set_camera(picp_t* h, int rows, int cols, const float K[9]);
/* Replaces PICPSolver's implicit copy constructor (src/picp_solver.h:21-82: every member is
 * copied, the world/image pointers included, so the copy keeps solving the same problem).  The
 * new handle is on the same device with its own copies of the points, the correspondences, the
 * camera and the pose. */
int picp_clone(const picp_t* src, picp_t** out);

/* Replaces PICPSolver::init's world/image arguments (src/picp_solver.cpp:17-23).  The
 * arrays are COPIED to device memory (the reference stores raw pointers; its icp_test
 * passes temporaries, exec/icp_test.cpp:81-85). */
int picp_set_points(picp_t* h, const float* world_xyz, int64_t n_world,
                    const float* image_uv, int64_t n_image);

/* Correspondences for the following rounds (the argument of PICPSolver::oneRound,
 * src/picp_solver.h:59).  Indices are range-checked (PICP_ERR_RANGE); an identical
 * repeated array is detected and not re-uploaded. */
int picp_set_correspondences(picp_t* h, const int32_t* pairs, int64_t m);

/* Camera::setWorldInCameraPose / worldInCameraPose (src/camera.h:51-52) */
int picp_set_pose(picp_t* h, const float T_wc[16]);
int picp_get_pose(picp_t* h, float T_wc[16]);

/* PICPSolver::oneRound (src/picp_solver.cpp:93-105): linearize + damping + min-inlier
 * check + LDLT solve + left update.  Returns PICP_OK, or PICP_TOO_FEW_INLIERS when the
 * reference returns false.  stats may be NULL. */
int picp_one_round(picp_t* h, float threshold, float damping, int min_inliers,
                   int keep_outliers, picp_stats* stats);

/* The whole exec/icp_test.cpp:88-107 loop fused on the device (one graph launch, no host
 * round trip per round). */
int picp_solve(picp_t* h, const picp_params* params, picp_stats* stats);

/* Linearize at the current pose without updating it (H 6x6 column-major, b 6), for
 * parity testing against PICPSolver::linearize (src/picp_solver.cpp:56-91). */
int picp_linearize(picp_t* h, float threshold, int keep_outliers, double H[36], double b[6],
                   picp_stats* stats);

/* ---------------- which correspondences a pose rests on (read-only observation) ---------------- */

/* state of one correspondence at a pose (src/picp_solver.cpp:62-89) */
#define PICP_CORR_SKIPPED 0  /* projectPoint returned false: the reference counts it nowhere */
#define PICP_CORR_INLIER  1  /* projected and !(chi2 > threshold)  (strict gate, NaN passes) */
#define PICP_CORR_OUTLIER 2  /* projected and chi2 > threshold                               */

/* Classify the current correspondences (index k = correspondence k of picp_set_correspondences)
 * at the handle's current pose (picp_get_pose), with the solve kernels' own projection, bounds
 * test, error and chi2 (bit-identical to errorAndJacobian at that pose).  Needs points and
 * correspondences set (PICP_ERR_STATE otherwise); m = 0 gives counts 0/0/0.  Blocking.  Changes
 * neither the pose nor the stats nor the bits of a later solve.  Every output but counts may be
 * NULL.  inlier_idx: only its first counts[1] entries are written. */
int picp_classify(picp_t* h, float threshold,
                  uint8_t* state,       /* m,   nullable */
                  float* chi2,          /* m,   nullable; -1 where SKIPPED */
                  float* proj_uv,       /* 2*m, nullable; (-1,-1) where SKIPPED (Camera::projectPoints' point_outside) */
                  int32_t* inlier_idx,  /* m,   nullable; correspondence indices of the inliers, ascending */
                  int64_t counts[3]);   /* required: number of SKIPPED / INLIER / OUTLIER */

/* ---------------- batched independent problems (frames) on one device ---------------- */

/* corr_offsets[n_problems+1]: problem i owns correspondences [off[i], off[i+1]) of the
 * arrays given to picp_batch_set_data.  Camera shared by all problems. */
int picp_batch_create(picp_batch_t** out, int device, int n_problems,
                      const int64_t* corr_offsets, int rows, int cols, const float K[9]);
int picp_batch_destroy(picp_batch_t* b);

/* Matched correspondences, already gathered: xyz[3*total] world points and uv[2*total]
 * image points (pairs (i,i)); copied to the device SoA planes. */
int picp_batch_set_data(picp_batch_t* b, const float* xyz, const float* uv);
/* Device-resident variant: the five SoA planes of length total, already on this device
 * (e.g. produced by a previous kernel); copied device-to-device. */
int picp_batch_set_data_device(picp_batch_t* b, const float* d_x, const float* d_y,
                               const float* d_z, const float* d_u, const float* d_v);

/* The initial poses of the following solves.  They also become the batch's current poses: what
 * picp_batch_get_poses returns until the next solve completes (before, it returned the last
 * solve's poses, or zeros before any solve); the stats are not touched. */
int picp_batch_set_poses(picp_batch_t* b, const float* T_wc /* 16*n_problems */);
int picp_batch_get_poses(picp_batch_t* b, float* T_wc /* 16*n_problems */);
int picp_batch_get_stats(picp_batch_t* b, picp_stats* stats /* n_problems */);

/* Fused icp_test loop for every problem; blocking. */
int picp_batch_solve(picp_batch_t* b, const picp_params* params);
/* Same, enqueued on the batch's stream (graph replay); pair with picp_batch_sync. */
int picp_batch_solve_async(picp_batch_t* b, const picp_params* params);
int picp_batch_sync(picp_batch_t* b);

/* Run `reps` back-to-back fused solves on the batch's stream between two HIP events and nothing
 * else.  total_ms = event time of the whole region; launch_us (nullable) = mean launch period
 * of the dominant kernel in it (total / (reps x launches per solve): max_rounds round launches in
 * graph mode, one launch otherwise).  Blocking; results readable with picp_batch_get_poses/stats
 * afterwards. */
int picp_batch_time(picp_batch_t* b, const picp_params* params, int reps, float* total_ms,
                    float* launch_us);
/* Diagnostic: one solve with an event pair around every launch (graph mode: the mean over its
 * round launches; otherwise the single launch), an upper bound that adds the event overhead. */
int picp_batch_time_single(picp_batch_t* b, const picp_params* params, float* us);
/* Introspection: total correspondences, blocks per launch, and the execution mode chosen for
 * the batch: 0 = one launch per GN round replayed from a hipGraph (any batch); 1 = the whole
 * loop in one persistent launch; 2 = one block (or a few cooperating blocks) per problem
 * (env PICP_MODE=graph|persistent|block forces one where the batch is eligible). */
int picp_batch_info(picp_batch_t* b, int64_t* total_corr, int* n_blocks, int* mode);
/* Co-residency of the layout's cross-block hand-off launch (persistent mode, or block mode with
 * two or four blocks per problem): grid = its blocks, resident = blocks the device holds at once
 * for that kernel (occupancy query x CUs; 0/0 when the layout considered none).  Such a launch is
 * used only when grid <= resident; if a hand-off wait still times out (CUs held by other work),
 * the solve is re-run without hand-offs and the batch keeps that layout: fallbacks counts it. */
int picp_batch_residency(picp_batch_t* b, int* grid, int* resident, int* fallbacks);

/* picp_classify for every problem of the batch in one pass (PICP_CORR_* per correspondence, in
 * the caller's packed order).  T_wc: the poses to classify at, or NULL for the batch's current
 * poses: what picp_batch_get_poses returns now, i.e. the last completed solve's results, or the
 * poses of a picp_batch_set_poses made since (which that call now also reports).  inlier_idx
 * holds, problem after problem, the ascending indices of each problem's inliers relative to its
 * first correspondence: problem p's are inlier_idx[inlier_off[p] .. inlier_off[p+1]).  counts[3p
 * .. 3p+2] = SKIPPED / INLIER / OUTLIER of problem p.  Blocking; read-only like picp_classify. */
int picp_batch_classify(picp_batch_t* b, float threshold,
                        const float* T_wc,    /* 16*n_problems, or NULL = what picp_batch_get_poses returns now */
                        uint8_t* state, float* chi2,          /* total, caller's packed order (corr_offsets); nullable */
                        int64_t* inlier_off,  /* n_problems+1, nullable */
                        int32_t* inlier_idx,  /* total, nullable; per problem ascending, relative to the problem's first correspondence */
                        int64_t* counts);     /* 3*n_problems, required */

/* device time of one classify pass (kernels only, no copies), mean of reps; diagnostic.  The pass
 * runs at the batch's current poses and writes what the batch's last picp_batch_classify asked
 * for (state and the inlier indices always; chi2 if that call passed a chi2 array). */
int picp_batch_classify_time(picp_batch_t* b, float threshold, int reps, float* us_per_pass);

/* ---------------- batch split across GPUs: one process per GPU ---------------- */

/* The node's GPUs each run one process with its own picp_batch holding a contiguous shard of the
 * independent problems; the only collective is one RCCL all-gather (over xGMI) of the results.
 * The communicator wraps an RCCL communicator created from a 128-byte unique id that rank 0 makes
 * with picp_comm_unique_id and the launcher hands to every rank out of band.  librccl is loaded
 * on the first picp_comm_* call (dlopen), so single-GPU use never needs it. */
#define PICP_COMM_ID_BYTES 128
typedef struct picp_comm picp_comm_t;

/* Contiguous balanced split of n_items over world ranks: rank owns [*first, *last); sizes differ
 * by at most one (lower ranks take the remainder). */
int picp_shard_range(int64_t n_items, int world, int rank, int64_t* first, int64_t* last);
/* The layout picp_batch_allgather moves: every rank contributes its shard padded to
 * picp_shard_pad(n_items, world) = ceil(n_items / world) items, the all-gather concatenates them
 * in rank order, and picp_shard_unpack turns that padded buffer (world * pad items of item_bytes
 * each) back into the n_items items in problem order (rank r's items at picp_shard_range's
 * [first, last)).  Host memory, no device: the CPU tests drive it for ragged shards. */
int64_t picp_shard_pad(int64_t n_items, int world);
int picp_shard_unpack(int64_t n_items, int world, int64_t item_bytes, const void* padded, void* out);
int picp_comm_unique_id(uint8_t id[PICP_COMM_ID_BYTES]);
/* Collective over the world: blocks until every rank has joined. */
int picp_comm_create(picp_comm_t** out, int device, int world, int rank,
                     const uint8_t id[PICP_COMM_ID_BYTES]);
int picp_comm_destroy(picp_comm_t* c);
int picp_comm_info(picp_comm_t* c, int* device, int* world, int* rank);
/* Element-wise max over ranks of n (1..64) host doubles, in place (e.g. the timed region's wall
 * time); blocking. */
int picp_comm_allreduce_max(picp_comm_t* c, double* values, int n);
int picp_comm_barrier(picp_comm_t* c);
/* After a solve of this rank's batch (which must hold exactly picp_shard_range(n_total, world,
 * rank)'s problems): completes it, then all-gathers every rank's per-problem results so that
 * T_all[16 * n_total] (column-major camera poses, problem order) and st_all[n_total] (nullable)
 * hold all of them on every rank.  Collective: every rank calls it.  Every rank's local checks
 * (shard size, the solve's completion, the staging buffer) are agreed on by one max-allreduce
 * BEFORE the all-gather, so a rank that fails makes every rank return an error instead of
 * leaving the others blocked in the collective. */
int picp_batch_allgather(picp_batch_t* b, picp_comm_t* c, int64_t n_total, float* T_all,
                         picp_stats* st_all);
/* The same gather with the byte exchange supplied by the caller instead of RCCL, for launchers
 * whose ranks cannot form an RCCL communicator (several ranks on one GPU -- RCCL refuses a
 * duplicate device -- or a CPU process group) and for testing the split at any world size.
 * exchange(user, send, recv, bytes) must all-gather `bytes` from every rank's host buffer `send`
 * into `recv` (world * bytes, rank order) and return 0.  One exchange per call: each rank sends
 * a 16-byte header (its local status) and its shard's 128-byte states padded to
 * picp_shard_pad(n_total, world) -- the layout picp_batch_allgather moves -- so a rank whose local
 * checks failed makes every rank return an error after the one exchange.  A non-zero return of
 * exchange is returned as PICP_ERR_STATE. */
typedef int (*picp_exchange_fn)(void* user, const void* send, void* recv, size_t bytes);
int picp_batch_allgather_host(picp_batch_t* b, int world, int rank, picp_exchange_fn exchange, void* user,
                              int64_t n_total, float* T_all, picp_stats* st_all);

/* ---------------- linear triangulation (cv::triangulatePoints replacement) ---------------- */

/* src/cam.cpp:94-140: per point DLT with two 3x4 row-major projection matrices, then
 * dehomogenisation.  uv1/uv2: float[2*q]; xyz_out: float[3*q].  Host pointers.
 * A point with a non-finite (NaN or Inf) pixel coordinate in either view comes out as three NaNs,
 * and every point does when P1 or P2 has a non-finite entry (cv::triangulatePoints gives NaN
 * there too); the other points of the call are not affected.  The VO sequence's bootstrap and
 * append steps triangulate by the same rule. */
int picp_triangulate(int device, const float P1[12], const float P2[12], const float* uv1,
                     const float* uv2, int64_t q, float* xyz_out);
/* Helper: P = K * inverse(T_cw)(0:3,0:4) from a camera-in-world pose (src/cam.cpp:109-112). */
int picp_projection_matrix(const float K[9], const float T_cw[16], float P[12]);

/* ---------------- multi-view refinement of map points (structure-only Gauss-Newton) ---------------- */

/* Refine 3-D points against ALL of their observations with the poses held fixed: the structure-only
 * counterpart of picp_solve (the same projection, bounds test, strict chi2 gate, robust weight and
 * damped Gauss-Newton; a 3x3 system per point).  Alternated with the pose solves it is a bundle
 * adjustment; on its own it is N-view triangulation.
 *
 * Per point X, independently, for up to max_rounds rounds:
 *   accumulate over the point's observations (k, uv) in track order: pc = R_k X + t_k; skipped
 *     (counted nowhere) if pc.z <= 0 or the projection leaves [0, cols-1] x [0, rows-1]; else
 *     n_projected++, e = proj - uv, chi = e.e; chi > threshold: lambda = sqrt(threshold / chi),
 *     chi_out += chi; else lambda = 1, chi_in += chi, n_in++; inliers (and outliers with
 *     keep_outliers) add H += J^T J lambda, b += J^T e lambda with J = Jp K R_k (2x3);
 *   the recorded stats are those of this linearisation, before the update (as in picp_solve);
 *   n_in < min_inliers: ok = 0, the point keeps its value and stops;
 *   H += damping I, solve H dx = -b; H not positive definite or dx not finite: ok = 0, the point
 *     keeps its value and stops; else X += dx, rounds++;
 *   picp_solve's convergence rule on chi_in (conv_eps < 0 disables it).
 * All rounds of all points run in one launch; results are bit-reproducible from run to run. */
typedef struct picp_refine picp_refine_t;

typedef struct picp_refine_params {
  float threshold;       /* chi2 gate, 3000 (exec/icp_test.cpp:86)                       */
  float damping;         /* 1                                                            */
  int32_t min_inliers;   /* 2: one view does not fix a point                             */
  int32_t keep_outliers; /* 0                                                            */
  int32_t max_rounds;    /* 10                                                           */
  float conv_eps;        /* 1e-5 relative chi_in change; < 0 disables                    */
} picp_refine_params;

void picp_refine_params_default(picp_refine_params* p);
int picp_refine_create(picp_refine_t** out, int device, int rows, int cols, const float K[9]);
int picp_refine_destroy(picp_refine_t* h);
/* World-in-camera poses, 16 floats each, column-major as for picp_set_pose.  Copied. */
int picp_refine_set_poses(picp_refine_t* h, const float* T_wc /* 16*n_poses */, int n_poses);
/* Tracks in CSR form: point i owns observations [track_off[i], track_off[i+1]) of obs_pose (an
 * index into the poses) and obs_uv (float2 pixels).  track_off[0] must be 0, the offsets must not
 * decrease and their end must fit an int32 (PICP_ERR_ARG); a pose index outside [0, n_poses) is
 * PICP_ERR_RANGE (checked at picp_refine_run when the poses are set after the tracks).  Copied.
 * Changing n_points drops the points (set them again). */
int picp_refine_set_tracks(picp_refine_t* h, int64_t n_points, const int64_t* track_off,
                           const int32_t* obs_pose, const float* obs_uv);
int picp_refine_set_points(picp_refine_t* h, const float* xyz /* 3*n_points */);
/* Refines the current points in place (a second run continues from the first's result).
 * PICP_ERR_STATE before poses, tracks or points were set.  n_points == 0 launches nothing.
 * Blocking. */
int picp_refine_run(picp_refine_t* h, const picp_refine_params* params);
int picp_refine_get_points(picp_refine_t* h, float* xyz /* 3*n_points */);
/* Per point: the stats of its last linearisation, ok, rounds (updates applied), converged. */
int picp_refine_get_stats(picp_refine_t* h, picp_stats* stats /* n_points */);
/* Mean device time of one run over `reps` runs (HIP events around the kernel launches only).  The
 * points are restored before every repetition (outside the timed spans), so every repetition does
 * the same work; afterwards the points and stats are those of one run from the points the call
 * found. */
int picp_refine_time(picp_refine_t* h, const picp_refine_params* params, int reps, float* us_per_run);

/* ---------------- alternating pose / point adjustment (resection, intersection, repeat) ---------------- */

/* The refiner's poses can move too.  A POSE STEP solves, for every movable pose k (not fixed, and
 * observed by at least one track), exactly the picp_batch_solve problem whose correspondences are
 * the pose's observations (current point j, pixel) in CANONICAL ORDER -- ascending position in the
 * arrays given to picp_refine_set_tracks: ascending point, then place in the track; a point observed
 * twice by one pose appears twice -- from the handle's current pose, with a picp_params; problems in
 * ascending pose order, laid out as a picp_batch of those sizes is.  A solved pose with a non-finite
 * entry is not written back: the pose keeps its value and its stats get ok = 0.  Fixed poses and
 * poses no track observes keep their bits and have all-zero stats.
 * The pose-major view of the tracks is built on the device at the first call that needs it and
 * dropped by picp_refine_set_tracks; the gather of the points into the solver's planes and the
 * write-back of the solved poses are device kernels; the solve is the one host wait of a step.
 * One SWEEP is a point step (picp_refine_run) followed by a pose step; picp_refine_adjust is exactly
 * that sequence, `sweeps` times, and gives its bits.  Everything is bit-reproducible from run to run. */
typedef struct picp_adjust_params {
  picp_refine_params points;  /* point step: as picp_refine_run            */
  picp_params poses;          /* pose step: as picp_batch_solve            */
  int32_t sweeps;             /* default 3; 0 launches nothing             */
  int32_t reserved;
} picp_adjust_params;
typedef struct picp_adjust_sweep {  /* one per sweep, in order */
  double chi_in_points, chi_in_poses;   /* sums of the steps' per-item stats.chi_in */
  int64_t n_in_points, n_in_poses, ok_points, ok_poses;
} picp_adjust_sweep;
/* points = picp_refine_params_default, poses = picp_params_default with threshold 3000 (the
 * gate both steps share, exec/icp_test.cpp:86), sweeps = 3. */
void picp_adjust_params_default(picp_adjust_params* p);
/* fixed[k] != 0: pose k never moves.  NULL: none.  PICP_ERR_ARG before picp_refine_set_poses, which
 * also resets the mask (and the sweep records). */
int picp_refine_set_fixed_poses(picp_refine_t* h, const uint8_t* fixed /* n_poses; NULL: none */);
/* PICP_ERR_STATE before poses, tracks or points were set; PICP_ERR_ARG on a NaN parameter or a
 * negative sweeps / max_rounds; a failed call launches nothing.  Blocking. */
int picp_refine_run_poses(picp_refine_t* h, const picp_params* params);
int picp_refine_adjust(picp_refine_t* h, const picp_adjust_params* params);
/* The current poses (column-major 4x4, world-in-camera; a pose that never moved has the bits it
 * was set with) and the stats of the last pose step (PICP_ERR_STATE before one). */
int picp_refine_get_poses(picp_refine_t* h, float* T_wc /* 16*n_poses */);
int picp_refine_get_pose_stats(picp_refine_t* h, picp_stats* stats /* n_poses */);
/* The pose-major view: pose k owns entries [pose_off[k], pose_off[k+1]) of obs_point (the owning
 * point) and obs_uv (float2), in canonical order.  Arrays nullable; sizes n_poses+1 / n_obs / 2 n_obs. */
int picp_refine_get_pose_view(picp_refine_t* h, int64_t* pose_off, int32_t* obs_point, float* obs_uv);
/* The records of the last picp_refine_adjust: *n = its sweeps, the first min(n, cap) are copied.
 * Summed on the device in a fixed order. */
int picp_refine_get_sweeps(picp_refine_t* h, picp_adjust_sweep* out, int cap, int* n);
/* Diagnostic: mean device time in us over reps of the view build (build_us, per build) and, per
 * sweep, of the gather and write-back kernels (gather_us), the pose batch's solve with its result
 * read-back (pose_us) and the point step (point_us).  Points and poses are restored before every
 * repetition, outside the timed spans; leaves the results of one picp_refine_adjust. */
int picp_refine_adjust_time(picp_refine_t* h, const picp_adjust_params* params, int reps,
                            float* build_us, float* gather_us, float* pose_us, float* point_us);

/* ---------------- descriptor matching (match_points replacement) ---------------- */

/* src/my_utilities.h:70-120: for each of the n1 descriptors of set 1 (float[dim], packed) the
 * nearest set-2 descriptor by squared L2 (best_idx, -1 if set 2 is empty), its distance and the
 * second-nearest distance; accepted[i] = best < dist_thr && best/second < ratio_thr (the
 * reference uses 0.2 and 0.8, src/my_utilities.h:44-46).  The accepted (i, best_idx[i]) pairs
 * are the reference's IntPairVector.  dim in [1, 32].  Host pointers. */
int picp_match(int device, const float* desc1, int64_t n1, const float* desc2, int64_t n2, int dim,
               float dist_thr, float ratio_thr, int32_t* best_idx, float* best_dist,
               float* second_dist, int32_t* accepted);
/* Many independent (set 1, set 2) pairs in one launch: problem i matches desc1 rows
 * [off1[i], off1[i+1]) against desc2 rows [off2[i], off2[i+1]); best_idx is relative to
 * off2[i].  n_problems <= 65535. */
int picp_match_batch(int device, int n_problems, const int64_t* off1, const int64_t* off2,
                     const float* desc1, const float* desc2, int dim, float dist_thr,
                     float ratio_thr, int32_t* best_idx, float* best_dist, float* second_dist,
                     int32_t* accepted);
/* picp_match_batch in an explicit kernel form:
 *   PICP_MATCH_FORM_FULL        the default (MFMA pre-filter + exact rescan; every output);
 *   PICP_MATCH_FORM_ACCEPT_ONLY the radius form the VO sequence runs: only accepted[] and
 *                               best_idx of accepted queries are defined (the others are not);
 *   PICP_MATCH_FORM_EXACT       the exact full scan (the same bits as FULL; a check path). */
#define PICP_MATCH_FORM_FULL 0
#define PICP_MATCH_FORM_ACCEPT_ONLY 1
#define PICP_MATCH_FORM_EXACT 2
int picp_match_batch_form(int device, int n_problems, const int64_t* off1, const int64_t* off2,
                          const float* desc1, const float* desc2, int dim, float dist_thr,
                          float ratio_thr, int32_t* best_idx, float* best_dist, float* second_dist,
                          int32_t* accepted, int form);

/* ---------------- essential-matrix bootstrap (src/cam.cpp:37-91) ---------------- */

/* Cam::computeEssentialAndRecoverPose: cv::findEssentialMat(p1, p2, K, cv::RANSAC) then
 * cv::recoverPose(E, p1, p2, K, R, t, mask), for many independent two-view problems.  The RANSAC
 * subsets are OpenCV's (its RNG((uint64)-1) stream), the minimal solver is Nister's five-point
 * algorithm, and the selection rule and adaptive iteration bound are OpenCV's. */
typedef struct picp_essential_params {
  double prob;       /* findEssentialMat prob      (default 0.999) */
  double threshold;  /* findEssentialMat threshold (default 1.0 px) */
  int max_iters;     /* findEssentialMat maxIters  (default 1000) */
  int reserved;
  double dist;       /* recoverPose distanceThresh (default 50) */
} picp_essential_params;

void picp_essential_params_default(picp_essential_params* p);

/* Problem i: the pixel pairs (p1[k], p2[k]) for k in [offs[i], offs[i+1]) (float x, y each).
 * K: column-major 3x3.  prm may be NULL (defaults).  Out, per problem: T_out[16 i ..] = the
 * camera-in-world pose of the second view with the first at the origin, [R | t]^-1 column-major
 * (Cam::getPose, src/cam.cpp:81,227; unit baseline), inliers = findEssentialMat's inlier count
 * (0: no model, T = I), good = recoverPose's count.  mask (may be NULL): offs[n] bytes, 1 for
 * the points recoverPose keeps.  Any n_problems >= 1: batches above 65535 problems run in slices
 * of 65535 on the device, inside the one call. */
int picp_essential_batch(int device, int n_problems, const int64_t* offs, const float* p1,
                         const float* p2, const float K[9], const picp_essential_params* prm,
                         float* T_out, int32_t* inliers, int32_t* good, uint8_t* mask);

/* ---------------- device-resident VO sequence (exec/icp_test.cpp:36-136) ---------------- */

/* The reference's per-frame loop (match next<->map, PICP from the previous pose, match
 * curr<->next, add_new_world_points, triangulate, append) run entirely on the GPU over
 * independent SEGMENTS of a sequence that advance in lockstep.  Segment s
 * covers frames first[s] .. first[s]+steps[s]: it bootstraps its map by triangulating the
 * matches of its first two frames with the given camera-in-world poses (a stand-in for
 * computeEssentialAndRecoverPose, exec/icp_test.cpp:44-58), then estimates frames
 * first[s]+1 .. first[s]+steps[s].  Matching uses DISTANCE_THRESHOLD 0.2 / RATIO 0.8. */
typedef struct picp_vo picp_vo_t;

/* One pose slot's record; slot 0 of a segment is its bootstrap (only n_new set). */
typedef struct {
  int32_t n_corr;   /* map correspondences of the frame (size of the PICP problem) */
  int32_t n_in;     /* numInliers() after the last round */
  int32_t rounds;   /* oneRound calls */
  int32_t n_new;    /* points triangulated into the map after this frame */
  float chi_in;
  float chi_out;
  int32_t converged;
  int32_t n_projected;
} picp_vo_step;

/* Upload (copy) a packed sequence: frame f = observations [frame_off[f], frame_off[f+1]) of
 * uv (float2, meas-*.dat "point" u v) and desc (float[dim]); frame_off[0] == 0. */
int picp_vo_create(picp_vo_t** out, int device, int rows, int cols, const float K[9],
                   int64_t n_frames, const int64_t* frame_off, const float* uv,
                   const float* desc, int dim);
int picp_vo_destroy(picp_vo_t* h);
/* boot_poses: per segment two column-major 4x4 camera-in-world poses (frames first, first+1).
 * params: threshold (icp_test: 3000), damping, min_inliers, keep_outliers, max_rounds,
 * conv_eps of the per-frame PICP loop. */
int picp_vo_set_segments(picp_vo_t* h, int n_seg, const int64_t* first, const int32_t* steps,
                         const float* boot_poses, const picp_params* params);
int picp_vo_run(picp_vo_t* h);        /* enqueue the whole sequence and wait */
int picp_vo_run_async(picp_vo_t* h);
int picp_vo_sync(picp_vo_t* h);
/* poses: sum(steps+1) camera-in-world 4x4 (segment-major; slot 0 = the bootstrap pose) */
int picp_vo_get_poses(picp_vo_t* h, float* poses);
int picp_vo_get_steps(picp_vo_t* h, picp_vo_step* steps);
/* segment map: *n = its size; the first min(n, cap) points are copied to xyz / desc (nullable) */
int picp_vo_get_map(picp_vo_t* h, int seg, int64_t cap, float* xyz, float* desc, int64_t* n);
/* Per-map-point track counters, off by default; read-only (poses, step records and maps keep
 * their bits).  May be switched any time before a run; the counters are zeroed at the start of
 * every run.  After a run, for map point j of segment seg:
 *   n_matched[j] = accepted frame->map matches whose best index was j, over the segment's steps;
 *   n_inlier[j]  = those of them that are PICP_CORR_INLIER, at the segment parameters' threshold,
 *                  at the step's FINAL PICP pose (the pose after the last update, world-in-camera:
 *                  the one picp_vo_get_poses reports inverted).  picp_vo_step.n_in counts the
 *                  inliers of the last LINEARISATION point instead, one update earlier, so the
 *                  sum of n_inlier over a step's matches need not equal its n_in.
 * picp_vo_get_map_stats: *n = the segment's map size; the first min(n, cap) entries are copied
 * (n_matched / n_inlier nullable), as in picp_vo_get_map.  PICP_ERR_STATE with tracking off. */
int picp_vo_set_track_stats(picp_vo_t* h, int enable);
int picp_vo_get_map_stats(picp_vo_t* h, int seg, int64_t cap,
                          int32_t* n_matched, int32_t* n_inlier, int64_t* n);
/* Observation tracks of a run, off by default; read-only like the track counters (poses, step
 * records and maps keep their bits).  May be switched any time before a run.  With the log on, a
 * run records on the device which observation matched which map point; afterwards the tracks are
 * built on the device in the refiner's CSR form (picp_refine_set_tracks), lazily at the first call
 * that needs them.
 * The track of map point j of segment seg (picp_vo_get_map's order): the point was created from
 * the pair (x in frame first+c, y in frame first+c+1), c = 0 for a bootstrap point and c = t for a
 * point appended by step t.  Its track holds x, y, and every accepted frame->map match of the
 * segment whose best index is j except the match whose observation is y itself (step 0 matches
 * frame first+1 against the bootstrap map and usually finds the observation that created the
 * point; it does not count twice).  Several observations of one frame matching one point all
 * stay.  Ascending by global observation index (inside a segment: by slot, then by index in the
 * frame); the same from run to run and under every schedule.
 * Slots: slot 0's pose is the first bootstrap pose; the second bootstrap pose is in no slot, as in
 * the reference (exec/icp_test.cpp keeps T0 only); slot 1 is step 0's estimate.
 * PICP_ERR_STATE: the log is off, or no run has completed since it was switched on or since the
 * last picp_vo_set_segments.  PICP_ERR_ARG: null handle, segment out of range, or more than
 * INT32_MAX observations in all tracks. */
int picp_vo_set_track_log(picp_vo_t* h, int enable);
/* Segment seg's tracks: point j owns entries [track_off[j], track_off[j+1]) of obs_slot (the pose
 * slot inside the segment, 0..steps) and obs_index (the global observation index into the uv /
 * desc arrays given to picp_vo_create).  Arrays nullable; a call with all arrays NULL returns
 * *n_points (= the map size) and *n_obs.  Non-null arrays must hold n_points+1 / n_obs / n_obs
 * entries. */
int picp_vo_get_tracks(picp_vo_t* h, int seg, int64_t* track_off, int32_t* obs_slot,
                       int64_t* obs_index, int64_t* n_points, int64_t* n_obs);
/* The pose table the refinement uses: sum(steps+1) WORLD-IN-CAMERA 4x4, column-major,
 * segment-major like picp_vo_get_poses.  Slot k's entry is the float32 rigid inverse
 * (R^T, -(R^T t) summed left to right, no fused multiply-add) of the pose picp_vo_get_poses
 * reports for that slot.  Same state conditions as picp_vo_get_tracks. */
int picp_vo_get_poses_wc(picp_vo_t* h, float* T_wc);
/* Structure-only refinement of every segment's map against its tracks with the poses fixed: one
 * launch of the picp_refine_* kernel over all segments' points (bit-equal to picp_refine_run on
 * the same tracks, poses and points).  prm NULL = picp_refine_params_default.  Blocking.  Starts
 * from the run's map every time (a second call repeats the first); the map, poses, step records
 * and any later picp_vo_run keep their bits.
 * picp_vo_get_refined_map: as picp_vo_get_map (xyz / stats nullable; stats as
 * picp_refine_get_stats); PICP_ERR_STATE before any picp_vo_refine_map since the last run. */
int picp_vo_refine_map(picp_vo_t* h, const picp_refine_params* prm);
int picp_vo_get_refined_map(picp_vo_t* h, int seg, int64_t cap, float* xyz, picp_stats* stats, int64_t* n);
/* Diagnostic: mean device time (us) over reps >= 1 of (a) the CSR build and (b) the refine launch,
 * HIP events around the kernels only.  Leaves the results of one picp_vo_refine_map. */
int picp_vo_refine_time(picp_vo_t* h, const picp_refine_params* prm, int reps,
                        float* build_us, float* refine_us);
/* Alternating adjustment of every segment's poses and map (picp_refine_adjust) on the tracks and
 * the pose table of picp_vo_refine_map, with slot 0 of every segment fixed (the segment's world
 * frame): bit-equal to picp_refine_adjust on a refiner given the same tracks, poses, points and
 * mask.  prm NULL = picp_adjust_params_default.  Blocking.  Same state conditions as
 * picp_vo_get_tracks.  Starts from the run's map and poses every time (a second call repeats the
 * first); the run's map, poses and step records, any later picp_vo_run and any picp_vo_refine_map
 * keep their bits.
 * picp_vo_get_adjusted_poses_wc: the layout of picp_vo_get_poses_wc; picp_vo_get_adjusted_map: as
 * picp_vo_get_refined_map (the stats of the last point step).  PICP_ERR_STATE before any
 * picp_vo_adjust since the last run. */
int picp_vo_adjust(picp_vo_t* h, const picp_adjust_params* prm);
int picp_vo_get_adjusted_poses_wc(picp_vo_t* h, float* T_wc);
int picp_vo_get_adjusted_map(picp_vo_t* h, int seg, int64_t cap, float* xyz, picp_stats* stats, int64_t* n);
/* mean device time of `reps` back-to-back runs (HIP events on the handle's stream) */
int picp_vo_time(picp_vo_t* h, int reps, float* ms_per_run);
int picp_vo_info(picp_vo_t* h, int64_t* n_obs, int64_t* n_slots, int64_t* map_slots, int* npt);
/* Diagnostic: the last run's match outputs per observation (n_obs int32): which = 0 frame->next
 * best index, 1 its accept flag, 2 frame->map best index, 3 its accept flag.  Best indices are
 * defined only where the flag is 1 (the sequence runs the matcher's accept-only form). */
int picp_vo_debug_matches(picp_vo_t* h, int which, int32_t* dst);
/* Diagnostic: with PICP_VO_GUARD=1 at create, every device buffer of the handle is bracketed by
 * 1 MiB pads of a fixed pattern; *bad_bytes = pad bytes that changed, *bad_buffer = 2 * (buffer
 * index in allocation order) + (0 before / 1 after) of the first changed pad, or -1. */
int picp_vo_debug_guard(picp_vo_t* h, int64_t* bad_bytes, int* bad_buffer);

/* ---------------- absolute pose without a prior: P3P RANSAC ---------------- */
/* "Here are 2D-3D matches against a map, where is the camera?" when no nearby pose is known (lost
 * tracking, a new frame against an existing map): a minimal absolute-pose solver (Grunert's P3P,
 * in double) inside RANSAC, scored with the solver's own gate (a correspondence counts when it is
 * PICP_CORR_INLIER at the hypothesis with `threshold`), to be polished by picp_solve /
 * picp_batch_solve from the returned pose.  All hypotheses are scored (no adaptive stop, no local
 * optimisation).  Problems are ragged: problem i owns correspondences [offs[i], offs[i+1]) of xyz
 * (3 floats each) and uv (2 floats each); offs[0] = 0.
 *
 * The samples.  Hypothesis h of problem i (its position in the batch) with n >= 4 correspondences
 * draws three distinct indices in [0, n) as a pure function of (seed, i, h).  With 64-bit wrapping
 * arithmetic and
 *   mix(x): z = x + 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *           z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)      (splitmix64)
 *   key = mix(seed ^ mix((i << 32) | h)),  r_j = mix(key + j) >> 32  for j = 0, 1, 2:
 *   a = (r_0 * n) >> 32
 *   b = (r_1 * (n - 1)) >> 32,  then b += 1 if b >= a
 *   c = (r_2 * (n - 2)) >> 32,  then c += 1 if c >= min(a, b),  then c += 1 if c >= max(a, b)
 * (skipping past the indices already chosen: no rejection loop).  The triple is (a, b, c).
 *
 * The result of problem i: the (hypothesis, root) with the largest count, then the lowest
 * hypothesis, then the lowest root.  found[i] = 1 and T_out its float32 world-in-camera pose -- the
 * pose that was scored -- when n >= 4, some hypothesis has a root and the count >= min_inliers;
 * otherwise found[i] = 0, T_out the identity, mask all 0, and inliers[i] the best count seen (0
 * when no hypothesis has a root).  mask (nullable, one byte per correspondence): 1 where the
 * correspondence is an inlier at T_out.  The same inputs give the same bits on every call.
 * n_problems * hypotheses is limited to 2^24 per call. */
typedef struct picp_pnp_params {
  float threshold;      /* squared pixels, the solver's strict gate; default 9 */
  int32_t hypotheses;   /* per problem, default 256, 1..65536 */
  int32_t min_inliers;  /* default 4 */
  int32_t reserved;
  uint64_t seed;        /* default 0 */
} picp_pnp_params;

void picp_pnp_params_default(picp_pnp_params* p);

/* prm NULL = picp_pnp_params_default.  n_problems == 0 returns PICP_OK. */
int picp_pnp_batch(int device, int n_problems, const int64_t* offs, const float* xyz, const float* uv,
                   const float K[9], int rows, int cols, const picp_pnp_params* prm, float* T_out,
                   int32_t* inliers, int32_t* found, uint8_t* mask);

/* picp_pnp_batch with the intermediate arrays, for tests; every output pointer may be NULL.  With
 * H = hypotheses, per problem: samples 3 H indices, n_roots H, hyp_T H x 4 poses of 16 floats
 * (column-major 4x4; zero beyond a hypothesis' n_roots), hyp_count H x 4 (0 beyond n_roots). */
int picp_pnp_batch_debug(int device, int n_problems, const int64_t* offs, const float* xyz, const float* uv,
                         const float K[9], int rows, int cols, const picp_pnp_params* prm, float* T_out,
                         int32_t* inliers, int32_t* found, uint8_t* mask, int32_t* samples, int32_t* n_roots,
                         float* hyp_T, int32_t* hyp_count);

/* mean device time in us of the four stages (samples, solve, score, select) over `reps`
 * repetitions after one untimed pass; us[4] */
int picp_pnp_batch_time(int device, int n_problems, const int64_t* offs, const float* xyz, const float* uv,
                        const float K[9], int rows, int cols, const picp_pnp_params* prm, int reps, float* us);

/* Single frame: the RANSAC above on the handle's points and current correspondences (problem
 * index 0).  On success the handle's pose is set to the winner, *inliers (nullable) to its count
 * and PICP_OK returned; when nothing is found PICP_TOO_FEW_INLIERS is returned, *inliers is the
 * best count seen and the handle's pose keeps its bits.  The caller's picp_stats are not touched
 * either way.  Follow with picp_solve. */
int picp_relocalize(picp_t* h, const picp_pnp_params* prm, int32_t* inliers);

/* ---------------- 3D-3D alignment: Sim(3) RANSAC ---------------- */
/* "Here are 3D-3D matches between two point sets, which scale, rotation and translation map one
 * onto the other?" (map to map, map to a surveyed reference, a revisited place to its first
 * visit), robust to wrong matches: Umeyama's closed form on three pairs inside RANSAC, every
 * hypothesis scored, then local optimisation (the least-squares transform of the inliers, `refits`
 * times).  Problems are ragged: problem i owns pairs [offs[i], offs[i+1]) of src and dst (3 floats
 * each); offs[0] = 0.  The transform is dst ~ M src + t with M = c R, c > 0, det R = +1.
 *
 * The samples are those of picp_pnp_batch: hypothesis h of problem i with n >= 4 pairs draws the
 * triple (a, b, c) of (seed, i, h, n) stated there.  Its transform is the closed form of the three
 * pairs, computed in double and rounded to float32; that float32 transform is the one scored.  A
 * triple gives no transform (and is never the winner) when a coordinate is not finite or the
 * three points of either set coincide or lie on a line (sigma_2 <= 1e-10 sigma_1 of their
 * covariance).
 *
 * The inlier test, in float32 without contraction, with m_rc the element of M in row r, column c,
 * p = (x, y, z) the src point and q the dst point, per row r:
 *   e_r = (((m_r0 * x + m_r1 * y) + m_r2 * z) + t_r) - q_r
 *   d2 = (e_0 * e_0 + e_1 * e_1) + e_2 * e_2
 * The pair is an inlier iff d2 < threshold (strict: a NaN fails).
 *
 * The winner is the valid hypothesis with the largest count, then the lowest index: candidate 0.
 * Refit r = 1..refits is the least-squares transform (in double, rounded to float32) of the
 * inliers of candidate r - 1, its count taken by the test above; a refit that gives no transform
 * (fewer than 3 inliers, rank < 2) ends the chain.  The moments are summed about the inlier of
 * the lowest index, so a cloud far from the origin keeps its digits.  The result is the
 * candidate with the largest count, the latest on a tie (a refit that keeps the count is the
 * least-squares transform of as many inliers, where the winner is a three-point guess).
 *
 * found[i] = 1 when n >= 4, some hypothesis is valid and the result's count >= min_inliers:
 * S_out (16 floats, column-major 4x4 [[c R, t], [0, 1]]) is the result, scale[i] its c, inliers[i]
 * its count, rms[i] the root mean square distance of its inliers, mask (one byte per pair) its
 * inliers.  Otherwise found[i] = 0, S_out is the identity, scale 1, rms 0, the mask all 0 and
 * inliers[i] the best count seen (0 when no hypothesis is valid).  scale, rms and mask are
 * nullable.  The same inputs give the same bits on every call.  n_problems * hypotheses is
 * limited to 2^24 per call. */
typedef struct picp_sim3_params {
  float threshold;      /* squared distance in dst units, strict; default 0.01 */
  int32_t hypotheses;   /* per problem, default 256, 1..65536 */
  int32_t min_inliers;  /* default 4 */
  int32_t with_scale;   /* default 1; 0: rigid, c = 1 */
  int32_t refits;       /* default 2, 0..8 */
  int32_t reserved;
  uint64_t seed;        /* default 0 */
} picp_sim3_params;

void picp_sim3_params_default(picp_sim3_params* p);

/* prm NULL = picp_sim3_params_default.  n_problems == 0 returns PICP_OK. */
int picp_sim3_batch(int device, int n_problems, const int64_t* offs, const float* src, const float* dst,
                    const picp_sim3_params* prm, float* S_out, float* scale, int32_t* inliers, int32_t* found,
                    float* rms, uint8_t* mask);

/* picp_sim3_batch with the intermediate arrays, for tests; every output pointer may be NULL.  With
 * H = hypotheses, per problem: samples 3 H indices, hyp_valid H, hyp_S H x 16 floats (column-major
 * 4x4; zero where not valid), hyp_count H, refit_S refits x 16 (zero where the chain has ended),
 * refit_count refits (-1 where the chain has ended). */
int picp_sim3_batch_debug(int device, int n_problems, const int64_t* offs, const float* src, const float* dst,
                          const picp_sim3_params* prm, float* S_out, float* scale, int32_t* inliers,
                          int32_t* found, float* rms, uint8_t* mask, int32_t* samples, int32_t* hyp_valid,
                          float* hyp_S, int32_t* hyp_count, float* refit_S, int32_t* refit_count);

/* mean device time in us of the five stages (samples, hypotheses, score, select, refit) over
 * `reps` repetitions after one untimed pass; us[5] */
int picp_sim3_batch_time(int device, int n_problems, const int64_t* offs, const float* src, const float* dst,
                         const picp_sim3_params* prm, int reps, float* us);

/* The refit stage alone (the device counterpart of a least-squares alignment of two trajectories):
 * per problem the transform of all pairs whose six coordinates are finite, or with mask (one byte
 * per pair, nullable) of those among them whose byte is not 0; the same sums in the same order as
 * a refit over that set.  found[i] = 0 (S_out the identity, scale 1, rms 0) when the set gives no
 * transform.  scale and rms are nullable. */
int picp_sim3_fit_batch(int device, int n_problems, const int64_t* offs, const float* src, const float* dst,
                        const uint8_t* mask, int with_scale, float* S_out, float* scale, float* rms,
                        int32_t* found);

/* The first user: consecutive segments of a device-resident VO run, each in a world frame and
 * scale of its own, aligned through their shared landmarks.  For every s < n_seg - 1, problem s
 * is built on the device: segment s + 1's map descriptors are the queries and segment s's the
 * references of the matcher's full form at the sequence's thresholds (0.2 / 0.8), and the accepted
 * queries j, in ascending index, give the pairs src = xyz_{s+1}[j], dst = xyz_s[best[j]].  The
 * problems then run as picp_sim3_batch runs them (problem s at batch position s), and the outputs
 * have the bits of that call on the same pairs built on the host from picp_vo_get_map and
 * picp_match_batch: S_out[s] ((n_seg - 1) x 16) maps segment s + 1's frame into segment s's.
 * Blocking and read-only: the run's maps, poses and step records, and any later call, keep their
 * bits; the host reads back only the pair counts.  The state conditions are picp_vo_get_map's.
 * scale and n_pairs (the accepted matches per problem) are nullable.  One segment: nothing to do,
 * PICP_OK. */
int picp_vo_align_segments(picp_vo_t* h, const picp_sim3_params* prm, float* S_out, float* scale, int32_t* inliers,
                           int32_t* found, int64_t* n_pairs);

/* ---------------- pose-graph optimisation over Sim(3) ---------------- */
/* "Here are similarities measured between frames (or segments), more of them than a chain needs:
 * where does every frame go?"  Nodes are similarities, edges are measured relative similarities,
 * the result is the nonlinear least-squares placement that spreads the disagreement.
 *
 * The batch is ragged.  Graph g owns nodes [node_off[g], node_off[g+1]) and edges
 * [edge_off[g], edge_off[g+1]); both offsets start at 0.  Node k carries S_k (16 floats,
 * column-major 4x4 [[c R, t], [0, 1]], the layout of S_out of picp_sim3_batch), which maps node k's
 * frame into the common frame, and a `fixed` byte.  Edge e carries the local node indices
 * edge_idx[2 e] = i and edge_idx[2 e + 1] = j, a similarity Z_e (16 floats) that maps node j's
 * frame into node i's (what picp_vo_align_segments returns for i = s, j = s + 1), and a weight
 * w_e >= 0; weight NULL means 1.
 *
 * Canonical form: every input matrix is first replaced, in double, by its nearest similarity.
 * With M its upper 3x3: c = cbrt(det M), R the orthogonal polar factor of M / c (Newton's iteration
 * R <- (R + R^-T) / 2 to convergence), t the fourth column.
 *
 * Residual and cost: r_e = Log(Z_e^-1 S_i^-1 S_j) in R^7, ordered (upsilon, omega, sigma), Log the
 * Sim(3) logarithm: the 4x4 matrix logarithm read as [[omega^ + sigma I, upsilon], [0, 0]].
 * cost = 1/2 sum w_e r_e^T r_e.  with_scale = 0 gives the SE(3) form: c is 1 for every canonical
 * input, sigma is dropped from residual and update, 6 unknowns per node.
 *
 * Update: S_k <- S_k Exp(delta_k) for the nodes that are not fixed; fixed nodes keep their input
 * bits.  The Jacobians are the true ones: with E = Z^-1 S_i^-1 S_j and S_ij = S_i^-1 S_j,
 * d r / d delta_j = J_r^-1(r) and d r / d delta_i = -J_r^-1(r) Ad(S_ij^-1), Ad(S) for S = (c, R, t)
 * the 7x7 [[c R, t^ R, -t], [0, R, 0], [0, 0, 1]]; J_r^-1(r) is taken by seven central differences
 * of Log(E Exp(+-h e_c)), h = 2^-17, in double.
 *
 * Method: Gauss-Newton, `damping` added to the diagonal of H = sum w J^T J; the step solves the
 * normal equations exactly (a block skyline Cholesky in node order).  `iterations` steps are run;
 * with eps > 0 the steps end after the first one whose cost c satisfies c_before - c < eps c_before.
 * All state and arithmetic are double; the outputs are rounded to float32 once at the end.
 *
 * Outputs: S_out (16 floats per node); per graph the cost and the gradient's 2-norm at the inputs
 * and at the result (double), the steps run and a status.  Every output pointer except S_out is
 * nullable.  The same inputs give the same bits on every call, and a graph's outputs do not depend
 * on the other graphs of the batch.
 *
 * Status, per graph (the other graphs still run); a graph whose status is not PICP_PGO_OK gets
 * S_out = its inputs, bit for bit.  The first that applies:
 *   PICP_PGO_BAD_INPUT     an S or Z with an entry that is not finite or det M <= 0 (or whose
 *                          canonical form is not finite), a weight that is negative or not finite
 *   PICP_PGO_BAD_EDGE      an edge with i = j or an index outside [0, n)
 *   PICP_PGO_DISCONNECTED  a node that is not fixed and that no path of edges of positive weight
 *                          joins to a fixed node (a graph without edges is exempt)
 *   PICP_PGO_TOO_LARGE     the factor's envelope in node order (block row a starts at the lowest
 *                          free neighbour of free node a) has more than PICP_PGO_MAX_BLOCKS blocks
 *   PICP_PGO_NOT_PD        a diagonal block was not positive definite during a factorisation, or
 *                          the cost stopped being finite
 * A graph with no edge, or no node that is not fixed, succeeds with S_out = its inputs and 0 steps
 * (its cost is still reported).  A graph has at most 2^24 nodes and 2^24 edges (PICP_ERR_ARG). */
#define PICP_PGO_OK 0
#define PICP_PGO_BAD_INPUT 1
#define PICP_PGO_BAD_EDGE 2
#define PICP_PGO_DISCONNECTED 3
#define PICP_PGO_NOT_PD 4
#define PICP_PGO_TOO_LARGE 5
#define PICP_PGO_MAX_BLOCKS (1 << 18)

typedef struct picp_pgo_params {
  int32_t with_scale;  /* default 1; 0: SE(3) */
  int32_t iterations;  /* Gauss-Newton steps, default 10, 0..1000 */
  double damping;      /* added to H's diagonal, default 0, >= 0 */
  double eps;          /* relative cost decrease that ends the steps, default 0: run every step */
} picp_pgo_params;

void picp_pgo_params_default(picp_pgo_params* p);

/* prm NULL = picp_pgo_params_default.  n_graphs == 0 returns PICP_OK. */
int picp_pgo_batch(int device, int n_graphs, const int64_t* node_off, const int64_t* edge_off, const float* S,
                   const uint8_t* fixed, const int32_t* edge_idx, const float* Z, const float* weight,
                   const picp_pgo_params* prm, float* S_out, double* cost_initial, double* cost_final,
                   double* grad_initial, double* grad_final, int32_t* steps, int32_t* status);

/* mean device time in us of the solve's one launch over `reps` repetitions after one untimed pass
 * (device events; the plan and the upload are not timed); us[1] */
int picp_pgo_batch_time(int device, int n_graphs, const int64_t* node_off, const int64_t* edge_off, const float* S,
                        const uint8_t* fixed, const int32_t* edge_idx, const float* Z, const float* weight,
                        const picp_pgo_params* prm, int reps, float* us);

/* ---------------- self-test ---------------- */
/* The projection's reciprocal 1/z must be the correctly rounded one (src/camera.h:30; the
 * chi2 gate is bit-exact): the kernels use a 3-instruction form, valid for every float in
 * [2^-100, 2^100] iff it matches the IEEE division on every float of a binade range.  Counts
 * the mismatching floats of both signs with exponents in [e_lo, e_hi); expected 0. */
int picp_selftest_rcp(int device, int e_lo, int e_hi, uint64_t* mismatches);

/* The persistent kernel finishes a round with the pose update spread over the lanes of one wave
 * (lane l computes word l of the new pose); the round kernel of the graph path computes the whole
 * pose in every lane.  Both must give the same bits.  Runs both forms on n_cases inputs in one
 * launch and counts the output words that differ; expected 0.
 * A case is PICP_SELFTEST_FINISH_IN 32-bit words: 0-31 the round's converted totals (the 21
 * entries of the upper triangle of H + damping I, row-major, as float; the 6 entries of -b;
 * chi_in; chi_out; n_in and n_projected as int32; 0), 32-43 the pose (R column-major, t),
 * 44 chi_prev, 45 conv_eps, 46 min_inliers (int32), 47 max_rounds (int32), 48 the round's
 * number, counted from 1 (int32), 49-51 unused.
 * out (may be NULL): 2 * PICP_SELFTEST_FINISH_OUT words per case, the words that are compared,
 * first the lane-parallel form's and then the uniform form's: 0-11 the new pose, 12 done, 13 ok,
 * 14 converged, 15 chi_prev, 16 chi_in, 17 chi_out, 18 n_in, 19 n_projected. */
#define PICP_SELFTEST_FINISH_IN 52
#define PICP_SELFTEST_FINISH_OUT 20
int picp_selftest_finish(int device, int64_t n_cases, const uint32_t* cases, uint64_t* mismatches,
                         uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* PICP_C_H */
