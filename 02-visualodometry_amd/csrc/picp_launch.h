// picp_launch.h -- every symbol a host translation unit (.cpp) calls and a device translation
// unit (.hip) defines: the kernel launchers and the queries of the kernels' compile-time shapes.
// Included by the defining .hip and by every caller, so a signature that changes on one side only
// is a compile error.  Not installed; not part of the public C-ABI (include/picp_c.h).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "picp_c.h"
#include "picp_internal.h"
#include "picp_pgo_graph.h"

extern "C" {

// ---- picp_kernels.hip
hipError_t picp_launch_round(hipStream_t stream, int grid, int vec, const float* X, const float* Y,
                             const float* Z, const float* U, const float* V, const PicpArgs* args,
                             const PicpProblem* probs, const int4* blkinfo, const PicpState* st_in,
                             PicpState* st_out, unsigned long long* part, unsigned int* tickets, int j);
hipError_t picp_launch_gather(hipStream_t stream, const float* world, const float* image, const int2* pairs,
                              int64_t m, float* X, float* Y, float* Z, float* U, float* V, int64_t off);
hipError_t picp_launch_triangulate(hipStream_t stream, const float* P1, const float* P2, const float2* uv1,
                                   const float2* uv2, int64_t q, float* xyz);
// counts into *bad the floats of binades [e_lo, e_hi), both signs, whose rcp_rn differs from 1.0f / x
hipError_t picp_launch_rcp_check(hipStream_t stream, int e_lo, int e_hi, unsigned long long* bad);
// finish_round_pose against finish_round_lanes on n cases (device pointers; the layout of a case and
// of out -- both forms' words, may be null --: picp_c.h picp_selftest_finish); counts the differing
// words into *bad
hipError_t picp_launch_finish_check(hipStream_t stream, int64_t n, const unsigned* cases,
                                    unsigned long long* bad, unsigned* out);

// ---- picp_persistent.hip
hipError_t picp_launch_persistent(hipStream_t stream, int grid, int npt, const float* X, const float* Y,
                                  const float* Z, const float* U, const float* V, const PicpArgs* args,
                                  const PicpState* st_in, PicpState* st_out, unsigned long long* gpart,
                                  unsigned long long* gpose, unsigned int* err, unsigned int* tagbase,
                                  unsigned long long timeout_ticks);
int picp_persistent_block(void);
hipError_t picp_persistent_occupancy(int npt, const float K[9], int* blocks_per_cu);

// ---- picp_block.hip
hipError_t picp_launch_block(hipStream_t stream, int n_problems, int npt, const float* X, const float* Y,
                             const float* Z, const float* U, const float* V, const PicpArgs* args,
                             const PicpProblem* probs, const PicpState* st_in, PicpState* st_out, int max_n,
                             int split, unsigned long long* xg, unsigned int* err, unsigned int* tagbase,
                             unsigned long long timeout_ticks);
int picp_block_max_items(void);
int picp_block_threads(int split);
int picp_block_npt_cap(int split);
hipError_t picp_block_occupancy(int npt, int split, int max_n, const float K[9], int* blocks_per_cu);
int picp_vo_block_fusable(int npt, int64_t max_obs);
hipError_t picp_launch_vo_block(hipStream_t stream, const VoArgs* a, int t, int npt, const PicpArgs* args,
                                int64_t max_obs);

// ---- picp_vo.hip
hipError_t picp_launch_vo_gather(hipStream_t stream, const VoArgs* a, int t);
hipError_t picp_launch_vo_append(hipStream_t stream, const VoArgs* a, int t);

// ---- picp_vo_tracks.hip
// the track log of step t's append (t < 0: the bootstrap's), after it on the same stream
hipError_t picp_launch_vo_tracklog(hipStream_t stream, const VoArgs* a, int t, const VoTrackLog* L);
// the CSR build in two parts: counts and per-segment scan (cnt zeroed by the caller; then seg_tot
// is read and seg_base, n_obs and the observation arrays are set), and everything else
hipError_t picp_launch_vo_tracks_count(hipStream_t stream, const VoTrackCsr* B);
hipError_t picp_launch_vo_tracks_fill(hipStream_t stream, const VoTrackCsr* B);

// ---- picp_classify.hip
int picp_classify_tile(void);
hipError_t picp_launch_classify(hipStream_t stream, int nb, int np, const float* X, const float* Y,
                                const float* Z, const float* U, const float* V, const ClsArgs* a,
                                const int4* blk, const int2* pblk, const int64_t* plane_off,
                                const int64_t* pack_off, const PicpState* st, uint8_t* state, float* chi2,
                                float* uv, int* cnt, long long* base, long long* counts, long long* inl_off,
                                int32_t* idx);
hipError_t picp_launch_vo_track(hipStream_t stream, const VoArgs* a, int t, const ClsArgs* c, int* n_matched,
                                int* n_inlier);

// ---- picp_refine.hip
hipError_t picp_launch_refine(hipStream_t stream, const RefineArgs* a, const RefinePose* poses,
                              const int64_t* track_off, const int32_t* obs_pose, const float2* obs_uv,
                              float* xyz, picp_stats* stats);

// ---- picp_adjust.hip
// the pose-major view of the tracks: count, scan, fill, rank (cnt zeroed by the caller)
hipError_t picp_launch_adjust_view(hipStream_t stream, const AdjView* v);
int picp_adjust_rank_tile(void);
// the current points (write_uv: and the pixels) into the batch's planes, the poses into its initial states
hipError_t picp_launch_adjust_gather(hipStream_t stream, const AdjPose* g, int write_uv);
// the solved states `st` (n_problems) into the refiner's poses and pose stats (zeroed by the caller)
hipError_t picp_launch_adjust_writeback(hipStream_t stream, const AdjPose* g, const PicpState* st);
hipError_t picp_launch_adjust_sums(hipStream_t stream, const picp_stats* point_stats, int64_t n_points,
                                   const picp_stats* pose_stats, int64_t n_poses, picp_adjust_sweep* out);

// ---- picp_essential.hip
hipError_t picp_launch_essential(hipStream_t stream, const EssArgs* args, const int64_t* offs, const float* p1,
                                 const float* p2, int32_t* idx, double* Es, int32_t* ns, int32_t* cnt,
                                 float* T_out, int32_t* inliers, int32_t* good, uint8_t* mask);

// ---- picp_ransac.hip
// both RANSAC solvers' samples[3 (p * hyp + h) + k] (zeros where n < 4); prob0: problem 0's batch position
hipError_t picp_launch_ransac_samples(hipStream_t stream, uint64_t seed, int32_t prob0, int32_t n_problems,
                                      int32_t hyp, const int64_t* offs, int32_t* samples);

// ---- picp_pnp.hip
// Per-(problem, hypothesis) arrays are indexed p * hyp + h: samples 3, n_roots 1, hyp_T 4 poses of
// 12 floats (R column-major, then t), cnt 4 (zeroed by the caller before the score launch).
int picp_pnp_score_tile(void);  // correspondences one score block holds
int picp_pnp_hyp_tile(void);    // hypotheses per count tile (a slice of the score grid's y takes whole tiles)
hipError_t picp_launch_pnp_solve(hipStream_t stream, const PnpArgs* A, const PnpItems* I, const int32_t* samples,
                                 int32_t* n_roots, float* hyp_T);
// blk[nb]: (problem, first correspondence) of every score block; hsplit: hypothesis slices (grid y)
hipError_t picp_launch_pnp_score(hipStream_t stream, const PnpArgs* A, const PnpItems* I, int nb, const int2* blk,
                                 int hsplit, const int32_t* n_roots, const float* hyp_T, int32_t* cnt);
// mask (nullable) is indexed offs[p] + j
hipError_t picp_launch_pnp_select(hipStream_t stream, const PnpArgs* A, const PnpItems* I, const int32_t* n_roots,
                                  const float* hyp_T, const int32_t* cnt, float* T_out, int32_t* inliers,
                                  int32_t* found, uint8_t* mask);

// ---- picp_sim3.hip
// Per-(problem, hypothesis) arrays are indexed p * hyp + h: samples 3, hyp_valid 1, hyp_S 16 floats
// (M = c R column-major, t, c, 3 unused), cnt 1 (zeroed by the caller before the score launch).
int picp_sim3_score_tile(void);  // pairs one score block holds
int picp_sim3_hyp_tile(void);    // hypotheses per count tile (a slice of the score grid's y takes whole tiles)
hipError_t picp_launch_sim3_hyp(hipStream_t stream, const Sim3Args* A, const Sim3Items* I, const int32_t* samples,
                                int32_t* hyp_valid, float* hyp_S);
// blk[nb]: (problem, first pair) of every score block; hsplit: hypothesis slices (grid y)
hipError_t picp_launch_sim3_score(hipStream_t stream, const Sim3Args* A, const Sim3Items* I, int nb, const int2* blk,
                                  int hsplit, const int32_t* hyp_valid, const float* hyp_S, int32_t* cnt);
hipError_t picp_launch_sim3_select(hipStream_t stream, const Sim3Args* A, const int32_t* hyp_valid, const int32_t* cnt,
                                   int32_t* win);
// refit_S (refits x 16 floats per problem, as hyp_S), refit_count, scale, inliers, rms and mask
// (indexed offs[p] + j) are nullable; with A->fit_only, win and hyp_S are not read and fit_mask
// (nullable, indexed offs[p] + j) selects the pairs
hipError_t picp_launch_sim3_refit(hipStream_t stream, const Sim3Args* A, const Sim3Items* I, const int32_t* win,
                                  const float* hyp_S, const uint8_t* fit_mask, float* refit_S, int32_t* refit_count,
                                  float* S_out, float* scale, int32_t* inliers, int32_t* found, float* rms,
                                  uint8_t* mask);

// ---- picp_pgo.hip
// one workgroup per graph of graphs[n_run] (device): the whole pose-graph solve (picp_pgo_solve.h)
hipError_t picp_launch_pgo(hipStream_t stream, int n_run, const PgoGraph* graphs, const PgoArrays* A,
                           const PgoArgs* P);

// the glue of picp_vo_align_segments: the match problems (segment s + 1's map against segment s's)
// from the map counts, the accepted queries per problem, and the pairs (packed float3) in ascending
// query index at offs[s] (offs: the prefix sums of n_pairs)
hipError_t picp_launch_vo_align_probs(hipStream_t stream, const VoSegment* segs, const int64_t* map_n, int n_problems,
                                      MatchProblem* probs);
hipError_t picp_launch_vo_align_count(hipStream_t stream, const MatchProblem* probs, int n_problems,
                                      const int32_t* accepted, int64_t* n_pairs);
hipError_t picp_launch_vo_align_pairs(hipStream_t stream, const MatchProblem* probs, int n_problems,
                                      const int32_t* accepted, const int32_t* best, const float* map_xyz,
                                      const int64_t* offs, float* src, float* dst);

// ---- picp_match.hip
hipError_t picp_launch_match(hipStream_t stream, int n_problems, int64_t max_nq, const float* q_desc,
                             const float* r_desc, const MatchProblem* probs, int dim, float dist_thr,
                             float ratio_thr, int32_t* best_idx, float* best_dist, float* second_dist,
                             int32_t* accepted);
hipError_t picp_launch_match_prep(hipStream_t stream, const float* desc, int64_t n, int dim, _Float16* h,
                                  float* n1, float* n2);
hipError_t picp_launch_match_mfma(hipStream_t stream, int n_problems, int64_t max_nq, const float* q_desc,
                                  const float* r_desc, const _Float16* q_h, const float* q_n1,
                                  const _Float16* r_h, const float* r_n1, const float* r_n2,
                                  const MatchProblem* probs, int dim, float dist_thr, float ratio_thr,
                                  int32_t* best_idx, float* best_dist, float* second_dist, int32_t* accepted,
                                  int form, int ksplit, float4* part, int64_t part_cap);
hipError_t picp_launch_match_mfma_parts(hipStream_t stream, int n_problems, int64_t max_nq, const float* q_desc,
                                        const float* r_desc, const _Float16* q_h, const float* q_n1,
                                        const _Float16* r_h, const float* r_n1, const float* r_n2,
                                        const MatchProblem* probs, int dim, float dist_thr, float ratio_thr,
                                        int form, int ksplit, int slot0, float4* part, int64_t part_cap);
hipError_t picp_launch_match_merge(hipStream_t stream, const MatchProblem* probs, int n_problems, int64_t max_nq,
                                   int ksplit, int extra, const float4* part, int64_t part_cap, float dist_thr,
                                   float ratio_thr, int32_t* best_idx, float* best_dist, float* second_dist,
                                   int32_t* accepted);
// picp_match_ksplit reads PICP_MATCH_KSPLIT each call; picp_match_ksplit_forced takes the forced
// count (0: none) from the caller, so a handle can read the variable once and size its scratch and
// its launches from the same value
int picp_match_ksplit(int n_problems, int64_t max_nq, int64_t max_nr, int form);
int picp_match_ksplit_forced(int n_problems, int64_t max_nq, int64_t max_nr, int form, int force);
int picp_match_ksplit_env(void);
// float4 of scratch a split launch needs (the ranges' partials)
int64_t picp_match_split_scratch(int ksplit, int n_problems, int64_t max_nq);
int picp_match_prep_kch(int dim);

}  // extern "C"
