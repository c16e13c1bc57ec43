// picp_vo_host.h -- the VO sequence's handle, shared by the two runtime translation units that
// drive it: picp_vo_runtime.cpp (create, the segments, the run) and picp_vo_tracks_runtime.cpp (the
// track log, the CSR build, map refinement and adjustment after a run).  Not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <initializer_list>
#include <vector>

#include "picp_c.h"
#include "picp_host.h"
#include "picp_internal.h"
#include "picp_vo_plan.h"

struct picp_refine;

#pragma GCC visibility push(hidden)

// Diagnostic (PICP_VO_GUARD=1, read at create): every device buffer of the handle gets a
// VO_GUARD-byte pattern-filled pad before and after it; picp_vo_debug_guard counts pad bytes that
// no longer hold the pattern (an out-of-bounds store into or out of the buffer).
#define VO_GUARD (1 << 20)
#define VO_GUARD_BYTE 0xA5
struct VoGuarded {
  char* base;
  size_t bytes;
  const char* name;
};

struct picp_vo {
  int device = 0;
  hipStream_t stream = nullptr;
  int rows = 0, cols = 0, dim = 0;
  float K[9];
  int64_t n_frames = 0, n_obs = 0, max_obs = 0;
  std::vector<int64_t> frame_off;
  // sequence, resident
  int64_t* frame_off_d = nullptr;
  float2* uv_d = nullptr;
  float* desc_d = nullptr;
  int32_t *pm_bi = nullptr, *pm_acc = nullptr, *wm_bi = nullptr, *wm_acc = nullptr;
  float *pm_bd = nullptr, *pm_sd = nullptr, *wm_bd = nullptr, *wm_sd = nullptr;
  int dp = 16;                     // matcher prep row width (halves)
  _Float16* obs_h = nullptr;       // matcher prep of the observations
  float *obs_n1 = nullptr, *obs_n2 = nullptr;
  // What the plan reads of the environment (picp_vo_plan.h).  The default is the concurrent
  // schedule (overlap on, two chains), enqueued launch by launch: a hipGraph replay keeps neither
  // the streams' priorities nor the chains' phase offset.  The serial order
  // (PICP_VO_OVERLAP=0 PICP_VO_CHAINS=1) is captured once into a hipGraph and replayed
  // (PICP_VO_GRAPH=0: enqueued).  Every schedule gives the same bits.
  //   overlap: the frame->next match in chunks by step index (chunk k = frame f0+k of every
  //     segment with more than k steps), chunks 1.. on a side stream that runs beside the step
  //     chain (PICP_VO_OVERLAP=0: every chunk on the main stream, up front)
  //   chains: the segments in `chains` contiguous groups, each group's step chain on its own
  //     stream (group 0 on the handle's stream): one group's latency-bound PICP block kernel runs
  //     beside another group's throughput-bound world match.  Group c starts after group c-1's
  //     first world match (PICP_VO_PHASE=0: together), so the groups run out of phase.
  //   accept_only: the sequence reads only accepted matches (PICP_VO_MATCH_FULL=1: full form)
  //   split_env: the world match split by map age (PICP_VO_SPLIT=1; off by default: measured
  //     slower at every C5 shape -- 8e 44.5k -> 31.4-32.9k frames/s, the per-rank shape 162k ->
  //     75-77k, the default shape 797k -> 561k -- because the early parts, running beside the step
  //     chains for most of a step, slow the chains' short kernels: the append 20 -> 40-106 us, the
  //     merge 6 -> 40 us (profiles/r06/t13, t16, t17); neither a smaller early split nor CU-masked
  //     early queues helped).  Step t matches frame f0+t+1 against the map after step t-1's
  //     append.  The map is append-only, so that is the EARLY part -- the map as step t-2's append
  //     left it, which needs nothing from step t-1 and runs on the chain's early stream beside
  //     step t-1 -- and the LATE part, the points step t-1's append added.  Only the late part and
  //     the merge stay on the chain: the merge kernel folds the early ranges and then the late
  //     one, the reference's in-order scan over the whole map (the late indices are the map's:
  //     idx0).
  VoPlanOptions opt;
  // The current segments' layout (plan.n_seg == 0: none set).  Every launch's split count is
  // fixed here and the scratch sized from the same counts: a launch never uses more ranges than
  // its scratch holds.  Each chain's world match has its own scratch (the chains run
  // concurrently), the frame->next launches one between them (they run in stream order: chunk 0,
  // then the side stream's).
  VoPlan plan;
  void* seg_mem = nullptr;  // one allocation for everything sized by the segments
  PicpArgs pargs;
  VoArgs vargs;
  MatchProblem* pprobs_d = nullptr;
  MatchProblem* wprobs_d = nullptr;
  std::vector<float4*> part_w;  // [chains_eff]
  std::vector<float4*> part_e;  // [chains_eff][2]: early ranges + the late slot, by step parity
  float4* part_p = nullptr;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool use_graph = true;
  bool graph_env = false;
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr;
  std::vector<hipEvent_t> ev_chunk;
  bool phase = true;
  std::vector<hipStream_t> cstream;  // [chains], [0] unused (the handle's stream)
  std::vector<hipEvent_t> ev_cj;     // [chains]: group c's end (join), [0]: fork
  std::vector<hipEvent_t> ev_ph;     // [chains]: group c's first world match done
  std::vector<hipStream_t> estream;   // [chains]: the early world-match parts
  std::vector<hipEvent_t> ev_app;     // [chains]: the chain's latest merged match
  std::vector<hipEvent_t> ev_early;   // [chains][2]: the early part of step t done (by parity)
  // the step's gather runs inside the PICP block kernel (picp_launch_vo_block) when every frame's
  // items fit on-chip; PICP_VO_FUSE=0 keeps vo_gather_kernel + the plain block launch (A/B: the
  // same items in the same order, the same bits)
  // (the append fused after the rounds and a world match split into an early and a late part were
  // built in round 4, bit-identical, and measured slower: DESIGN.md §4.14, commit 1ffa87f)
  int fuse = 1;  // PICP_VO_FUSE: 0 separate gather, 1 gather in the PICP kernel
  // per-map-point track counters (picp_vo_set_track_stats; off by default): n_matched |
  // n_inlier, track_slots int32 each, zeroed at the start of every run and filled by one
  // vo_track_kernel launch per chain step between the PICP launch and the append
  bool track = false;
  int32_t* track_d = nullptr;
  int64_t track_slots = 0;
  // observation tracks (picp_vo_set_track_log; off by default): with the log on, one
  // vo_tracklog_kernel launch after every append of a run fills tlog_mem (sized by the segments:
  // the dense match log and the map slots' creation records); the first call that needs the
  // tracks after a run builds them into CSR form (vo_tracks_build: csr_a, csr_b, sized by the run)
  bool tlog = false;
  bool tlog_ran = false;  // a run with the log on since it was switched on / the segments were set
  void* tlog_mem = nullptr;
  VoTrackLog tl = {};
  bool csr_built = false, refined = false;
  void *csr_a = nullptr, *csr_b = nullptr;
  VoTrackCsr csr = {};
  std::vector<int64_t> pt_base, obs_base;  // per segment (+1): first point / first observation of the CSR
  float* xyz_ref = nullptr;                // picp_vo_refine_map's result
  picp_stats* stats_ref = nullptr;
  // picp_vo_adjust: a refiner of its own, loaded from the CSR build on the device (its buffers are
  // its own: the adjustment writes nothing of the run's or of picp_vo_refine_map's)
  picp_refine* adj = nullptr;
  bool adj_tracks = false, adjusted = false;  // adj holds this build's tracks / an adjustment of it
  bool guard = false;
  std::vector<VoGuarded> guards;
#ifdef PICP_VO_DIAG
  // picp_vo_debug_snap_set: per-step copies of the PICP launch's inputs/outputs.  The last member,
  // touched by picp_vo_runtime.cpp alone (which also creates and deletes the handle): the
  // diagnostic library links the tracks unit as built without the macro.
  char* snap = nullptr;
#endif
};

// picp_vo_runtime.cpp
hipError_t vo_malloc(picp_vo* h, void** p, size_t bytes, const char* name);
void vo_dfree(picp_vo* h, void* p);
// the captured sequence no longer matches what a run enqueues: capture again at the next run
void vo_drop_graph(picp_vo* h);
// The first min(count, cap) rows of each device array to its host destination (null: skipped);
// *n = count.
struct VoRows {
  void* dst;
  const void* src;
  size_t row_bytes;
};
int vo_copy_prefix(int64_t count, int64_t cap, int64_t* n, std::initializer_list<VoRows> arrays);

// picp_vo_tracks_runtime.cpp
// the track log's buffers for the current segments (log on, segments set)
int vo_tlog_alloc(picp_vo* h);
// the CSR build of the last run (release = true: and the log's segment-sized buffers)
void vo_tlog_free(picp_vo* h, bool release);

#pragma GCC visibility pop
