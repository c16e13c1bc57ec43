// picp_vo_plan.h -- how the segments of a VO sequence are laid out, as a pure plan: from the frame
// table, the segments, the handle's options and the matcher's two split rules to the segment
// table, the frame->next problem table and its chunks, every launch's split count and scratch
// size, and the carve-up of the one allocation sized by the segments.  Plain C++ (no HIP call, no
// HIP type): picp_vo_runtime.cpp applies a plan to device memory, tests/vo_plan/plan_main.cpp
// prints one on a machine without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <utility>
#include <vector>

#include "picp_problem.h"

#pragma GCC visibility push(hidden)

#define VO_MAX_GRID_Y 65535  // problems of one match launch, segments of one handle
// sizes of the device types the parts hold (picp_vo_runtime.cpp asserts each against its type)
#define VO_STATE_BYTES 128   // PicpState
#define VO_STEP_BYTES 32     // VoStep
#define VO_PAIR_BYTES 8      // int2
#define VO_HALF_BYTES 2      // _Float16
#define VO_FLOAT4_BYTES 16   // float4

// A carve-up of one allocation: parts at 256-B multiples.
struct VoPart {
  size_t off = 0, bytes = 0;
};
struct VoParts {
  size_t total = 0;
  VoPart add(size_t bytes) {
    const VoPart p{total, bytes};
    total += (bytes + 255) / 256 * 256;
    return p;
  }
};

// The handle's options (the environment, read at picp_vo_create; ks_force at picp_vo_set_segments).
struct VoPlanOptions {
  int chains = 2;              // PICP_VO_CHAINS
  bool overlap = true;         // PICP_VO_OVERLAP
  int accept_only = 1;         // PICP_VO_MATCH_FULL=1: 0
  int split_env = 0;           // PICP_VO_SPLIT: 0 off, 1 every chain, -1 auto
  bool early_streams = false;  // the early world-match streams exist (split_env != 0 at create)
  int ks_force = 0;            // picp_match_ksplit_env(): PICP_MATCH_KSPLIT
};

// The matcher's two rules (picp_match.hip).  The split rule asks the device for its CU count, so a
// host-only program passes stand-ins.
struct VoPlanCaps {
  std::function<int(int n_problems, int64_t max_nq, int64_t max_nr, int form, int force)> ksplit;  // picp_match_ksplit_forced
  std::function<int64_t(int ksplit, int n_problems, int64_t max_nq)> split_scratch;                // picp_match_split_scratch
};

struct VoPlan {
  int n_seg = 0, chains_eff = 1, max_steps = 0, npt = 1;
  int64_t map_slots = 0, n_slots = 0, cap_c = 0;
  int64_t max_map = 0;  // the largest segment map (the world match's reference set)
  std::vector<VoSegment> segs;
  // frame->next problems grouped by step index: pprobs[chunk_off[k] .. chunk_off[k+1]) is chunk k,
  // frame f0+k of every segment with more than k steps; a frame of overlapping segments is matched
  // once, in the first chunk that needs it
  std::vector<MatchProblem> pprobs;
  std::vector<size_t> chunk_off;
  // per chain: the world match's split count and scratch (float4); the split by map age
  std::vector<int> ks_w;
  std::vector<int64_t> cap_w;
  std::vector<char> split_c;
  std::vector<int64_t> cap_e;  // one of the chain's two early buffers, float4
  // the frame->next launches as vo_frame_match issues them: first problem, split count
  std::vector<std::pair<size_t, int>> ks_p;
  int64_t cap_p = 0;
  // the one allocation, in this order
  VoPart p_segs, p_boot, p_mxyz, p_mdesc, p_mn, p_planes, p_probs, p_stin, p_stout, p_wprobs, p_lprobs, p_eprobs,
      p_pprobs, p_poses, p_steps, p_pairs, p_mh, p_mn1, p_mn2;
  std::vector<VoPart> p_partw, p_parte;  // per chain
  VoPart p_partp;
  size_t total = 0;
};

// Plans the layout of segments (first[s], steps[s]) over the frame table frame_off (n_frames + 1
// entries; max_obs its largest frame; dim floats and dp matcher halves per descriptor).  Returns
// nullptr, or the message of the argument error (PICP_ERR_ARG) and leaves *out alone.
const char* picp_vo_plan(int64_t n_frames, const int64_t* frame_off, int64_t max_obs, int dim, int dp, int n_seg,
                         const int64_t* first, const int32_t* steps, const VoPlanOptions& opt, const VoPlanCaps& caps,
                         VoPlan* out);

#pragma GCC visibility pop
