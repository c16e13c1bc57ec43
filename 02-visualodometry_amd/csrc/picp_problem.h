// picp_problem.h -- the part of the device-visible layout (picp_internal.h) that the layout plans
// (picp_layout.h, picp_vo_plan.h) share with the kernels.  Plain C: no HIP type.
#pragma once
#include <stdint.h>

#define PICP_BLOCK 256            // threads per linearize block (4 waves of 64)
#define PICP_NPART 32             // floats per block partial (31 used)
// persistent mode: pose granule sets per problem -- solver g (g < 8) publishes an L2-kept copy
// (set 2g) and an agent-scope copy (set 2g + 1), 16 granules (one 128-B line) each
#define PICP_POSE_SETS 16

// Ragged batches only: per-problem partition (uniform batches compute it from blockIdx).
struct PicpProblem {
  int64_t offset;      // first item in the SoA planes (multiple of 4)
  int32_t n;           // number of correspondences
  int32_t blk0;        // first linearize block (index into partials) of this problem
  int32_t nblk;        // number of linearize blocks (>= 1)
  int32_t pad;
};
static_assert(sizeof(PicpProblem) % 8 == 0, "PicpProblem alignment");

// descriptor matching (picp_match.hip): query rows [q_off, q_off + nq) of the query
// descriptors against reference rows [r_off, r_off + nr); best_idx is relative to r_off.
struct MatchProblem {
  int64_t q_off, nq, r_off, nr;
  // the index of reference r_off in the caller's numbering (0: indices relative to r_off): a
  // problem over a later part of a reference set reports indices in the whole set's numbering
  int64_t idx0;
};
static_assert(sizeof(MatchProblem) == 40, "MatchProblem must be 40 B");

// device-resident VO sequence (picp_vo.hip): exec/icp_test.cpp:36-136 per segment
struct VoSegment {
  int64_t f0;       // first frame of the segment (bootstrap pair = f0, f0+1)
  int64_t map_off;  // first map slot of the segment
  int64_t slot0;    // first pose / step-record slot (steps + 1 slots)
  int32_t steps;    // PICP steps (frames f0+1 .. f0+steps are estimated)
  int32_t pad;
};
static_assert(sizeof(VoSegment) == 32, "VoSegment must be 32 B");
