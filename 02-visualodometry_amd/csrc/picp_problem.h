// picp_problem.h -- the part of the device-visible layout (picp_internal.h) that the layout plan
// (picp_layout.h) shares with the kernels.  Plain C: no HIP type.
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
