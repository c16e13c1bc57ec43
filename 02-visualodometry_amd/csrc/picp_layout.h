// picp_layout.h -- how a batch is laid out, as a pure plan: from the correspondence offsets, the
// device's limits and the environment overrides to the execution mode, the block partition and
// the carve-up of the sync area.  Plain C++ (no HIP call, no HIP type): picp_batch.cpp applies a
// plan to device memory, tests/layout_plan/plan_main.cpp prints one on a machine without a GPU.
#pragma once
#include <stdint.h>

#include <functional>
#include <vector>

#include "picp_problem.h"

#pragma GCC visibility push(hidden)

#define PICP_POSE_GRAN 16         // 8-B granules of one pose set
#define PICP_MAX_PBLK 256         // persistent mode: most blocks of one problem

#define PICP_MODE_GRAPH 0
#define PICP_MODE_PERSISTENT 1
#define PICP_MODE_BLOCK 2

// one row of the block table: the device reads it as an int4 (x, y, z, w)
struct LayoutBlock {
  int32_t problem, first, count, pad;
};
static_assert(sizeof(LayoutBlock) == 16, "LayoutBlock must be an int4");

// What the device and the kernels allow.  The occupancy queries answer in resident blocks per CU
// for the exact kernel variant; a failed query counts as 0.
struct LayoutCaps {
  int num_cu = 0;
  int block_max_items = 0;          // picp_block_max_items()
  int persistent_block = 0;         // picp_persistent_block()
  int (*block_threads)(int split) = nullptr;
  int (*block_npt_cap)(int split) = nullptr;
  std::function<int(int npt)> persistent_occupancy;
  std::function<int(int npt, int split, int max_n)> block_occupancy;
};

// The environment overrides, read once per layout (tests change them between batches).
struct LayoutEnv {
  struct Int {
    bool set = false;
    int v = 0;
  };
  int mode = -1;               // PICP_MODE=graph|persistent|block: the PICP_MODE_* to force
  int items_per_block = 0;     // PICP_ITEMS_PER_BLOCK (counts from 4 up)
  Int block_npt;               // PICP_BLOCK_NPT: cap on the block kernel's register items per lane
  Int persist_blocks;          // PICP_PERSIST_BLOCKS: cap on the persistent blocks per problem
  int block_split = 0;         // PICP_BLOCK_SPLIT=1|2|4
  double stream_share = 0.64;  // PICP_STREAM_SHARE: the older block's fraction of a CU pair's range;
                               // measured optimum (profiles/r01/sweep_share.log); 0.5 = equal slices
  // PICP_RESIDENT_BLOCKS_PER_CU caps the occupancy answers (a test hook that emulates a device
  // partly held by other work; 0 forces the layouts without cross-block waits)
  int resident_cap = INT32_MAX;
};
LayoutEnv picp_layout_env();

// Byte offsets into the sync area of a layout that hands off between blocks (bytes == 0: none).
//   persistent : error word | pose granule sets | partial granules (x2 parities) | tag bases
//   split block: error word | exchange granules (x2 parities, 64 per block) | tag bases
// The error word and every granule region start on a 128-B line of their own: an agent-scope
// store to a line drops it from the XCD's L2, so an L2-kept pose set must not share a line with
// anything stored agent-scope, and a block's 512-B exchange set sharing lines with its
// neighbour's cost C4 3.5 % at 128 frames (profiles/r05/xg_align/).
struct SyncLayout {
  int64_t err = 0;
  int64_t pose = 0, pose_bytes = 0;  // persistent only
  int64_t gran = 0, gran_bytes = 0;  // partial (persistent) or exchange (split block) granules
  int64_t tag = 0, tag_bytes = 0;
  int64_t bytes = 0;
};

struct LayoutPlan {
  int np = 0;
  int64_t total = 0;           // correspondences
  int mode = PICP_MODE_GRAPH;
  int split = 1;               // block mode: blocks per problem (1, 2 or 4)
  int npt = 1;                 // persistent / block: correspondences per lane held in registers
  int ipb = PICP_BLOCK;        // items per linearize block
  int vec = 1;                 // correspondences per lane per chunk (1 or 4)
  int uniform = 0;             // all problems the same size -> no block tables
  int n_u = 0;
  int64_t stride_u = 0;
  int64_t max_n = 0;           // largest problem (block mode sizes its LDS stage with it)
  std::vector<int64_t> plane_off;  // per problem offset into the SoA planes (mult. of 4)
  int64_t plane_len = 0;       // padded plane length (floats)
  int nblk = 0;                // linearize blocks per launch
  std::vector<PicpProblem> probs;
  std::vector<LayoutBlock> blocks;
  // co-residency: persistent and split block modes hand rounds between blocks of one launch
  int handoff_grid = 0;        // blocks of the hand-off launch (0: the mode has none)
  int handoff_resident = 0;    // blocks the device holds at once for it (occupancy x CUs)
  SyncLayout sync;
};

// Plans the layout for correspondence offsets `offs` (np + 1 entries).  no_handoff: a hand-off
// wait timed out once on this batch, lay it out without cross-block waits.  Returns nullptr, or
// the message of the argument error (PICP_ERR_ARG) and leaves *out alone.
const char* picp_layout_plan(const int64_t* offs, int np, bool no_handoff, const LayoutCaps& caps,
                             const LayoutEnv& env, LayoutPlan* out);

#pragma GCC visibility pop
