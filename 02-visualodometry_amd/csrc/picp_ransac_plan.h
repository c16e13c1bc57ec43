// picp_ransac_plan.h -- the score grid of a batched RANSAC run (picp_pnp.hip, picp_sim3.hip) as a
// pure plan.  Plain C++, no HIP: picp_ransac_host.h uploads a plan, bin/ransac_check prints one.
#pragma once
#include <limits.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

// One score block; the layout of the int2 the kernels read.
struct RansacBlock {
  int32_t problem, first;
};

// Plans problems of offs[i + 1] - offs[i] items (n_problems + 1 ascending offsets) scored in
// blocks of score_tile items against `hyp` hypotheses in tiles of hyp_tile: *nb blocks (grid x),
// *hsplit slices of the hypothesis tiles (grid y: with few blocks they fill the chip) and, when
// blk is not null, the blocks in problem order, then by first item.  Returns null, or the message
// of the argument error (PICP_ERR_ARG) as a format of the solver's name and of what its items are
// called; a rejected batch builds no table.
inline const char* picp_ransac_plan(const int64_t* offs, int n_problems, int hyp, int score_tile, int hyp_tile,
                                    int* nb, int* hsplit, std::vector<RansacBlock>* blk) {
  int64_t n_blocks = 0;
  for (int i = 0; i < n_problems; ++i) {
    if (offs[i + 1] - offs[i] > INT32_MAX - score_tile) return "%s: a problem has too many %s";
    n_blocks += (offs[i + 1] - offs[i] + score_tile - 1) / score_tile;
  }
  if (n_blocks > INT32_MAX / 4) return "%s: too many %s in one call";
  *nb = (int)n_blocks;
  const int tiles = (hyp + hyp_tile - 1) / hyp_tile;
  *hsplit = std::min(tiles, std::max(1, 1024 / std::max(*nb, 1)));
  for (int i = 0; blk && i < n_problems; ++i)
    for (int64_t first = 0; first < offs[i + 1] - offs[i]; first += score_tile)
      blk->push_back(RansacBlock{i, (int32_t)first});
  return nullptr;
}
