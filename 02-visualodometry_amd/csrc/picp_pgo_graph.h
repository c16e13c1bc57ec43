// picp_pgo_graph.h -- what the pose-graph plan (picp_pgo_plan.cpp) hands to the solve
// (picp_pgo_solve.h): one record per graph that runs, and the carve-up of its scratch.  Plain C++,
// no HIP type.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "picp_c.h"

// blocks (7x7 doubles) of one graph's envelope; a graph past it gets PICP_PGO_TOO_LARGE
#define PGO_MAX_BLOCKS PICP_PGO_MAX_BLOCKS
// nodes or edges of one graph
#define PGO_MAX_ITEMS (1 << 24)
// doubles of an envelope block (row-major 7x7; the SE(3) form uses its leading 6x6)
#define PGO_BLOCK 49
// doubles of an edge's record: r (7), d r / d delta_i (49, row-major 7x7), d r / d delta_j (49), 7 unused
#define PGO_EDGE_REC 112
#define PGO_EDGE_JI 7
#define PGO_EDGE_JJ 56

// A graph that runs.  Nodes and edges are indexed in the batch's arrays from node0 and edge0; the
// plan's arrays from the other bases, with local values: fidx[node0 + k] is node k's index among
// the free nodes or -1, first[free0 + a] the first block column of row a, row_off[row0 + a] the
// block index of (a, first[a]) (nf + 1 entries), task_slot[task0 + q] the block of gather task q,
// task_off[toff0 + q] its first entry (n_tasks + 1 entries) in entries[entry0 + ...].  An entry is
// 4 e + 2 sa + sb: edge e adds J_sa^T w J_sb, side 0 the Jacobian of node i and 1 of node j.  The
// first nf tasks are the diagonal blocks in node order (their entries also sum the gradient).
struct PgoGraph {
  int64_t node0, edge0, free0, row0, task0, toff0, entry0, scratch0;
  int32_t n, m, nf, n_tasks, n_blocks, batch_index;
};

// the batch's arrays, the plan's and the outputs (per graph of the batch: indexed by batch_index)
struct PgoArrays {
  const float* S;
  const int32_t* edge_idx;
  const float* Z;
  const float* weight;  // nullable
  const int32_t *fidx, *first, *row_off, *task_slot, *task_off, *entries;
  double* scratch;
  float* S_out;
  double *cost0, *cost1, *grad0, *grad1;
  int32_t *steps, *status;
};

struct PgoArgs {
  int32_t with_scale, iterations;
  double damping, eps;
};

// the scratch of one graph, in doubles: S (16 n), Z^-1 (16 m), the edge records, H (the envelope),
// the gradient and the step
struct PgoScratch {
  int64_t S, Zi, rec, H, g, x, total;
};

inline
#ifdef __HIPCC__
    __host__ __device__
#endif
    PgoScratch
    pgo_scratch(int64_t n, int64_t m, int64_t nf, int64_t n_blocks) {
  PgoScratch s;
  s.S = 0;
  s.Zi = s.S + 16 * n;
  s.rec = s.Zi + 16 * m;
  s.H = s.rec + PGO_EDGE_REC * m;
  s.g = s.H + PGO_BLOCK * n_blocks;
  s.x = s.g + 7 * nf;
  s.total = s.x + 7 * nf;
  return s;
}
