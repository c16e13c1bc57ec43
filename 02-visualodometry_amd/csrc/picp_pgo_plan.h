// picp_pgo_plan.h -- the pose-graph batch as a pure plan: every graph checked
// (inputs, edges, connectivity to a fixed node by union-find), and for each graph that runs the
// free nodes' numbering, the block envelope of the Cholesky factor in node order (first[], the row
// offsets), the gather lists that assemble H and the gradient, and the scratch it needs.  Plain
// C++ (no HIP call, no HIP type): picp_pgo_runtime.cpp uploads a plan, tests/pgo_check runs and
// prints one on a machine without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "picp_c.h"
#include "picp_pgo_graph.h"

#pragma GCC visibility push(hidden)

struct PgoPlan {
  std::vector<int32_t> status;   // per graph of the batch: PICP_PGO_*
  std::vector<PgoGraph> graphs;  // the graphs that run (status OK, an edge and a node), in batch order
  std::vector<int32_t> fidx;     // per node of the batch
  std::vector<int32_t> first, row_off, task_slot, task_off, entries;
  int64_t scratch = 0;  // doubles, all running graphs
};

// Plans a batch (the arrays of picp_pgo_batch; weight nullable).  Returns nullptr, or the message
// of an argument error (PICP_ERR_ARG: offsets that do not ascend from 0, a graph with more than
// PGO_MAX_ITEMS nodes or edges) and leaves *out alone.  Per graph, the first of these that applies
// is its status: BAD_INPUT (an S or Z with an entry that is not finite or an upper 3x3 of
// determinant <= 0 or not finite, a weight that is negative or not finite), BAD_EDGE (i == j or an
// index outside [0, n)), DISCONNECTED (a free node that no path of positive-weight edges joins to
// a fixed node; not applied to a graph without edges), TOO_LARGE (an envelope of more than
// PGO_MAX_BLOCKS blocks).  A graph with status OK runs when it has an edge; with no free node it
// runs only to report its cost.  Edges of weight 0 take no part in the envelope or the lists.
const char* picp_pgo_plan(int n_graphs, const int64_t* node_off, const int64_t* edge_off, const float* S,
                          const uint8_t* fixed, const int32_t* edge_idx, const float* Z, const float* weight,
                          PgoPlan* out);

#pragma GCC visibility pop
