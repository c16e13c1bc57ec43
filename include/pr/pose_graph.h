// pr/pose_graph.h -- pose-graph optimisation over Sim(3): "here are similarities measured between
// frames or segments, more of them than a chain needs: where does every one go?" (picp_pgo_batch,
// include/picp_c.h: Gauss-Newton with a block skyline Cholesky on the GPU).
#pragma once
#include <array>
#include <cstdint>
#include <vector>

#include "picp_c.h"

namespace pr {

struct PoseGraphParams : picp_pgo_params {
  PoseGraphParams() { picp_pgo_params_default(this); }
};

typedef std::array<float, 16> Similarity;  // column-major 4x4 [[c R, t], [0, 1]]

// Z maps node j's frame into node i's
struct PoseGraphEdge {
  int i = 0, j = 0;
  Similarity Z{};
  float weight = 1.0f;
};

struct PoseGraphResult {
  double cost_initial = 0.0, cost_final = 0.0, grad_initial = 0.0, grad_final = 0.0;
  int steps = 0, status = 0;  // PICP_PGO_*
};

// Moves the nodes that are not fixed to the least-squares placement of the edges.  true: `nodes`
// holds the result; false: an error (picp_last_error()) or a status that is not PICP_PGO_OK
// (result->status), and `nodes` keeps its bits.
inline bool optimizePoseGraph(std::vector<Similarity>& nodes, const std::vector<uint8_t>& fixed,
                              const std::vector<PoseGraphEdge>& edges, const PoseGraphParams& params,
                              PoseGraphResult* result = nullptr, int device = 0) {
  PoseGraphResult r;
  if (result) *result = r;
  if (fixed.size() != nodes.size()) return false;
  std::vector<int32_t> idx(2 * edges.size());
  std::vector<float> Z(16 * edges.size()), w(edges.size());
  for (size_t e = 0; e < edges.size(); ++e) {
    idx[2 * e] = edges[e].i;
    idx[2 * e + 1] = edges[e].j;
    w[e] = edges[e].weight;
    for (int k = 0; k < 16; ++k) Z[16 * e + k] = edges[e].Z[k];
  }
  const int64_t node_off[2] = {0, (int64_t)nodes.size()}, edge_off[2] = {0, (int64_t)edges.size()};
  std::vector<Similarity> out(nodes.size());
  int32_t steps = 0, status = 0;
  const float* S = nodes.empty() ? nullptr : nodes[0].data();
  float* So = out.empty() ? nullptr : out[0].data();
  if (picp_pgo_batch(device, 1, node_off, edge_off, S, fixed.data(), idx.data(), Z.data(), w.data(), &params, So,
                     &r.cost_initial, &r.cost_final, &r.grad_initial, &r.grad_final, &steps, &status) != PICP_OK)
    return false;
  r.steps = steps;
  r.status = status;
  if (result) *result = r;
  if (status != PICP_PGO_OK) return false;
  nodes = out;
  return true;
}

}  // namespace pr
