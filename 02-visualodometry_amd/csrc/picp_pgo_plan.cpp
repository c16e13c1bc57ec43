// picp_pgo_plan.cpp -- see picp_pgo_plan.h.
#include "picp_pgo_plan.h"

#include <math.h>

#include <algorithm>
#include <array>

namespace {

// the 16 entries finite and the upper 3x3 (column-major 4x4) of finite determinant > 0
bool similarity_like(const float* m) {
  for (int k = 0; k < 16; ++k)
    if (!(fabsf(m[k]) < INFINITY)) return false;
  const double a = m[0], b = m[4], c = m[8], d = m[1], e = m[5], f = m[9], g = m[2], h = m[6], i = m[10];
  const double det = (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g);
  return det > 0.0 && det < INFINITY;
}

int32_t find_root(std::vector<int32_t>& parent, int32_t x) {
  while (parent[x] != x) {
    parent[x] = parent[parent[x]];
    x = parent[x];
  }
  return x;
}

}  // namespace

const char* picp_pgo_plan(int n_graphs, const int64_t* node_off, const int64_t* edge_off, const float* S,
                          const uint8_t* fixed, const int32_t* edge_idx, const float* Z, const float* weight,
                          PgoPlan* out) {
  if (n_graphs < 0) return "pgo: negative graph count";
  if (n_graphs == 0) {
    *out = PgoPlan();
    return nullptr;
  }
  if (!node_off || !edge_off) return "pgo: null offsets";
  if (node_off[0] != 0 || edge_off[0] != 0) return "pgo: offsets do not start at 0";
  for (int g = 0; g < n_graphs; ++g) {
    if (node_off[g + 1] < node_off[g] || edge_off[g + 1] < edge_off[g]) return "pgo: offsets descend";
    if (node_off[g + 1] - node_off[g] > PGO_MAX_ITEMS || edge_off[g + 1] - edge_off[g] > PGO_MAX_ITEMS)
      return "pgo: a graph has more than 2^24 nodes or edges";
  }
  if (node_off[n_graphs] > 0 && (!S || !fixed)) return "pgo: null node array";
  if (edge_off[n_graphs] > 0 && (!edge_idx || !Z)) return "pgo: null edge array";

  PgoPlan P;
  P.status.assign((size_t)n_graphs, PICP_PGO_OK);
  P.fidx.assign((size_t)node_off[n_graphs], -1);
  std::vector<int32_t> parent, first;
  std::vector<char> anchored;
  std::vector<std::vector<int32_t>> diag;
  std::vector<std::array<int32_t, 4>> offd;  // a, b, e, code
  for (int g = 0; g < n_graphs; ++g) {
    const int64_t n0 = node_off[g], e0 = edge_off[g];
    const int32_t n = (int32_t)(node_off[g + 1] - n0), m = (int32_t)(edge_off[g + 1] - e0);
    const int32_t* idx = edge_idx ? edge_idx + 2 * e0 : nullptr;
    const float* w = weight ? weight + e0 : nullptr;
    int32_t& st = P.status[(size_t)g];
    for (int32_t k = 0; k < n && st == PICP_PGO_OK; ++k)
      if (!similarity_like(S + 16 * (n0 + k))) st = PICP_PGO_BAD_INPUT;
    for (int32_t e = 0; e < m && st == PICP_PGO_OK; ++e) {
      if (!similarity_like(Z + 16 * (e0 + e))) st = PICP_PGO_BAD_INPUT;
      if (w && !(w[e] >= 0.0f && w[e] < INFINITY)) st = PICP_PGO_BAD_INPUT;
    }
    for (int32_t e = 0; e < m && st == PICP_PGO_OK; ++e) {
      const int32_t i = idx[2 * e], j = idx[2 * e + 1];
      if (i < 0 || i >= n || j < 0 || j >= n || i == j) st = PICP_PGO_BAD_EDGE;
    }
    if (st != PICP_PGO_OK || m == 0) continue;
    auto active = [&](int32_t e) { return !w || w[e] > 0.0f; };
    // the free nodes keep their order
    int32_t nf = 0;
    for (int32_t k = 0; k < n; ++k)
      if (!fixed[n0 + k]) P.fidx[(size_t)(n0 + k)] = nf++;
    // every free node reaches a fixed one through edges of positive weight
    parent.resize((size_t)n);
    for (int32_t k = 0; k < n; ++k) parent[(size_t)k] = k;
    for (int32_t e = 0; e < m; ++e)
      if (active(e)) {
        const int32_t a = find_root(parent, idx[2 * e]), b = find_root(parent, idx[2 * e + 1]);
        if (a != b) parent[(size_t)std::max(a, b)] = std::min(a, b);
      }
    anchored.assign((size_t)n, 0);
    for (int32_t k = 0; k < n; ++k)
      if (fixed[n0 + k]) anchored[(size_t)find_root(parent, k)] = 1;
    for (int32_t k = 0; k < n && st == PICP_PGO_OK; ++k)
      if (!fixed[n0 + k] && !anchored[(size_t)find_root(parent, k)]) st = PICP_PGO_DISCONNECTED;
    if (st != PICP_PGO_OK) {
      for (int32_t k = 0; k < n; ++k) P.fidx[(size_t)(n0 + k)] = -1;
      continue;
    }
    // the envelope: row a starts at its lowest free neighbour
    first.resize((size_t)nf);
    for (int32_t a = 0; a < nf; ++a) first[(size_t)a] = a;
    diag.assign((size_t)nf, std::vector<int32_t>());
    offd.clear();
    for (int32_t e = 0; e < m; ++e) {
      if (!active(e)) continue;
      const int32_t fi = P.fidx[(size_t)(n0 + idx[2 * e])], fj = P.fidx[(size_t)(n0 + idx[2 * e + 1])];
      if (fi >= 0) diag[(size_t)fi].push_back(4 * e + 0);
      if (fj >= 0) diag[(size_t)fj].push_back(4 * e + 3);
      if (fi >= 0 && fj >= 0) {
        // row a = the later node; sa is its side of the edge
        if (fi > fj)
          offd.push_back({fi, fj, e, 4 * e + 1});  // sa = 0 (i), sb = 1 (j)
        else
          offd.push_back({fj, fi, e, 4 * e + 2});  // sa = 1 (j), sb = 0 (i)
        const int32_t a = std::max(fi, fj), b = std::min(fi, fj);
        first[(size_t)a] = std::min(first[(size_t)a], b);
      }
    }
    int64_t blocks = 0;
    for (int32_t a = 0; a < nf; ++a) blocks += a - first[(size_t)a] + 1;
    if (blocks > PGO_MAX_BLOCKS) {
      st = PICP_PGO_TOO_LARGE;
      for (int32_t k = 0; k < n; ++k) P.fidx[(size_t)(n0 + k)] = -1;
      continue;
    }
    PgoGraph G;
    G.node0 = n0, G.edge0 = e0;
    G.free0 = (int64_t)P.first.size(), G.row0 = (int64_t)P.row_off.size();
    G.task0 = (int64_t)P.task_slot.size(), G.toff0 = (int64_t)P.task_off.size();
    G.entry0 = (int64_t)P.entries.size(), G.scratch0 = P.scratch;
    G.n = n, G.m = m, G.nf = nf, G.n_blocks = (int32_t)blocks, G.batch_index = g;
    int32_t off = 0;
    for (int32_t a = 0; a < nf; ++a) {
      P.first.push_back(first[(size_t)a]);
      P.row_off.push_back(off);
      off += a - first[(size_t)a] + 1;
    }
    P.row_off.push_back(off);
    const int64_t row0 = G.row0, ent0 = G.entry0;
    auto slot = [&](int32_t a, int32_t b) { return P.row_off[(size_t)(row0 + a)] + (b - first[(size_t)a]); };
    for (int32_t a = 0; a < nf; ++a) {
      P.task_slot.push_back(slot(a, a));
      P.task_off.push_back((int32_t)((int64_t)P.entries.size() - ent0));
      P.entries.insert(P.entries.end(), diag[(size_t)a].begin(), diag[(size_t)a].end());
    }
    std::sort(offd.begin(), offd.end());  // by (a, b, e)
    for (size_t q = 0; q < offd.size(); ++q) {
      if (q == 0 || offd[q][0] != offd[q - 1][0] || offd[q][1] != offd[q - 1][1]) {
        P.task_slot.push_back(slot(offd[q][0], offd[q][1]));
        P.task_off.push_back((int32_t)((int64_t)P.entries.size() - ent0));
      }
      P.entries.push_back(offd[q][3]);
    }
    P.task_off.push_back((int32_t)((int64_t)P.entries.size() - ent0));
    G.n_tasks = (int32_t)((int64_t)P.task_slot.size() - G.task0);
    P.scratch += pgo_scratch(n, m, nf, blocks).total;
    P.graphs.push_back(G);
  }
  *out = std::move(P);
  return nullptr;
}
