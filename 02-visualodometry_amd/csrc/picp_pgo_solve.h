// picp_pgo_solve.h -- the solve of one pose graph, written once for the device
// and the host: `nt` workers, worker `tid`, meet at PGO_SYNC().  picp_pgo.hip runs it with one
// workgroup per graph and PGO_SYNC() = __syncthreads(); under PICP_LIE_HOST it is plain host C++
// with nt = 1 and no barrier (bin/pgo_check, bin/pgo_ref), the same statements in the same order
// apart from the order of the two sums over all edges and all gradient entries (pgo_sum).
//
// Every loop bound comes from the plan (picp_pgo_plan.h), never from a computed value, and every
// worker takes every barrier: the trip counts and the early exits are the same for all of them.
#pragma once
#include <stdint.h>

#include "picp_c.h"
#include "picp_pgo_graph.h"
#include "picp_sim3_lie.h"

#ifdef PICP_LIE_HOST
#define PGO_SYNC() ((void)0)
#else
#define PGO_SYNC() __syncthreads()
#endif

#pragma clang fp contract(off)

#define PGO_THREADS 256  // workers of a graph on the device (a power of two)

namespace {

// what the workers share (LDS on the device)
struct PgoShared {
  double red[PGO_THREADS];
  double T[PGO_BLOCK];
  double v[8];
  int32_t flag;
};

// the graph's arrays, resolved
struct PgoView {
  int32_t n, m, nf, n_tasks, n_blocks, dim;
  const float *S_in, *Z_in, *weight;
  const int32_t *idx, *fidx, *first, *row_off, *task_slot, *task_off, *entries;
  double *S, *Zi, *rec, *H, *g, *x;
};

// the sum of every worker's v: by worker in a fixed tree, the same bits on every run
PICP_LIE_FN double pgo_sum(PgoShared* sh, double v, int tid, int nt) {
  sh->red[tid] = v;
  PGO_SYNC();
  for (int s = nt >> 1; s > 0; s >>= 1) {
    if (tid < s) sh->red[tid] += sh->red[tid + s];
    PGO_SYNC();
  }
  const double r = sh->red[0];
  PGO_SYNC();
  return r;
}

PICP_LIE_FN double pgo_weight(const PgoView& V, int32_t e) { return V.weight ? (double)V.weight[e] : 1.0; }

// One lane per edge: r = Log(Z^-1 S_i^-1 S_j), d r / d delta_j = J_r^-1(r) and
// d r / d delta_i = -J_r^-1(r) Ad(S_j^-1 S_i) into the edge's record.  Returns the cost.
PICP_LIE_FN double pgo_linearise(const PgoView& V, PgoShared* sh, int tid, int nt) {
  const int D = V.dim;
  double part = 0.0;
  for (int32_t e = tid; e < V.m; e += nt) {
    const double w = pgo_weight(V, e);
    if (!(w > 0.0)) continue;
    LieSim3 Si, Sj, Zi, A, B;
    lie_load(&Si, V.S + LIE_SIM3 * (int64_t)V.idx[2 * e]);
    lie_load(&Sj, V.S + LIE_SIM3 * (int64_t)V.idx[2 * e + 1]);
    lie_load(&Zi, V.Zi + LIE_SIM3 * (int64_t)e);
    lie_inv(&A, Si);
    lie_mul(&B, A, Sj);  // S_ij
    lie_mul(&A, Zi, B);  // E
    double* rec = V.rec + PGO_EDGE_REC * (int64_t)e;
    double r[7];
    lie_log(r, A);
    double rr = 0.0;
    for (int k = 0; k < 7; ++k) {
      if (k >= D) r[k] = 0.0;
      rec[k] = r[k];
      rr += r[k] * r[k];
    }
    part += w * rr;
    double* Jj = rec + PGO_EDGE_JJ;
    double* Ji = rec + PGO_EDGE_JI;
    lie_jr_inv(Jj, A, D);
    lie_inv(&A, B);  // S_ij^-1
    double Ad[49];
    lie_adjoint(Ad, A);
    for (int a = 0; a < D; ++a)
      for (int c = 0; c < D; ++c) {
        double s = 0.0;
        for (int k = 0; k < D; ++k) s += Jj[7 * a + k] * Ad[7 * k + c];
        Ji[7 * a + c] = -s;
      }
  }
  return 0.5 * pgo_sum(sh, part, tid, nt);
}

// H (the envelope, zero where no edge contributes) and the gradient from the edge records: every
// block entry sums its edges in ascending edge index.  Returns the gradient's 2-norm.
PICP_LIE_FN double pgo_gather(const PgoView& V, double damping, PgoShared* sh, int tid, int nt) {
  const int D = V.dim;
  for (int64_t q = tid; q < (int64_t)PGO_BLOCK * V.n_blocks; q += nt) V.H[q] = 0.0;
  PGO_SYNC();
  for (int64_t q = tid; q < (int64_t)PGO_BLOCK * V.n_tasks; q += nt) {
    const int32_t task = (int32_t)(q / PGO_BLOCK), el = (int32_t)(q % PGO_BLOCK), r = el / 7, c = el % 7;
    if (r >= D || c >= D) continue;
    double acc = 0.0;
    for (int32_t p = V.task_off[task]; p < V.task_off[task + 1]; ++p) {
      const int32_t code = V.entries[p], e = code >> 2;
      const double* rec = V.rec + PGO_EDGE_REC * (int64_t)e;
      const double* JA = rec + ((code & 2) ? PGO_EDGE_JJ : PGO_EDGE_JI);
      const double* JB = rec + ((code & 1) ? PGO_EDGE_JJ : PGO_EDGE_JI);
      double s = 0.0;
      for (int k = 0; k < D; ++k) s += JA[7 * k + r] * JB[7 * k + c];
      acc += pgo_weight(V, e) * s;
    }
    if (task < V.nf && r == c) acc += damping;
    V.H[(int64_t)PGO_BLOCK * V.task_slot[task] + el] = acc;
  }
  double part = 0.0;
  for (int64_t q = tid; q < (int64_t)7 * V.nf; q += nt) {
    const int32_t a = (int32_t)(q / 7), r = (int32_t)(q % 7);
    double acc = 0.0;
    if (r < D)
      for (int32_t p = V.task_off[a]; p < V.task_off[a + 1]; ++p) {
        const int32_t code = V.entries[p], e = code >> 2;
        const double* rec = V.rec + PGO_EDGE_REC * (int64_t)e;
        const double* JA = rec + ((code & 2) ? PGO_EDGE_JJ : PGO_EDGE_JI);
        double s = 0.0;
        for (int k = 0; k < D; ++k) s += JA[7 * k + r] * rec[k];
        acc += pgo_weight(V, e) * s;
      }
    V.g[q] = acc;
    part += acc * acc;
  }
  return sqrt(pgo_sum(sh, part, tid, nt));
}

PICP_LIE_FN double* pgo_block(const PgoView& V, int32_t row, int32_t col) {
  return V.H + (int64_t)PGO_BLOCK * (V.row_off[row] + (col - V.first[row]));
}

// The block skyline Cholesky H = L L^T in place, by rows: block (j, k) needs the rows above and the
// blocks of row j to its left, all inside the envelope.  false when a diagonal block is not
// positive definite.
PICP_LIE_FN bool pgo_factorise(const PgoView& V, PgoShared* sh, int tid, int nt) {
  const int D = V.dim;
  for (int32_t j = 0; j < V.nf; ++j) {
    const int32_t fj = V.first[j];
    for (int32_t k = fj; k < j; ++k) {
      const int32_t m0 = fj > V.first[k] ? fj : V.first[k];
      double* Ljk = pgo_block(V, j, k);
      for (int el = tid; el < PGO_BLOCK; el += nt) {
        const int r = el / 7, c = el % 7;
        if (r >= D || c >= D) continue;
        double acc = Ljk[el];
        for (int32_t m = m0; m < k; ++m) {
          const double* Ljm = pgo_block(V, j, m);
          const double* Lkm = pgo_block(V, k, m);
          for (int q = 0; q < D; ++q) acc -= Ljm[7 * r + q] * Lkm[7 * c + q];
        }
        sh->T[el] = acc;
      }
      PGO_SYNC();
      for (int r = tid; r < D; r += nt) {  // row r of T L_kk^-T
        const double* Lkk = pgo_block(V, k, k);
        double x[7];
        for (int c = 0; c < D; ++c) {
          double v = sh->T[7 * r + c];
          for (int q = 0; q < c; ++q) v -= x[q] * Lkk[7 * c + q];
          x[c] = v / Lkk[7 * c + c];
          Ljk[7 * r + c] = x[c];
        }
      }
      PGO_SYNC();
    }
    double* Ljj = pgo_block(V, j, j);
    for (int el = tid; el < PGO_BLOCK; el += nt) {
      const int r = el / 7, c = el % 7;
      if (r >= D || c >= D) continue;
      double acc = Ljj[el];
      for (int32_t m = fj; m < j; ++m) {
        const double* Ljm = pgo_block(V, j, m);
        for (int q = 0; q < D; ++q) acc -= Ljm[7 * r + q] * Ljm[7 * c + q];
      }
      sh->T[el] = acc;
    }
    PGO_SYNC();
    if (tid == 0) sh->flag = lie_chol(sh->T, D) ? 1 : 0;
    PGO_SYNC();
    if (!sh->flag) return false;
    for (int el = tid; el < PGO_BLOCK; el += nt)
      if (el / 7 < D && el % 7 < D) Ljj[el] = sh->T[el];
    PGO_SYNC();
  }
  return true;
}

// x = -H^-1 g from the factor: L y = -g by rows, L^T x = y by columns
PICP_LIE_FN void pgo_solve(const PgoView& V, PgoShared* sh, int tid, int nt) {
  const int D = V.dim;
  for (int64_t q = tid; q < (int64_t)7 * V.nf; q += nt) V.x[q] = -V.g[q];
  PGO_SYNC();
  for (int32_t j = 0; j < V.nf; ++j) {
    const int32_t fj = V.first[j];
    for (int r = tid; r < D; r += nt) {
      double v = V.x[7 * (int64_t)j + r];
      for (int32_t k = fj; k < j; ++k) {
        const double* Ljk = pgo_block(V, j, k);
        for (int q = 0; q < D; ++q) v -= Ljk[7 * r + q] * V.x[7 * (int64_t)k + q];
      }
      sh->v[r] = v;
    }
    PGO_SYNC();
    if (tid == 0) {
      lie_forward(pgo_block(V, j, j), sh->v, D);
      for (int q = 0; q < D; ++q) V.x[7 * (int64_t)j + q] = sh->v[q];
    }
    PGO_SYNC();
  }
  for (int32_t j = V.nf - 1; j >= 0; --j) {
    const int32_t fj = V.first[j];
    if (tid == 0) {
      for (int q = 0; q < D; ++q) sh->v[q] = V.x[7 * (int64_t)j + q];
      lie_backward(pgo_block(V, j, j), sh->v, D);
      for (int q = 0; q < D; ++q) V.x[7 * (int64_t)j + q] = sh->v[q];
    }
    PGO_SYNC();
    for (int64_t q = tid; q < (int64_t)(j - fj) * D; q += nt) {
      const int32_t k = fj + (int32_t)(q / D), rr = (int32_t)(q % D);
      const double* Ljk = pgo_block(V, j, k);
      double s = 0.0;
      for (int q2 = 0; q2 < D; ++q2) s += Ljk[7 * q2 + rr] * sh->v[q2];
      V.x[7 * (int64_t)k + rr] -= s;
    }
    PGO_SYNC();
  }
}

// S_k <- S_k Exp(delta_k) for the free nodes
PICP_LIE_FN void pgo_update(const PgoView& V, int tid, int nt) {
  for (int32_t k = tid; k < V.n; k += nt) {
    const int32_t a = V.fidx[k];
    if (a < 0) continue;
    double d[7];
    for (int q = 0; q < 7; ++q) d[q] = q < V.dim ? V.x[7 * (int64_t)a + q] : 0.0;
    LieSim3 S, X, Y;
    lie_load(&S, V.S + LIE_SIM3 * (int64_t)k);
    lie_exp(&X, d);
    lie_mul(&Y, S, X);
    lie_store(V.S + LIE_SIM3 * (int64_t)k, Y);
  }
  PGO_SYNC();
}

// The whole solve of graph G: canonical inputs, `iterations` Gauss-Newton steps (none for a graph
// without a free node), the outputs.
PICP_LIE_FN void pgo_solve_graph(const PgoGraph& G, const PgoArrays& A, const PgoArgs& P, PgoShared* sh, int tid,
                                 int nt) {
  const PgoScratch sc = pgo_scratch(G.n, G.m, G.nf, G.n_blocks);
  double* base = A.scratch + G.scratch0;
  PgoView V;
  V.n = G.n, V.m = G.m, V.nf = G.nf, V.n_tasks = G.n_tasks, V.n_blocks = G.n_blocks;
  V.dim = P.with_scale ? 7 : 6;
  V.S_in = A.S + 16 * G.node0, V.Z_in = A.Z + 16 * G.edge0;
  V.weight = A.weight ? A.weight + G.edge0 : nullptr;
  V.idx = A.edge_idx + 2 * G.edge0, V.fidx = A.fidx + G.node0;
  V.first = A.first + G.free0, V.row_off = A.row_off + G.row0;
  V.task_slot = A.task_slot + G.task0, V.task_off = A.task_off + G.toff0, V.entries = A.entries + G.entry0;
  V.S = base + sc.S, V.Zi = base + sc.Zi, V.rec = base + sc.rec, V.H = base + sc.H, V.g = base + sc.g;
  V.x = base + sc.x;

  if (tid == 0) sh->flag = 1;
  PGO_SYNC();
  for (int32_t k = tid; k < V.n; k += nt) {
    LieSim3 S;
    if (lie_canonical(&S, V.S_in + 16 * (int64_t)k, P.with_scale))
      lie_store(V.S + LIE_SIM3 * (int64_t)k, S);
    else
      sh->flag = 0;
  }
  for (int32_t e = tid; e < V.m; e += nt) {
    LieSim3 Z, Zi;
    if (lie_canonical(&Z, V.Z_in + 16 * (int64_t)e, P.with_scale)) {
      lie_inv(&Zi, Z);
      lie_store(V.Zi + LIE_SIM3 * (int64_t)e, Zi);
    } else {
      sh->flag = 0;
    }
  }
  PGO_SYNC();
  int32_t status = sh->flag ? PICP_PGO_OK : PICP_PGO_BAD_INPUT, steps = 0;
  PGO_SYNC();
  double cost0 = 0.0, grad0 = 0.0, cost = 0.0, grad = 0.0;
  if (status == PICP_PGO_OK) {
    cost0 = cost = pgo_linearise(V, sh, tid, nt);
    grad0 = grad = pgo_gather(V, P.damping, sh, tid, nt);
    const int32_t iters = V.nf > 0 ? P.iterations : 0;
    for (int32_t it = 0; it < iters; ++it) {
      if (!pgo_factorise(V, sh, tid, nt)) {
        status = PICP_PGO_NOT_PD;
        break;
      }
      pgo_solve(V, sh, tid, nt);
      pgo_update(V, tid, nt);
      ++steps;
      const double prev = cost;
      cost = pgo_linearise(V, sh, tid, nt);
      grad = pgo_gather(V, P.damping, sh, tid, nt);
      if (P.eps > 0.0 && (prev - cost) < P.eps * prev) break;
    }
    if (status == PICP_PGO_OK && !(fabs(cost) < INFINITY && fabs(grad) < INFINITY)) status = PICP_PGO_NOT_PD;
  }
  for (int32_t k = tid; k < V.n; k += nt) {
    float* o = A.S_out + 16 * (G.node0 + k);
    if (status == PICP_PGO_OK && V.fidx[k] >= 0) {
      LieSim3 S;
      lie_load(&S, V.S + LIE_SIM3 * (int64_t)k);
      lie_to_float(o, S);
    } else {
      for (int q = 0; q < 16; ++q) o[q] = V.S_in[16 * (int64_t)k + q];
    }
  }
  if (tid == 0) {
    A.cost0[G.batch_index] = cost0, A.cost1[G.batch_index] = cost;
    A.grad0[G.batch_index] = grad0, A.grad1[G.batch_index] = grad;
    A.steps[G.batch_index] = steps, A.status[G.batch_index] = status;
  }
}

}  // namespace
