// picp_pgo.hip -- pose-graph optimisation over Sim(3) for a ragged batch of graphs (DESIGN.md
// §4.14).  One launch: one workgroup per graph runs the whole solve of picp_pgo_solve.h, every
// Gauss-Newton step of it, because a graph's steps are serial and the batch supplies the
// parallelism (the reasoning of the Sim(3) refit stage):
//   per step  1. one lane per edge: the residual Log(Z^-1 S_i^-1 S_j), J_r^-1 and Ad, in double;
//             2. the 7x7 blocks of H and the gradient gathered from the edge records, every block
//                entry summing its edges in ascending edge index (the plan's lists);
//             3. the block skyline Cholesky in node order, in place in global scratch (L2-resident
//                at these sizes) with the block at hand and the reductions in LDS; the two
//                triangular solves; S_k <- S_k Exp(delta_k); the cost.
// Block barriers only: no block waits for another, no atomics.  All arithmetic is double with
// contraction off; the outputs are rounded to float32 once.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "picp_launch.h"
#include "picp_pgo_solve.h"

#pragma clang fp contract(off)

extern "C" __global__ __launch_bounds__(PGO_THREADS) void picp_pgo_kernel(const PgoGraph* __restrict__ graphs,
                                                                         PgoArrays A, PgoArgs P) {
  __shared__ PgoShared sh;
  const PgoGraph G = graphs[blockIdx.x];
  pgo_solve_graph(G, A, P, &sh, (int)threadIdx.x, PGO_THREADS);
}

extern "C" hipError_t picp_launch_pgo(hipStream_t stream, int n_run, const PgoGraph* graphs, const PgoArrays* A,
                                      const PgoArgs* P) {
  if (n_run <= 0) return hipSuccess;
  hipLaunchKernelGGL(picp_pgo_kernel, dim3((unsigned)n_run), dim3(PGO_THREADS), 0, stream, graphs, *A, *P);
  return hipGetLastError();
}
