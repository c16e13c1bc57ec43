// picp_pgo_runtime.cpp -- pose-graph optimisation over Sim(3) (picp_pgo.hip): argument checks, the
// plan (picp_pgo_plan.h), upload, the one launch and the download, on the pattern of
// picp_sim3_runtime.cpp.  A batch in which no graph runs (each one failed its checks or has nothing
// to solve) is answered on the host and needs no device.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <vector>

#include "picp_c.h"
#include "picp_host.h"
#include "picp_launch.h"
#include "picp_pgo_plan.h"

extern "C" void picp_pgo_params_default(picp_pgo_params* p) {
  if (!p) return;
  p->with_scale = 1;
  p->iterations = 10;
  p->damping = 0.0;
  p->eps = 0.0;
}

namespace {

int pgo_args(PgoArgs* A, const picp_pgo_params* prm) {
  picp_pgo_params dp;
  picp_pgo_params_default(&dp);
  const picp_pgo_params& P = prm ? *prm : dp;
  CHECK_ARG(P.iterations >= 0 && P.iterations <= 1000, "pgo: iterations out of range [0, 1000]");
  CHECK_ARG(P.damping >= 0.0 && P.damping < INFINITY, "pgo: damping is negative or not finite");
  CHECK_ARG(P.eps >= 0.0 && P.eps < INFINITY, "pgo: eps is negative or not finite");
  A->with_scale = P.with_scale ? 1 : 0;
  A->iterations = P.iterations;
  A->damping = P.damping;
  A->eps = P.eps;
  return PICP_OK;
}

template <class T>
int upload(DevBuf<T>* d, const T* src, size_t n) {
  int rc = d->grow((int64_t)n);
  if (rc) return rc;
  if (n) HIP_TRY(hipMemcpy(d->p, src, n * sizeof(T), hipMemcpyHostToDevice));
  return PICP_OK;
}

// the plan and the batch on the device
struct PgoRun {
  PgoArgs args;
  PgoPlan plan;
  PgoArrays A;
  DevBuf<PgoGraph> graphs;
  DevBuf<float> S, Z, weight, S_out;
  DevBuf<int32_t> edge_idx, fidx, first, row_off, task_slot, task_off, entries, steps, status;
  DevBuf<double> scratch, figures;  // figures: cost0, cost1, grad0, grad1, n_graphs each
};

// arguments and plan; no device call
int pgo_plan(PgoRun* R, const char* what, int n_graphs, const int64_t* node_off, const int64_t* edge_off,
             const float* S, const uint8_t* fixed, const int32_t* edge_idx, const float* Z, const float* weight,
             const picp_pgo_params* prm) {
  int rc = pgo_args(&R->args, prm);
  if (rc) return rc;
  if (const char* msg = picp_pgo_plan(n_graphs, node_off, edge_off, S, fixed, edge_idx, Z, weight, &R->plan))
    return picp_set_err(PICP_ERR_ARG, "%s: %s", what, msg);
  return PICP_OK;
}

int pgo_upload(PgoRun* R, const char* what, int device, int n_graphs, const int64_t* node_off,
               const int64_t* edge_off, const float* S, const int32_t* edge_idx, const float* Z, const float* weight) {
  int rc = select_device(what, device);
  if (rc) return rc;
  const PgoPlan& P = R->plan;
  const size_t nn = (size_t)node_off[n_graphs], ne = (size_t)edge_off[n_graphs], ng = (size_t)n_graphs;
  if ((rc = upload(&R->graphs, P.graphs.data(), P.graphs.size()))) return rc;
  if ((rc = upload(&R->S, S, 16 * nn)) || (rc = upload(&R->Z, Z, 16 * ne))) return rc;
  if ((rc = upload(&R->edge_idx, edge_idx, 2 * ne))) return rc;
  if (weight && (rc = upload(&R->weight, weight, ne))) return rc;
  if ((rc = upload(&R->fidx, P.fidx.data(), P.fidx.size())) || (rc = upload(&R->first, P.first.data(), P.first.size())) ||
      (rc = upload(&R->row_off, P.row_off.data(), P.row_off.size())) ||
      (rc = upload(&R->task_slot, P.task_slot.data(), P.task_slot.size())) ||
      (rc = upload(&R->task_off, P.task_off.data(), P.task_off.size())) ||
      (rc = upload(&R->entries, P.entries.data(), P.entries.size())))
    return rc;
  if ((rc = R->scratch.grow(P.scratch)) || (rc = R->S_out.grow(16 * (int64_t)nn)) ||
      (rc = R->figures.grow(4 * (int64_t)ng)) || (rc = R->steps.grow((int64_t)ng)) ||
      (rc = R->status.grow((int64_t)ng)))
    return rc;
  PgoArrays& A = R->A;
  A.S = R->S, A.edge_idx = R->edge_idx, A.Z = R->Z, A.weight = weight ? (const float*)R->weight : nullptr;
  A.fidx = R->fidx, A.first = R->first, A.row_off = R->row_off, A.task_slot = R->task_slot;
  A.task_off = R->task_off, A.entries = R->entries, A.scratch = R->scratch, A.S_out = R->S_out;
  A.cost0 = R->figures, A.cost1 = R->figures + ng, A.grad0 = R->figures + 2 * ng, A.grad1 = R->figures + 3 * ng;
  A.steps = R->steps, A.status = R->status;
  return PICP_OK;
}

}  // namespace

extern "C" int picp_pgo_batch(int device, int n_graphs, const int64_t* node_off, const int64_t* edge_off,
                              const float* S, const uint8_t* fixed, const int32_t* edge_idx, const float* Z,
                              const float* weight, const picp_pgo_params* prm, float* S_out, double* cost_initial,
                              double* cost_final, double* grad_initial, double* grad_final, int32_t* steps,
                              int32_t* status) {
  PgoRun R;
  int rc = pgo_plan(&R, "picp_pgo_batch", n_graphs, node_off, edge_off, S, fixed, edge_idx, Z, weight, prm);
  if (rc) return rc;
  if (n_graphs == 0) return PICP_OK;
  const size_t nn = (size_t)node_off[n_graphs], ng = (size_t)n_graphs;
  CHECK_ARG(S_out || nn == 0, "picp_pgo_batch: null output");
  // the graphs that do not run: their inputs, no cost, their status
  if (nn) memcpy(S_out, S, 16 * nn * sizeof(float));
  for (size_t g = 0; g < ng; ++g) {
    if (cost_initial) cost_initial[g] = 0.0;
    if (cost_final) cost_final[g] = 0.0;
    if (grad_initial) grad_initial[g] = 0.0;
    if (grad_final) grad_final[g] = 0.0;
    if (steps) steps[g] = 0;
    if (status) status[g] = R.plan.status[g];
  }
  if (R.plan.graphs.empty()) return PICP_OK;
  if ((rc = pgo_upload(&R, "picp_pgo_batch", device, n_graphs, node_off, edge_off, S, edge_idx, Z, weight))) return rc;
  HIP_TRY(picp_launch_pgo(nullptr, (int)R.plan.graphs.size(), R.graphs, &R.A, &R.args));
  std::vector<float> So(16 * nn);
  std::vector<double> fig(4 * ng);
  std::vector<int32_t> st(ng), sp(ng);
  HIP_TRY(hipMemcpy(So.data(), R.S_out, So.size() * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(fig.data(), R.figures, fig.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(st.data(), R.status, ng * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(sp.data(), R.steps, ng * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipDeviceSynchronize());
  for (const PgoGraph& G : R.plan.graphs) {
    const size_t g = (size_t)G.batch_index;
    memcpy(S_out + 16 * G.node0, So.data() + 16 * G.node0, 16 * (size_t)G.n * sizeof(float));
    if (cost_initial) cost_initial[g] = fig[g];
    if (cost_final) cost_final[g] = fig[ng + g];
    if (grad_initial) grad_initial[g] = fig[2 * ng + g];
    if (grad_final) grad_final[g] = fig[3 * ng + g];
    if (steps) steps[g] = sp[g];
    if (status) status[g] = st[g];
  }
  return PICP_OK;
}

extern "C" int picp_pgo_batch_time(int device, int n_graphs, const int64_t* node_off, const int64_t* edge_off,
                                   const float* S, const uint8_t* fixed, const int32_t* edge_idx, const float* Z,
                                   const float* weight, const picp_pgo_params* prm, int reps, float* us) {
  CHECK_ARG(us && reps > 0 && reps <= 1000 && n_graphs >= 1, "picp_pgo_batch_time: bad argument");
  PgoRun R;
  int rc = pgo_plan(&R, "picp_pgo_batch_time", n_graphs, node_off, edge_off, S, fixed, edge_idx, Z, weight, prm);
  if (rc) return rc;
  CHECK_ARG(!R.plan.graphs.empty(), "picp_pgo_batch_time: no graph of the batch runs");
  if ((rc = pgo_upload(&R, "picp_pgo_batch_time", device, n_graphs, node_off, edge_off, S, edge_idx, Z, weight)))
    return rc;
  TimedSpans span(reps);
  HIP_TRY(span.create());
  const int n_run = (int)R.plan.graphs.size();
  HIP_TRY(picp_launch_pgo(nullptr, n_run, R.graphs, &R.A, &R.args));
  for (int r = 0; r < reps; ++r) {
    HIP_TRY(span.begin(r, nullptr));
    HIP_TRY(picp_launch_pgo(nullptr, n_run, R.graphs, &R.A, &R.args));
    HIP_TRY(span.end(r, nullptr));
  }
  double ms = 0.0;
  HIP_TRY(span.sum_ms(nullptr, &ms));
  us[0] = (float)(1000.0 * ms / reps);
  return PICP_OK;
}
