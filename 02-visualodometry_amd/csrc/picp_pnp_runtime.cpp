// picp_pnp_runtime.cpp -- absolute pose by P3P RANSAC (picp_pnp.hip): the run shared with the
// single-problem handle (picp_pnp_host.h) and the stateless batch calls, which upload, launch and
// download like the other front-end entry points (the parts shared with Sim(3): picp_ransac_host.h).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "picp_c.h"
#include "picp_host.h"
#include "picp_launch.h"
#include "picp_pnp_host.h"

extern "C" void picp_pnp_params_default(picp_pnp_params* p) {
  if (!p) return;
  p->threshold = 9.0f;
  p->hypotheses = 256;
  p->min_inliers = 4;
  p->reserved = 0;
  p->seed = 0;
}

int pnp_args(PnpArgs* A, const float K[9], int rows, int cols, const picp_pnp_params* prm, int n_problems) {
  picp_pnp_params dp;
  picp_pnp_params_default(&dp);
  const picp_pnp_params& P = prm ? *prm : dp;
  CHECK_ARG(rows > 0 && cols > 0, "pnp: rows/cols must be positive");
  CHECK_ARG(!(P.threshold != P.threshold), "pnp: threshold is NaN");
  CHECK_ARG(P.hypotheses >= 1 && P.hypotheses <= 65536, "pnp: hypotheses out of range [1, 65536]");
  CHECK_ARG((int64_t)n_problems * P.hypotheses <= RANSAC_MAX_HYP, "pnp: more than 2^24 hypotheses in one call");
  memset(A, 0, sizeof(*A));
  memcpy(A->K, K, sizeof(A->K));
  A->maxx = (float)(cols - 1);
  A->maxy = (float)(rows - 1);
  A->threshold = P.threshold;
  A->seed = P.seed;
  A->n_problems = n_problems;
  A->hyp = P.hypotheses;
  A->min_inliers = P.min_inliers;
  // K^-1 by the adjugate, in double; m(r, c) = K(r, c) of the column-major K
  auto m = [&](int r, int c) { return (double)K[c * 3 + r]; };
  const double det = m(0, 0) * (m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1)) - m(0, 1) * (m(1, 0) * m(2, 2) - m(1, 2) * m(2, 0)) +
                     m(0, 2) * (m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0));
  CHECK_ARG(det != 0.0 && fabs(det) <= 1.7976931348623157e308, "pnp: K is singular or not finite");
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
      A->Kinv[3 * r + c] = (m(r1, c1) * m(r2, c2) - m(r1, c2) * m(r2, c1)) / det;  // cofactor(c, r) / det
    }
  return PICP_OK;
}

int pnp_prepare(PnpRun* R, hipStream_t st, const int64_t* offs, bool want_mask) {
  const int np = R->A.n_problems, H = R->A.hyp;
  int rc = ransac_grid_prepare(&R->grid, st, offs, np, H, picp_pnp_score_tile(), picp_pnp_hyp_tile(), "pnp",
                               "correspondences");
  if (rc) return rc;
  const int64_t G = (int64_t)np * H;
  if ((rc = R->samples.grow(3 * G))) return rc;
  if ((rc = R->n_roots.grow(G))) return rc;
  if ((rc = R->cnt.grow(4 * G))) return rc;
  if ((rc = R->hyp_T.grow(48 * G))) return rc;
  if ((rc = R->T.grow(16 * (int64_t)np))) return rc;
  if ((rc = R->inliers.grow(np))) return rc;
  if ((rc = R->found.grow(np))) return rc;
  if (want_mask && (rc = R->mask.grow(offs[np]))) return rc;
  return PICP_OK;
}

hipError_t pnp_enqueue(PnpRun* R, hipStream_t st, TimedSpans* spans, int rep) {
  const int64_t G = (int64_t)R->A.n_problems * R->A.hyp;
  const RansacGrid& g = R->grid;
  hipError_t e = hipSuccess;
  auto begin = [&](int s) { return spans ? spans[s].begin(rep, st) : hipSuccess; };
  auto end = [&](int s) { return spans ? spans[s].end(rep, st) : hipSuccess; };
  if ((e = begin(0)) != hipSuccess) return e;
  e = picp_launch_ransac_samples(st, R->A.seed, R->A.prob0, R->A.n_problems, R->A.hyp, R->I.offs, R->samples);
  if (e != hipSuccess) return e;
  if ((e = end(0)) != hipSuccess || (e = begin(1)) != hipSuccess) return e;
  if ((e = picp_launch_pnp_solve(st, &R->A, &R->I, R->samples, R->n_roots, R->hyp_T)) != hipSuccess) return e;
  if ((e = end(1)) != hipSuccess || (e = begin(2)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(R->cnt, 0, (size_t)G * 4 * sizeof(int32_t), st)) != hipSuccess) return e;
  if ((e = picp_launch_pnp_score(st, &R->A, &R->I, g.nb, g.blk, g.hsplit, R->n_roots, R->hyp_T, R->cnt)) != hipSuccess)
    return e;
  if ((e = end(2)) != hipSuccess || (e = begin(3)) != hipSuccess) return e;
  if ((e = picp_launch_pnp_select(st, &R->A, &R->I, R->n_roots, R->hyp_T, R->cnt, R->T, R->inliers, R->found,
                                  R->mask)) != hipSuccess)
    return e;
  return end(3);
}

namespace {

int check_batch_args(int n_problems, const int64_t* offs, const float* xyz, const float* uv, const float* K) {
  CHECK_ARG(n_problems >= 0, "picp_pnp_batch: negative problem count");
  CHECK_ARG(offs && K, "picp_pnp_batch: null argument");
  return check_ragged_batch("picp_pnp_batch", n_problems, offs, xyz, uv);
}

// everything up to the launches: arguments, device, upload (a: xyz, b: uv), buffers
int pnp_setup(PnpRun* R, RansacUpload* U, int device, int n_problems, const int64_t* offs, const float* xyz,
              const float* uv, const float K[9], int rows, int cols, const picp_pnp_params* prm, bool want_mask) {
  int rc = pnp_args(&R->A, K, rows, cols, prm, n_problems);
  if (rc) return rc;
  if ((rc = select_device("picp_pnp_batch", device))) return rc;
  if ((rc = ransac_upload(U, n_problems, offs, xyz, 3, uv, 2))) return rc;
  R->I = PnpItems{U->a, U->a + 1, U->a + 2, U->b, U->b + 1, 3, 2, U->offs, U->offs};
  return pnp_prepare(R, nullptr, offs, want_mask);
}

}  // namespace

extern "C" int picp_pnp_batch_debug(int device, int n_problems, const int64_t* offs, const float* xyz,
                                    const float* uv, const float K[9], int rows, int cols,
                                    const picp_pnp_params* prm, float* T_out, int32_t* inliers, int32_t* found,
                                    uint8_t* mask, int32_t* samples, int32_t* n_roots, float* hyp_T,
                                    int32_t* hyp_count) {
  int rc = check_batch_args(n_problems, offs, xyz, uv, K);
  if (rc) return rc;
  PnpRun R;
  RansacUpload U;
  if (n_problems == 0) return pnp_args(&R.A, K, rows, cols, prm, 0);
  if ((rc = pnp_setup(&R, &U, device, n_problems, offs, xyz, uv, K, rows, cols, prm, mask != nullptr))) return rc;
  HIP_TRY(pnp_enqueue(&R, nullptr, nullptr, 0));
  const size_t np = (size_t)n_problems, G = np * (size_t)R.A.hyp;
  if (T_out) HIP_TRY(hipMemcpy(T_out, R.T, np * 16 * sizeof(float), hipMemcpyDeviceToHost));
  if (inliers) HIP_TRY(hipMemcpy(inliers, R.inliers, np * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (found) HIP_TRY(hipMemcpy(found, R.found, np * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (mask && offs[n_problems]) HIP_TRY(hipMemcpy(mask, R.mask, (size_t)offs[n_problems], hipMemcpyDeviceToHost));
  if (samples) HIP_TRY(hipMemcpy(samples, R.samples, G * 3 * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (n_roots) HIP_TRY(hipMemcpy(n_roots, R.n_roots, G * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (hyp_count) HIP_TRY(hipMemcpy(hyp_count, R.cnt, G * 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (hyp_T) {
    std::vector<float> dev(G * 48);
    std::vector<int32_t> nr(G);
    HIP_TRY(hipMemcpy(dev.data(), R.hyp_T, dev.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(nr.data(), R.n_roots, G * sizeof(int32_t), hipMemcpyDeviceToHost));
    memset(hyp_T, 0, G * 64 * sizeof(float));
    for (size_t g = 0; g < G; ++g)
      for (int r = 0; r < nr[g]; ++r) {
        PicpState s;
        memcpy(s.R, &dev[(g * 4 + r) * 12], 9 * sizeof(float));  // R column-major, then t
        memcpy(s.t, &dev[(g * 4 + r) * 12 + 9], 3 * sizeof(float));
        state_to_pose(s, hyp_T + (g * 4 + r) * 16);
      }
  }
  HIP_TRY(hipDeviceSynchronize());
  return PICP_OK;
}

extern "C" int picp_pnp_batch(int device, int n_problems, const int64_t* offs, const float* xyz, const float* uv,
                              const float K[9], int rows, int cols, const picp_pnp_params* prm, float* T_out,
                              int32_t* inliers, int32_t* found, uint8_t* mask) {
  CHECK_ARG(n_problems <= 0 || (T_out && inliers && found), "picp_pnp_batch: null output");
  return picp_pnp_batch_debug(device, n_problems, offs, xyz, uv, K, rows, cols, prm, T_out, inliers, found, mask,
                              nullptr, nullptr, nullptr, nullptr);
}

extern "C" int picp_pnp_batch_time(int device, int n_problems, const int64_t* offs, const float* xyz,
                                   const float* uv, const float K[9], int rows, int cols,
                                   const picp_pnp_params* prm, int reps, float* us) {
  CHECK_ARG(us && reps > 0 && reps <= 1000 && n_problems >= 1, "picp_pnp_batch_time: bad argument");
  int rc = check_batch_args(n_problems, offs, xyz, uv, K);
  if (rc) return rc;
  PnpRun R;
  RansacUpload U;
  if ((rc = pnp_setup(&R, &U, device, n_problems, offs, xyz, uv, K, rows, cols, prm, false))) return rc;
  return ransac_time_stages(4, reps, us, [&](TimedSpans* s, int r) { return pnp_enqueue(&R, nullptr, s, r); });
}
