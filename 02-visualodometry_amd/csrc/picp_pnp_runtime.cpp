// picp_pnp_runtime.cpp -- absolute pose by P3P RANSAC (picp_pnp.hip): the run shared with the
// single-problem handle (picp_pnp_host.h) and the stateless batch calls, which upload, launch and
// download like the other front-end entry points.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "picp_c.h"
#include "picp_host.h"
#include "picp_launch.h"
#include "picp_pnp_host.h"

#define PNP_MAX_HYP_PER_CALL (1 << 24)

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
  CHECK_ARG((int64_t)n_problems * P.hypotheses <= PNP_MAX_HYP_PER_CALL, "pnp: more than 2^24 hypotheses in one call");
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
  const int tile = picp_pnp_score_tile();
  int64_t nb64 = 0;
  for (int i = 0; i < np; ++i) {
    CHECK_ARG(offs[i + 1] - offs[i] <= INT32_MAX - tile, "pnp: a problem has too many correspondences");
    nb64 += (offs[i + 1] - offs[i] + tile - 1) / tile;
  }
  CHECK_ARG(nb64 <= INT32_MAX / 4, "pnp: too many correspondences in one call");
  R->nb = (int)nb64;
  // few blocks: the hypothesis tiles are dealt to slices of the grid's y so the chip fills
  const int tiles = (H + picp_pnp_hyp_tile() - 1) / picp_pnp_hyp_tile();
  R->hsplit = std::min(tiles, std::max(1, 1024 / std::max(R->nb, 1)));
  const int64_t G = (int64_t)np * H;
  int rc;
  if ((rc = R->blk.grow(R->nb))) return rc;
  if ((rc = R->samples.grow(3 * G))) return rc;
  if ((rc = R->n_roots.grow(G))) return rc;
  if ((rc = R->cnt.grow(4 * G))) return rc;
  if ((rc = R->hyp_T.grow(48 * G))) return rc;
  if ((rc = R->T.grow(16 * (int64_t)np))) return rc;
  if ((rc = R->inliers.grow(np))) return rc;
  if ((rc = R->found.grow(np))) return rc;
  if (want_mask && (rc = R->mask.grow(offs[np]))) return rc;
  // a handle that relocalizes frames of one size keeps its table
  const bool same = R->blk_offs.size() == (size_t)np + 1 && std::equal(R->blk_offs.begin(), R->blk_offs.end(), offs);
  if (R->nb && !same) {
    std::vector<int2> blk((size_t)R->nb);
    size_t k = 0;
    for (int i = 0; i < np; ++i)
      for (int64_t first = 0; first < offs[i + 1] - offs[i]; first += tile) blk[k++] = make_int2(i, (int)first);
    HIP_TRY(hipMemcpyAsync(R->blk, blk.data(), blk.size() * sizeof(int2), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // blk is a local
    R->blk_offs.assign(offs, offs + np + 1);
  }
  return PICP_OK;
}

hipError_t pnp_enqueue(PnpRun* R, hipStream_t st, TimedSpans* spans, int rep) {
  const int64_t G = (int64_t)R->A.n_problems * R->A.hyp;
  hipError_t e = hipSuccess;
  auto begin = [&](int s) { return spans ? spans[s].begin(rep, st) : hipSuccess; };
  auto end = [&](int s) { return spans ? spans[s].end(rep, st) : hipSuccess; };
  if ((e = begin(0)) != hipSuccess) return e;
  if ((e = picp_launch_pnp_samples(st, &R->A, &R->I, R->samples)) != hipSuccess) return e;
  if ((e = end(0)) != hipSuccess || (e = begin(1)) != hipSuccess) return e;
  if ((e = picp_launch_pnp_solve(st, &R->A, &R->I, R->samples, R->n_roots, R->hyp_T)) != hipSuccess) return e;
  if ((e = end(1)) != hipSuccess || (e = begin(2)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(R->cnt, 0, (size_t)G * 4 * sizeof(int32_t), st)) != hipSuccess) return e;
  if ((e = picp_launch_pnp_score(st, &R->A, &R->I, R->nb, R->blk, R->hsplit, R->n_roots, R->hyp_T, R->cnt)) != hipSuccess)
    return e;
  if ((e = end(2)) != hipSuccess || (e = begin(3)) != hipSuccess) return e;
  if ((e = picp_launch_pnp_select(st, &R->A, &R->I, R->n_roots, R->hyp_T, R->cnt, R->T, R->inliers, R->found,
                                  R->mask)) != hipSuccess)
    return e;
  return end(3);
}

namespace {

// the packed inputs of a stateless call on the device
struct PnpUpload {
  DevBuf<int64_t> offs;
  DevBuf<float> xyz, uv;
};

int check_batch_args(int n_problems, const int64_t* offs, const float* xyz, const float* uv, const float* K) {
  CHECK_ARG(n_problems >= 0, "picp_pnp_batch: negative problem count");
  CHECK_ARG(offs && K, "picp_pnp_batch: null argument");
  CHECK_ARG(offs[0] == 0, "picp_pnp_batch: offsets must start at 0");
  for (int i = 0; i < n_problems; ++i)
    CHECK_ARG(offs[i + 1] >= offs[i] && offs[i + 1] - offs[i] <= INT32_MAX, "picp_pnp_batch: bad offsets");
  CHECK_ARG(offs[n_problems] == 0 || (xyz && uv), "picp_pnp_batch: null points");
  return PICP_OK;
}

// everything up to the launches: arguments, device, upload, buffers
int pnp_setup(PnpRun* R, PnpUpload* U, int device, int n_problems, const int64_t* offs, const float* xyz,
              const float* uv, const float K[9], int rows, int cols, const picp_pnp_params* prm, bool want_mask) {
  int rc = pnp_args(&R->A, K, rows, cols, prm, n_problems);
  if (rc) return rc;
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  CHECK_ARG(device >= 0 && device < ndev, "picp_pnp_batch: no such HIP device");
  HIP_TRY(hipSetDevice(device));
  const int64_t total = offs[n_problems];
  if ((rc = U->offs.grow(n_problems + 1))) return rc;
  if ((rc = U->xyz.grow(3 * total))) return rc;
  if ((rc = U->uv.grow(2 * total))) return rc;
  HIP_TRY(hipMemcpy(U->offs, offs, (size_t)(n_problems + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  if (total) {
    HIP_TRY(hipMemcpy(U->xyz, xyz, (size_t)total * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(U->uv, uv, (size_t)total * 2 * sizeof(float), hipMemcpyHostToDevice));
  }
  R->I = PnpItems{U->xyz, U->xyz + 1, U->xyz + 2, U->uv, U->uv + 1, 3, 2, U->offs, U->offs};
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
  PnpUpload U;
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
  PnpUpload U;
  if ((rc = pnp_setup(&R, &U, device, n_problems, offs, xyz, uv, K, rows, cols, prm, false))) return rc;
  TimedSpans spans[4] = {TimedSpans(reps), TimedSpans(reps), TimedSpans(reps), TimedSpans(reps)};
  for (TimedSpans& s : spans) HIP_TRY(s.create());
  HIP_TRY(pnp_enqueue(&R, nullptr, nullptr, 0));  // untimed: first-launch costs
  for (int r = 0; r < reps; ++r) HIP_TRY(pnp_enqueue(&R, nullptr, spans, r));
  for (int s = 0; s < 4; ++s) {
    double ms = 0.0;
    HIP_TRY(spans[s].sum_ms(nullptr, &ms));
    us[s] = (float)(1000.0 * ms / reps);
  }
  return PICP_OK;
}
