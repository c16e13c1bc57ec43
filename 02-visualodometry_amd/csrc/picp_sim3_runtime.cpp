// picp_sim3_runtime.cpp -- 3D-3D alignment by Sim(3) RANSAC (picp_sim3.hip): the run and the
// stateless batch calls, which upload, launch and download like the other front-end entry points
// (the parts shared with the P3P: picp_ransac_host.h).
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "picp_c.h"
#include "picp_host.h"
#include "picp_launch.h"
#include "picp_sim3_host.h"

#define SIM3_XF 16  // floats of a stored transform (picp_umeyama.h)

extern "C" void picp_sim3_params_default(picp_sim3_params* p) {
  if (!p) return;
  p->threshold = 0.01f;
  p->hypotheses = 256;
  p->min_inliers = 4;
  p->with_scale = 1;
  p->refits = 2;
  p->reserved = 0;
  p->seed = 0;
}

int sim3_args(Sim3Args* A, const picp_sim3_params* prm, int n_problems) {
  picp_sim3_params dp;
  picp_sim3_params_default(&dp);
  const picp_sim3_params& P = prm ? *prm : dp;
  CHECK_ARG(!(P.threshold != P.threshold), "sim3: threshold is NaN");
  CHECK_ARG(P.hypotheses >= 1 && P.hypotheses <= 65536, "sim3: hypotheses out of range [1, 65536]");
  CHECK_ARG(P.refits >= 0 && P.refits <= 8, "sim3: refits out of range [0, 8]");
  CHECK_ARG((int64_t)n_problems * P.hypotheses <= RANSAC_MAX_HYP, "sim3: more than 2^24 hypotheses in one call");
  memset(A, 0, sizeof(*A));
  A->threshold = P.threshold;
  A->with_scale = P.with_scale ? 1 : 0;
  A->seed = P.seed;
  A->n_problems = n_problems;
  A->hyp = P.hypotheses;
  A->min_inliers = P.min_inliers;
  A->refits = P.refits;
  return PICP_OK;
}

int sim3_prepare(Sim3Run* R, hipStream_t st, const int64_t* offs, bool want_mask, bool debug) {
  const int np = R->A.n_problems, H = R->A.hyp;
  int rc = ransac_grid_prepare(&R->grid, st, offs, np, H, picp_sim3_score_tile(), picp_sim3_hyp_tile(), "sim3",
                               "pairs");
  if (rc) return rc;
  const int64_t G = (int64_t)np * H;
  if ((rc = R->samples.grow(3 * G))) return rc;
  if ((rc = R->hyp_valid.grow(G))) return rc;
  if ((rc = R->cnt.grow(G))) return rc;
  if ((rc = R->hyp_S.grow(SIM3_XF * G))) return rc;
  if ((rc = R->win.grow(np))) return rc;
  if ((rc = R->S.grow(16 * (int64_t)np))) return rc;
  if ((rc = R->scale.grow(np))) return rc;
  if ((rc = R->rms.grow(np))) return rc;
  if ((rc = R->inliers.grow(np))) return rc;
  if ((rc = R->found.grow(np))) return rc;
  if (want_mask && (rc = R->mask.grow(offs[np]))) return rc;
  if (debug && R->A.refits) {
    if ((rc = R->refit_S.grow(SIM3_XF * (int64_t)np * R->A.refits))) return rc;
    if ((rc = R->refit_count.grow((int64_t)np * R->A.refits))) return rc;
  }
  return PICP_OK;
}

hipError_t sim3_enqueue(Sim3Run* R, hipStream_t st, TimedSpans* spans, int rep) {
  const int64_t G = (int64_t)R->A.n_problems * R->A.hyp;
  const RansacGrid& g = R->grid;
  hipError_t e = hipSuccess;
  auto begin = [&](int s) { return spans ? spans[s].begin(rep, st) : hipSuccess; };
  auto end = [&](int s) { return spans ? spans[s].end(rep, st) : hipSuccess; };
  if ((e = begin(0)) != hipSuccess) return e;
  e = picp_launch_ransac_samples(st, R->A.seed, R->A.prob0, R->A.n_problems, R->A.hyp, R->I.offs, R->samples);
  if (e != hipSuccess) return e;
  if ((e = end(0)) != hipSuccess || (e = begin(1)) != hipSuccess) return e;
  if ((e = picp_launch_sim3_hyp(st, &R->A, &R->I, R->samples, R->hyp_valid, R->hyp_S)) != hipSuccess) return e;
  if ((e = end(1)) != hipSuccess || (e = begin(2)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(R->cnt, 0, (size_t)G * sizeof(int32_t), st)) != hipSuccess) return e;
  if ((e = picp_launch_sim3_score(st, &R->A, &R->I, g.nb, g.blk, g.hsplit, R->hyp_valid, R->hyp_S, R->cnt)) !=
      hipSuccess)
    return e;
  if ((e = end(2)) != hipSuccess || (e = begin(3)) != hipSuccess) return e;
  if ((e = picp_launch_sim3_select(st, &R->A, R->hyp_valid, R->cnt, R->win)) != hipSuccess) return e;
  if ((e = end(3)) != hipSuccess || (e = begin(4)) != hipSuccess) return e;
  if ((e = picp_launch_sim3_refit(st, &R->A, &R->I, R->win, R->hyp_S, nullptr, R->refit_S, R->refit_count, R->S,
                                  R->scale, R->inliers, R->found, R->rms, R->mask)) != hipSuccess)
    return e;
  return end(4);
}

namespace {

int check_batch_args(int n_problems, const int64_t* offs, const float* src, const float* dst) {
  CHECK_ARG(n_problems >= 0, "picp_sim3_batch: negative problem count");
  CHECK_ARG(offs, "picp_sim3_batch: null argument");
  return check_ragged_batch("picp_sim3_batch", n_problems, offs, src, dst);
}

// the device and the packed inputs on it (a: src, b: dst)
int sim3_upload(Sim3Items* I, RansacUpload* U, int device, int n_problems, const int64_t* offs, const float* src,
                const float* dst) {
  int rc = select_device("picp_sim3_batch", device);
  if (rc) return rc;
  if ((rc = ransac_upload(U, n_problems, offs, src, 3, dst, 3))) return rc;
  *I = Sim3Items{U->a, U->a + 1, U->a + 2, U->b, U->b + 1, U->b + 2, 3, 3, U->offs, U->offs};
  return PICP_OK;
}

// everything up to the launches: arguments, device, upload, buffers
int sim3_setup(Sim3Run* R, RansacUpload* U, int device, int n_problems, const int64_t* offs, const float* src,
               const float* dst, const picp_sim3_params* prm, bool want_mask, bool debug) {
  int rc = sim3_args(&R->A, prm, n_problems);
  if (rc) return rc;
  if ((rc = sim3_upload(&R->I, U, device, n_problems, offs, src, dst))) return rc;
  return sim3_prepare(R, nullptr, offs, want_mask, debug);
}

// the stored transforms (M column-major, t, c) of `n` slots as column-major 4x4; an all-zero slot stays zero
void xf_to_4x4(const float* dev, size_t n, const int32_t* valid, float* out) {
  memset(out, 0, n * 16 * sizeof(float));
  for (size_t g = 0; g < n; ++g) {
    if (!valid[g]) continue;
    for (int c = 0; c < 3; ++c)
      for (int r = 0; r < 3; ++r) out[16 * g + 4 * c + r] = dev[SIM3_XF * g + 3 * c + r];
    for (int r = 0; r < 3; ++r) out[16 * g + 12 + r] = dev[SIM3_XF * g + 9 + r];
    out[16 * g + 15] = 1.0f;
  }
}

}  // namespace

extern "C" int picp_sim3_batch_debug(int device, int n_problems, const int64_t* offs, const float* src,
                                     const float* dst, const picp_sim3_params* prm, float* S_out, float* scale,
                                     int32_t* inliers, int32_t* found, float* rms, uint8_t* mask, int32_t* samples,
                                     int32_t* hyp_valid, float* hyp_S, int32_t* hyp_count, float* refit_S,
                                     int32_t* refit_count) {
  int rc = check_batch_args(n_problems, offs, src, dst);
  if (rc) return rc;
  Sim3Run R;
  RansacUpload U;
  if (n_problems == 0) return sim3_args(&R.A, prm, 0);
  const bool debug = refit_S || refit_count;
  if ((rc = sim3_setup(&R, &U, device, n_problems, offs, src, dst, prm, mask != nullptr, debug))) return rc;
  HIP_TRY(sim3_enqueue(&R, nullptr, nullptr, 0));
  const size_t np = (size_t)n_problems, G = np * (size_t)R.A.hyp, NR = np * (size_t)R.A.refits;
  if (S_out) HIP_TRY(hipMemcpy(S_out, R.S, np * 16 * sizeof(float), hipMemcpyDeviceToHost));
  if (scale) HIP_TRY(hipMemcpy(scale, R.scale, np * sizeof(float), hipMemcpyDeviceToHost));
  if (inliers) HIP_TRY(hipMemcpy(inliers, R.inliers, np * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (found) HIP_TRY(hipMemcpy(found, R.found, np * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (rms) HIP_TRY(hipMemcpy(rms, R.rms, np * sizeof(float), hipMemcpyDeviceToHost));
  if (mask && offs[n_problems]) HIP_TRY(hipMemcpy(mask, R.mask, (size_t)offs[n_problems], hipMemcpyDeviceToHost));
  if (samples) HIP_TRY(hipMemcpy(samples, R.samples, G * 3 * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (hyp_valid) HIP_TRY(hipMemcpy(hyp_valid, R.hyp_valid, G * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (hyp_count) HIP_TRY(hipMemcpy(hyp_count, R.cnt, G * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (hyp_S) {
    std::vector<float> dev(G * SIM3_XF);
    std::vector<int32_t> ok(G);
    HIP_TRY(hipMemcpy(dev.data(), R.hyp_S, dev.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ok.data(), R.hyp_valid, G * sizeof(int32_t), hipMemcpyDeviceToHost));
    xf_to_4x4(dev.data(), G, ok.data(), hyp_S);
  }
  if (debug && NR) {
    std::vector<float> dev(NR * SIM3_XF);
    std::vector<int32_t> c(NR);
    HIP_TRY(hipMemcpy(dev.data(), R.refit_S, dev.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(c.data(), R.refit_count, NR * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (refit_count) memcpy(refit_count, c.data(), NR * sizeof(int32_t));
    for (int32_t& v : c) v = v >= 0;
    if (refit_S) xf_to_4x4(dev.data(), NR, c.data(), refit_S);
  }
  HIP_TRY(hipDeviceSynchronize());
  return PICP_OK;
}

extern "C" int picp_sim3_batch(int device, int n_problems, const int64_t* offs, const float* src, const float* dst,
                               const picp_sim3_params* prm, float* S_out, float* scale, int32_t* inliers,
                               int32_t* found, float* rms, uint8_t* mask) {
  CHECK_ARG(n_problems <= 0 || (S_out && inliers && found), "picp_sim3_batch: null output");
  return picp_sim3_batch_debug(device, n_problems, offs, src, dst, prm, S_out, scale, inliers, found, rms, mask,
                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int picp_sim3_batch_time(int device, int n_problems, const int64_t* offs, const float* src,
                                    const float* dst, const picp_sim3_params* prm, int reps, float* us) {
  CHECK_ARG(us && reps > 0 && reps <= 1000 && n_problems >= 1, "picp_sim3_batch_time: bad argument");
  int rc = check_batch_args(n_problems, offs, src, dst);
  if (rc) return rc;
  Sim3Run R;
  RansacUpload U;
  if ((rc = sim3_setup(&R, &U, device, n_problems, offs, src, dst, prm, false, false))) return rc;
  return ransac_time_stages(5, reps, us, [&](TimedSpans* s, int r) { return sim3_enqueue(&R, nullptr, s, r); });
}

extern "C" int picp_sim3_fit_batch(int device, int n_problems, const int64_t* offs, const float* src,
                                   const float* dst, const uint8_t* mask, int with_scale, float* S_out, float* scale,
                                   float* rms, int32_t* found) {
  int rc = check_batch_args(n_problems, offs, src, dst);
  if (rc) return rc;
  if (n_problems == 0) return PICP_OK;
  CHECK_ARG(S_out && found, "picp_sim3_fit_batch: null output");
  for (int i = 0; i < n_problems; ++i)
    CHECK_ARG(offs[i + 1] - offs[i] <= INT32_MAX - 1, "picp_sim3_fit_batch: a problem has too many pairs");
  Sim3Args A;
  memset(&A, 0, sizeof(A));
  A.with_scale = with_scale ? 1 : 0;
  A.n_problems = n_problems;
  A.fit_only = 1;
  Sim3Items I;
  RansacUpload U;
  if ((rc = sim3_upload(&I, &U, device, n_problems, offs, src, dst))) return rc;
  const size_t np = (size_t)n_problems, total = (size_t)offs[n_problems];
  DevBuf<uint8_t> mask_d;
  if (mask && total) {
    if ((rc = mask_d.grow((int64_t)total))) return rc;
    HIP_TRY(hipMemcpy(mask_d, mask, total, hipMemcpyHostToDevice));
  }
  DevBuf<float> S, sc, rm;
  DevBuf<int32_t> fo;
  if ((rc = S.grow(16 * (int64_t)np)) || (rc = sc.grow(np)) || (rc = rm.grow(np)) || (rc = fo.grow(np))) return rc;
  HIP_TRY(picp_launch_sim3_refit(nullptr, &A, &I, nullptr, nullptr, (mask && total) ? (const uint8_t*)mask_d : nullptr,
                                 nullptr, nullptr, S, sc, nullptr, fo, rm, nullptr));
  HIP_TRY(hipMemcpy(S_out, S, np * 16 * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(found, fo, np * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (scale) HIP_TRY(hipMemcpy(scale, sc, np * sizeof(float), hipMemcpyDeviceToHost));
  if (rms) HIP_TRY(hipMemcpy(rms, rm, np * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipDeviceSynchronize());
  return PICP_OK;
}
