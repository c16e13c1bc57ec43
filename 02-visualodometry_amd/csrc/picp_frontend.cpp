// picp_frontend.cpp -- the stateless entry points of the VO front end: projection matrix,
// triangulation, essential-matrix bootstrap and descriptor matching (each call uploads, launches
// and downloads), and the self-test of the projection's reciprocal.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "picp_c.h"
#include "picp_host.h"
#include "picp_launch.h"
#include "picp_ransac_host.h"

#define set_err picp_set_err

// ------------------------------------------------------------------------------------
// triangulation
// ------------------------------------------------------------------------------------
extern "C" int picp_projection_matrix(const float K[9], const float T_cw[16], float P[12]) {
  CHECK_ARG(K && T_cw && P, "picp_projection_matrix: null argument");
  // inverse of a rigid transform (Eigen Isometry3f::inverse), then K * [R|t]
  float Ri[9], ti[3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Ri[j * 3 + i] = T_cw[i * 4 + j];
  for (int i = 0; i < 3; ++i) {
    float s = Ri[0 * 3 + i] * T_cw[12 + 0];
    s = s + Ri[1 * 3 + i] * T_cw[12 + 1];
    s = s + Ri[2 * 3 + i] * T_cw[12 + 2];
    ti[i] = -s;
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) {
      float m0 = (j < 3) ? Ri[j * 3 + 0] : ti[0];
      float m1 = (j < 3) ? Ri[j * 3 + 1] : ti[1];
      float m2 = (j < 3) ? Ri[j * 3 + 2] : ti[2];
      float s = K[0 * 3 + i] * m0;
      s = s + K[1 * 3 + i] * m1;
      s = s + K[2 * 3 + i] * m2;
      P[i * 4 + j] = s;
    }
  return PICP_OK;
}

extern "C" int picp_triangulate(int device, const float P1[12], const float P2[12],
                                const float* uv1, const float* uv2, int64_t q, float* xyz) {
  CHECK_ARG(P1 && P2, "picp_triangulate: null projection matrix");
  CHECK_ARG(q >= 0 && (q == 0 || (uv1 && uv2 && xyz)), "picp_triangulate: bad arrays");
  if (q == 0) return PICP_OK;
  if (int rc = select_device("picp_triangulate", device)) return rc;
  const size_t bytes = 2 * 12 * sizeof(float) + (size_t)q * (2 + 2 + 3) * sizeof(float);
  char* buf = nullptr;
  HIP_TRY(hipMalloc(&buf, bytes));
  float* dP = (float*)buf;
  float* duv1 = dP + 24;
  float* duv2 = duv1 + 2 * q;
  float* dxyz = duv2 + 2 * q;
  hipError_t e = hipMemcpy(dP, P1, 12 * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dP + 12, P2, 12 * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(duv1, uv1, (size_t)q * 2 * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(duv2, uv2, (size_t)q * 2 * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = picp_launch_triangulate(nullptr, dP, dP + 12, (const float2*)duv1, (const float2*)duv2, q, dxyz);
  if (e == hipSuccess) e = hipMemcpy(xyz, dxyz, (size_t)q * 3 * sizeof(float), hipMemcpyDeviceToHost);
  hipFree(buf);
  if (e != hipSuccess) return set_err(PICP_ERR_DEVICE, "picp_triangulate: %s", hipGetErrorString(e));
  return PICP_OK;
}

// ------------------------------------------------------------------------------------
// essential-matrix bootstrap (src/cam.cpp:37-91: findEssentialMat + recoverPose)
// ------------------------------------------------------------------------------------
extern "C" void picp_essential_params_default(picp_essential_params* p) {
  if (!p) return;
  p->prob = 0.999;       // cv::findEssentialMat defaults (src/cam.cpp:49-54 passes none)
  p->threshold = 1.0;
  p->max_iters = 1000;
  p->dist = 50.0;        // cv::recoverPose distanceThresh default
}

extern "C" int picp_essential_batch(int device, int n_problems, const int64_t* offs, const float* p1,
                                    const float* p2, const float K[9], const picp_essential_params* prm,
                                    float* T_out, int32_t* inliers, int32_t* good, uint8_t* mask) {
  CHECK_ARG(n_problems >= 1 && offs && K && T_out && inliers && good, "picp_essential_batch: null argument");
  if (int rc = check_ragged_batch("picp_essential_batch", n_problems, offs, p1, p2)) return rc;
  const int64_t total = offs[n_problems];
  picp_essential_params dp;
  picp_essential_params_default(&dp);
  const picp_essential_params& P = prm ? *prm : dp;
  CHECK_ARG(P.max_iters >= 1 && P.max_iters <= 100000, "picp_essential_batch: max_iters out of range");
  CHECK_ARG(P.threshold > 0.0 && P.prob > 0.0 && P.prob < 1.0 && P.dist > 0.0, "picp_essential_batch: bad params");
  CHECK_ARG(K[0] != 0.0f && K[4] != 0.0f, "picp_essential_batch: K has a zero focal length");
  if (int rc = select_device("picp_essential_batch", device)) return rc;
  EssArgs A;
  memset(&A, 0, sizeof(A));
  A.n_problems = n_problems;
  A.max_iters = P.max_iters;
  A.fx = K[0];  // column-major 3x3 (src/camera.h:45): K(0,0), K(1,1), K(0,2), K(1,2)
  A.fy = K[4];
  A.cx = K[6];
  A.cy = K[7];
  A.prob = P.prob;
  A.threshold = P.threshold;
  A.dist = P.dist;
  const size_t H = (size_t)n_problems * P.max_iters;
  const size_t pts = (size_t)std::max<int64_t>(total, 1) * 2 * sizeof(float);
  // one allocation carved into 256-byte-aligned sub-buffers (sizes rounded the same way)
  auto r256 = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t bytes = r256((size_t)(n_problems + 1) * 8) + 2 * r256(pts) + r256(H * 5 * 4) + r256(H * 90 * 8) +
                       r256(H * 4) + r256(H * 10 * 4) + r256((size_t)n_problems * 16 * 4) +
                       2 * r256((size_t)n_problems * 4) + r256((size_t)std::max<int64_t>(total, 1));
  char* buf = nullptr;
  HIP_TRY(hipMalloc(&buf, bytes));
  size_t at = 0;
  auto carve = [&](size_t b) { char* q = buf + at; at += r256(b); return q; };
  int64_t* d_offs = (int64_t*)carve((size_t)(n_problems + 1) * 8);
  float* d_p1 = (float*)carve(pts);
  float* d_p2 = (float*)carve(pts);
  int32_t* d_idx = (int32_t*)carve(H * 5 * 4);
  double* d_Es = (double*)carve(H * 90 * 8);
  int32_t* d_ns = (int32_t*)carve(H * 4);
  int32_t* d_cnt = (int32_t*)carve(H * 10 * 4);
  float* d_T = (float*)carve((size_t)n_problems * 16 * 4);
  int32_t* d_in = (int32_t*)carve((size_t)n_problems * 4);
  int32_t* d_good = (int32_t*)carve((size_t)n_problems * 4);
  uint8_t* d_mask = mask ? (uint8_t*)carve((size_t)std::max<int64_t>(total, 1)) : nullptr;
  hipError_t e = hipMemcpy(d_offs, offs, (size_t)(n_problems + 1) * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess && total > 0) e = hipMemcpy(d_p1, p1, (size_t)total * 2 * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess && total > 0) e = hipMemcpy(d_p2, p2, (size_t)total * 2 * sizeof(float), hipMemcpyHostToDevice);
  const char* stage = "upload";
  if (e == hipSuccess) {
    stage = "launch";
    e = picp_launch_essential(nullptr, &A, d_offs, d_p1, d_p2, d_idx, d_Es, d_ns, d_cnt, d_T, d_in, d_good, d_mask);
  }
  if (e == hipSuccess) {
    stage = "download T";
    e = hipMemcpy(T_out, d_T, (size_t)n_problems * 16 * 4, hipMemcpyDeviceToHost);
  }
  if (e == hipSuccess) {
    stage = "download inliers";
    e = hipMemcpy(inliers, d_in, (size_t)n_problems * 4, hipMemcpyDeviceToHost);
  }
  if (e == hipSuccess) {
    stage = "download good";
    e = hipMemcpy(good, d_good, (size_t)n_problems * 4, hipMemcpyDeviceToHost);
  }
  if (e == hipSuccess && mask && total > 0) {
    stage = "download mask";
    e = hipMemcpy(mask, d_mask, (size_t)total, hipMemcpyDeviceToHost);
  }
  hipFree(buf);
  if (e != hipSuccess) return set_err(PICP_ERR_DEVICE, "picp_essential_batch (%s): %s", stage, hipGetErrorString(e));
  return PICP_OK;
}

// ------------------------------------------------------------------------------------
// descriptor matching (match_points, src/my_utilities.h:70-120)
// ------------------------------------------------------------------------------------
extern "C" int picp_match_batch_form(int device, int n_problems, const int64_t* off1, const int64_t* off2,
                                     const float* desc1, const float* desc2, int dim, float dist_thr,
                                     float ratio_thr, int32_t* best_idx, float* best_dist,
                                     float* second_dist, int32_t* accepted, int form) {
  CHECK_ARG(form == PICP_MATCH_FORM_FULL || form == PICP_MATCH_FORM_ACCEPT_ONLY || form == PICP_MATCH_FORM_EXACT,
            "picp_match_batch_form: unknown form");
  CHECK_ARG(n_problems >= 1 && n_problems <= 65535 && off1 && off2, "picp_match_batch: bad problem table");
  CHECK_ARG(dim >= 1 && dim <= 32, "picp_match_batch: dim must be in [1, 32]");
  for (int i = 0; i < n_problems; ++i)
    CHECK_ARG(off1[0] == 0 && off2[0] == 0 && off1[i + 1] >= off1[i] && off2[i + 1] >= off2[i],
              "picp_match_batch: offsets must be prefix sums from 0");
  const int64_t n1 = off1[n_problems], n2 = off2[n_problems];
  CHECK_ARG((n1 == 0 || (desc1 && best_idx && best_dist && second_dist && accepted)) && (n2 == 0 || desc2),
            "picp_match_batch: null array");
  if (n1 == 0) return PICP_OK;
  if (int rc = select_device("picp_match_batch", device)) return rc;
  std::vector<MatchProblem> probs((size_t)n_problems);
  int64_t max_nq = 0;
  for (int i = 0; i < n_problems; ++i) {
    probs[i] = MatchProblem{off1[i], off1[i + 1] - off1[i], off2[i], off2[i + 1] - off2[i]};
    max_nq = std::max(max_nq, probs[i].nq);
  }
  const size_t b_probs = probs.size() * sizeof(MatchProblem);
  const size_t b_d1 = (size_t)n1 * dim * sizeof(float), b_d2 = (size_t)std::max<int64_t>(n2, 1) * dim * sizeof(float);
  const size_t b_out = (size_t)n1 * 4;
  const int dp = 16 * picp_match_prep_kch(dim);
  const size_t n2a = (size_t)std::max<int64_t>(n2, 1);
  const size_t b_prep = ((size_t)n1 + n2a) * (dp * sizeof(_Float16) + 2 * sizeof(float));
  // the reference-range split's scratch (picp_match_ksplit: few problems against many references)
  int64_t max_nr = 0;
  for (const MatchProblem& q : probs) max_nr = std::max(max_nr, q.nr);
  // (form bit 2 for the split rule: the folded form needs dim <= 12)
  const int ks = picp_match_ksplit(n_problems, max_nq, max_nr, form | (dim <= 12 ? 4 : 0));
  const int64_t part_cap = picp_match_split_scratch(ks, n_problems, max_nq);
  const size_t b_part = (size_t)part_cap * sizeof(float4);
  char* buf = nullptr;
  HIP_TRY(hipMalloc(&buf, b_probs + b_d1 + b_d2 + 4 * b_out + b_prep + b_part + 512));
  char* cur = buf;
  auto carve = [&](size_t bytes) { char* r = cur; cur += (bytes + 15) / 16 * 16; return r; };
  MatchProblem* d_probs = (MatchProblem*)carve(b_probs);
  float* d_d1 = (float*)carve(b_d1);
  float* d_d2 = (float*)carve(b_d2);
  int32_t* d_bi = (int32_t*)carve(b_out);
  float* d_bd = (float*)carve(b_out);
  float* d_sd = (float*)carve(b_out);
  int32_t* d_acc = (int32_t*)carve(b_out);
  _Float16* q_h = (_Float16*)carve((size_t)n1 * dp * sizeof(_Float16));
  float* q_n1 = (float*)carve((size_t)n1 * 4);
  float* q_n2 = (float*)carve((size_t)n1 * 4);
  _Float16* r_h = (_Float16*)carve(n2a * dp * sizeof(_Float16));
  float* r_n1 = (float*)carve(n2a * 4);
  float* r_n2 = (float*)carve(n2a * 4);
  float4* d_part = ks > 1 ? (float4*)carve(b_part) : nullptr;
  hipError_t e = hipMemcpy(d_probs, probs.data(), b_probs, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_d1, desc1, b_d1, hipMemcpyHostToDevice);
  if (e == hipSuccess && n2) e = hipMemcpy(d_d2, desc2, (size_t)n2 * dim * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = picp_launch_match_prep(nullptr, d_d1, n1, dim, q_h, q_n1, q_n2);
  if (e == hipSuccess && n2) e = picp_launch_match_prep(nullptr, d_d2, n2, dim, r_h, r_n1, r_n2);
  if (e == hipSuccess)
    e = picp_launch_match_mfma(nullptr, n_problems, max_nq, d_d1, d_d2, q_h, q_n1, r_h, r_n1, r_n2, d_probs,
                               dim, dist_thr, ratio_thr, d_bi, d_bd, d_sd, d_acc, form, ks, d_part,
                               part_cap);
  if (e == hipSuccess) e = hipMemcpy(best_idx, d_bi, b_out, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(best_dist, d_bd, b_out, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(second_dist, d_sd, b_out, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(accepted, d_acc, b_out, hipMemcpyDeviceToHost);
  hipFree(buf);
  if (e != hipSuccess) return set_err(PICP_ERR_DEVICE, "picp_match_batch: %s", hipGetErrorString(e));
  return PICP_OK;
}

extern "C" int picp_match_batch(int device, int n_problems, const int64_t* off1, const int64_t* off2,
                                const float* desc1, const float* desc2, int dim, float dist_thr,
                                float ratio_thr, int32_t* best_idx, float* best_dist,
                                float* second_dist, int32_t* accepted) {
  return picp_match_batch_form(device, n_problems, off1, off2, desc1, desc2, dim, dist_thr, ratio_thr, best_idx,
                               best_dist, second_dist, accepted, PICP_MATCH_FORM_FULL);
}

extern "C" int picp_match(int device, const float* desc1, int64_t n1, const float* desc2, int64_t n2,
                          int dim, float dist_thr, float ratio_thr, int32_t* best_idx,
                          float* best_dist, float* second_dist, int32_t* accepted) {
  CHECK_ARG(n1 >= 0 && n2 >= 0, "picp_match: negative size");
  const int64_t o1[2] = {0, n1}, o2[2] = {0, n2};
  return picp_match_batch(device, 1, o1, o2, desc1, desc2, dim, dist_thr, ratio_thr, best_idx, best_dist,
                          second_dist, accepted);
}

// ------------------------------------------------------------------------------------
// self-test: the fast correctly rounded reciprocal of the projection (picp_recip.h rcp_rn)
// ------------------------------------------------------------------------------------
extern "C" int picp_selftest_rcp(int device, int e_lo, int e_hi, uint64_t* mismatches) {
  CHECK_ARG(mismatches && e_lo >= -126 && e_hi <= 127 && e_lo < e_hi, "picp_selftest_rcp: bad argument");
  HIP_TRY(hipSetDevice(device));
  unsigned long long* d = nullptr;
  HIP_TRY(hipMalloc(&d, sizeof(unsigned long long)));
  hipError_t e = hipMemset(d, 0, sizeof(unsigned long long));
  if (e == hipSuccess) e = picp_launch_rcp_check(nullptr, e_lo, e_hi, d);
  unsigned long long h = 0;
  if (e == hipSuccess) e = hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost);
  hipFree(d);
  if (e != hipSuccess) return set_err(PICP_ERR_DEVICE, "picp_selftest_rcp: %s", hipGetErrorString(e));
  *mismatches = h;
  return PICP_OK;
}

// ------------------------------------------------------------------------------------
// self-test: the lane-parallel finish of a round against the uniform one (picp_solve6.h)
// ------------------------------------------------------------------------------------
extern "C" int picp_selftest_finish(int device, int64_t n_cases, const uint32_t* cases, uint64_t* mismatches,
                                    uint32_t* out) {
  CHECK_ARG(mismatches && cases && n_cases > 0 && n_cases <= (1 << 24), "picp_selftest_finish: bad argument");
  HIP_TRY(hipSetDevice(device));
  const size_t b_in = (size_t)n_cases * PICP_SELFTEST_FINISH_IN * 4, b_out = (size_t)n_cases * 2 * PICP_SELFTEST_FINISH_OUT * 4;
  const size_t o_out = (b_in + 255) & ~(size_t)255, o_bad = o_out + ((b_out + 255) & ~(size_t)255);
  char* buf = nullptr;
  HIP_TRY(hipMalloc(&buf, o_bad + sizeof(unsigned long long)));
  hipError_t e = hipMemcpy(buf, cases, b_in, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(buf + o_out, 0, o_bad + sizeof(unsigned long long) - o_out);
  if (e == hipSuccess)
    e = picp_launch_finish_check(nullptr, n_cases, (const unsigned*)buf, (unsigned long long*)(buf + o_bad),
                                 (unsigned*)(buf + o_out));
  unsigned long long h = 0;
  if (e == hipSuccess) e = hipMemcpy(&h, buf + o_bad, sizeof(h), hipMemcpyDeviceToHost);
  if (e == hipSuccess && out) e = hipMemcpy(out, buf + o_out, b_out, hipMemcpyDeviceToHost);
  hipFree(buf);
  if (e != hipSuccess) return set_err(PICP_ERR_DEVICE, "picp_selftest_finish: %s", hipGetErrorString(e));
  *mismatches = h;
  return PICP_OK;
}
