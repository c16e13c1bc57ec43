// picp_handle.cpp -- the single-problem handle picp_t (the pr::PICPSolver drop-in): device copies
// of the world and image points, the current correspondences gathered into the planes of a
// one-problem batch (picp_batch.h), and the pose.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "picp_c.h"
#include "picp_batch.h"
#include "picp_host.h"
#include "picp_launch.h"
#include "picp_pnp_host.h"

#define set_err picp_set_err

struct picp_handle {
  picp_batch* b = nullptr;
  DevBuf<float> world_d, image_d;
  int64_t n_world = 0, n_image = 0;
  DevBuf<int2> pairs_d;
  DevBuf<int64_t> pnp_offs;      // picp_relocalize: {0, m, the planes' offset}
  PnpRun pnp;                    // picp_relocalize: its device buffers, kept between calls
  std::vector<int32_t> pairs_h;  // cached copy of the current correspondences
  int64_t m = -1;                // -1: none set
  bool have_points = false;
  bool gathered = false;
  float pose[16];
};

static void identity16(float T[16]) {
  memset(T, 0, 16 * sizeof(float));
  T[0] = T[5] = T[10] = T[15] = 1.0f;
}

extern "C" int picp_create(picp_t** out, int device, int rows, int cols, const float K[9]) {
  CHECK_ARG(out && K, "picp_create: null argument");
  picp_handle* h = new picp_handle();
  identity16(h->pose);
  const int64_t offs[2] = {0, 0};
  int rc = batch_create(&h->b, device, 1, offs, rows, cols, K);
  if (rc) {
    delete h;
    return rc;
  }
  *out = h;
  return PICP_OK;
}

extern "C" int picp_destroy(picp_t* h) {
  if (!h) return PICP_OK;
  if (h->b) {
    hipSetDevice(h->b->device);
    hipStreamSynchronize(h->b->stream);
  }
  picp_batch_destroy(h->b);
  delete h;  // the device buffers free themselves
  return PICP_OK;
}

extern "C" int picp_set_camera(picp_t* h, int rows, int cols, const float K[9]) {
  CHECK_ARG(h && K, "picp_set_camera: null argument");
  CHECK_ARG(rows > 0 && cols > 0, "picp_set_camera: rows/cols must be positive");
  h->b->rows = rows;
  h->b->cols = cols;
  memcpy(h->b->K, K, sizeof(h->b->K));
  h->b->params_set = false;
  return PICP_OK;
}

// The copy constructor of the reference's PICPSolver copies every member, including the
// non-owning world/image pointers (src/picp_solver.h:72-81), so a copy solves the same problem.
// Here the points live on the device: the clone gets its own copies of them, the current
// correspondences and the pose (the cached gather is redone lazily).
extern "C" int picp_clone(const picp_t* src, picp_t** out) {
  CHECK_ARG(src && out, "picp_clone: null argument");
  const picp_batch* sb = src->b;
  picp_t* h = nullptr;
  int rc = picp_create(&h, sb->device, sb->rows, sb->cols, sb->K);
  if (rc) return rc;
  memcpy(h->pose, src->pose, sizeof(h->pose));
  auto fail = [&](int code) {
    picp_destroy(h);
    return code;
  };
  if (src->have_points) {
    HIP_TRY(hipSetDevice(sb->device));
    rc = h->world_d.grow(3 * src->n_world);
    if (rc) return fail(rc);
    rc = h->image_d.grow(2 * src->n_image);
    if (rc) return fail(rc);
    // the source's stream is drained first: its uploads may still be in flight
    hipError_t e = hipStreamSynchronize(sb->stream);
    if (e == hipSuccess && src->n_world)
      e = hipMemcpyAsync(h->world_d, src->world_d, (size_t)src->n_world * 3 * sizeof(float),
                         hipMemcpyDeviceToDevice, h->b->stream);
    if (e == hipSuccess && src->n_image)
      e = hipMemcpyAsync(h->image_d, src->image_d, (size_t)src->n_image * 2 * sizeof(float),
                         hipMemcpyDeviceToDevice, h->b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->b->stream);
    if (e != hipSuccess) return fail(set_err(PICP_ERR_DEVICE, "picp_clone: %s", hipGetErrorString(e)));
    h->n_world = src->n_world;
    h->n_image = src->n_image;
    h->have_points = true;
  }
  h->pairs_h = src->pairs_h;
  h->m = src->m;
  h->gathered = false;
  *out = h;
  return PICP_OK;
}

extern "C" int picp_set_points(picp_t* h, const float* world, int64_t n_world, const float* image,
                               int64_t n_image) {
  CHECK_ARG(h, "picp_set_points: null handle");
  CHECK_ARG(n_world >= 0 && n_image >= 0, "picp_set_points: negative size");
  CHECK_ARG((n_world == 0 || world) && (n_image == 0 || image), "picp_set_points: null array");
  HIP_TRY(hipSetDevice(h->b->device));
  int rc = h->world_d.grow(3 * n_world);
  if (rc) return rc;
  rc = h->image_d.grow(2 * n_image);
  if (rc) return rc;
  if (n_world) HIP_TRY(hipMemcpyAsync(h->world_d, world, (size_t)n_world * 3 * sizeof(float), hipMemcpyHostToDevice, h->b->stream));
  if (n_image) HIP_TRY(hipMemcpyAsync(h->image_d, image, (size_t)n_image * 2 * sizeof(float), hipMemcpyHostToDevice, h->b->stream));
  HIP_TRY(hipStreamSynchronize(h->b->stream));
  h->n_world = n_world;
  h->n_image = n_image;
  h->have_points = true;
  h->gathered = false;
  // the cached correspondences stay valid as indices but must be re-checked and re-gathered
  if (h->m >= 0) {
    for (int64_t k = 0; k < h->m; ++k) {
      if (h->pairs_h[2 * k] < 0 || h->pairs_h[2 * k] >= n_image || h->pairs_h[2 * k + 1] < 0 || h->pairs_h[2 * k + 1] >= n_world) {
        h->m = -1;
        h->pairs_h.clear();
        break;
      }
    }
  }
  return PICP_OK;
}

// Upload + gather the correspondences into the SoA planes if anything changed.
static int handle_prepare(picp_handle* h) {
  if (!h->have_points) return set_err(PICP_ERR_STATE, "points not set (call picp_set_points first)");
  if (h->m < 0) return set_err(PICP_ERR_STATE, "correspondences not set");
  if (h->gathered) return PICP_OK;
  picp_batch* b = h->b;
  HIP_TRY(hipSetDevice(b->device));
  if (b->total != h->m) {
    const int64_t offs[2] = {0, h->m};
    int rc = batch_layout(b, offs, 1);
    if (rc) return rc;
  }
  if (h->m > 0) {
    int rc = h->pairs_d.grow(h->m);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(h->pairs_d, h->pairs_h.data(), (size_t)h->m * sizeof(int2), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(picp_launch_gather(b->stream, h->world_d, h->image_d, h->pairs_d, h->m, b->X(), b->Y(), b->Z(), b->U(), b->V(), b->plane_off[0]));
  }
  HIP_TRY(hipStreamSynchronize(b->stream));
  h->gathered = true;
  return PICP_OK;
}

extern "C" int picp_set_correspondences(picp_t* h, const int32_t* pairs, int64_t m) {
  CHECK_ARG(h, "picp_set_correspondences: null handle");
  CHECK_ARG(m >= 0 && (m == 0 || pairs), "picp_set_correspondences: bad array");
  CHECK_ARG(m <= INT32_MAX, "picp_set_correspondences: too many correspondences");
  if (h->m == m && (m == 0 || memcmp(h->pairs_h.data(), pairs, (size_t)m * 2 * sizeof(int32_t)) == 0))
    return PICP_OK;  // same array as last time: keep the gathered planes
  if (!h->have_points) return set_err(PICP_ERR_STATE, "picp_set_correspondences: points not set");
  for (int64_t k = 0; k < m; ++k) {
    const int32_t ii = pairs[2 * k], wi = pairs[2 * k + 1];
    if (ii < 0 || ii >= h->n_image || wi < 0 || wi >= h->n_world)
      return set_err(PICP_ERR_RANGE, "correspondence %lld = (%d,%d) out of range (image %lld, world %lld)",
                     (long long)k, ii, wi, (long long)h->n_image, (long long)h->n_world);
  }
  h->pairs_h.assign(pairs, pairs + 2 * m);
  h->m = m;
  h->gathered = false;
  return PICP_OK;
}

extern "C" int picp_set_pose(picp_t* h, const float T[16]) {
  CHECK_ARG(h && T, "picp_set_pose: null argument");
  memcpy(h->pose, T, sizeof(h->pose));
  return PICP_OK;
}

extern "C" int picp_get_pose(picp_t* h, float T[16]) {
  CHECK_ARG(h && T, "picp_get_pose: null argument");
  memcpy(T, h->pose, sizeof(h->pose));
  return PICP_OK;
}

static int handle_upload_pose(picp_handle* h) {
  picp_batch* b = h->b;
  pose_to_state(h->pose, b->init_h[0]);
  HIP_TRY(hipMemcpyAsync(b->init_d, b->init_h.data(), sizeof(PicpState), hipMemcpyHostToDevice, b->stream));
  return PICP_OK;
}

extern "C" int picp_one_round(picp_t* h, float threshold, float damping, int min_inliers,
                              int keep_outliers, picp_stats* stats) {
  CHECK_ARG(h, "picp_one_round: null handle");
  int rc = handle_prepare(h);
  if (rc) return rc;
  picp_batch* b = h->b;
  picp_params prm;
  prm.threshold = threshold;
  prm.damping = damping;
  prm.min_inliers = min_inliers;
  prm.keep_outliers = keep_outliers;
  prm.max_rounds = 1;
  prm.conv_eps = -1.0f;  // the caller's loop owns the convergence test
  HIP_TRY(hipSetDevice(b->device));
  rc = batch_upload_params(b, &prm);
  if (rc) return rc;
  rc = handle_upload_pose(h);
  if (rc) return rc;
  HIP_TRY(graph_prologue(b));
  HIP_TRY(launch_round(b, 0));
  batch_solve_enqueued(b, 1, true);
  rc = batch_read_results(b);
  if (rc) return rc;
  const PicpState& s = b->result_h[0];
  if (stats) state_to_stats(s, *stats);
  if (!s.ok) return PICP_TOO_FEW_INLIERS;
  state_to_pose(s, h->pose);
  return PICP_OK;
}

extern "C" int picp_solve(picp_t* h, const picp_params* prm, picp_stats* stats) {
  CHECK_ARG(h && prm, "picp_solve: null argument");
  int rc = handle_prepare(h);
  if (rc) return rc;
  picp_batch* b = h->b;
  HIP_TRY(hipSetDevice(b->device));
  rc = handle_upload_pose(h);
  if (rc) return rc;
  rc = picp_batch_solve(b, prm);
  if (rc) return rc;
  const PicpState& s = b->result_h[0];
  if (stats) state_to_stats(s, *stats);
  state_to_pose(s, h->pose);
  return PICP_OK;
}

extern "C" int picp_linearize(picp_t* h, float threshold, int keep_outliers, double H[36],
                              double bvec[6], picp_stats* stats) {
  CHECK_ARG(h && H && bvec, "picp_linearize: null argument");
  int rc = handle_prepare(h);
  if (rc) return rc;
  picp_batch* b = h->b;
  picp_params prm;
  picp_params_default(&prm);
  prm.threshold = threshold;
  prm.keep_outliers = keep_outliers;
  prm.max_rounds = 1;
  prm.conv_eps = -1.0f;
  HIP_TRY(hipSetDevice(b->device));
  rc = batch_upload_params(b, &prm);
  if (rc) return rc;
  rc = handle_upload_pose(h);
  if (rc) return rc;
  HIP_TRY(graph_prologue(b));
  HIP_TRY(launch_round(b, 0));
  std::vector<float> part((size_t)b->nblk * PICP_NPART);  // the published words are float pairs
  HIP_TRY(hipMemcpyAsync(part.data(), b->part_d, part.size() * sizeof(float), hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  double tot[PICP_NPART] = {0};
  for (int k = 0; k < b->nblk; ++k)
    for (int e = 0; e < PICP_NPART; ++e) tot[e] += (double)part[(size_t)k * PICP_NPART + e];
  int idx = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) {
      H[c * 6 + r] = tot[PICP_P_H + idx];
      H[r * 6 + c] = tot[PICP_P_H + idx];
      ++idx;
    }
  for (int r = 0; r < 6; ++r) bvec[r] = tot[PICP_P_B + r];
  if (stats) {
    stats->chi_in = (float)tot[PICP_P_CHI_IN];
    stats->chi_out = (float)tot[PICP_P_CHI_OUT];
    stats->n_in = (int32_t)tot[PICP_P_N_IN];
    stats->n_projected = (int32_t)tot[PICP_P_N_PROJ];
    stats->ok = 1;
    stats->rounds = 0;
    stats->converged = 0;
    stats->reserved = 0;
  }
  return PICP_OK;
}

extern "C" int picp_classify(picp_t* h, float threshold, uint8_t* state, float* chi2, float* proj_uv,
                             int32_t* inlier_idx, int64_t counts[3]) {
  CHECK_ARG(h && counts, "picp_classify: null argument");
  int rc = handle_prepare(h);
  if (rc) return rc;
  return batch_classify(h->b, threshold, h->pose, state, chi2, proj_uv, nullptr, inlier_idx, counts);
}

// P3P RANSAC on the gathered planes (picp_pnp_host.h): problem 0 of a one-problem batch
extern "C" int picp_relocalize(picp_t* h, const picp_pnp_params* prm, int32_t* inliers) {
  CHECK_ARG(h, "picp_relocalize: null handle");
  int rc = handle_prepare(h);
  if (rc) return rc;
  picp_batch* b = h->b;
  PnpRun& R = h->pnp;
  rc = pnp_args(&R.A, b->K, b->rows, b->cols, prm, 1);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(b->device));
  const int64_t offs[3] = {0, h->m, h->m > 0 ? b->plane_off[0] : 0};
  if ((rc = h->pnp_offs.grow(3))) return rc;
  HIP_TRY(hipMemcpyAsync(h->pnp_offs, offs, sizeof(offs), hipMemcpyHostToDevice, b->stream));
  R.I = PnpItems{b->X(), b->Y(), b->Z(), b->U(), b->V(), 1, 1, h->pnp_offs, h->pnp_offs + 2};
  if ((rc = pnp_prepare(&R, b->stream, offs, false))) return rc;
  HIP_TRY(pnp_enqueue(&R, b->stream, nullptr, 0));
  float T[16];
  int32_t n_in = 0, found = 0;
  HIP_TRY(hipMemcpyAsync(T, R.T, sizeof(T), hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipMemcpyAsync(&n_in, R.inliers, sizeof(n_in), hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipMemcpyAsync(&found, R.found, sizeof(found), hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (inliers) *inliers = n_in;
  if (!found) return PICP_TOO_FEW_INLIERS;
  memcpy(h->pose, T, sizeof(h->pose));
  return PICP_OK;
}
