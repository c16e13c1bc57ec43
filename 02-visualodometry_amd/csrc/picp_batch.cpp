// picp_batch.cpp -- the batch solver behind picp_batch_* (include/picp_c.h): applies a layout plan
// (picp_layout.h) to device memory, enqueues the fused R-round solve in the plan's mode -- block /
// persistent mode one launch; graph mode a hipGraph of 1 memcpy node + 1 ticket memset node + R
// round launches, each finished in-launch by its last arriving block -- reads the results back,
// and falls back to a layout without hand-offs when a cross-block wait timed out.
#include <hip/hip_runtime.h>

#include <float.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "picp_c.h"
#include "picp_batch.h"
#include "picp_comm.h"
#include "picp_host.h"
#include "picp_launch.h"

#define set_err picp_set_err

// persistent launches and split block launches hand off through granules and report a timed-out
// wait in the error word at the head of the sync area
static bool uses_err_word(const picp_batch* b) {
  return b->mode == PICP_MODE_PERSISTENT || (b->mode == PICP_MODE_BLOCK && b->split > 1);
}

static void drop_graph(picp_batch* b) {
  if (b->gexec) hipGraphExecDestroy(b->gexec);
  if (b->graph) hipGraphDestroy(b->graph);
  b->gexec = nullptr;
  b->graph = nullptr;
  b->g_rounds = -1;
}

static_assert(sizeof(LayoutBlock) == sizeof(int4), "a block-table row is read as an int4");

// the limits of this device and of the kernels as built, for the layout plan
static LayoutCaps layout_caps(const picp_batch* b) {
  LayoutCaps c;
  c.num_cu = b->num_cu;
  c.block_max_items = picp_block_max_items();
  c.persistent_block = picp_persistent_block();
  c.block_threads = picp_block_threads;
  c.block_npt_cap = picp_block_npt_cap;
  c.persistent_occupancy = [b](int npt) {
    int occ = 0;
    return picp_persistent_occupancy(npt, b->K, &occ) == hipSuccess ? occ : 0;
  };
  c.block_occupancy = [b](int npt, int split, int max_n) {
    int occ = 0;
    return picp_block_occupancy(npt, split, max_n, b->K, &occ) == hipSuccess ? occ : 0;
  };
  return c;
}

// frees *p and, for n > 0, allocates n elements anew (the old contents are not kept)
template <class T>
static hipError_t renew(T** p, size_t n) {
  if (*p) hipFree(*p);
  *p = nullptr;
  return n ? hipMalloc(p, n * sizeof(T)) : hipSuccess;
}

// Device memory for the plan the batch holds: what is too small is discarded and allocated anew
// (a capacity reads 0 while its buffers are gone).  New planes and states are zero-filled.
static int batch_ensure_capacity(picp_batch* b) {
  const size_t np = (size_t)b->np, nblk = (size_t)b->nblk;
  if (b->plane_len > b->plane_cap) {
    const int64_t cap = round_up(b->plane_len, 1024);
    b->plane_cap = 0;
    hipError_t e = renew(&b->planes, (size_t)cap * 5);
    if (e != hipSuccess) return set_err(PICP_ERR_NOMEM, "hipMalloc planes (%lld floats): %s", (long long)cap * 5, hipGetErrorString(e));
    HIP_TRY(hipMemsetAsync(b->planes, 0, (size_t)cap * 5 * sizeof(float), b->stream));
    b->plane_cap = cap;
  }
  if (b->nblk > b->nblk_cap) {
    b->nblk_cap = 0;
    HIP_TRY(renew(&b->blk_d, nblk));
    HIP_TRY(renew(&b->part_d, nblk * (PICP_NPART / 2)));
    b->nblk_cap = b->nblk;
  }
  if (b->np > b->np_cap) {
    b->np_cap = 0;
    HIP_TRY(renew(&b->tickets_d, np));
    HIP_TRY(hipMemsetAsync(b->tickets_d, 0, np * sizeof(unsigned int), b->stream));
    HIP_TRY(renew(&b->probs_d, np));
    HIP_TRY(renew(&b->init_d, np));
    for (int k = 0; k < 2; ++k) {
      HIP_TRY(renew(&b->st_d[k], np));
      HIP_TRY(hipMemsetAsync(b->st_d[k], 0, np * sizeof(PicpState), b->stream));
    }
    if (b->st_pinned) hipHostFree(b->st_pinned);
    b->st_pinned = nullptr;
    HIP_TRY(hipHostMalloc((void**)&b->st_pinned, np * sizeof(PicpState), hipHostMallocDefault));
    b->np_cap = b->np;
  }
  if ((size_t)b->sync.bytes > b->sync_cap) {
    b->sync_cap = 0;
    HIP_TRY(renew(&b->sync_d, (size_t)b->sync.bytes));
    b->sync_cap = (size_t)b->sync.bytes;
  }
  return PICP_OK;
}

// (Re)build the partition for correspondence offsets `offs` (np+1 entries): plan (picp_layout.cpp),
// make room, upload.  Nothing of the batch is touched before the arguments are found good.
int batch_layout(picp_batch* b, const int64_t* offs, int np) {
  HIP_TRY(hipSetDevice(b->device));
  LayoutPlan plan;
  if (const char* msg = picp_layout_plan(offs, np, b->no_handoff, layout_caps(b), picp_layout_env(), &plan))
    return set_err(PICP_ERR_ARG, "%s", msg);
  if (offs != b->offs.data()) b->offs.assign(offs, offs + np + 1);  // the fallback passes b->offs itself
  static_cast<LayoutPlan&>(*b) = std::move(plan);
  int rc = batch_ensure_capacity(b);
  if (rc) return rc;
  if (b->sync.bytes) {
    // a new layout maps problems onto granules other problems tagged: start every tag from zero
    HIP_TRY(hipMemsetAsync(b->sync_d, 0, (size_t)b->sync.bytes, b->stream));
    b->tag_rounds = 0;
  }
  HIP_TRY(hipMemcpyAsync(b->blk_d, b->blocks.data(), (size_t)b->nblk * sizeof(int4), hipMemcpyHostToDevice, b->stream));
  HIP_TRY(hipMemcpyAsync(b->probs_d, b->probs.data(), (size_t)np * sizeof(PicpProblem), hipMemcpyHostToDevice, b->stream));
  // identity initial poses by default
  b->init_h.assign(np, PicpState{});
  for (int i = 0; i < np; ++i) {
    memset(&b->init_h[i], 0, sizeof(PicpState));
    b->init_h[i].R[0] = b->init_h[i].R[4] = b->init_h[i].R[8] = 1.0f;
    // the loop state at entry (what a zero-round solve returns; the kernels set it again)
    b->init_h[i].chi_prev = FLT_MAX;
    b->init_h[i].ok = 1;
  }
  HIP_TRY(hipMemcpyAsync(b->init_d, b->init_h.data(), (size_t)np * sizeof(PicpState), hipMemcpyHostToDevice, b->stream));
  b->result_h.assign(np, PicpState{});
  b->params_set = false;
  b->cls.ready = false;
  drop_graph(b);
  HIP_TRY(hipStreamSynchronize(b->stream));
  return PICP_OK;
}

int batch_upload_params(picp_batch* b, const picp_params* prm) {
  CHECK_ARG(prm, "null params");
  CHECK_ARG(prm->max_rounds >= 0 && prm->max_rounds <= 100000, "params.max_rounds out of range");
  CHECK_ARG(!(prm->threshold != prm->threshold), "params.threshold is NaN");
  if (b->params_set && memcmp(&b->params, prm, sizeof(picp_params)) == 0) return PICP_OK;
  PicpArgs& A = b->args;
  memset(&A, 0, sizeof(A));
  memcpy(A.K, b->K, sizeof(A.K));
  A.maxx = (float)(b->cols - 1);
  A.maxy = (float)(b->rows - 1);
  A.threshold = prm->threshold;
  A.damping = prm->damping;
  A.conv_eps = prm->conv_eps;
  A.min_inliers = prm->min_inliers;
  A.keep_outliers = prm->keep_outliers ? 1 : 0;
  A.max_rounds = prm->max_rounds;
  A.uniform = b->uniform;
  A.n_u = b->n_u;
  A.nblk_u = b->uniform ? b->nblk / b->np : 0;
  A.ipb = b->ipb;
  A.stride_u = b->stride_u;
  b->params = *prm;
  b->params_set = true;
  drop_graph(b);  // the arguments are baked into the captured launches
  return PICP_OK;
}

// graph mode: launch j reads st_d[(j+1)&1] and its last arrivers write st_d[j&1]; the initial
// states go to st_d[1], so after R launches the result is in st_d[(R-1)&1] (st_d[1] if R == 0)
hipError_t launch_round(picp_batch* b, int j) {
  const int in_buf = (j + 1) & 1;
  return picp_launch_round(b->stream, b->nblk, b->vec, b->X(), b->Y(), b->Z(), b->U(), b->V(), &b->args,
                           b->probs_d, b->blk_d, b->st_d[in_buf], b->st_d[in_buf ^ 1], b->part_d,
                           b->tickets_d, j);
}

static int graph_result_idx(int R) { return R >= 1 ? ((R - 1) & 1) : 1; }

void batch_solve_enqueued(picp_batch* b, int R, bool round_launches) {
  b->last_rounds = R;
  b->result_idx = round_launches ? graph_result_idx(R) : 0;
  b->last_persistent = !round_launches && uses_err_word(b);
}

// graph-mode prologue of every solve: initial states in, arrival tickets zeroed
hipError_t graph_prologue(picp_batch* b) {
  hipError_t e = hipMemcpyAsync(b->st_d[1], b->init_d, (size_t)b->np * sizeof(PicpState),
                                hipMemcpyDeviceToDevice, b->stream);
  if (e != hipSuccess) return e;
  return hipMemsetAsync(b->tickets_d, 0, (size_t)b->np * sizeof(unsigned int), b->stream);
}

// Enqueue a fused R-round solve on the stream: block / persistent mode one launch; graph mode
// the initial-state copy, the ticket memset and R round launches.
static hipError_t enqueue_solve(picp_batch* b, int R) {
  // hand-off modes: no memset per launch, the granule tags continue from the tag bases the previous
  // launch left (picp_persistent.hip, picp_block.hip), so nothing a previous launch wrote can match
  const SyncLayout& S = b->sync;
  unsigned int* err = S.bytes ? reinterpret_cast<unsigned int*>(b->sync_d + S.err) : nullptr;
  unsigned long long* gran = S.bytes ? reinterpret_cast<unsigned long long*>(b->sync_d + S.gran) : nullptr;
  unsigned int* tagbase = S.bytes ? reinterpret_cast<unsigned int*>(b->sync_d + S.tag) : nullptr;
  if (b->mode == PICP_MODE_BLOCK)
    return picp_launch_block(b->stream, b->np, b->npt, b->X(), b->Y(), b->Z(), b->U(), b->V(), &b->args,
                             b->probs_d, b->init_d, b->st_d[0], (int)b->max_n, b->split, gran, err, tagbase,
                             b->timeout_ticks);
  if (b->mode == PICP_MODE_PERSISTENT)
    return picp_launch_persistent(b->stream, b->nblk, b->npt, b->X(), b->Y(), b->Z(), b->U(), b->V(),
                                  &b->args, b->init_d, b->st_d[0], gran,
                                  reinterpret_cast<unsigned long long*>(b->sync_d + S.pose), err, tagbase,
                                  b->timeout_ticks);
  hipError_t e = graph_prologue(b);
  if (e != hipSuccess) return e;
  for (int j = 0; j < R; ++j) {
    e = launch_round(b, j);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

static int ensure_graph(picp_batch* b, int R) {
  if (b->gexec && b->g_rounds == R) return PICP_OK;
  drop_graph(b);
  HIP_TRY(hipStreamBeginCapture(b->stream, hipStreamCaptureModeThreadLocal));
  hipError_t e = enqueue_solve(b, R);
  hipGraph_t g = nullptr;
  hipError_t e2 = hipStreamEndCapture(b->stream, &g);
  if (e != hipSuccess) { if (g) hipGraphDestroy(g); return set_err(PICP_ERR_DEVICE, "capture: %s", hipGetErrorString(e)); }
  if (e2 != hipSuccess) return set_err(PICP_ERR_DEVICE, "end capture: %s", hipGetErrorString(e2));
  b->graph = g;
  HIP_TRY(hipGraphInstantiate(&b->gexec, g, nullptr, nullptr, 0));
  b->g_rounds = R;
  return PICP_OK;
}

// Persistent and split block modes: the 32-bit granule tags grow by up to max_rounds per solve.
// Zero the sync area (tags and error word) on the stream before they could wrap (long before 2^32).
static hipError_t persistent_tag_guard(picp_batch* b, int R, int solves) {
  if (!uses_err_word(b) || !b->sync_d) return hipSuccess;
  const uint64_t add = (uint64_t)std::max(R, 1) * (uint64_t)solves;
  if (b->tag_rounds + add > (1ull << 31)) {
    hipError_t e = hipMemsetAsync(b->sync_d, 0, (size_t)b->sync.bytes, b->stream);
    if (e != hipSuccess) return e;
    b->tag_rounds = 0;
  }
  b->tag_rounds += add;
  return hipSuccess;
}

// Enqueue one fused solve.  Persistent and block modes are ONE kernel launch: it goes to the
// stream directly (back-to-back launches queue behind each other with only the kernel-boundary
// gap; a one-node graph replay measured ~10 us more per solve).  Graph mode replays the captured
// prologue + R round launches.
static int enqueue_fused(picp_batch* b, int R) {
  if (b->mode == PICP_MODE_GRAPH) {
    int rc = ensure_graph(b, R);
    if (rc) return rc;
    HIP_TRY(hipGraphLaunch(b->gexec, b->stream));
  } else {
    HIP_TRY(enqueue_solve(b, R));
  }
  return PICP_OK;
}

static int batch_solve_async(picp_batch* b, const picp_params* prm) {
  HIP_TRY(hipSetDevice(b->device));
  int rc = batch_upload_params(b, prm);
  if (rc) return rc;
  const int R = prm->max_rounds;
  HIP_TRY(persistent_tag_guard(b, R, 1));
  rc = enqueue_fused(b, R);
  if (rc) return rc;
  batch_solve_enqueued(b, R, b->mode == PICP_MODE_GRAPH);
  return PICP_OK;
}


// A cross-block hand-off wait timed out (the blocks were not all resident: another process or
// stream held CUs, or the device time-sliced the launch).  Lay the batch out again without
// hand-offs (persistent -> graph mode, split block -> one block per problem), keep its data and
// initial poses, and re-run the same solve; later solves keep that layout.
static int batch_rerun_without_handoff(picp_batch* b) {
  const std::vector<PicpState> init = b->init_h;
  const picp_params prm = b->params;
  const int R = b->last_rounds;
  b->no_handoff = true;
  b->fallbacks++;
  int rc = batch_layout(b, b->offs.data(), b->np);
  if (rc) return rc;
  b->init_h = init;
  HIP_TRY(hipMemcpyAsync(b->init_d, b->init_h.data(), (size_t)b->np * sizeof(PicpState), hipMemcpyHostToDevice, b->stream));
  picp_params p2 = prm;
  p2.max_rounds = R;
  rc = batch_upload_params(b, &p2);
  if (rc) return rc;
  rc = enqueue_fused(b, R);
  if (rc) return rc;
  batch_solve_enqueued(b, R, b->mode == PICP_MODE_GRAPH);
  return PICP_OK;
}

int batch_read_results(picp_batch* b) {
  HIP_TRY(hipMemcpyAsync(b->st_pinned, b->st_d[b->result_idx], (size_t)b->np * sizeof(PicpState),
                         hipMemcpyDeviceToHost, b->stream));
  unsigned int err = 0;
  if (b->last_persistent && b->sync_d)
    HIP_TRY(hipMemcpyAsync(&err, b->sync_d + b->sync.err, sizeof(err), hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  memcpy(b->result_h.data(), b->st_pinned, (size_t)b->np * sizeof(PicpState));
  if (err) {
    // the error word is sticky (persistent launches no longer zero it): reset the whole sync
    // area so the next solve starts clean, then report
    HIP_TRY(hipMemsetAsync(b->sync_d, 0, (size_t)b->sync.bytes, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    b->tag_rounds = 0;
    if (b->no_handoff)  // cannot happen: that layout has no cross-block waits
      return set_err(PICP_ERR_DEVICE, "solve: a cross-block hand-off wait timed out (code %u)", err);
    int rc = batch_rerun_without_handoff(b);
    if (rc) return rc;
    return batch_read_results(b);
  }
  return PICP_OK;
}

int batch_create(picp_batch** out, int device, int np, const int64_t* offs, int rows,
                        int cols, const float K[9]) {
  CHECK_ARG(out && offs && K, "picp_batch_create: null argument");
  CHECK_ARG(rows > 0 && cols > 0, "picp_batch_create: rows/cols must be positive");
  if (int rc = select_device("picp_batch_create", device)) return rc;
  picp_batch* b = new picp_batch();
  b->device = device;
  b->rows = rows;
  b->cols = cols;
  memcpy(b->K, K, sizeof(b->K));
  picp_params_default(&b->params);
  hipError_t e = hipDeviceGetAttribute(&b->num_cu, hipDeviceAttributeMultiprocessorCount, device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
  if (const char* t = getenv("PICP_TIMEOUT_MS")) b->timeout_ticks = (unsigned long long)(atof(t) * 1e5);
  if (e != hipSuccess) {
    delete b;
    return set_err(PICP_ERR_DEVICE, "stream create: %s", hipGetErrorString(e));
  }
  int rc = batch_layout(b, offs, np);
  if (rc) {
    picp_batch_destroy(b);
    return rc;
  }
  *out = b;
  return PICP_OK;
}

extern "C" int picp_batch_create(picp_batch_t** out, int device, int n_problems,
                                 const int64_t* corr_offsets, int rows, int cols,
                                 const float K[9]) {
  return batch_create(out, device, n_problems, corr_offsets, rows, cols, K);
}

extern "C" int picp_batch_destroy(picp_batch_t* b) {
  if (!b) return PICP_OK;
  hipSetDevice(b->device);
  if (b->stream) hipStreamSynchronize(b->stream);
  drop_graph(b);
  renew(&b->planes, 0);
  renew(&b->blk_d, 0);
  renew(&b->part_d, 0);
  renew(&b->tickets_d, 0);
  renew(&b->probs_d, 0);
  renew(&b->init_d, 0);
  for (int k = 0; k < 2; ++k) renew(&b->st_d[k], 0);
  renew(&b->sync_d, 0);
  if (b->st_pinned) hipHostFree(b->st_pinned);
  if (b->cls.pinned) hipHostFree(b->cls.pinned);
  if (b->stream) hipStreamDestroy(b->stream);
  delete b;  // the classify pass's device buffers free themselves
  return PICP_OK;
}

extern "C" int picp_batch_set_data(picp_batch_t* b, const float* xyz, const float* uv) {
  CHECK_ARG(b && (b->total == 0 || (xyz && uv)), "picp_batch_set_data: null argument");
  HIP_TRY(hipSetDevice(b->device));
  std::vector<float> host((size_t)b->plane_len * 5, 0.0f);
  float* hx = host.data();
  float* hy = hx + b->plane_len;
  float* hz = hy + b->plane_len;
  float* hu = hz + b->plane_len;
  float* hv = hu + b->plane_len;
  for (int i = 0; i < b->np; ++i) {
    const int64_t n = b->offs[i + 1] - b->offs[i], src = b->offs[i], dst = b->plane_off[i];
    for (int64_t k = 0; k < n; ++k) {
      hx[dst + k] = xyz[3 * (src + k) + 0];
      hy[dst + k] = xyz[3 * (src + k) + 1];
      hz[dst + k] = xyz[3 * (src + k) + 2];
      hu[dst + k] = uv[2 * (src + k) + 0];
      hv[dst + k] = uv[2 * (src + k) + 1];
    }
  }
  for (int c = 0; c < 5; ++c)
    HIP_TRY(hipMemcpyAsync(b->planes + (size_t)c * b->plane_cap, host.data() + (size_t)c * b->plane_len,
                           (size_t)b->plane_len * sizeof(float), hipMemcpyHostToDevice, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return PICP_OK;
}

extern "C" int picp_batch_set_data_device(picp_batch_t* b, const float* dx, const float* dy,
                                          const float* dz, const float* du, const float* dv) {
  CHECK_ARG(b && (b->total == 0 || (dx && dy && dz && du && dv)), "picp_batch_set_data_device: null argument");
  HIP_TRY(hipSetDevice(b->device));
  const float* src[5] = {dx, dy, dz, du, dv};
  for (int i = 0; i < b->np; ++i) {
    const int64_t n = b->offs[i + 1] - b->offs[i];
    if (n == 0) continue;
    for (int c = 0; c < 5; ++c)
      HIP_TRY(hipMemcpyAsync(b->planes + (size_t)c * b->plane_cap + b->plane_off[i], src[c] + b->offs[i],
                             (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, b->stream));
  }
  HIP_TRY(hipStreamSynchronize(b->stream));
  return PICP_OK;
}

extern "C" int picp_batch_set_poses(picp_batch_t* b, const float* T) {
  CHECK_ARG(b && T, "picp_batch_set_poses: null argument");
  HIP_TRY(hipSetDevice(b->device));
  for (int i = 0; i < b->np; ++i) pose_to_state(T + 16 * (size_t)i, b->init_h[i]);
  HIP_TRY(hipMemcpyAsync(b->init_d, b->init_h.data(), (size_t)b->np * sizeof(PicpState), hipMemcpyHostToDevice, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  // the batch's current poses (picp_batch_get_poses, picp_batch_classify's default) are these
  // until the next solve completes; the stats of the last solve stay
  for (int i = 0; i < b->np; ++i) pose_to_state(T + 16 * (size_t)i, b->result_h[i]);
  return PICP_OK;
}

extern "C" int picp_batch_get_poses(picp_batch_t* b, float* T) {
  CHECK_ARG(b && T, "picp_batch_get_poses: null argument");
  for (int i = 0; i < b->np; ++i) state_to_pose(b->result_h[i], T + 16 * (size_t)i);
  return PICP_OK;
}

extern "C" int picp_batch_get_stats(picp_batch_t* b, picp_stats* st) {
  CHECK_ARG(b && st, "picp_batch_get_stats: null argument");
  for (int i = 0; i < b->np; ++i) state_to_stats(b->result_h[i], st[i]);
  return PICP_OK;
}

extern "C" int picp_batch_solve_async(picp_batch_t* b, const picp_params* prm) {
  CHECK_ARG(b, "picp_batch_solve_async: null batch");
  return batch_solve_async(b, prm);
}

extern "C" int picp_batch_sync(picp_batch_t* b) {
  CHECK_ARG(b, "picp_batch_sync: null batch");
  HIP_TRY(hipSetDevice(b->device));
  return batch_read_results(b);
}

extern "C" int picp_batch_solve(picp_batch_t* b, const picp_params* prm) {
  CHECK_ARG(b, "picp_batch_solve: null batch");
  int rc = batch_solve_async(b, prm);
  if (rc) return rc;
  return batch_read_results(b);
}

extern "C" int picp_batch_info(picp_batch_t* b, int64_t* total, int* nblk, int* mode) {
  CHECK_ARG(b, "picp_batch_info: null batch");
  if (total) *total = b->total;
  if (nblk) *nblk = b->nblk;
  if (mode) *mode = b->mode;
  return PICP_OK;
}


extern "C" int picp_batch_time(picp_batch_t* b, const picp_params* prm, int reps,
                               float* total_ms, float* launch_us) {
  CHECK_ARG(b && prm && reps > 0, "picp_batch_time: bad argument");
  HIP_TRY(hipSetDevice(b->device));
  // A hand-off wait that timed out inside the region is only seen by batch_read_results after
  // it, which re-runs the solve without hand-offs (fallbacks + 1).  The region's time then
  // includes the timed-out launches, so it is measured once more under the new layout.
  for (int attempt = 0;; ++attempt) {
    int rc = batch_upload_params(b, prm);
    if (rc) return rc;
    const int R = prm->max_rounds;
    if (b->mode == PICP_MODE_GRAPH) {
      rc = ensure_graph(b, R);  // captured before the timed region
      if (rc) return rc;
    }
    EventPair ev;
    HIP_TRY(ev.create());
    HIP_TRY(persistent_tag_guard(b, R, reps));
    HIP_TRY(hipEventRecord(ev.a, b->stream));
    for (int r = 0; r < reps; ++r) {
      rc = enqueue_fused(b, R);
      if (rc) return rc;
    }
    HIP_TRY(hipEventRecord(ev.b, b->stream));
    HIP_TRY(hipEventSynchronize(ev.b));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
    if (total_ms) *total_ms = ms;
    batch_solve_enqueued(b, R, b->mode == PICP_MODE_GRAPH);
    // mean launch period of the dominant kernel inside the region (graph mode: R round launches
    // per solve; otherwise one launch per solve); back-to-back launches, so this is the
    // per-launch duration a kernel trace reports plus the boundary gap
    const int launches = (b->mode == PICP_MODE_GRAPH) ? std::max(R, 1) : 1;
    if (launch_us) *launch_us = 1000.0f * ms / (float)(reps * launches);
    const int fb0 = b->fallbacks;
    rc = batch_read_results(b);
    if (rc || b->fallbacks == fb0) return rc;
    if (attempt >= 1)
      return set_err(PICP_ERR_STATE, "picp_batch_time: hand-off waits timed out again after the fallback");
  }
}

extern "C" int picp_batch_time_single(picp_batch_t* b, const picp_params* prm, float* us) {
  CHECK_ARG(b && prm && us, "picp_batch_time_single: bad argument");
  HIP_TRY(hipSetDevice(b->device));
  int rc = batch_upload_params(b, prm);
  if (rc) return rc;
  const int R = prm->max_rounds;
  HIP_TRY(persistent_tag_guard(b, R, 1));
  if (b->mode != PICP_MODE_GRAPH) {
    EventPair ev;
    HIP_TRY(ev.create());
    HIP_TRY(hipEventRecord(ev.a, b->stream));
    HIP_TRY(enqueue_solve(b, R));
    HIP_TRY(hipEventRecord(ev.b, b->stream));
    HIP_TRY(hipEventSynchronize(ev.b));
    float t = 0.0f;
    HIP_TRY(hipEventElapsedTime(&t, ev.a, ev.b));
    *us = 1000.0f * t;
    batch_solve_enqueued(b, R, false);
    return batch_read_results(b);
  }
  std::vector<EventPair> ev((size_t)std::max(R, 1));
  for (auto& e : ev) HIP_TRY(e.create());
  HIP_TRY(graph_prologue(b));
  for (int j = 0; j < R; ++j) {
    HIP_TRY(hipEventRecord(ev[j].a, b->stream));
    HIP_TRY(launch_round(b, j));
    HIP_TRY(hipEventRecord(ev[j].b, b->stream));
  }
  if (R > 0) HIP_TRY(hipEventSynchronize(ev[R - 1].b));
  double sum = 0.0;
  for (int j = 0; j < R; ++j) {
    float t = 0.0f;
    HIP_TRY(hipEventElapsedTime(&t, ev[j].a, ev[j].b));
    sum += 1000.0 * t;
  }
  *us = R > 0 ? (float)(sum / R) : 0.0f;
  batch_solve_enqueued(b, R, true);
  return batch_read_results(b);
}

extern "C" int picp_batch_residency(picp_batch_t* b, int* grid, int* resident, int* fallbacks) {
  CHECK_ARG(b, "picp_batch_residency: null batch");
  if (grid) *grid = b->handoff_grid;
  if (resident) *resident = b->handoff_resident;
  if (fallbacks) *fallbacks = b->fallbacks;
  return PICP_OK;
}

static void gather_to_poses(const PicpState* all, int64_t n_total, float* T_all, picp_stats* st_all) {
  for (int64_t k = 0; k < n_total; ++k) {
    state_to_pose(all[k], T_all + 16 * k);
    if (st_all) state_to_stats(all[k], st_all[k]);
  }
}

// Gather every rank's results of the batch split: this rank's batch holds the
// problems picp_shard_range(n_total, world, rank) gives it; after its solve, one RCCL all-gather
// of the 128-B per-problem states (on the batch's stream, device to device over xGMI) and one
// copy to the host give every rank all n_total poses and stats in problem order.
extern "C" int picp_batch_allgather(picp_batch_t* b, picp_comm_t* c, int64_t n_total, float* T_all,
                                    picp_stats* st_all) {
  CHECK_ARG(c, "picp_batch_allgather: null communicator");
  const int world = picp_comm_world(c), rank = picp_comm_rank(c);
  // Local checks first, agreed on by every rank before the collective: a rank that returned here
  // alone would leave the others blocked in the all-gather.
  int rc = PICP_OK;
  int64_t f0 = 0, f1 = 0;
  void* send = nullptr;
  const int64_t maxn = std::max<int64_t>(picp_shard_pad(n_total, world), 1);
  const size_t bytes = (size_t)maxn * sizeof(PicpState);
  if (!b || !T_all) rc = set_err(PICP_ERR_ARG, "picp_batch_allgather: null argument");
  else if (picp_comm_device(c) != b->device)
    rc = set_err(PICP_ERR_ARG, "picp_batch_allgather: communicator and batch are on different devices");
  else if ((rc = picp_shard_range(n_total, world, rank, &f0, &f1)) == PICP_OK && f1 - f0 != b->np)
    rc = set_err(PICP_ERR_ARG, "picp_batch_allgather: the batch does not hold this rank's shard of n_total");
  if (rc == PICP_OK && hipSetDevice(b->device) != hipSuccess)
    rc = set_err(PICP_ERR_DEVICE, "picp_batch_allgather: hipSetDevice failed");
  if (rc == PICP_OK) rc = batch_read_results(b);  // the solve is complete (re-run if a hand-off timed out)
  if (rc == PICP_OK && !(send = picp_comm_send_buffer(c, bytes)))
    rc = set_err(PICP_ERR_NOMEM, "picp_batch_allgather: staging buffer of %zu B", bytes);
  double fail = (rc == PICP_OK) ? 0.0 : 1.0;
  const std::string local_err = rc ? picp_last_error() : "";
  const int rc2 = picp_comm_allreduce_max(c, &fail, 1);
  if (rc) return set_err(rc, "%s", local_err.c_str());
  if (rc2) return rc2;
  if (fail != 0.0) return set_err(PICP_ERR_STATE, "picp_batch_allgather: another rank failed before the all-gather");
  HIP_TRY(hipMemcpyAsync(send, b->st_d[b->result_idx], (size_t)b->np * sizeof(PicpState), hipMemcpyDeviceToDevice,
                         b->stream));
  const void* recv = nullptr;
  rc = picp_comm_allgather_dev(c, send, bytes, b->stream, &recv);
  if (rc) return rc;
  std::vector<PicpState> padded((size_t)world * maxn), all((size_t)std::max<int64_t>(n_total, 1));
  HIP_TRY(hipMemcpyAsync(padded.data(), recv, padded.size() * sizeof(PicpState), hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  rc = picp_shard_unpack(n_total, world, sizeof(PicpState), padded.data(), all.data());
  if (rc) return rc;
  gather_to_poses(all.data(), n_total, T_all, st_all);
  return PICP_OK;
}

// The gather with a caller-supplied byte exchange (include/picp_c.h): the same shard check,
// completion and padded state layout as picp_batch_allgather, staged through host memory.  Each
// rank's send buffer is [16-B header: int32 status][maxn states]; one exchange carries both, so
// the failure agreement needs no second collective.
extern "C" int picp_batch_allgather_host(picp_batch_t* b, int world, int rank, picp_exchange_fn exchange,
                                         void* user, int64_t n_total, float* T_all, picp_stats* st_all) {
  CHECK_ARG(exchange && world >= 1 && rank >= 0 && rank < world && n_total >= 0,
            "picp_batch_allgather_host: bad exchange or world/rank");
  int rc = PICP_OK;
  int64_t f0 = 0, f1 = 0;
  const int64_t maxn = std::max<int64_t>(picp_shard_pad(n_total, world), 1);
  constexpr size_t HDR = 16;
  const size_t bytes = HDR + (size_t)maxn * sizeof(PicpState);
  if (!b || !T_all) rc = set_err(PICP_ERR_ARG, "picp_batch_allgather_host: null argument");
  else if ((rc = picp_shard_range(n_total, world, rank, &f0, &f1)) == PICP_OK && f1 - f0 != b->np)
    rc = set_err(PICP_ERR_ARG, "picp_batch_allgather_host: the batch does not hold this rank's shard of n_total");
  if (rc == PICP_OK && hipSetDevice(b->device) != hipSuccess)
    rc = set_err(PICP_ERR_DEVICE, "picp_batch_allgather_host: hipSetDevice failed");
  if (rc == PICP_OK) rc = batch_read_results(b);  // the solve is complete (re-run if a hand-off timed out)
  const std::string local_err = rc ? picp_last_error() : "";
  std::vector<char> send(bytes, 0), recv(bytes * (size_t)world, 0);
  const int32_t status = rc;
  memcpy(send.data(), &status, sizeof(status));
  if (rc == PICP_OK) memcpy(send.data() + HDR, b->result_h.data(), (size_t)b->np * sizeof(PicpState));
  const int xr = exchange(user, send.data(), recv.data(), bytes);
  if (rc) return set_err(rc, "%s", local_err.c_str());
  if (xr != 0) return set_err(PICP_ERR_STATE, "picp_batch_allgather_host: the exchange failed (%d)", xr);
  std::vector<PicpState> padded((size_t)world * maxn), all((size_t)std::max<int64_t>(n_total, 1));
  for (int r = 0; r < world; ++r) {
    int32_t st = 0;
    memcpy(&st, recv.data() + (size_t)r * bytes, sizeof(st));
    if (st != PICP_OK)
      return set_err(PICP_ERR_STATE, "picp_batch_allgather_host: rank %d failed before the exchange (%d)", r, st);
    memcpy(padded.data() + (size_t)r * maxn, recv.data() + (size_t)r * bytes + HDR, (size_t)maxn * sizeof(PicpState));
  }
  rc = picp_shard_unpack(n_total, world, sizeof(PicpState), padded.data(), all.data());
  if (rc) return rc;
  gather_to_poses(all.data(), n_total, T_all, st_all);
  return PICP_OK;
}
