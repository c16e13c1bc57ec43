// picp_batch_classify.cpp -- the classify pass of a batch (picp_classify.hip): which
// correspondences a pose rests on.  Reads the planes and nothing else of the solver: its poses,
// tables and outputs are its own buffers, so a solve before or after it runs on exactly the data
// it would have without it.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "picp_c.h"
#include "picp_batch.h"
#include "picp_host.h"
#include "picp_launch.h"

static int64_t align256(int64_t x) { return round_up(x, 256); }

struct ClsLayout {  // byte offsets inside cls.tables and cls.scan
  int64_t blk, pblk, plane_off, pack_off, tables_bytes;
  int64_t cnt, base, counts, inl_off, scan_bytes;
};

static ClsLayout cls_layout(int nb, int np) {
  ClsLayout L;
  L.blk = 0;
  L.pblk = align256(L.blk + (int64_t)nb * sizeof(int4));
  L.plane_off = align256(L.pblk + (int64_t)np * sizeof(int2));
  L.pack_off = align256(L.plane_off + (int64_t)np * sizeof(int64_t));
  L.tables_bytes = align256(L.pack_off + (int64_t)np * sizeof(int64_t));
  L.cnt = 0;
  L.base = align256(L.cnt + 3 * (int64_t)nb * sizeof(int));
  L.counts = align256(L.base + 3 * ((int64_t)nb + 1) * sizeof(long long));
  L.inl_off = align256(L.counts + 3 * (int64_t)np * sizeof(long long));
  L.scan_bytes = align256(L.inl_off + ((int64_t)np + 1) * sizeof(long long));
  return L;
}

// Tables, tile counts and staging of the classify pass for the batch's current layout.
static int cls_prepare(picp_batch* b) {
  picp_batch::Classify& c = b->cls;
  if (c.ready) return PICP_OK;
  const int tile = picp_classify_tile();
  const int np = b->np;
  int64_t nb64 = 0;
  for (int i = 0; i < np; ++i) nb64 += std::max<int64_t>(1, (b->offs[i + 1] - b->offs[i] + tile - 1) / tile);
  CHECK_ARG(nb64 <= INT32_MAX / 4, "classify: too many tiles");
  const int nb = (int)nb64;
  const ClsLayout L = cls_layout(nb, np);
  int rc = c.tables.grow(L.tables_bytes);
  if (rc) return rc;
  rc = c.scan.grow(L.scan_bytes);
  if (rc) return rc;
  rc = c.st.grow(np);
  if (rc) return rc;
  const int64_t words = 4 * (int64_t)np + 1;
  if (words > c.pinned_cap) {
    if (c.pinned) hipHostFree(c.pinned);
    c.pinned = nullptr;
    c.pinned_cap = 0;
    HIP_TRY(hipHostMalloc((void**)&c.pinned, (size_t)words * sizeof(long long), hipHostMallocDefault));
    c.pinned_cap = words;
  }
  std::vector<char> host((size_t)L.tables_bytes, 0);
  int4* blk = reinterpret_cast<int4*>(host.data() + L.blk);
  int2* pblk = reinterpret_cast<int2*>(host.data() + L.pblk);
  int64_t* plane_off = reinterpret_cast<int64_t*>(host.data() + L.plane_off);
  int64_t* pack_off = reinterpret_cast<int64_t*>(host.data() + L.pack_off);
  int k = 0;
  for (int i = 0; i < np; ++i) {
    const int64_t n = b->offs[i + 1] - b->offs[i];
    const int nbp = (int)std::max<int64_t>(1, (n + tile - 1) / tile);
    pblk[i] = make_int2(k, nbp);
    plane_off[i] = b->plane_off[i];
    pack_off[i] = b->offs[i];
    for (int q = 0; q < nbp; ++q) {
      const int64_t first = (int64_t)q * tile;
      blk[k++] = make_int4(i, (int)first, (int)std::max<int64_t>(0, std::min<int64_t>(tile, n - first)), 0);
    }
  }
  HIP_TRY(hipMemcpyAsync(c.tables, host.data(), (size_t)L.tables_bytes, hipMemcpyHostToDevice, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));  // host is a local
  c.nb = nb;
  c.st_h.assign((size_t)np, PicpState{});
  c.ready = true;
  return PICP_OK;
}

// enqueue one pass at the poses in cls.st
static hipError_t cls_enqueue(picp_batch* b, float threshold, bool want_chi2, bool want_uv, bool want_idx) {
  picp_batch::Classify& c = b->cls;
  const ClsLayout L = cls_layout(c.nb, b->np);
  ClsArgs a;
  memset(&a, 0, sizeof(a));
  memcpy(a.K, b->K, sizeof(a.K));
  a.maxx = (float)(b->cols - 1);
  a.maxy = (float)(b->rows - 1);
  a.threshold = threshold;
  char* t = (char*)c.tables;
  char* s = (char*)c.scan;
  return picp_launch_classify(b->stream, c.nb, b->np, b->X(), b->Y(), b->Z(), b->U(), b->V(), &a,
                              (const int4*)(t + L.blk), (const int2*)(t + L.pblk), (const int64_t*)(t + L.plane_off),
                              (const int64_t*)(t + L.pack_off), c.st, c.state, want_chi2 ? c.chi2.p : nullptr,
                              want_uv ? c.uv.p : nullptr, (int*)(s + L.cnt), (long long*)(s + L.base),
                              (long long*)(s + L.counts), (long long*)(s + L.inl_off), want_idx ? c.idx.p : nullptr);
}

// the per-item device outputs a pass needs, and the poses (T: 16 per problem, or the batch's
// current ones) in cls.st
static int cls_setup_pass(picp_batch* b, const float* T, bool want_chi2, bool want_uv, bool want_idx) {
  int rc = cls_prepare(b);
  if (rc) return rc;
  picp_batch::Classify& c = b->cls;
  rc = c.state.grow(b->total + 4);
  if (rc) return rc;
  if (want_chi2 && (rc = c.chi2.grow(b->total))) return rc;
  if (want_uv && (rc = c.uv.grow(2 * b->total))) return rc;
  if (want_idx && (rc = c.idx.grow(b->total))) return rc;
  for (int i = 0; i < b->np; ++i) {
    if (T) {
      memset(&c.st_h[i], 0, sizeof(PicpState));
      pose_to_state(T + 16 * (size_t)i, c.st_h[i]);
    } else {
      c.st_h[i] = b->result_h[i];
    }
  }
  // pageable source: the copy has left st_h when the call returns
  HIP_TRY(hipMemcpyAsync(c.st, c.st_h.data(), (size_t)b->np * sizeof(PicpState), hipMemcpyHostToDevice, b->stream));
  return PICP_OK;
}

int batch_classify(picp_batch* b, float threshold, const float* T, uint8_t* state, float* chi2,
                          float* uv, int64_t* inlier_off, int32_t* inlier_idx, int64_t* counts) {
  CHECK_ARG(!(threshold != threshold), "classify: threshold is NaN");
  HIP_TRY(hipSetDevice(b->device));
  int rc = cls_setup_pass(b, T, chi2 != nullptr, uv != nullptr, inlier_idx != nullptr);
  if (rc) return rc;
  picp_batch::Classify& c = b->cls;
  HIP_TRY(cls_enqueue(b, threshold, chi2 != nullptr, uv != nullptr, inlier_idx != nullptr));
  const ClsLayout L = cls_layout(c.nb, b->np);
  const int np = b->np;
  // counts and inlier offsets are contiguous up to padding: two copies into the pinned words
  HIP_TRY(hipMemcpyAsync(c.pinned, (char*)c.scan + L.counts, 3 * (size_t)np * sizeof(long long), hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipMemcpyAsync(c.pinned + 3 * (size_t)np, (char*)c.scan + L.inl_off, ((size_t)np + 1) * sizeof(long long),
                         hipMemcpyDeviceToHost, b->stream));
  if (state && b->total) HIP_TRY(hipMemcpyAsync(state, c.state, (size_t)b->total, hipMemcpyDeviceToHost, b->stream));
  if (chi2 && b->total) HIP_TRY(hipMemcpyAsync(chi2, c.chi2, (size_t)b->total * sizeof(float), hipMemcpyDeviceToHost, b->stream));
  if (uv && b->total) HIP_TRY(hipMemcpyAsync(uv, c.uv, 2 * (size_t)b->total * sizeof(float), hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  for (int64_t i = 0; i < 3 * (int64_t)np; ++i) counts[i] = c.pinned[i];
  const long long* off = c.pinned + 3 * (size_t)np;
  if (inlier_off)
    for (int i = 0; i <= np; ++i) inlier_off[i] = off[i];
  if (inlier_idx && off[np] > 0) {
    HIP_TRY(hipMemcpyAsync(inlier_idx, c.idx, (size_t)off[np] * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
  }
  return PICP_OK;
}

extern "C" int picp_batch_classify(picp_batch_t* b, float threshold, const float* T_wc, uint8_t* state,
                                   float* chi2, int64_t* inlier_off, int32_t* inlier_idx, int64_t* counts) {
  CHECK_ARG(b && counts, "picp_batch_classify: null argument");
  b->cls.want_chi2 = chi2 != nullptr;
  return batch_classify(b, threshold, T_wc, state, chi2, nullptr, inlier_off, inlier_idx, counts);
}

extern "C" int picp_batch_classify_time(picp_batch_t* b, float threshold, int reps, float* us_per_pass) {
  CHECK_ARG(b && us_per_pass && reps > 0, "picp_batch_classify_time: bad argument");
  CHECK_ARG(!(threshold != threshold), "classify: threshold is NaN");
  HIP_TRY(hipSetDevice(b->device));
  const bool want_chi2 = b->cls.want_chi2;
  int rc = cls_setup_pass(b, nullptr, want_chi2, false, true);
  if (rc) return rc;
  EventPair ev;
  HIP_TRY(ev.create());
  HIP_TRY(cls_enqueue(b, threshold, want_chi2, false, true));  // untimed: first-launch costs
  HIP_TRY(hipEventRecord(ev.a, b->stream));
  for (int r = 0; r < reps; ++r) HIP_TRY(cls_enqueue(b, threshold, want_chi2, false, true));
  HIP_TRY(hipEventRecord(ev.b, b->stream));
  HIP_TRY(hipEventSynchronize(ev.b));
  float ms = 0.0f;
  HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
  *us_per_pass = 1000.0f * ms / (float)reps;
  return PICP_OK;
}
