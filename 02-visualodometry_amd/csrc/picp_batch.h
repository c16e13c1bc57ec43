// picp_batch.h -- the batch solver's state and the parts of it the other runtime translation
// units use (the single-problem handle drives a one-problem batch).  Not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <vector>

#include "picp_c.h"
#include "picp_host.h"
#include "picp_internal.h"
#include "picp_layout.h"

#pragma GCC visibility push(hidden)

// A batch is its current layout plan (mode, partition, tables, sync carve-up: picp_layout.h) and
// the device memory, stream and graph the plan is applied to.
struct picp_batch : LayoutPlan {
  int device = 0;
  hipStream_t stream = nullptr;
  int rows = 0, cols = 0;
  float K[9];
  std::vector<int64_t> offs;   // user correspondence offsets (np+1)
  int64_t plane_cap = 0;       // allocated plane length
  float* planes = nullptr;     // 5 * plane_cap floats: X | Y | Z | U | V
  int nblk_cap = 0;
  int np_cap = 0;
  PicpProblem* probs_d = nullptr;
  int4* blk_d = nullptr;
  PicpState* init_d = nullptr;
  PicpState* st_d[2] = {nullptr, nullptr};
  unsigned long long* part_d = nullptr;  // graph mode: published block partials (16 words each)
  unsigned int* tickets_d = nullptr;     // graph mode: per-problem arrival tickets
  PicpState* st_pinned = nullptr;  // np_cap states
  std::vector<PicpState> init_h;
  std::vector<PicpState> result_h;
  bool params_set = false;
  picp_params params;
  PicpArgs args;               // by-value kernel arguments (baked into the captured graph)
  int num_cu = 256;            // compute units of the device
  unsigned char* sync_d = nullptr;  // hand-off modes: the sync area, carved up by `sync` (SyncLayout)
  size_t sync_cap = 0;
  uint64_t tag_rounds = 0;     // hand-off modes: rounds enqueued since the sync area was last zeroed
  int result_idx = 0;          // st_d[] holding the final state of the last solve
  bool last_persistent = false;  // the last solve was a hand-off launch (check its error word)
  unsigned long long timeout_ticks = 20000000ull;  // 200 ms of s_memrealtime (100 MHz)
  bool no_handoff = false;     // a hand-off wait timed out once: lay out without cross-block waits
  int fallbacks = 0;           // solves re-run in graph mode after a timed-out hand-off
  // graph cache
  hipGraphExec_t gexec = nullptr;
  hipGraph_t graph = nullptr;
  int g_rounds = -1;
  int last_rounds = 0;  // R of the last solve (final state in st_d[R&1])
  // classify pass (picp_batch_classify): its own tiling of the planes and its own outputs, sized
  // once per layout (tables, tile counts, staging) or on first use (the per-item outputs)
  struct Classify {
    bool ready = false;          // the tables below describe the current layout
    int nb = 0;                  // tiles
    DevBuf<char> tables;         // int4 blk[nb] | int2 pblk[np] | int64 plane_off[np] | int64 pack_off[np]
    DevBuf<char> scan;           // int cnt[3 nb] | int64 base[3 (nb+1)] | int64 counts[3 np] | int64 inl_off[np+1]
    DevBuf<PicpState> st;        // np poses to classify at
    DevBuf<uint8_t> state;
    DevBuf<float> chi2;
    DevBuf<float> uv;
    DevBuf<int32_t> idx;
    long long* pinned = nullptr; // counts[3 np] | inl_off[np+1]
    int64_t pinned_cap = 0;      // int64 words
    std::vector<PicpState> st_h;
    bool want_chi2 = false;      // what the last picp_batch_classify asked for (picp_batch_classify_time)
  } cls;

  float* X() const { return planes; }
  float* Y() const { return planes + plane_cap; }
  float* Z() const { return planes + 2 * plane_cap; }
  float* U() const { return planes + 3 * plane_cap; }
  float* V() const { return planes + 4 * plane_cap; }
};

// picp_batch.cpp
int batch_create(picp_batch** out, int device, int np, const int64_t* offs, int rows, int cols, const float K[9]);
// (re)builds the layout for correspondence offsets `offs` (np + 1 entries; may be b->offs itself)
int batch_layout(picp_batch* b, const int64_t* offs, int np);
int batch_upload_params(picp_batch* b, const picp_params* prm);
// graph-mode prologue of every solve (initial states in, arrival tickets zeroed) and round j
hipError_t graph_prologue(picp_batch* b);
hipError_t launch_round(picp_batch* b, int j);
// After enqueuing a solve of R rounds: where its final states are and whether a hand-off wait
// could have timed out in it.  round_launches: the rounds went out one launch each (graph mode,
// and picp_one_round in any mode), else as the one launch of the batch's mode.
void batch_solve_enqueued(picp_batch* b, int R, bool round_launches);
int batch_read_results(picp_batch* b);

// picp_batch_classify.cpp
int batch_classify(picp_batch* b, float threshold, const float* T, uint8_t* state, float* chi2, float* uv,
                   int64_t* inlier_off, int32_t* inlier_idx, int64_t* counts);

#pragma GCC visibility pop
