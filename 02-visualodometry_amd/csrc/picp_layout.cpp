// picp_layout.cpp -- the layout plan of a batch (picp_layout.h): arithmetic on the offsets, the
// device's limits and the overrides.  No HIP call and no HIP type.
#include "picp_layout.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>

static int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

LayoutEnv picp_layout_env() {
  LayoutEnv env;
  auto get = [](const char* name, LayoutEnv::Int* out) {
    if (const char* e = getenv(name)) *out = {true, atoi(e)};
  };
  if (const char* m = getenv("PICP_MODE")) {
    if (strcmp(m, "graph") == 0) env.mode = PICP_MODE_GRAPH;
    if (strcmp(m, "persistent") == 0) env.mode = PICP_MODE_PERSISTENT;
    if (strcmp(m, "block") == 0) env.mode = PICP_MODE_BLOCK;
  }
  LayoutEnv::Int v;
  get("PICP_ITEMS_PER_BLOCK", &v);
  env.items_per_block = v.v;
  get("PICP_BLOCK_NPT", &env.block_npt);
  get("PICP_PERSIST_BLOCKS", &env.persist_blocks);
  v = {};
  get("PICP_BLOCK_SPLIT", &v);
  env.block_split = v.v;
  if (const char* e = getenv("PICP_STREAM_SHARE")) env.stream_share = atof(e);
  v = {};
  get("PICP_RESIDENT_BLOCKS_PER_CU", &v);
  if (v.set) env.resident_cap = std::max(0, v.v);
  return env;
}

static int items_per_block(int64_t total, int num_cu, const LayoutEnv& env) {
  if (env.items_per_block >= 4) return (int)round_up(env.items_per_block, 4);
  // Latency-bound single frames: one correspondence per lane (spread over every SIMD).
  // Large batches (HBM streaming): float4 per lane and several chunks per lane to amortise the
  // block reduction and the partial traffic.
  if (total <= ((int64_t)1 << 18)) return 2 * PICP_BLOCK;  // measured best for C2 (tools/sweep.py)
  // streaming: about two resident 256-thread blocks per CU (all blocks in flight at once),
  // each streaming its slice through the prefetch ring (profiles/r01/sweep_*m_*.log)
  if (total < (int64_t)2 << 20) return PICP_BLOCK * 4 * 2;
  if (total < (int64_t)8 << 20) return PICP_BLOCK * 4 * 8;
  // Round the block count to a multiple of 2 x CUs so every CU carries the same load: with 489
  // blocks on 256 CUs some CUs hold one block and some two, and the round waits for the slowest
  // (16M: 489 blocks 69.0 us/round, 512 blocks 66.5 us; at 2M/4M the difference is in the noise;
  // profiles/r01/sweep_balance.log).
  const int64_t target = PICP_BLOCK * 4 * 32;
  const int64_t unit = 2 * (int64_t)std::max(1, num_cu);
  int64_t nb = ((total + target - 1) / target + unit / 2) / unit * unit;
  nb = std::max(nb, unit);
  return (int)round_up((total + nb - 1) / nb, 4);
}

// register items per lane for `items` on `threads` lanes: the power of two that holds them, capped
static int items_per_lane(int64_t items, int threads, int cap) {
  int npt = 1;
  while (npt < cap && (int64_t)npt * threads < items) npt *= 2;
  return npt;
}

// the block kernel's cap on register items per lane (a 512-thread block holds block_max_items)
static int block_npt_cap(const LayoutCaps& caps, const LayoutEnv& env, int split) {
  int cap = caps.block_max_items / 512;
  if (split > 1) cap = std::min(cap, caps.block_npt_cap(split));
  if (env.block_npt.set) cap = std::max(1, std::min(cap, env.block_npt.v));
  return cap;
}

// blocks of a split block launch: `split` per problem, rounded up to whole groups of 8 problems
static int split_grid(int np, int split) { return ((split * np + 8 * split - 1) / (8 * split)) * (8 * split); }

// Persistent candidate: the partition of uniform problems over the CUs, every block resident at
// once (the blocks of a problem wait on each other every round).  False: not eligible.
static bool plan_persistent(const LayoutPlan& P, bool no_handoff, const LayoutCaps& caps, const LayoutEnv& env,
                            int* npt_out, int* grid, int* resident) {
  int bpp = caps.num_cu / P.np;  // blocks per problem available
  if (env.persist_blocks.set) bpp = std::max(1, std::min(bpp, env.persist_blocks.v));
  if (no_handoff || !P.uniform || bpp < 1) return false;
  const int pbs = caps.persistent_block;
  const int64_t per_block = std::max<int64_t>(1, (P.n_u + bpp - 1) / bpp);
  const int npt = items_per_lane(per_block, pbs, 32);
  const int64_t nb = std::max<int64_t>(1, (P.n_u + (int64_t)npt * pbs - 1) / ((int64_t)npt * pbs));
  if (npt > 8 || nb > PICP_MAX_PBLK || nb * P.np > caps.num_cu) return false;
  *npt_out = npt;
  *grid = (int)nb * P.np;
  *resident = std::min(caps.persistent_occupancy(npt), env.resident_cap) * caps.num_cu;
  return *grid <= *resident;
}

// Block mode: blocks per problem and register items per lane.
//  * two blocks per problem when every pair still gets its own CUs (C4: 128 frames on 256 CUs)
//    and the halves are big enough to pay for the per-round partner exchange;
//  * four 512-thread parts per problem, two blocks per CU from different problems, when four
//    times the problems still fit two per CU and a part keeps >= 2048 correspondences (the C4
//    per-rank shape at N = 8, 128 frames x 10k): one block's round tail (at issue priority 3)
//    runs under the other's linearize; 22.0-22.4M vs 21.2-21.4M it/s for split 2
//    (profiles/r04/p1/).  256-thread parts (round 1) were 5 % slower;
//  * PICP_BLOCK_SPLIT=1|2|4 forces, within the same grid limits.
// The parts of a split problem wait on each other every round: a split is kept only if the
// occupancy query says its whole grid is resident at once, else the next smaller one is tried.
static void plan_block(LayoutPlan& P, bool no_handoff, const LayoutCaps& caps, const LayoutEnv& env) {
  const int np = P.np;
  int split = (split_grid(np, 2) <= caps.num_cu && P.max_n >= 4096) ? 2 : 1;
  if (split_grid(np, 4) <= 2 * caps.num_cu && P.max_n >= 8192 && caps.block_threads(4) == 512) split = 4;
  if (env.block_split == 1) split = 1;
  if (env.block_split == 2 && split_grid(np, 2) <= caps.num_cu) split = 2;
  if (env.block_split == 4 && split_grid(np, 4) <= 2 * caps.num_cu) split = 4;
  if (no_handoff) split = 1;
  for (; split > 1; split = (split == 4) ? 2 : 1) {
    const int64_t part = round_up((P.max_n + split - 1) / split, 4);
    const int npt = items_per_lane(part, caps.block_threads(split), block_npt_cap(caps, env, split));
    const int resident = std::min(caps.block_occupancy(npt, split, (int)P.max_n), env.resident_cap) * caps.num_cu;
    if (split_grid(np, split) > resident) continue;
    P.npt = npt;
    P.handoff_grid = split_grid(np, split);
    P.handoff_resident = resident;
    break;
  }
  P.split = split;
  if (split == 1) P.npt = items_per_lane(P.max_n, 512, block_npt_cap(caps, env, 1));
}

// Block table: problem i on ceil(n / ipb) blocks of ipb items (an empty problem: one block of none).
static void plan_tables(LayoutPlan& P, const int64_t* offs) {
  P.plane_off.resize(P.np);
  P.probs.resize(P.np);
  P.blocks.clear();
  int64_t pos = 0;
  for (int i = 0; i < P.np; ++i) {
    const int64_t n = offs[i + 1] - offs[i];
    const int nb = (int)std::max<int64_t>(1, (n + P.ipb - 1) / P.ipb);
    P.plane_off[i] = pos;
    P.probs[i] = PicpProblem{pos, (int32_t)n, (int32_t)P.blocks.size(), nb, 0};
    for (int k = 0; k < nb; ++k) {
      const int64_t first = (int64_t)k * P.ipb;
      P.blocks.push_back({i, (int32_t)first, (int32_t)std::max<int64_t>(0, std::min<int64_t>(P.ipb, n - first)), 0});
    }
    pos = round_up(pos + n, 4);
  }
  P.plane_len = std::max<int64_t>(pos, 4);
  P.nblk = (int)P.blocks.size();
}

// Streaming single frame on two blocks per CU (nblk == 2 x CUs): the hardware issues the older
// block of a CU first, so with equal slices the first num_cu blocks finish a round at ~2/3 of the
// time the second ones need and their CUs then stream at half parallelism
// (tools/stamps_place.py).  Pair block q with q + num_cu over a contiguous range
// and give q the larger share (PICP_STREAM_SHARE, the first block's fraction).
static void plan_stream_share(LayoutPlan& P, int num_cu, double share) {
  if (!(P.mode == PICP_MODE_GRAPH && P.np == 1 && P.vec == 4 && P.nblk == 2 * num_cu)) return;
  if (!(share > 0.5 && share < 0.9)) return;
  const int64_t n = P.total;
  const int64_t pair = round_up((n + num_cu - 1) / num_cu, 4);
  const int64_t hi = round_up((int64_t)(pair * share), 4);
  for (int q = 0; q < num_cu; ++q) {
    const int64_t f0 = std::min<int64_t>(n, q * pair);
    const int64_t f1 = std::min<int64_t>(n, f0 + hi);
    const int64_t f2 = std::min<int64_t>(n, (q + 1) * pair);
    P.blocks[q] = {0, (int32_t)f0, (int32_t)(f1 - f0), 0};
    P.blocks[q + num_cu] = {0, (int32_t)f1, (int32_t)(f2 - f1), 0};
  }
  P.uniform = 0;  // the kernel reads the block table
}

static SyncLayout plan_sync(const LayoutPlan& P) {
  SyncLayout S;
  if (P.mode == PICP_MODE_PERSISTENT) {
    S.pose = 128;
    S.pose_bytes = (int64_t)P.np * PICP_POSE_SETS * PICP_POSE_GRAN * 8;
    S.gran_bytes = 2 * (int64_t)P.nblk * PICP_NPART * 8;
    S.tag_bytes = (int64_t)P.np * 4;
  } else if (P.mode == PICP_MODE_BLOCK && P.split > 1) {
    const int64_t grid = split_grid(P.np, P.split);  // one granule set and one tag base per block
    S.gran_bytes = 2 * grid * 64 * 8;
    S.tag_bytes = grid * 4;
  } else {
    return S;
  }
  S.gran = 128 + S.pose_bytes;
  S.tag = S.gran + S.gran_bytes;
  S.bytes = round_up(S.tag + S.tag_bytes, 256);
  return S;
}

const char* picp_layout_plan(const int64_t* offs, int np, bool no_handoff, const LayoutCaps& caps,
                             const LayoutEnv& env, LayoutPlan* out) {
  if (np < 1) return "batch: n_problems must be >= 1";
  for (int i = 0; i < np; ++i)
    if (!(offs[i + 1] >= offs[i] && offs[0] == 0)) return "batch: corr_offsets must be a prefix sum from 0";
  LayoutPlan P;
  P.np = np;
  P.total = offs[np];
  P.uniform = 1;
  for (int i = 0; i < np; ++i) {
    const int64_t n = offs[i + 1] - offs[i];
    if (n > INT32_MAX) return "batch: a problem has more than 2^31-1 correspondences";
    if (n != offs[1] - offs[0]) P.uniform = 0;
    P.max_n = std::max(P.max_n, n);
  }
  P.n_u = (int)(offs[1] - offs[0]);
  P.stride_u = round_up(P.n_u, 4);
  // Execution mode:
  //  * BLOCK      -- one block per problem (or 2 / 4 partner blocks), all rounds in-block, problem
  //                  held in registers: batches of >= 2 problems small enough for one CU;
  //  * PERSISTENT -- one launch, blocks of one problem hand off through granules: when every
  //                  block of the batch is resident at once (uniform problems);
  //  * GRAPH      -- one launch per round, replayed from a hipGraph: everything else.
  // PICP_MODE=graph|persistent|block forces a mode when the batch is eligible for it.
  const bool block_ok = P.max_n <= ((int64_t)1 << 16);
  int pnpt = 0, pgrid = 0, pres = 0;
  const bool persistent_ok = plan_persistent(P, no_handoff, caps, env, &pnpt, &pgrid, &pres);
  if (env.mode == PICP_MODE_GRAPH) P.mode = PICP_MODE_GRAPH;
  else if (env.mode == PICP_MODE_BLOCK && block_ok) P.mode = PICP_MODE_BLOCK;
  else if (env.mode == PICP_MODE_PERSISTENT && persistent_ok) P.mode = PICP_MODE_PERSISTENT;
  else if (np >= 2 && block_ok) P.mode = PICP_MODE_BLOCK;
  else if (persistent_ok) P.mode = PICP_MODE_PERSISTENT;
  P.ipb = items_per_block(P.total, caps.num_cu, env);
  if (P.mode == PICP_MODE_PERSISTENT) {
    P.npt = pnpt;
    P.ipb = pnpt * caps.persistent_block;
    P.handoff_grid = pgrid;
    P.handoff_resident = pres;
  } else if (P.mode == PICP_MODE_BLOCK) {
    plan_block(P, no_handoff, caps, env);
  }
  P.vec = (P.ipb >= 4 * PICP_BLOCK && P.mode == PICP_MODE_GRAPH) ? 4 : 1;
  plan_tables(P, offs);
  plan_stream_share(P, caps.num_cu, env.stream_share);
  P.sync = plan_sync(P);
  *out = std::move(P);
  return nullptr;
}
