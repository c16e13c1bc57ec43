// picp_vo_plan.cpp -- the segment layout of a VO sequence as a pure plan (picp_vo_plan.h): no HIP
// call, no HIP type, nothing of the handle.  Owns every decision picp_vo_set_segments applies.
#include "picp_vo_plan.h"

#include <stdio.h>

#include <algorithm>

const char* picp_vo_plan(int64_t n_frames, const int64_t* frame_off, int64_t max_obs, int dim, int dp, int n_seg,
                         const int64_t* first, const int32_t* steps, const VoPlanOptions& opt, const VoPlanCaps& caps,
                         VoPlan* out) {
  if (!(n_seg >= 1 && n_seg <= VO_MAX_GRID_Y)) return "picp_vo_set_segments: n_seg must be in [1, 65535]";
  for (int s = 0; s < n_seg; ++s)
    if (!(steps[s] >= 1 && first[s] >= 0 && first[s] + steps[s] < n_frames))
      return "picp_vo_set_segments: segment out of range (needs frames first .. first+steps, steps >= 1)";
  // The world match writes its outputs (wm_*) at the query frame's observation offsets.  Step t of
  // segment s queries frame first[s] + t + 1, so two segments query one frame at the same step
  // exactly when their first frames are equal: they would write the same rows in one launch, and
  // that layout is rejected.  Segments querying one frame at different steps are fine in one step
  // chain (the launches are ordered) but not across chains (PICP_VO_CHAINS=2 runs the groups'
  // world matches concurrently), so such a layout runs the serial order.
  {
    std::vector<int64_t> f0s(first, first + n_seg);
    std::sort(f0s.begin(), f0s.end());
    for (int s = 1; s < n_seg; ++s)
      if (f0s[s] == f0s[s - 1]) {
        static thread_local char msg[160];
        snprintf(msg, sizeof(msg), "picp_vo_set_segments: two segments start at frame %lld (they would "
                 "query frame %lld at the same step)", (long long)f0s[s], (long long)f0s[s] + 1);
        return msg;
      }
  }
  VoPlan P;
  P.n_seg = n_seg;
  P.chains_eff = std::min(opt.chains, n_seg);
  {
    std::vector<int> q_group((size_t)n_frames, -1);
    const int C = P.chains_eff;
    for (int s = 0; s < n_seg; ++s) {
      int grp = 0;
      while (grp + 1 < C && s >= (int)((int64_t)n_seg * (grp + 1) / C)) ++grp;
      for (int t = 0; t < steps[s]; ++t) {
        const int64_t f = first[s] + t + 1;
        if (q_group[f] >= 0 && q_group[f] != grp) P.chains_eff = 1;
        q_group[f] = grp;
      }
    }
  }
  auto frame_n = [&](int64_t f) { return frame_off[f + 1] - frame_off[f]; };
  P.segs.resize((size_t)n_seg);
  for (int s = 0; s < n_seg; ++s) {
    VoSegment& G = P.segs[s];
    G.f0 = first[s];
    G.steps = steps[s];
    G.pad = 0;
    G.map_off = P.map_slots;
    G.slot0 = P.n_slots;
    int64_t cap = frame_n(G.f0);  // bootstrap adds <= |frame f0|, step t adds <= |frame f0+t|
    for (int t = 0; t < G.steps; ++t) cap += frame_n(G.f0 + t);
    P.map_slots += std::max<int64_t>(cap, 1);
    P.max_map = std::max(P.max_map, cap);
    P.n_slots += G.steps + 1;
    P.max_steps = std::max(P.max_steps, (int)G.steps);
  }
  // frame->next problems grouped by step index (the bootstrap and step 0 read chunk 0, step t
  // reads chunk t)
  P.chunk_off.assign(1, 0);
  std::vector<char> done((size_t)n_frames, 0);
  for (int k = 0; k < P.max_steps; ++k) {
    for (int s = 0; s < n_seg; ++s) {
      const int64_t f = first[s] + k;
      if (k < steps[s] && !done[f] && frame_n(f) > 0) {
        done[f] = 1;
        P.pprobs.push_back(MatchProblem{frame_off[f], frame_n(f), frame_off[f + 1], frame_n(f + 1), 0});
      }
    }
    P.chunk_off.push_back(P.pprobs.size());
  }
  P.cap_c = (std::max<int64_t>(max_obs, 1) + 3) / 4 * 4;
  // register-resident items per lane of picp_block_kernel: the largest power of two whose
  // 512 * npt slots the biggest frame fills (masked slots cost as much as live ones every
  // round; the few items past npt * 512 take the kernel's streamed-remainder path)
  while (P.npt < 8 && (int64_t)P.npt * 2 * 512 <= max_obs) P.npt *= 2;

  // one allocation for everything sized by the segments
  VoParts A;
  const size_t ns = (size_t)n_seg, ms = (size_t)P.map_slots, sl = (size_t)P.n_slots;
  P.p_segs = A.add(ns * sizeof(VoSegment));
  P.p_boot = A.add(ns * 32 * sizeof(float));
  P.p_mxyz = A.add(ms * 3 * sizeof(float));
  P.p_mdesc = A.add(ms * dim * sizeof(float));
  P.p_mn = A.add(ns * sizeof(int64_t));
  P.p_planes = A.add((size_t)5 * n_seg * P.cap_c * sizeof(float));
  P.p_probs = A.add(ns * sizeof(PicpProblem));
  P.p_stin = A.add(ns * VO_STATE_BYTES);
  P.p_stout = A.add(ns * VO_STATE_BYTES);
  P.p_wprobs = A.add(ns * sizeof(MatchProblem));
  P.p_lprobs = A.add(ns * sizeof(MatchProblem));
  P.p_eprobs = A.add(2 * ns * sizeof(MatchProblem));
  P.p_pprobs = A.add(std::max<size_t>(P.pprobs.size(), 1) * sizeof(MatchProblem));
  P.p_poses = A.add(sl * 16 * sizeof(float));
  P.p_steps = A.add(sl * VO_STEP_BYTES);
  P.p_pairs = A.add((size_t)n_seg * P.cap_c * VO_PAIR_BYTES);
  P.p_mh = A.add(ms * dp * VO_HALF_BYTES);
  P.p_mn1 = A.add(ms * sizeof(float));
  P.p_mn2 = A.add(ms * sizeof(float));
  // split scratch: each chain's world match (its n_seg_c problems) and the frame->next launches
  // the split rule's form: the folded accept-only form needs dim <= 12 (bit 2)
  const int ks_form = opt.accept_only | (dim <= 12 ? 4 : 0);
  const int C = P.chains_eff;
  auto chain_segs = [&](int c) { return (int)((int64_t)n_seg * (c + 1) / C - (int64_t)n_seg * c / C); };
  P.ks_w.assign((size_t)C, 1);
  P.cap_w.assign((size_t)C, 0);
  for (int c = 0; c < C; ++c) {
    P.ks_w[c] = caps.ksplit(chain_segs(c), max_obs, P.max_map, ks_form, opt.ks_force);
    P.cap_w[c] = caps.split_scratch(P.ks_w[c], chain_segs(c), max_obs);
    P.p_partw.push_back(A.add((size_t)P.cap_w[c] * VO_FLOAT4_BYTES));
  }
  // the split by map age: a chain's early part takes the whole world match's range split, plus one
  // slot for the late part (2 buffers: step t's merge and step t+2's early part overlap)
  P.split_c.assign((size_t)C, 0);
  P.cap_e.assign((size_t)C, 0);
  for (int c = 0; c < C; ++c) {
    P.split_c[c] = opt.early_streams && (opt.split_env == 1 || (opt.split_env < 0 && P.ks_w[c] > 1));
    if (P.split_c[c]) P.cap_e[c] = (int64_t)(P.ks_w[c] + 1) * chain_segs(c) * std::max<int64_t>(max_obs, 1);
    P.p_parte.push_back(A.add((size_t)2 * P.cap_e[c] * VO_FLOAT4_BYTES));
  }
  // the frame->next launches, as vo_frame_match issues them: the whole table up front (overlap off)
  // or chunk by chunk, each in launches of at most VO_MAX_GRID_Y problems
  auto launches = [&](size_t p0, size_t p1) {
    for (size_t q = p0; q < p1; q += VO_MAX_GRID_Y) {
      const int n = (int)std::min<size_t>(VO_MAX_GRID_Y, p1 - q);
      const int k = caps.ksplit(n, max_obs, max_obs, ks_form, opt.ks_force);
      P.ks_p.emplace_back(q, k);
      P.cap_p = std::max(P.cap_p, caps.split_scratch(k, n, max_obs));
    }
  };
  const size_t nck = P.chunk_off.size() - 1;
  if (opt.overlap && nck > 1) {
    for (size_t k = 0; k < nck; ++k) launches(P.chunk_off[k], P.chunk_off[k + 1]);
  } else {
    launches(0, P.pprobs.size());
  }
  P.p_partp = A.add((size_t)P.cap_p * VO_FLOAT4_BYTES);
  P.total = A.total;
  *out = std::move(P);
  return nullptr;
}
