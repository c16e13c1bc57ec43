// plan_main.cpp -- prints the layout plan (csrc/picp_layout.h) of one case as JSON; host only,
// built with the sanitizers (tests/test_layout_plan_cpu.py runs it).
//
//   layout_plan <num_cu> <no_handoff> <occ_persistent> <occ_block1> <occ_block2> <occ_block4> <n>...
//
// <n>...: the problem sizes.  occ_*: the occupancy answers (resident blocks per CU) of the
// persistent kernel and of the block kernel at split 1, 2 and 4.  The overrides are read from the
// environment, as the library reads them.  The kernel limits are fixed: a block holds 4096 items,
// every block has 512 threads, 4 register items per lane at split 4 and 8 otherwise.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "picp_layout.h"

int main(int argc, char** argv) {
  if (argc < 7) {
    fprintf(stderr, "usage: %s num_cu no_handoff occ_persistent occ_block1 occ_block2 occ_block4 [n...]\n", argv[0]);
    return 2;
  }
  LayoutCaps caps;
  caps.num_cu = atoi(argv[1]);
  const bool no_handoff = atoi(argv[2]) != 0;
  const int occ_p = atoi(argv[3]);
  const int occ_b[5] = {0, atoi(argv[4]), atoi(argv[5]), 0, atoi(argv[6])};
  caps.block_max_items = 4096;
  caps.persistent_block = 512;
  caps.block_threads = [](int) { return 512; };
  caps.block_npt_cap = [](int split) { return split == 4 ? 4 : 8; };
  caps.persistent_occupancy = [&](int) { return occ_p; };
  caps.block_occupancy = [&](int, int split, int) { return occ_b[split]; };
  std::vector<int64_t> offs(1, 0);
  for (int i = 7; i < argc; ++i) offs.push_back(offs.back() + atoll(argv[i]));
  LayoutPlan P;
  if (const char* msg = picp_layout_plan(offs.data(), (int)offs.size() - 1, no_handoff, caps, picp_layout_env(), &P)) {
    printf("{\"error\": \"%s\"}\n", msg);
    return 0;
  }
  printf("{\"mode\": %d, \"split\": %d, \"npt\": %d, \"ipb\": %d, \"vec\": %d, \"uniform\": %d, \"n_u\": %d,\n", P.mode,
         P.split, P.npt, P.ipb, P.vec, P.uniform, P.n_u);
  printf(" \"stride_u\": %lld, \"max_n\": %lld, \"plane_len\": %lld, \"nblk\": %d, \"total\": %lld,\n",
         (long long)P.stride_u, (long long)P.max_n, (long long)P.plane_len, P.nblk, (long long)P.total);
  printf(" \"handoff_grid\": %d, \"handoff_resident\": %d,\n", P.handoff_grid, P.handoff_resident);
  const SyncLayout& S = P.sync;
  printf(" \"sync\": {\"bytes\": %lld, \"err\": [%lld, 4], \"pose\": [%lld, %lld], \"gran\": [%lld, %lld], \"tag\": [%lld, %lld]},\n",
         (long long)S.bytes, (long long)S.err, (long long)S.pose, (long long)S.pose_bytes, (long long)S.gran,
         (long long)S.gran_bytes, (long long)S.tag, (long long)S.tag_bytes);
  printf(" \"plane_off\": [");
  for (size_t i = 0; i < P.plane_off.size(); ++i) printf("%s%lld", i ? ", " : "", (long long)P.plane_off[i]);
  printf("],\n \"probs\": [");  // offset, n, blk0, nblk
  for (size_t i = 0; i < P.probs.size(); ++i)
    printf("%s[%lld, %d, %d, %d]", i ? ", " : "", (long long)P.probs[i].offset, P.probs[i].n, P.probs[i].blk0,
           P.probs[i].nblk);
  printf("],\n \"blocks\": [");  // problem, first, count
  for (size_t i = 0; i < P.blocks.size(); ++i)
    printf("%s[%d, %d, %d]", i ? ", " : "", P.blocks[i].problem, P.blocks[i].first, P.blocks[i].count);
  printf("]}\n");
  return 0;
}
