// plan_main.cpp -- prints the segment layout plan (csrc/picp_vo_plan.h) of one case as JSON; host
// only, built with the sanitizers (tests/test_vo_plan_cpu.py runs it).
//
//   vo_plan <num_cu> <dim> <dp> <chains> <overlap> <accept_only> <split_env> <early_streams> <ks_force>
//           <first:steps,first:steps,...> <obs>...
//
// A segment entry `first:steps*count+stride` stands for count segments of equal steps, stride
// frames apart.
// <obs>...: the observation counts of the frames, each `n` or `reps x n` written `<reps>x<n>`.
// The split rule is the matcher's (picp_match.hip picp_match_ksplit_forced: four waves per block,
// 256 reference rows per tile, caps 16 / 32 / 65536) with the CU count taken from <num_cu>; the
// scratch rule is the matcher's as it stands.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "picp_vo_plan.h"

static void part(const char* name, const VoPart& p, const char* sep) {
  printf("\"%s\": [%zu, %zu]%s", name, p.off, p.bytes, sep);
}

static void parts(const char* name, const std::vector<VoPart>& v, const char* sep) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) printf("%s[%zu, %zu]", i ? ", " : "", v[i].off, v[i].bytes);
  printf("]%s", sep);
}

template <class T>
static void ints(const char* name, const std::vector<T>& v, const char* sep) {
  printf(" \"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) printf("%s%lld", i ? ", " : "", (long long)v[i]);
  printf("]%s", sep);
}

int main(int argc, char** argv) {
  if (argc < 12) {
    fprintf(stderr, "usage: %s num_cu dim dp chains overlap accept_only split_env early_streams ks_force "
            "first:steps,... obs...\n", argv[0]);
    return 2;
  }
  const int64_t num_cu = atoi(argv[1]);
  const int dim = atoi(argv[2]), dp = atoi(argv[3]);
  VoPlanOptions opt;
  opt.chains = atoi(argv[4]);
  opt.overlap = atoi(argv[5]) != 0;
  opt.accept_only = atoi(argv[6]);
  opt.split_env = atoi(argv[7]);
  opt.early_streams = atoi(argv[8]) != 0;
  opt.ks_force = atoi(argv[9]);
  std::vector<int64_t> first;
  std::vector<int32_t> steps;
  for (const char* p = argv[10]; *p;) {  // first:steps, or first:steps*count+stride
    char* end = nullptr;
    const long long f0 = strtoll(p, &end, 10);
    const long st = *end == ':' ? strtol(end + 1, &end, 10) : 0;
    const long long count = *end == '*' ? strtoll(end + 1, &end, 10) : 1;
    const long long stride = *end == '+' ? strtoll(end + 1, &end, 10) : 0;
    for (long long k = 0; k < count; ++k) {
      first.push_back(f0 + k * stride);
      steps.push_back((int32_t)st);
    }
    if (*end != ',') break;
    p = end + 1;
  }
  std::vector<int64_t> off(1, 0);
  int64_t max_obs = 0;
  for (int i = 11; i < argc; ++i) {
    const char* x = strchr(argv[i], 'x');
    const long long reps = x ? atoll(argv[i]) : 1, n = atoll(x ? x + 1 : argv[i]);
    for (long long r = 0; r < reps; ++r) off.push_back(off.back() + n);
    if (reps > 0) max_obs = std::max<int64_t>(max_obs, n);
  }
  VoPlanCaps caps;
  caps.ksplit = [num_cu](int n_problems, int64_t max_nq, int64_t max_nr, int form, int force) {
    if (form & 2) return 1;
    const int64_t base = (int64_t)n_problems * ((max_nq + 32 * 4 - 1) / (32 * 4));
    int64_t k = (4 * num_cu + base - 1) / std::max<int64_t>(base, 1);
    k = std::max<int64_t>(1, std::min<int64_t>(k, 16));
    if ((form & 1) && (form & 4)) {
      const int64_t b2 = (int64_t)n_problems * ((max_nq + 64 * 4 - 1) / (64 * 4));
      const int64_t k2 = (4 * num_cu) / std::max<int64_t>(b2, 1);
      if (k2 >= 8 && max_nr >= k2 * 4096) k = std::min<int64_t>(k2, 32);
    }
    if (force > 0) k = std::min<int64_t>(force, 65536);
    const int64_t k_range = (max_nr + ((int64_t)256 << 12) - 1) / ((int64_t)256 << 12);
    return (int)std::min<int64_t>(std::max<int64_t>(k, k_range), 65536);
  };
  caps.split_scratch = [](int ksplit, int n_problems, int64_t max_nq) {
    return ksplit > 1 ? (int64_t)ksplit * n_problems * max_nq : (int64_t)0;
  };
  VoPlan P;
  if (const char* msg = picp_vo_plan((int64_t)off.size() - 1, off.data(), max_obs, dim, dp, (int)first.size(),
                                     first.data(), steps.data(), opt, caps, &P)) {
    printf("{\"error\": \"%s\"}\n", msg);
    return 0;
  }
  printf("{\"n_seg\": %d, \"chains_eff\": %d, \"max_steps\": %d, \"npt\": %d, \"map_slots\": %lld, \"n_slots\": %lld,\n",
         P.n_seg, P.chains_eff, P.max_steps, P.npt, (long long)P.map_slots, (long long)P.n_slots);
  printf(" \"max_map\": %lld, \"cap_c\": %lld, \"cap_p\": %lld, \"total\": %zu,\n", (long long)P.max_map,
         (long long)P.cap_c, (long long)P.cap_p, P.total);
  printf(" \"segs\": [");  // f0, map_off, slot0, steps
  for (size_t i = 0; i < P.segs.size(); ++i)
    printf("%s[%lld, %lld, %lld, %d]", i ? ", " : "", (long long)P.segs[i].f0, (long long)P.segs[i].map_off,
           (long long)P.segs[i].slot0, P.segs[i].steps);
  printf("],\n \"pprobs\": [");  // q_off, nq, r_off, nr, idx0
  for (size_t i = 0; i < P.pprobs.size(); ++i)
    printf("%s[%lld, %lld, %lld, %lld, %lld]", i ? ", " : "", (long long)P.pprobs[i].q_off, (long long)P.pprobs[i].nq,
           (long long)P.pprobs[i].r_off, (long long)P.pprobs[i].nr, (long long)P.pprobs[i].idx0);
  printf("],\n");
  ints("chunk_off", P.chunk_off, ",\n");
  ints("ks_w", P.ks_w, ",\n");
  ints("cap_w", P.cap_w, ",\n");
  ints("split_c", P.split_c, ",\n");
  ints("cap_e", P.cap_e, ",\n");
  printf(" \"ks_p\": [");
  for (size_t i = 0; i < P.ks_p.size(); ++i) printf("%s[%zu, %d]", i ? ", " : "", P.ks_p[i].first, P.ks_p[i].second);
  printf("],\n \"parts\": {");
  part("segs", P.p_segs, ", ");
  part("boot", P.p_boot, ", ");
  part("mxyz", P.p_mxyz, ", ");
  part("mdesc", P.p_mdesc, ", ");
  part("mn", P.p_mn, ", ");
  part("planes", P.p_planes, ", ");
  part("probs", P.p_probs, ", ");
  part("stin", P.p_stin, ", ");
  part("stout", P.p_stout, ", ");
  part("wprobs", P.p_wprobs, ", ");
  part("lprobs", P.p_lprobs, ", ");
  part("eprobs", P.p_eprobs, ", ");
  part("pprobs", P.p_pprobs, ", ");
  part("poses", P.p_poses, ", ");
  part("steps", P.p_steps, ", ");
  part("pairs", P.p_pairs, ", ");
  part("mh", P.p_mh, ", ");
  part("mn1", P.p_mn1, ", ");
  part("mn2", P.p_mn2, ", ");
  parts("partw", P.p_partw, ", ");
  parts("parte", P.p_parte, ", ");
  part("partp", P.p_partp, "}}\n");
  return 0;
}
