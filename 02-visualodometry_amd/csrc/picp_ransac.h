// picp_ransac.h -- what the batched RANSAC solvers share on the device (picp_pnp.hip,
// picp_sim3.hip): the sampling function of include/picp_c.h and the winner
// search.  Under PICP_RANSAC_HOST the sampling function alone is plain host C++ (bin/ransac_check).
#pragma once
#ifdef PICP_RANSAC_HOST
#define PICP_RANSAC_FN inline
#else
#include <hip/hip_runtime.h>
#define PICP_RANSAC_FN __device__ __forceinline__
#endif

#include <stdint.h>

namespace picp {

// splitmix64's output function of the state x + golden gamma
PICP_RANSAC_FN uint64_t mix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the sampling function of include/picp_c.h (n >= 3): hypothesis h of the problem at batch position i
PICP_RANSAC_FN void sample_triple(uint64_t seed, uint32_t i, uint32_t h, uint32_t n, int32_t id[3]) {
  const uint64_t key = mix64(seed ^ mix64(((uint64_t)i << 32) | h));
  const uint64_t r0 = mix64(key) >> 32, r1 = mix64(key + 1) >> 32, r2 = mix64(key + 2) >> 32;
  const uint32_t a = (uint32_t)((r0 * n) >> 32);
  uint32_t b = (uint32_t)((r1 * (n - 1)) >> 32);
  b += (b >= a) ? 1u : 0u;
  uint32_t c = (uint32_t)((r2 * (n - 2)) >> 32);
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
  c += (c >= lo) ? 1u : 0u;
  c += (c >= hi) ? 1u : 0u;
  id[0] = (int32_t)a;
  id[1] = (int32_t)b;
  id[2] = (int32_t)c;
}

#ifndef PICP_RANSAC_HOST

// The winner of a problem's entries, the same in every thread of the block: the largest count,
// then the lowest valid entry.  The key of entry e is (count + 1) above ~e, so the maximum does
// not depend on who finds it and 0 means none.  s_key: BS / 64 words of LDS, which every thread
// reads after the one barrier here: it must not be written again without another.
template <int BS, class Valid>
__device__ __forceinline__ unsigned long long block_winner(int entries, const int32_t* __restrict__ cnt,
                                                           unsigned long long* s_key, Valid valid) {
  const int tid = threadIdx.x;
  unsigned long long key = 0;
  for (int e = tid; e < entries; e += BS) {
    if (!valid(e)) continue;
    const unsigned long long k = ((unsigned long long)((unsigned)cnt[e] + 1u) << 32) | (unsigned)~(unsigned)e;
    key = k > key ? k : key;
  }
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(key, m);
    key = o > key ? o : key;
  }
  if ((tid & 63) == 0) s_key[tid >> 6] = key;
  __syncthreads();
  key = s_key[0];
  for (int w = 1; w < BS / 64; ++w) key = s_key[w] > key ? s_key[w] : key;
  return key;
}
__device__ __forceinline__ unsigned winner_entry(unsigned long long key) { return (unsigned)~(unsigned)key; }
__device__ __forceinline__ int winner_count(unsigned long long key) { return key ? (int)(key >> 32) - 1 : 0; }

#endif  // !PICP_RANSAC_HOST

}  // namespace picp
