// picp_ransac.hip -- the first launch of both batched RANSAC solvers (picp_pnp.hip, picp_sim3.hip):
// the samples, one lane per (problem, hypothesis) (picp_ransac.h, include/picp_c.h).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "picp_launch.h"
#include "picp_ransac.h"

#define RANSAC_SAMPLES_BS 256

// the samples of (problem, hypothesis) g = p * hyp + h; a problem of fewer than 4 items gets zeros
extern "C" __global__ __launch_bounds__(RANSAC_SAMPLES_BS) void picp_ransac_samples_kernel(
    uint64_t seed, int32_t prob0, int32_t n_problems, int32_t hyp, const int64_t* __restrict__ offs,
    int32_t* __restrict__ samples) {
  const int64_t g = (int64_t)blockIdx.x * RANSAC_SAMPLES_BS + threadIdx.x;
  if (g >= (int64_t)n_problems * hyp) return;
  const int p = (int)(g / hyp), h = (int)(g % hyp);
  const int64_t n = offs[p + 1] - offs[p];
  int32_t id[3] = {0, 0, 0};
  if (n >= 4) picp::sample_triple(seed, (uint32_t)(prob0 + p), (uint32_t)h, (uint32_t)n, id);
  for (int k = 0; k < 3; ++k) samples[3 * g + k] = id[k];
}

extern "C" hipError_t picp_launch_ransac_samples(hipStream_t stream, uint64_t seed, int32_t prob0, int32_t n_problems,
                                                 int32_t hyp, const int64_t* offs, int32_t* samples) {
  const int64_t g = (int64_t)n_problems * hyp;
  hipLaunchKernelGGL(picp_ransac_samples_kernel, dim3((unsigned)((g + RANSAC_SAMPLES_BS - 1) / RANSAC_SAMPLES_BS)),
                     dim3(RANSAC_SAMPLES_BS), 0, stream, seed, prob0, n_problems, hyp, offs, samples);
  return hipGetLastError();
}
