// picp_sim3.hip -- 3D-3D alignment robust to wrong matches: Umeyama's closed form inside RANSAC for
// a ragged batch of matched point sets, with local optimisation.  Five launches;
// what the P3P solver has too is in picp_ransac.h:
//   1. picp_ransac_samples_kernel (picp_ransac.hip): three distinct indices per (problem, hypothesis);
//   2. picp_sim3_hyp_kernel      one lane per (problem, hypothesis), in double with contraction
//                                off: the moments of the three pairs about the first, the closed
//                                form (picp_umeyama.h), the transform rounded to float32;
//   3. picp_sim3_score_kernel    the hot path: a block keeps up to S3_TILE pairs of one problem in
//                                registers and loops over the problem's transforms (each one
//                                wave-uniform: scalar loads); counts are ballots and scalar
//                                popcounts, gathered per S3_HT hypotheses in LDS and added to the
//                                table with integer atomics (order-free);
//   4. picp_sim3_select_kernel   one block per problem: the largest count, then the lowest hypothesis;
//   5. picp_sim3_refit_kernel    one block per problem: `refits` times the least-squares transform
//                                of the current inliers (moments in double, summed in a fixed
//                                order) and its count; the best candidate, its mask and its RMS.
// No block waits for another; no float atomics.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "picp_internal.h"
#include "picp_launch.h"
#include "picp_ransac.h"
#include "picp_umeyama.h"
#include "picp_wave.h"

#pragma clang fp contract(off)

#define S3_BS 256
#define S3_NPT 4
#define S3_TILE (S3_BS * S3_NPT)  // pairs a score block keeps in registers
#define S3_HT 64                  // hypotheses per LDS count tile
#define S3_T SIM3_XF              // floats of a stored transform: M = c R column-major, t, c, 3 unused

namespace {

// the squared distance of M p + t from q in float32, in the order include/picp_c.h states
__device__ __forceinline__ float sim3_d2(const float* S, float x, float y, float z, float qx, float qy, float qz) {
  const float rx = (((S[0] * x + S[3] * y) + S[6] * z) + S[9]) - qx;
  const float ry = (((S[1] * x + S[4] * y) + S[7] * z) + S[10]) - qy;
  const float rz = (((S[2] * x + S[5] * y) + S[8] * z) + S[11]) - qz;
  return (rx * rx + ry * ry) + rz * rz;
}

struct Pair {
  float x, y, z, qx, qy, qz;
};

__device__ __forceinline__ Pair load_pair(const Sim3Items& I, int64_t e) {
  Pair a;
  a.x = I.px[e * I.sp];
  a.y = I.py[e * I.sp];
  a.z = I.pz[e * I.sp];
  a.qx = I.qx[e * I.sq];
  a.qy = I.qy[e * I.sq];
  a.qz = I.qz[e * I.sq];
  return a;
}

// The members of a problem that one refit pass runs over: the inliers of the transform S (by_S),
// or, for picp_sim3_fit_batch, the finite pairs whose mask byte (mask != null) is set.
struct Members {
  float S[12];
  float thr;
  bool by_S;
  const uint8_t* mask;  // at the problem's first pair
  __device__ __forceinline__ bool has(const Pair& a, int64_t j) const {
    if (by_S) return sim3_d2(S, a.x, a.y, a.z, a.qx, a.qy, a.qz) < thr;
    const bool fin = fabsf(a.x) < INFINITY && fabsf(a.y) < INFINITY && fabsf(a.z) < INFINITY &&
                     fabsf(a.qx) < INFINITY && fabsf(a.qy) < INFINITY && fabsf(a.qz) < INFINITY;
    return fin && (!mask || mask[j] != 0);
  }
};

__device__ __forceinline__ Members inliers_of(const float* S, float thr) {
  Members M;
#pragma unroll
  for (int k = 0; k < 12; ++k) M.S[k] = S[k];
  M.thr = thr;
  M.by_S = true;
  M.mask = nullptr;
  return M;
}

__device__ __forceinline__ Members finite_of(const uint8_t* mask) {
  Members M;
#pragma unroll
  for (int k = 0; k < 12; ++k) M.S[k] = 0.0f;
  M.thr = 0.0f;
  M.by_S = false;
  M.mask = mask;
  return M;
}

// sums of K doubles per thread over the block, the same bits in every thread: the xor tree inside
// a wave, then the waves in order.  s: S3_BS / 64 * K doubles of LDS.
template <int K>
__device__ __forceinline__ void block_sum(double* v, double* s) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; ++k)
    for (int m = 32; m >= 1; m >>= 1) v[k] += __shfl_xor(v[k], m);
  __syncthreads();  // s may still be read from an earlier call
  if ((tid & 63) == 0)
    for (int k = 0; k < K; ++k) s[(tid >> 6) * K + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double t = s[k];
    for (int w = 1; w < S3_BS / 64; ++w) t += s[w * K + k];
    v[k] = t;
  }
}

// the number of members and the lowest member index (INT32_MAX: none), in every thread
__device__ __forceinline__ void count_first(const Sim3Items& I, int64_t b, int n, const Members& M, int* s,
                                            int* count, int* first) {
  const int tid = threadIdx.x;
  int c = 0, f = INT32_MAX;
  for (int64_t j = tid; j < n; j += S3_BS) {
    if (M.has(load_pair(I, b + j), j)) {
      ++c;
      f = (int)j < f ? (int)j : f;
    }
  }
  for (int m = 32; m >= 1; m >>= 1) {
    c += __shfl_xor(c, m);
    const int o = __shfl_xor(f, m);
    f = o < f ? o : f;
  }
  __syncthreads();
  if ((tid & 63) == 0) {
    s[tid >> 6] = c;
    s[S3_BS / 64 + (tid >> 6)] = f;
  }
  __syncthreads();
  c = 0, f = INT32_MAX;
  for (int w = 0; w < S3_BS / 64; ++w) {
    c += s[w];
    f = s[S3_BS / 64 + w] < f ? s[S3_BS / 64 + w] : f;
  }
  *count = c;
  *first = f;
}

// The least-squares transform of the members (count of them, the lowest at `first`), float32 in
// out[S3_T]; the moments are summed about the pair `first`: per thread over its strided pairs in
// ascending order, then block_sum.  false: no transform (out zeroed).
__device__ __forceinline__ bool fit_members(const Sim3Items& I, int64_t b, int n, const Members& M, int count,
                                            int first, int with_scale, double* s, float* out) {
  for (int k = 0; k < S3_T; ++k) out[k] = 0.0f;
  if (count < 3) return false;  // block-uniform
  const Pair a0 = load_pair(I, b + first);
  const double pp[3] = {(double)a0.x, (double)a0.y, (double)a0.z}, pq[3] = {(double)a0.qx, (double)a0.qy, (double)a0.qz};
  double m[SIM3_MOMENTS];
  for (int k = 0; k < SIM3_MOMENTS; ++k) m[k] = 0.0;
  for (int64_t j = threadIdx.x; j < n; j += S3_BS) {
    const Pair a = load_pair(I, b + j);
    if (!M.has(a, j)) continue;
    const double p[3] = {(double)a.x - pp[0], (double)a.y - pp[1], (double)a.z - pp[2]};
    const double q[3] = {(double)a.qx - pq[0], (double)a.qy - pq[1], (double)a.qz - pq[2]};
    sim3_accumulate(m, p, q);
  }
  block_sum<SIM3_MOMENTS>(m, s);
  return sim3_from_pivot_moments((double)count, m, pp, pq, with_scale, out);
}

}  // namespace

// 2. the transform of (problem, hypothesis) g
extern "C" __global__ __launch_bounds__(64) void picp_sim3_hyp_kernel(Sim3Args A, Sim3Items I,
                                                                      const int32_t* __restrict__ samples,
                                                                      int32_t* __restrict__ hyp_valid,
                                                                      float* __restrict__ hyp_S) {
  const int64_t g = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (g >= (int64_t)A.n_problems * A.hyp) return;
  const int p = (int)(g / A.hyp);
  const int64_t n = I.offs[p + 1] - I.offs[p], b = I.base[p];
  float out[S3_T];
  for (int k = 0; k < S3_T; ++k) out[k] = 0.0f;
  bool ok = false;
  if (n >= 4) {
    double m[SIM3_MOMENTS], pp[3], pq[3];
    for (int k = 0; k < SIM3_MOMENTS; ++k) m[k] = 0.0;
    for (int k = 0; k < 3; ++k) {
      const Pair a = load_pair(I, b + samples[3 * g + k]);
      if (k == 0) {
        pp[0] = (double)a.x, pp[1] = (double)a.y, pp[2] = (double)a.z;
        pq[0] = (double)a.qx, pq[1] = (double)a.qy, pq[2] = (double)a.qz;
      }
      const double pk[3] = {(double)a.x - pp[0], (double)a.y - pp[1], (double)a.z - pp[2]};
      const double qk[3] = {(double)a.qx - pq[0], (double)a.qy - pq[1], (double)a.qz - pq[2]};
      sim3_accumulate(m, pk, qk);
    }
    ok = sim3_from_pivot_moments(3.0, m, pp, pq, A.with_scale, out);
  }
  for (int k = 0; k < S3_T; ++k) hyp_S[(size_t)g * S3_T + k] = out[k];
  hyp_valid[g] = ok ? 1 : 0;
}

// 3. the inlier counts.  Block blockIdx.x holds pairs [first, first + S3_TILE) of problem
// blk[blockIdx.x].x; slice blockIdx.y of gridDim.y takes every gridDim.y-th tile of S3_HT
// hypotheses.  cnt (hyp per problem) is zeroed by the caller.
extern "C" __global__ __launch_bounds__(S3_BS) void picp_sim3_score_kernel(Sim3Args A, Sim3Items I,
                                                                           const int2* __restrict__ blk,
                                                                           const int32_t* __restrict__ hyp_valid,
                                                                           const float* __restrict__ hyp_S,
                                                                           int32_t* __restrict__ cnt) {
  __shared__ int s_cnt[S3_HT];
  const int tid = threadIdx.x;
  const int2 bi = blk[blockIdx.x];
  const int p = bi.x, first = bi.y;
  const int n = (int)(I.offs[p + 1] - I.offs[p]);
  const int64_t b = I.base[p];
  Pair a[S3_NPT];
  unsigned long long in[S3_NPT];  // the wave's lanes that hold a pair
#pragma unroll
  for (int k = 0; k < S3_NPT; ++k) {
    const int64_t j = (int64_t)first + k * S3_BS + tid;  // n may be close to INT32_MAX
    in[k] = __builtin_amdgcn_ballot_w64(j < n);
    a[k] = load_pair(I, b + (j < n ? j : first));  // a lane past the end re-reads a valid pair, masked below
  }
  const float thr = A.threshold;
  const size_t ph0 = (size_t)p * A.hyp;
  for (int h0 = blockIdx.y * S3_HT; h0 < A.hyp; h0 += gridDim.y * S3_HT) {
    if (tid < S3_HT) s_cnt[tid] = 0;
    __syncthreads();
    const int h1 = (h0 + S3_HT < A.hyp) ? h0 + S3_HT : A.hyp;
    for (int h = h0; h < h1; ++h) {
      if (!hyp_valid[ph0 + h]) continue;  // wave-uniform: scalar loads, as the transform below
      const float* S = hyp_S + (ph0 + h) * S3_T;
      unsigned c = 0;
#pragma unroll
      for (int k = 0; k < S3_NPT; ++k) {
        const bool near = sim3_d2(S, a[k].x, a[k].y, a[k].z, a[k].qx, a[k].qy, a[k].qz) < thr;
        c += (unsigned)__builtin_popcountll(in[k] & __builtin_amdgcn_ballot_w64(near));
      }
      if ((tid & 63) == 0 && c) atomicAdd(&s_cnt[h - h0], (int)c);
    }
    __syncthreads();
    if (tid < S3_HT) {
      const int mine = s_cnt[tid];
      if (mine) atomicAdd(&cnt[ph0 + h0 + tid], mine);
    }
    __syncthreads();
  }
}

// 4. the winner of problem blockIdx.x: win[p] its hypothesis, -1 when none is valid
extern "C" __global__ __launch_bounds__(S3_BS) void picp_sim3_select_kernel(Sim3Args A,
                                                                            const int32_t* __restrict__ hyp_valid,
                                                                            const int32_t* __restrict__ cnt,
                                                                            int32_t* __restrict__ win) {
  __shared__ unsigned long long s_key[S3_BS / 64];
  const int p = blockIdx.x;
  const size_t ph0 = (size_t)p * A.hyp;
  const unsigned long long key =
      picp::block_winner<S3_BS>(A.hyp, cnt + ph0, s_key, [&](int h) { return hyp_valid[ph0 + h] != 0; });
  if (threadIdx.x == 0) win[p] = key ? (int32_t)picp::winner_entry(key) : -1;
}

// 5. the refits of problem blockIdx.x and its result.  Candidate 0 is the winner's transform;
// refit r is the least-squares transform of the inliers of candidate r - 1, and the chain ends at a
// refit that gives no transform (its count is -1).  The result is the candidate with the largest
// count, the latest on a tie.  With A.fit_only there is no chain: the result is the transform of
// the finite pairs (of those whose `fit_mask` byte is set) and found says whether there is one.
extern "C" __global__ __launch_bounds__(S3_BS) void picp_sim3_refit_kernel(
    Sim3Args A, Sim3Items I, const int32_t* __restrict__ win, const float* __restrict__ hyp_S,
    const uint8_t* __restrict__ fit_mask, float* __restrict__ refit_S, int32_t* __restrict__ refit_count,
    float* __restrict__ S_out, float* __restrict__ scale, int32_t* __restrict__ inliers,
    int32_t* __restrict__ found, float* __restrict__ rms, uint8_t* __restrict__ mask) {
  __shared__ double s_d[S3_BS / 64 * SIM3_MOMENTS];
  __shared__ int s_i[2 * (S3_BS / 64)];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n = (int)(I.offs[p + 1] - I.offs[p]);
  const int64_t b = I.base[p], o = I.offs[p];
  float cur[S3_T], res[S3_T];
  for (int k = 0; k < S3_T; ++k) cur[k] = res[k] = 0.0f;
  int res_count = -1, count = 0, first = INT32_MAX;
  bool ok;
  if (A.fit_only) {
    const Members M = finite_of(fit_mask ? fit_mask + o : nullptr);
    count_first(I, b, n, M, s_i, &count, &first);
    ok = fit_members(I, b, n, M, count, first, A.with_scale, s_d, res);
    res_count = count;
  } else {
    const int w = win[p];
    bool have = w >= 0 && n >= 4;
    if (have) {
      for (int k = 0; k < S3_T; ++k) cur[k] = res[k] = hyp_S[((size_t)p * A.hyp + w) * S3_T + k];
      const Members M = inliers_of(cur, A.threshold);
      count_first(I, b, n, M, s_i, &count, &first);
      res_count = count;
    }
    for (int r = 0; r < A.refits; ++r) {
      float nxt[S3_T];
      int c = -1;
      if (have) {
        const Members M = inliers_of(cur, A.threshold);
        have = fit_members(I, b, n, M, count, first, A.with_scale, s_d, nxt);
      }
      if (have) {
        for (int k = 0; k < S3_T; ++k) cur[k] = nxt[k];
        const Members M = inliers_of(cur, A.threshold);
        count_first(I, b, n, M, s_i, &count, &first);
        c = count;
        if (c >= res_count) {  // a tie goes to the refit: the least-squares answer of as many inliers
          res_count = c;
          for (int k = 0; k < S3_T; ++k) res[k] = cur[k];
        }
      } else {
        for (int k = 0; k < S3_T; ++k) nxt[k] = 0.0f;
      }
      if (refit_S && tid < S3_T) {
        float v = 0.0f;
        for (int k = 0; k < S3_T; ++k) v = (k == tid) ? nxt[k] : v;
        refit_S[((size_t)p * A.refits + r) * S3_T + tid] = v;
      }
      if (refit_count && tid == 0) refit_count[(size_t)p * A.refits + r] = c;
    }
    ok = res_count >= 0 && res_count >= A.min_inliers;
  }
  // the result's RMS distance over its members, and the mask
  double sum[1] = {0.0};
  if (ok) {
    const Members M = A.fit_only ? finite_of(fit_mask ? fit_mask + o : nullptr) : inliers_of(res, A.threshold);
    for (int64_t j = tid; j < n; j += S3_BS) {
      const Pair a = load_pair(I, b + j);
      const bool in = M.has(a, j);
      if (in) sum[0] += (double)sim3_d2(res, a.x, a.y, a.z, a.qx, a.qy, a.qz);
      if (mask) mask[o + j] = in ? 1 : 0;
    }
    block_sum<1>(sum, s_d);
  } else if (mask) {
    for (int64_t j = tid; j < n; j += S3_BS) mask[o + j] = 0;
  }
  if (tid < 16) {
    float val = (tid % 5 == 0) ? 1.0f : 0.0f;  // the identity, and the bottom row
    const int r = tid & 3, c = tid >> 2;
    if (ok && r < 3) {
      const int at = (c < 3) ? 3 * c + r : 9 + r;
      for (int k = 0; k < 12; ++k) val = (k == at) ? res[k] : val;
    }
    S_out[16 * (size_t)p + tid] = val;
  }
  if (tid == 0) {
    if (scale) scale[p] = ok ? res[12] : 1.0f;
    if (inliers) inliers[p] = res_count > 0 ? res_count : 0;
    found[p] = ok ? 1 : 0;
    if (rms) rms[p] = (ok && res_count > 0) ? (float)sqrt(sum[0] / (double)res_count) : 0.0f;
  }
}

// ------------------------------- the VO hookup's glue -------------------------------
// picp_vo_align_segments: problem s matches segment s + 1's map (the queries) against segment s's
// (the references); its accepted queries, in ascending query index, become the pairs.

// the match problems from the segments' map counts; matcher rows are map slots
extern "C" __global__ __launch_bounds__(64) void picp_vo_align_probs_kernel(const VoSegment* __restrict__ segs,
                                                                            const int64_t* __restrict__ map_n,
                                                                            int n_problems,
                                                                            MatchProblem* __restrict__ probs) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= n_problems) return;
  MatchProblem q;
  q.q_off = segs[s + 1].map_off;
  q.nq = map_n[s + 1];
  q.r_off = segs[s].map_off;
  q.nr = map_n[s];
  q.idx0 = 0;
  probs[s] = q;
}

// the accepted queries of problem blockIdx.x
extern "C" __global__ __launch_bounds__(S3_BS) void picp_vo_align_count_kernel(const MatchProblem* __restrict__ probs,
                                                                               const int32_t* __restrict__ accepted,
                                                                               int64_t* __restrict__ n_pairs) {
  __shared__ int s_w[S3_BS / 64];
  const MatchProblem q = probs[blockIdx.x];
  int c = 0;
  for (int64_t j = threadIdx.x; j < q.nq; j += S3_BS) c += accepted[q.q_off + j] != 0 ? 1 : 0;
  int total;
  picp::block_scan<S3_BS / 64>(c, s_w, &total);
  if (threadIdx.x == 0) n_pairs[blockIdx.x] = total;
}

// the pairs of problem blockIdx.x at offs[blockIdx.x], in ascending query index: src the query's
// point, dst its best reference's (packed float3 each)
extern "C" __global__ __launch_bounds__(S3_BS) void picp_vo_align_pairs_kernel(
    const MatchProblem* __restrict__ probs, const int32_t* __restrict__ accepted, const int32_t* __restrict__ best,
    const float* __restrict__ map_xyz, const int64_t* __restrict__ offs, float* __restrict__ src,
    float* __restrict__ dst) {
  __shared__ int s_w[S3_BS / 64];
  const MatchProblem q = probs[blockIdx.x];
  const int64_t o = offs[blockIdx.x], room = offs[blockIdx.x + 1] - o;
  int64_t done = 0;
  for (int64_t j0 = 0; j0 < q.nq; j0 += S3_BS) {
    const int64_t j = j0 + threadIdx.x;
    const bool acc = j < q.nq && accepted[q.q_off + j] != 0;
    int total;
    const int64_t k = done + picp::block_scan<S3_BS / 64>(acc ? 1 : 0, s_w, &total);
    if (acc && k < room) {  // room is the count of the same flags: always true
      int64_t r = best[q.q_off + j];
      r = r < 0 ? 0 : (r >= q.nr ? q.nr - 1 : r);  // an accepted query has a best reference in range
      for (int c = 0; c < 3; ++c) {
        src[3 * (o + k) + c] = map_xyz[3 * (q.q_off + j) + c];
        dst[3 * (o + k) + c] = map_xyz[3 * (q.r_off + r) + c];
      }
    }
    done += total;
    __syncthreads();  // s_w is written again
  }
}

// ------------------------------- host launch wrappers -------------------------------
// Every per-(problem, hypothesis) array is indexed p * hyp + h; problems sit on grid x.
extern "C" int picp_sim3_score_tile(void) { return S3_TILE; }
extern "C" int picp_sim3_hyp_tile(void) { return S3_HT; }

extern "C" hipError_t picp_launch_sim3_hyp(hipStream_t stream, const Sim3Args* A, const Sim3Items* I,
                                           const int32_t* samples, int32_t* hyp_valid, float* hyp_S) {
  const int64_t g = (int64_t)A->n_problems * A->hyp;
  hipLaunchKernelGGL(picp_sim3_hyp_kernel, dim3((unsigned)((g + 63) / 64)), dim3(64), 0, stream, *A, *I, samples,
                     hyp_valid, hyp_S);
  return hipGetLastError();
}

extern "C" hipError_t picp_launch_sim3_score(hipStream_t stream, const Sim3Args* A, const Sim3Items* I, int nb,
                                             const int2* blk, int hsplit, const int32_t* hyp_valid,
                                             const float* hyp_S, int32_t* cnt) {
  if (nb <= 0) return hipSuccess;  // no problem has a pair
  hipLaunchKernelGGL(picp_sim3_score_kernel, dim3((unsigned)nb, (unsigned)hsplit), dim3(S3_BS), 0, stream, *A, *I, blk,
                     hyp_valid, hyp_S, cnt);
  return hipGetLastError();
}

extern "C" hipError_t picp_launch_sim3_select(hipStream_t stream, const Sim3Args* A, const int32_t* hyp_valid,
                                              const int32_t* cnt, int32_t* win) {
  hipLaunchKernelGGL(picp_sim3_select_kernel, dim3((unsigned)A->n_problems), dim3(S3_BS), 0, stream, *A, hyp_valid,
                     cnt, win);
  return hipGetLastError();
}

extern "C" hipError_t picp_launch_sim3_refit(hipStream_t stream, const Sim3Args* A, const Sim3Items* I,
                                             const int32_t* win, const float* hyp_S, const uint8_t* fit_mask,
                                             float* refit_S, int32_t* refit_count, float* S_out, float* scale,
                                             int32_t* inliers, int32_t* found, float* rms, uint8_t* mask) {
  hipLaunchKernelGGL(picp_sim3_refit_kernel, dim3((unsigned)A->n_problems), dim3(S3_BS), 0, stream, *A, *I, win, hyp_S,
                     fit_mask, refit_S, refit_count, S_out, scale, inliers, found, rms, mask);
  return hipGetLastError();
}

extern "C" hipError_t picp_launch_vo_align_probs(hipStream_t stream, const VoSegment* segs, const int64_t* map_n,
                                                 int n_problems, MatchProblem* probs) {
  hipLaunchKernelGGL(picp_vo_align_probs_kernel, dim3((unsigned)((n_problems + 63) / 64)), dim3(64), 0, stream, segs,
                     map_n, n_problems, probs);
  return hipGetLastError();
}

extern "C" hipError_t picp_launch_vo_align_count(hipStream_t stream, const MatchProblem* probs, int n_problems,
                                                 const int32_t* accepted, int64_t* n_pairs) {
  hipLaunchKernelGGL(picp_vo_align_count_kernel, dim3((unsigned)n_problems), dim3(S3_BS), 0, stream, probs, accepted,
                     n_pairs);
  return hipGetLastError();
}

extern "C" hipError_t picp_launch_vo_align_pairs(hipStream_t stream, const MatchProblem* probs, int n_problems,
                                                 const int32_t* accepted, const int32_t* best, const float* map_xyz,
                                                 const int64_t* offs, float* src, float* dst) {
  hipLaunchKernelGGL(picp_vo_align_pairs_kernel, dim3((unsigned)n_problems), dim3(S3_BS), 0, stream, probs, accepted,
                     best, map_xyz, offs, src, dst);
  return hipGetLastError();
}
