// picp_classify.hip -- which correspondences a pose rests on (include/picp_c.h picp_classify,
// picp_batch_classify, picp_vo_set_track_stats).  Read-only observers of the solvers' data: no
// kernel here writes a pose, a stat, a plane or a map.
//
//   picp_classify_kernel : streams the batch's SoA planes (20 B per item) tile by tile, writes the
//                          state byte of every item (and chi2 / the projection when asked) in the
//                          caller's packed order, and the tile's inlier and outlier counts.
//   picp_classify_scan_kernel    : one block: exclusive scan of the tile counts over the whole
//                          grid; per-problem counts and inlier offsets are differences of it.
//   picp_classify_scatter_kernel : re-reads the state bytes and writes the inlier indices at
//                          scan value + rank inside the tile.
// A tile never straddles a problem and tiles are in problem order, so the compaction is
// problem-major ascending by construction; ranks come from wave ballots, a popcount prefix and an
// LDS scan over the block's waves (the scheme of vo_block_rank), never from the arrival order of
// an atomic.  The tiling is the pass's own (CLS_TILE), independent of the solve layout's mode,
// items per block or split.
//
//   vo_track_kernel      : the VO sequence's per-map-point counters: one block per segment over
//                          the step's frame->map matches (shaped like vo_gather_kernel).
#include "picp_item.h"
#include "picp_launch.h"
#include "picp_pose.h"
#include "picp_variant.h"
#include "picp_wave.h"

using namespace picp;

#define CLS_BLOCK 256
#define CLS_WAVES (CLS_BLOCK / 64)
#define CLS_TILE (4 * CLS_BLOCK)  // items per block: one float4 per plane and lane
#define CLS_SCAN_BLOCK 1024
#define CLS_SCAN_WAVES (CLS_SCAN_BLOCK / 64)
#define CLS_SCAN_PER 8  // consecutive tiles per lane and round of the scan

// blk[b] = (problem, first item of the tile inside the problem, items in the tile, -);
// plane_off[p] / pack_off[p] = the problem's first item in the planes (a multiple of 4) and in the
// caller's packed arrays; cnt[3 b ..] = the tile's skipped / inlier / outlier counts.
__global__ __launch_bounds__(CLS_BLOCK) void picp_classify_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ Z,
    const float* __restrict__ U, const float* __restrict__ V, const ClsArgs a,
    const int4* __restrict__ blk, const int64_t* __restrict__ plane_off,
    const int64_t* __restrict__ pack_off, const PicpState* __restrict__ st,
    uint8_t* __restrict__ state, float* __restrict__ chi2, float* __restrict__ uv,
    int* __restrict__ cnt) {
  __shared__ int s_cnt[CLS_WAVES][2];
  const int4 bi = blk[blockIdx.x];
  const int n = bi.z;
  const int64_t pbase = plane_off[bi.x] + bi.y;  // multiple of 4: float4 loads
  const int64_t obase = pack_off[bi.x] + bi.y;
  Pose T;
  Cam C;
  pose_load(st[bi.x].R, st[bi.x].t, T);
  cam_load(a.K, a.maxx, a.maxy, C);
  const int i0 = 4 * (int)threadIdx.x;
  float x[4] = {0, 0, 0, 0}, y[4] = {0, 0, 0, 0}, z[4] = {0, 0, 0, 0}, u[4] = {0, 0, 0, 0}, v[4] = {0, 0, 0, 0};
  if (i0 < n) {  // planes are padded to a multiple of 4 per problem: the whole float4 is in bounds
    const float4 fx = *reinterpret_cast<const float4*>(X + pbase + i0);
    const float4 fy = *reinterpret_cast<const float4*>(Y + pbase + i0);
    const float4 fz = *reinterpret_cast<const float4*>(Z + pbase + i0);
    const float4 fu = *reinterpret_cast<const float4*>(U + pbase + i0);
    const float4 fv = *reinterpret_cast<const float4*>(V + pbase + i0);
    x[0] = fx.x; x[1] = fx.y; x[2] = fx.z; x[3] = fx.w;
    y[0] = fy.x; y[1] = fy.y; y[2] = fy.z; y[3] = fy.w;
    z[0] = fz.x; z[1] = fz.y; z[2] = fz.z; z[3] = fz.w;
    u[0] = fu.x; u[1] = fu.y; u[2] = fu.z; u[3] = fu.w;
    v[0] = fv.x; v[1] = fv.y; v[2] = fv.z; v[3] = fv.w;
  }
  int s[4];
  float chi[4], pu[4], pv[4];
  int n_in = 0, n_out = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool in_range = i0 + k < n;
    s[k] = classify_item(T, C, a.threshold, a.pinhole != 0, x[k], y[k], z[k], u[k], v[k], &chi[k], &pu[k], &pv[k]);
    n_in += __popcll(__ballot(in_range && s[k] == 1));
    n_out += __popcll(__ballot(in_range && s[k] == 2));
  }
  // the packed position of the tile is a multiple of 4 unless an earlier problem's size is not:
  // whole-vector stores then, element stores otherwise and in the problem's last lanes
  const bool vec = ((obase & 3) == 0) && (i0 + 3 < n);
  if (vec) {
    *reinterpret_cast<uchar4*>(state + obase + i0) =
        make_uchar4((unsigned char)s[0], (unsigned char)s[1], (unsigned char)s[2], (unsigned char)s[3]);
    if (chi2) *reinterpret_cast<float4*>(chi2 + obase + i0) = make_float4(chi[0], chi[1], chi[2], chi[3]);
    if (uv) {
      float4* o = reinterpret_cast<float4*>(uv + 2 * (obase + i0));
      o[0] = make_float4(pu[0], pv[0], pu[1], pv[1]);
      o[1] = make_float4(pu[2], pv[2], pu[3], pv[3]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (i0 + k < n) {
        state[obase + i0 + k] = (uint8_t)s[k];
        if (chi2) chi2[obase + i0 + k] = chi[k];
        if (uv) {
          uv[2 * (obase + i0 + k)] = pu[k];
          uv[2 * (obase + i0 + k) + 1] = pv[k];
        }
      }
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    s_cnt[w][0] = n_in;
    s_cnt[w][1] = n_out;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int ti = 0, to = 0;
#pragma unroll
    for (int k = 0; k < CLS_WAVES; ++k) {
      ti += s_cnt[k][0];
      to += s_cnt[k][1];
    }
    cnt[3 * (int64_t)blockIdx.x + 0] = n - ti - to;
    cnt[3 * (int64_t)blockIdx.x + 1] = ti;
    cnt[3 * (int64_t)blockIdx.x + 2] = to;
  }
}

// One block.  base[c * (nb + 1) + b] = the number of class-c items in tiles 0 .. b-1 (entry nb:
// the batch's total).  pblk[p] = (first tile, tiles) of problem p: its counts and its first
// inlier's position are differences / entries of the scan.
// A lane owns CLS_SCAN_PER consecutive tiles of a round and loads all their counts before it uses
// any (one memory round trip per round, not one per tile); a round covers CLS_SCAN_BLOCK x
// CLS_SCAN_PER tiles (8.4M items) and its sums fit an int, the running totals between rounds are
// 64-bit.
__global__ __launch_bounds__(CLS_SCAN_BLOCK) void picp_classify_scan_kernel(
    const int* __restrict__ cnt, int nb, long long* base, const int2* __restrict__ pblk, int np,
    long long* __restrict__ counts, long long* __restrict__ inl_off) {
  __shared__ int s_w[3][CLS_SCAN_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  long long carry[3] = {0, 0, 0};
  for (int64_t r0 = 0; r0 < nb; r0 += (int64_t)CLS_SCAN_BLOCK * CLS_SCAN_PER) {
    const int64_t lo = r0 + (int64_t)tid * CLS_SCAN_PER;
    int v[CLS_SCAN_PER][3];
#pragma unroll
    for (int k = 0; k < CLS_SCAN_PER; ++k) {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[k][c] = (lo + k < nb) ? cnt[3 * (lo + k) + c] : 0;
    }
    int sum[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < CLS_SCAN_PER; ++k) {
#pragma unroll
      for (int c = 0; c < 3; ++c) sum[c] += v[k][c];
    }
    int excl[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int inc = wave_scan(sum[c], lane);
      if (lane == 63) s_w[c][w] = inc;
      excl[c] = inc - sum[c];
    }
    __syncthreads();
    long long run[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int pre, tot;
      wave_totals<CLS_SCAN_WAVES>(s_w[c], w, &pre, &tot);
      run[c] = carry[c] + pre + excl[c];
      carry[c] += tot;
    }
#pragma unroll
    for (int k = 0; k < CLS_SCAN_PER; ++k) {
      if (lo + k < nb) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          base[(int64_t)c * (nb + 1) + lo + k] = run[c];
          run[c] += v[k][c];
        }
      }
    }
    __syncthreads();  // s_w is reused by the next round
  }
  if (tid == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) base[(int64_t)c * (nb + 1) + nb] = carry[c];
    inl_off[np] = carry[1];
  }
  // The block's own stores to base are read back below: the barrier's workgroup-scope fence is
  // enough (one CU, one vector cache).  A device-scope fence here wrote the L2 back, with it the
  // state bytes the classify kernel had just stored: 50 us at 16M items, 9 us at 1M.
  __syncthreads();
  for (int p = tid; p < np; p += CLS_SCAN_BLOCK) {
    const int2 pb = pblk[p];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const volatile long long* bc = base + (int64_t)c * (nb + 1);
      counts[3 * (int64_t)p + c] = bc[pb.x + pb.y] - bc[pb.x];
    }
    inl_off[p] = ((const volatile long long*)base)[(int64_t)(nb + 1) + pb.x];
  }
}

__global__ __launch_bounds__(CLS_BLOCK) void picp_classify_scatter_kernel(
    const int4* __restrict__ blk, const int64_t* __restrict__ pack_off,
    const uint8_t* __restrict__ state, const long long* __restrict__ base_inl,
    int32_t* __restrict__ idx) {
  __shared__ int s_cnt[CLS_WAVES];
  const long long b0 = base_inl[blockIdx.x];
  if (base_inl[blockIdx.x + 1] == b0) return;  // uniform: a tile without inliers
  const int4 bi = blk[blockIdx.x];
  const int n = bi.z;
  const int64_t obase = pack_off[bi.x] + bi.y;
  const int i0 = 4 * (int)threadIdx.x;
  bool f[4] = {false, false, false, false};
  if (((obase & 3) == 0) && (i0 + 3 < n)) {
    const uchar4 q = *reinterpret_cast<const uchar4*>(state + obase + i0);
    f[0] = q.x == 1; f[1] = q.y == 1; f[2] = q.z == 1; f[3] = q.w == 1;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = (i0 + k < n) && state[obase + i0 + k] == 1;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long lt = (1ull << lane) - 1ull;
  int below = 0, wave = 0;  // inliers of the wave's lower lanes / of the whole wave
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long m = __ballot(f[k]);
    below += __popcll(m & lt);
    wave += __popcll(m);
  }
  if (lane == 0) s_cnt[w] = wave;
  __syncthreads();
  int pre = 0;
#pragma unroll
  for (int k = 0; k < CLS_WAVES; ++k) pre += (k < w) ? s_cnt[k] : 0;
  long long pos = b0 + pre + below;  // item order = lane-major, then k: ascending index
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (f[k]) idx[pos++] = bi.y + i0 + k;
  }
}

// One block per segment, one thread per observation of frame f0 + t + 1 (vo_gather_kernel's
// shape): every accepted frame->map match counts for its map point, and counts as an inlier when
// it is one at the step's final PICP pose (st_out, the block kernel's result state).  Several
// observations of a frame can match one map point: the adds are atomic (integer adds: the
// counters do not depend on their order).
__global__ __launch_bounds__(CLS_BLOCK) void vo_track_kernel(const VoArgs a, int t, const ClsArgs c,
                                                           int* __restrict__ n_matched,
                                                           int* __restrict__ n_inlier) {
  const int s = a.seg0 + (int)blockIdx.x;
  const VoSegment G = a.segs[s];
  if (t >= G.steps) return;  // uniform: segment finished
  const int64_t nf = G.f0 + t + 1;
  const int64_t on = a.frame_off[nf], nn = a.frame_off[nf + 1] - on;
  const int64_t moff = G.map_off;
  Pose T;
  Cam C;
  pose_load(a.st_out[s].R, a.st_out[s].t, T);
  cam_load(c.K, c.maxx, c.maxy, C);
  for (int64_t i = threadIdx.x; i < nn; i += CLS_BLOCK) {
    if (a.wm_acc[on + i] == 0) continue;
    const int64_t j = moff + a.wm_bi[on + i];
    const float2 z = a.uv[on + i];
    float chi, pu, pv;
    const int st = classify_item(T, C, c.threshold, c.pinhole != 0, a.map_xyz[3 * j + 0], a.map_xyz[3 * j + 1],
                                 a.map_xyz[3 * j + 2], z.x, z.y, &chi, &pu, &pv);
    atomicAdd(n_matched + j, 1);
    if (st == 1) atomicAdd(n_inlier + j, 1);
  }
}

extern "C" int picp_classify_tile(void) { return CLS_TILE; }

// the three launches of one classify pass over nb tiles (idx == nullptr: no compaction)
extern "C" hipError_t picp_launch_classify(hipStream_t stream, int nb, int np, const float* X, const float* Y,
                                           const float* Z, const float* U, const float* V, const ClsArgs* a,
                                           const int4* blk, const int2* pblk, const int64_t* plane_off,
                                           const int64_t* pack_off, const PicpState* st, uint8_t* state,
                                           float* chi2, float* uv, int* cnt, long long* base,
                                           long long* counts, long long* inl_off, int32_t* idx) {
  if (!a || nb <= 0 || np <= 0) return hipErrorInvalidValue;
  ClsArgs ca = *a;
  ca.pinhole = picp_use_pinhole(ca.K) ? 1 : 0;  // the camera path the solve kernels take
  hipLaunchKernelGGL(picp_classify_kernel, dim3(nb), dim3(CLS_BLOCK), 0, stream, X, Y, Z, U, V, ca, blk, plane_off,
                     pack_off, st, state, chi2, uv, cnt);
  hipLaunchKernelGGL(picp_classify_scan_kernel, dim3(1), dim3(CLS_SCAN_BLOCK), 0, stream, cnt, nb, base, pblk, np,
                     counts, inl_off);
  if (idx)
    hipLaunchKernelGGL(picp_classify_scatter_kernel, dim3(nb), dim3(CLS_BLOCK), 0, stream, blk, pack_off, state,
                       base + (int64_t)(nb + 1), idx);
  return hipGetLastError();
}

extern "C" hipError_t picp_launch_vo_track(hipStream_t stream, const VoArgs* a, int t, const ClsArgs* c,
                                           int* n_matched, int* n_inlier) {
  if (!a || !c || a->n_seg <= 0 || !n_matched || !n_inlier) return hipErrorInvalidValue;
  ClsArgs ca = *c;
  ca.pinhole = picp_use_pinhole(ca.K) ? 1 : 0;
  hipLaunchKernelGGL(vo_track_kernel, dim3(a->n_seg), dim3(CLS_BLOCK), 0, stream, *a, t, ca, n_matched, n_inlier);
  return hipGetLastError();
}
