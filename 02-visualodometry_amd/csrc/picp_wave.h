// picp_wave.h -- cross-lane and cross-wave primitives: DPP and permlane moves, the wave64 sum of
// the 32 normal-equation terms, sums over a 16-lane DPP row, and the integer scans (a wave's
// inclusive scan, a block's exclusive scan).
#pragma once
#include <hip/hip_runtime.h>

namespace picp {

// Cross-lane moves without the LDS crossbar.  gfx950 v_permlane32_swap / v_permlane16_swap
// exchange half-waves / odd-even 16-lane rows between two registers; DPP reads a partner
// lane inside a 16-lane row (row_mirror l^15, row_half_mirror l^7, quad_perm l^2, l^1).
// bound_ctrl on: a lane whose source lane is disabled in EXEC reads 0, so the result never depends
// on the destination's old contents (every call site runs with EXEC full, where no source lane is
// disabled).  Passing the source as DPP "old" instead (round 4) tied the destination to it and
// cost a register copy per move: C2/C3 1-2 % slower in interleaved A/B (profiles/r05/ab_regress/).
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}
#define DPP_ROW_MIRROR 0x140
#define DPP_ROW_HALF_MIRROR 0x141
#define DPP_QUAD_XOR2 0x4E  // quad_perm [2,3,0,1]
#define DPP_QUAD_XOR1 0xB1  // quad_perm [1,0,3,2]

// Halving-butterfly step inside a 16-lane row: lanes l and P(l) (P an involution that flips
// bit HB) exchange the half of the 2*HALF values the other keeps.
template <int CTRL, int HB, int HALF>
__device__ __forceinline__ void bfly_dpp(float* v, int lane) {
  const bool hi = (lane >> HB) & 1;
#pragma unroll
  for (int i = 0; i < HALF; ++i) {
    const float send = hi ? v[i] : v[i + HALF];
    const float keep = hi ? v[i + HALF] : v[i];
    v[i] = keep + dpp<CTRL>(send);
  }
}

// Sum 32 per-lane values over the 64 lanes of a wave (32 -> 16 -> 8 -> 4 -> 2 -> 1 values per
// lane).  The swap steps need no select: after v_permlane32_swap(a=v[i], b=v[i+16]) the low
// half holds (own v[i], partner v[i]) and the high half (partner v[i+16], own v[i+16]), so a+b
// is the pair sum of the half each lane keeps.  Returns, in every lane, the wave total of value
// index (lane >> 1).
__device__ __forceinline__ float wave_reduce32_bperm(float* v, int lane) {
  // the half-wave exchanges through ds_bpermute (bit-identical sums in the same order)
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const bool hi = (lane & 32) != 0;
    const float send = hi ? v[i] : v[i + 16], keep = hi ? v[i + 16] : v[i];
    v[i] = keep + __shfl_xor(send, 32);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const bool hi = (lane & 16) != 0;
    const float send = hi ? v[i] : v[i + 8], keep = hi ? v[i + 8] : v[i];
    v[i] = keep + __shfl_xor(send, 16);
  }
  bfly_dpp<DPP_ROW_MIRROR, 3, 4>(v, lane);
  bfly_dpp<DPP_ROW_HALF_MIRROR, 2, 2>(v, lane);
  bfly_dpp<DPP_QUAD_XOR2, 1, 1>(v, lane);
  return v[0] + dpp<DPP_QUAD_XOR1>(v[0]);
}

__device__ __forceinline__ float wave_reduce32(float* v, int lane) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[i]), __float_as_uint(v[i + 16]), false, false);
    v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[i]), __float_as_uint(v[i + 8]), false, false);
    v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
  bfly_dpp<DPP_ROW_MIRROR, 3, 4>(v, lane);
  bfly_dpp<DPP_ROW_HALF_MIRROR, 2, 2>(v, lane);
  bfly_dpp<DPP_QUAD_XOR2, 1, 1>(v, lane);
  return v[0] + dpp<DPP_QUAD_XOR1>(v[0]);
}

// x + (x of the lane 16, or 32, away) for a double, through the swaps of wave_reduce32 on its two
// halves (no LDS round trip, unlike __shfl_xor's ds_bpermute).  With both operands x, the swap
// leaves (own, partner) in one half of the pair and (partner, own) in the other: the sum is
// own + partner or partner + own, the same bits (IEEE addition commutes).
template <int DIST>
__device__ __forceinline__ double wave_add_xor_f64(double x) {
  static_assert(DIST == 16 || DIST == 32, "the two swap distances");
  const unsigned lo = (unsigned)__double_as_longlong(x), hi = (unsigned)(__double_as_longlong(x) >> 32);
  unsigned a_lo, a_hi, b_lo, b_hi;
  if constexpr (DIST == 16) {
    const auto rl = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto rh = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    a_lo = rl[0]; b_lo = rl[1]; a_hi = rh[0]; b_hi = rh[1];
  } else {
    const auto rl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto rh = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    a_lo = rl[0]; b_lo = rl[1]; a_hi = rh[0]; b_hi = rh[1];
  }
  const double a = __longlong_as_double((long long)(((unsigned long long)a_hi << 32) | a_lo));
  const double b = __longlong_as_double((long long)(((unsigned long long)b_hi << 32) | b_lo));
  return a + b;
}

// dpp() for a double: its two halves moved separately
template <int CTRL>
__device__ __forceinline__ double dpp64(double v) {
  const long long q = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_mov_dpp((int)q, CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp((int)(q >> 32), CTRL, 0xF, 0xF, true);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// v summed over the 16 lanes of a DPP row, the same bits in every lane: each step adds the partner
// of an involution, so both partners form the same (commutative) sum.  EXEC must be full.
__device__ __forceinline__ int row_sum(int v) {
  v += __builtin_amdgcn_mov_dpp(v, DPP_ROW_MIRROR, 0xF, 0xF, true);
  v += __builtin_amdgcn_mov_dpp(v, DPP_ROW_HALF_MIRROR, 0xF, 0xF, true);
  v += __builtin_amdgcn_mov_dpp(v, DPP_QUAD_XOR2, 0xF, 0xF, true);
  return v + __builtin_amdgcn_mov_dpp(v, DPP_QUAD_XOR1, 0xF, 0xF, true);
}

__device__ __forceinline__ double row_sum(double v) {
  v += dpp64<DPP_ROW_MIRROR>(v);
  v += dpp64<DPP_ROW_HALF_MIRROR>(v);
  v += dpp64<DPP_QUAD_XOR2>(v);
  return v + dpp64<DPP_QUAD_XOR1>(v);
}

// inclusive scan over the wave's lanes
__device__ __forceinline__ int wave_scan(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    v += (lane >= d) ? o : 0;
  }
  return v;
}

// From the WAVES wave totals in s_w (LDS, written before a barrier): the sum of the waves below
// wave w, and of all of them.
template <int WAVES>
__device__ __forceinline__ void wave_totals(const int* s_w, int w, int* pre, int* tot) {
  int p = 0, t = 0;
#pragma unroll
  for (int k = 0; k < WAVES; ++k) {
    p += (k < w) ? s_w[k] : 0;
    t += s_w[k];
  }
  *pre = p;
  *tot = t;
}

// Exclusive scan of v over the threads of a block of WAVES waves, and the block's total.  s_w:
// WAVES ints of LDS.  Contains one barrier (every thread calls); the caller puts another before
// s_w is used again.
template <int WAVES>
__device__ __forceinline__ int block_scan(int v, int* s_w, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int inc = wave_scan(v, lane);
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  int pre;
  wave_totals<WAVES>(s_w, w, &pre, total);
  return pre + inc - v;
}

}  // namespace picp
