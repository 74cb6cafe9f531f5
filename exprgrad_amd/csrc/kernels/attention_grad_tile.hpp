// What the float32 backward kernels share (attention_grad_f32.hip: dQ, dK/dV; attention_dbias_f32.hip: dBias): a tile's part
// of O, delta and 1 / L of its 64 rows, and the way a block's accumulators leave through LDS.  One copy for the three kernels:
// the same dO and O rows give the same delta bits in each.
#pragma once

#include "attention_tile.hpp"

namespace eg {
namespace attention {

// A quarter of each of the tile's 64 rows of O per thread: thread tid holds columns 16 n + 4 (tid & 3) + {0, 1, 2, 3} of row
// tid >> 2.  Zero outside rows x D, where nothing is read.
template <int DP>
struct OPart {
  f32x4 r[DP / 16];
};

template <int DP>
__device__ __forceinline__ void load_o_part(OPart<DP>& o, const float* __restrict__ base, long ld, long rows, int width, bool vec, int tid) {
  const int row = tid >> 2, part = tid & 3;
#pragma unroll
  for (int n = 0; n < DP / 16; ++n) {
    const int col = 16 * n + 4 * part;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row < rows && col < width) {
      const float* p = base + (long)row * ld + col;
      if (vec && col + 4 <= width) {
        v = *reinterpret_cast<const f32x4*>(p);
      } else {
        v[0] = p[0];
        if (col + 1 < width) v[1] = p[1];
        if (col + 2 < width) v[2] = p[2];
        if (col + 3 < width) v[3] = p[3];
      }
    }
    o.r[n] = v;
  }
}

// delta of row tid >> 2 of a dO tile in LDS (row step `stride`) against the thread's part of O: each of the row's four
// threads adds its columns in ascending order with fused multiply-adds, then the four fold by xor 1 and xor 2.  The one
// summation order of both kernels: the same dO and O rows give the same bits in either.
template <int DP>
__device__ __forceinline__ float row_delta(const float* __restrict__ dOs, int stride, const OPart<DP>& o, int tid) {
  const float* const d = dOs + (tid >> 2) * stride + 4 * (tid & 3);
  float acc = 0.f;
#pragma unroll
  for (int n = 0; n < DP / 16; ++n) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(d + 16 * n);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __fmaf_rn(x[e], o.r[n][e], acc);
  }
  acc += __shfl_xor(acc, 1);
  acc += __shfl_xor(acc, 2);
  return acc;
}

// The row sums of a tile's 64 rows: threads 0 .. 15 hold four each.  Rows outside the problem are not read.
__device__ __forceinline__ f32x4 load_sums(const float* __restrict__ S, long rows, bool vec, int tid) {
  f32x4 v = {1.f, 1.f, 1.f, 1.f};
  const int r0 = 4 * tid;
  if (tid < 16 && r0 < rows) {
    if (vec && r0 + 4 <= rows) {
      v = *reinterpret_cast<const f32x4*>(S + r0);
    } else {
      v[0] = S[r0];
      if (r0 + 1 < rows) v[1] = S[r0 + 1];
      if (r0 + 2 < rows) v[2] = S[r0 + 2];
      if (r0 + 3 < rows) v[3] = S[r0 + 3];
    }
  }
  return v;
}

// St[SW * row] = 1 / L of the tile's rows, 0 for rows outside the problem; SW the floats St holds per row
template <int SW = 2>
__device__ __forceinline__ void store_inverse_sums(const f32x4& v, float* __restrict__ St, long rows, int tid) {
  if (tid < 16) {
#pragma unroll
    for (int e = 0; e < 4; ++e) St[SW * (4 * tid + e)] = 4 * tid + e < rows ? 1.f / v[e] : 0.f;
  }
}

// St[SW * row + 2] = the row maximum of the tile's rows (eg_attention_stable_grad), loaded as load_sums loads: a row outside
// the problem holds 1, and its 1 / L of 0 makes its terms 0
template <int SW>
__device__ __forceinline__ void store_maxima(const f32x4& v, float* __restrict__ St, int tid) {
  if (tid < 16) {
#pragma unroll
    for (int e = 0; e < 4; ++e) St[SW * (4 * tid + e) + 2] = v[e];
  }
}

// The wave's accumulators (rows 4 g + r of its 16, columns 16 nb + c) into a [64][STRIDE] LDS tile
template <int WP, int STRIDE>
__device__ __forceinline__ void stage_acc(const f32x4 (&acc)[WP / 16], float* __restrict__ lds, int w, int c, int g) {
#pragma unroll
  for (int nb = 0; nb < WP / 16; ++nb) {
#pragma unroll
    for (int r = 0; r < 4; ++r) lds[(w * 16 + 4 * g + r) * STRIDE + nb * 16 + c] = acc[nb][r];
  }
}

// Rows [0, rows) x columns [0, width) of a [64][STRIDE] LDS tile to `base` (row step ld), chunk by chunk as load_rows reads:
// whole chunks as 16-byte stores when `vec`, everything else element by element; nothing outside is written, and nothing is
// read unless `accumulate`.
template <int WP, int STRIDE>
__device__ __forceinline__ void store_out(const float* __restrict__ lds, float* __restrict__ base, long ld, long rows, int width, bool vec,
                                          bool accumulate, int tid) {
  constexpr int CPR = WP / 4;
#pragma unroll
  for (int i = 0; i < WP / 16; ++i) {
    const int idx = tid + i * THREADS;
    const int row = idx / CPR, col = (idx % CPR) * 4;
    if (row < rows && col < width) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(&lds[row * STRIDE + col]);
      float* const p = base + (long)row * ld + col;
      if (vec && col + 4 <= width) {
        f32x4 x = v;
        if (accumulate) x = *reinterpret_cast<const f32x4*>(p) + v;
        *reinterpret_cast<f32x4*>(p) = x;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (col + e < width) p[e] = accumulate ? p[e] + v[e] : v[e];
      }
    }
  }
}

}  // namespace attention
}  // namespace eg
