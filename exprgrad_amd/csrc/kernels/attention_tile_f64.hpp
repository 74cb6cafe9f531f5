// What the float64 attention kernels share (attention_f64.hip, attention_grad_f64.hip): a [ROWS][WP] tile of doubles in the
// registers of a block's 256 threads on its way from global memory to LDS, and the two MFMA loops over such tiles on
// v_mfma_f64_16x16x4_f64.  The f32 helpers of attention_tile.hpp are not instantiated on doubles: the f64 instruction hands a
// lane rows g + 4 r, not four neighbours, and a 16-byte chunk holds two elements.
#pragma once

#include "attention_tile.hpp"   // Arg, THREADS, wave_sync, the launcher
#include "gemm_f64_tile.hpp"    // d4, d2

namespace eg {
namespace attention {

using eg::f64tile::d2;
using eg::f64tile::d4;

using InD = Arg<const double>;
using OutD = Arg<double>;

// ---- tiles ------------------------------------------------------------------------------------------------------------
// A [ROWS][WP] tile in the registers of 256 threads: ROWS * WP / 512 chunks of two doubles each, chunk idx = tid + 256 * i at
// row idx / (WP / 2), column 2 * (idx % (WP / 2)).
template <int ROWS, int WP>
struct TileRegsD {
  static_assert(ROWS * WP % (2 * THREADS) == 0, "whole chunks per thread");
  static constexpr int N = ROWS * WP / (2 * THREADS);
  d2 r[N];
};

// Rows [0, rows) x columns [0, width) of `base` (row step ld); everything else of the tile is zero and nothing else is read.
// A chunk that the view holds whole is one 16-byte load when `vec`; a row's odd last element and every chunk of an operand
// that is not 16-byte aligned are 8-byte loads.
template <int ROWS, int WP>
__device__ __forceinline__ void load_rows(TileRegsD<ROWS, WP>& t, const double* __restrict__ base, long ld, long rows, int width, bool vec, int tid) {
  constexpr int CPR = WP / 2;
#pragma unroll
  for (int i = 0; i < TileRegsD<ROWS, WP>::N; ++i) {
    const int idx = tid + i * THREADS;
    const int row = idx / CPR, col = (idx % CPR) * 2;
    d2 v = {0.0, 0.0};
    if (row < rows && col < width) {
      const double* p = base + (long)row * ld + col;
      if (vec && col + 2 <= width) {
        v = *reinterpret_cast<const d2*>(p);
      } else {
        v[0] = p[0];
        if (col + 1 < width) v[1] = p[1];
      }
    }
    t.r[i] = v;
  }
}

template <int ROWS, int WP, int STRIDE>
__device__ __forceinline__ void store_rows(const TileRegsD<ROWS, WP>& t, double* __restrict__ lds, int tid) {
  static_assert(STRIDE % 2 == 0, "16-byte LDS writes");
  constexpr int CPR = WP / 2;
#pragma unroll
  for (int i = 0; i < TileRegsD<ROWS, WP>::N; ++i) {
    const int idx = tid + i * THREADS;
    *reinterpret_cast<d2*>(&lds[(idx / CPR) * STRIDE + (idx % CPR) * 2]) = t.r[i];
  }
}

// ---- the products, on v_mfma_f64_16x16x4_f64 ----------------------------------------------------------------------------
// Lane (c, g) = (lane & 15, lane >> 4) gives A[row c][k = g] and B[k = g][col c] and receives D[row g + 4 r][col c] in
// element r.  The k step is outside and the column block inside: an accumulator sees its additions in k order.

// "NT": acc[nb] += A_rows * tile[16 nb .. 16 nb + 15][0, W)^T — 16 rows from registers against the tile's TJ rows.
template <int W, int STRIDE, int TJ>
__device__ __forceinline__ void mma_nt(const double (&a)[W / 4], const double* tile, int c, int g, d4 (&acc)[TJ / 16]) {
  const double* const p = tile + c * STRIDE + g;
#pragma unroll
  for (int kk = 0; kk < W / 4; ++kk) {
#pragma unroll
    for (int nb = 0; nb < TJ / 16; ++nb) acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], p[nb * 16 * STRIDE + 4 * kk], acc[nb], 0, 0, 0);
  }
}

// "NN": acc[nb] += rows * tile[0, TJ)[16 nb .. 16 nb + 15] — the wave's own [16][TJ] LDS rows (row step RS) against the
// tile's columns [0, WP).
template <int WP, int STRIDE, int RS, int TJ>
__device__ __forceinline__ void mma_nn(const double* rows, const double* tile, int c, int g, d4 (&acc)[WP / 16]) {
  const double* const pe = rows + c * RS + g;
  const double* const p = tile + g * STRIDE + c;
#pragma unroll
  for (int jj = 0; jj < TJ / 4; ++jj) {
    const double e = pe[4 * jj];
#pragma unroll
    for (int nb = 0; nb < WP / 16; ++nb) acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(e, p[4 * jj * STRIDE + nb * 16], acc[nb], 0, 0, 0);
  }
}

}  // namespace attention
}  // namespace eg
