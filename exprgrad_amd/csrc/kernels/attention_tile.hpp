// Device helpers shared by the attention kernels (attention_f32.hip, attention_grad_f32.hip): a [64][WP] tile in the
// registers of a block's 256 threads on its way from global memory to LDS, and the wave-private synchronisation between a
// wave's accumulator-layout writes to its own LDS rows and its A-operand reads of them.
#pragma once

#include "gemm_f32_mfma.hpp"   // f32x4
#include "attention_plan.hpp"  // THREADS

namespace eg {
namespace attention {

using eg::gemm::f32x4;

// A [64][WP] tile in the registers of 256 threads: WP / 16 chunks of four floats each, chunk idx = tid + 256 * i at row
// idx / (WP / 4), column 4 * (idx % (WP / 4)).
template <int WP>
struct TileRegs {
  f32x4 r[WP / 16];
};

// Rows [0, rows) x columns [0, width) of `base` (row step ld); everything else of the tile is zero and nothing else is read.
// A chunk that the view holds whole is one 16-byte load when `vec`; a row's ragged last chunk and every chunk of an operand
// that is not 16-byte aligned are element loads.
template <int WP>
__device__ __forceinline__ void load_rows(TileRegs<WP>& t, const float* __restrict__ base, long ld, long rows, int width, bool vec, int tid) {
  constexpr int CPR = WP / 4;
#pragma unroll
  for (int i = 0; i < WP / 16; ++i) {
    const int idx = tid + i * THREADS;
    const int row = idx / CPR, col = (idx % CPR) * 4;
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
    t.r[i] = v;
  }
}

template <int WP, int STRIDE>
__device__ __forceinline__ void store_rows(const TileRegs<WP>& t, float* __restrict__ lds, int tid) {
  constexpr int CPR = WP / 4;
#pragma unroll
  for (int i = 0; i < WP / 16; ++i) {
    const int idx = tid + i * THREADS;
    *reinterpret_cast<f32x4*>(&lds[(idx / CPR) * STRIDE + (idx % CPR) * 4]) = t.r[i];
  }
}

// What one wave wrote to its own LDS rows becomes visible to its other lanes: no block barrier.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace attention
}  // namespace eg
