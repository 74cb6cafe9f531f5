// What the attention kernels share (attention_f32.hip, attention_grad_f32.hip).  Device side: an operand as a kernel
// argument and the block's item of it, a [64][WP] tile in the registers of a block's 256 threads on its way from global
// memory to LDS, the three MFMA loops over such tiles, and the wave-private synchronisation between a wave's
// accumulator-layout writes to its own LDS rows and its A-operand reads of them.  Host side: the one launcher — the cut into
// launches, the padded K x padded D dispatch, the dynamic-LDS attribute.
#pragma once

#include <type_traits>

#include "../eg_internal.hpp"
#include "gemm_f32_mfma.hpp"   // f32x4
#include "attention_plan.hpp"  // THREADS, View, Cut
#include "item_launch.hpp"     // Items, block_item, item_base, for_each_launch

namespace eg {
namespace attention {

using eg::gemm::f32x4;

constexpr int ES = 64 + 4;   // floats per row of a wave's own [16][64] LDS rows

// ---- kernel arguments -------------------------------------------------------------------------------------------------
// One operand: item (0, 0), its view, and whether the plan gives it 16-byte accesses.
template <class T>
struct Arg {
  T* p;
  View v;
  int vec;
};
using In = Arg<const float>;
using Out = Arg<float>;

// The items of a launch, a block's item and the loop over a cut's launches are the item grid's (item_launch.hpp).
using eg::Items;
using eg::BlockItem;
using eg::block_item;
using eg::item_base;
using eg::for_each_launch;

template <class T>
__device__ __forceinline__ T* item_base(const Arg<T>& x, unsigned outer, unsigned inner) {
  return item_base(x.p, x.v, outer, inner);
}

// ---- tiles ------------------------------------------------------------------------------------------------------------
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

// ---- the products, on v_mfma_f32_16x16x4_f32 ----------------------------------------------------------------------------
// Lane (c, g) = (lane & 15, lane >> 4) gives A[row c][k = g] and B[k = g][col c] and receives D[row 4 g + r][col c] in
// element r.  Each loop has the k step outside and the column block inside: an accumulator sees its additions in k order.
// Each helper forms the lane's base address once and steps from it by compile-time constants, so that the steps land in
// the offset field of the LDS reads and no read needs an address register of its own.  mma_nt and mma_nn carry the forward's
// two products; the backward's kernels keep their seven product loops written out, because through these helpers the compiler
// allocates their registers differently and eg_attention_grad measured 2.5 % slower (profiles/attention_views.txt).

// Rows 16 w .. 16 w + 15 of a [64][STRIDE] LDS tile of width W as the A operands of every k step.
template <int W, int STRIDE>
__device__ __forceinline__ void read_a_rows(const float* tile, int w, int c, int g, float (&regs)[W / 4]) {
  const float* const p = tile + (w * 16 + c) * STRIDE + g;
#pragma unroll
  for (int kk = 0; kk < W / 4; ++kk) regs[kk] = p[4 * kk];
}

// "NT": acc[nb] += A_rows * tile[16 nb .. 16 nb + 15][0, W)^T — 16 rows from registers against the tile's 64 rows.
template <int W, int STRIDE>
__device__ __forceinline__ void mma_nt(const float (&a)[W / 4], const float* tile, int c, int g, f32x4 (&acc)[4]) {
  const float* const p = tile + c * STRIDE + g;
#pragma unroll
  for (int kk = 0; kk < W / 4; ++kk) {
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], p[nb * 16 * STRIDE + 4 * kk], acc[nb], 0, 0, 0);
  }
}

// "NN": acc[nb] += rows * tile[0, 64)[16 nb .. 16 nb + 15] — the wave's own [16][64] LDS rows (row step RS) against the
// tile's columns [0, WP).
template <int WP, int STRIDE, int RS>
__device__ __forceinline__ void mma_nn(const float* rows, const float* tile, int c, int g, f32x4 (&acc)[WP / 16]) {
  const float* const pe = rows + c * RS + g;
  const float* const p = tile + g * STRIDE + c;
#pragma unroll
  for (int jj = 0; jj < 64 / 4; ++jj) {
    const float e = pe[4 * jj];
#pragma unroll
    for (int nb = 0; nb < WP / 16; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(e, p[4 * jj * STRIDE + nb * 16], acc[nb], 0, 0, 0);
  }
}

// ---- the launcher -------------------------------------------------------------------------------------------------------
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// f(KP, DP) with the padded head dimensions as integral constants: the 9 instantiations of a kernel.
template <class F>
int dispatch_heads(int kp, int dp, F&& f) {
  auto with_kp = [&](auto KP) {
    switch (dp) {
      case 32: return f(KP, std::integral_constant<int, 32>());
      case 64: return f(KP, std::integral_constant<int, 64>());
      default: return f(KP, std::integral_constant<int, 128>());
    }
  };
  switch (kp) {
    case 32: return with_kp(std::integral_constant<int, 32>());
    case 64: return with_kp(std::integral_constant<int, 64>());
    default: return with_kp(std::integral_constant<int, 128>());
  }
}

// The dynamic-LDS limit of KERNELS (bytes[i] for the i-th), once per device and set of kernels.  The attribute belongs to
// the device that is current (set_device has made it the context's); a device index outside the table sets it every time.
template <auto... KERNELS>
int dynamic_lds_once(eg_ctx* ctx, const long (&bytes)[sizeof...(KERNELS)]) {
  constexpr int MAX_DEVICES = 64;
  static bool attr_set[MAX_DEVICES] = {};
  const bool known = ctx->device >= 0 && ctx->device < MAX_DEVICES;
  if (known && attr_set[ctx->device]) return EG_OK;
  const void* const kernels[] = {reinterpret_cast<const void*>(KERNELS)...};
  for (size_t i = 0; i < sizeof...(KERNELS); ++i)
    EG_HIP_CHECK(hipFuncSetAttribute(kernels[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes[i]));
  if (known) attr_set[ctx->device] = true;
  return EG_OK;
}

}  // namespace attention
}  // namespace eg
