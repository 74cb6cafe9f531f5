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

// ---- the additive score bias (eg_attention_bias, eg_attention_bias_grad) ------------------------------------------------
// The bias of a wave's 16 x 64 tile of scores, in the layout the accumulators have: x[nb][r] belongs to s[nb][r].  It goes
// from global memory straight into these 16 registers of a lane, one tile ahead of its use: no LDS, no barrier.
struct BiasTile {
  f32x4 x[4];
};

// Forward and dQ kernels: lane (c, g) holds rows 4 g + r of the wave's 16 query rows and keys 16 nb + c of the tile; `p` is
// the lane's element (nb, r) = (0, 0), `rows` and `keys` what the problem has left from there (either may be <= 0).  A wave's
// load (one nb, one r) reads four row segments of 64 bytes.  ldb == 0 makes the four rows one.  Rows i >= I and keys j >= J
// are 0 and not read.
__device__ __forceinline__ void load_bias(BiasTile& t, const float* __restrict__ p, long ldb, long rows, long keys) {
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
    for (int r = 0; r < 4; ++r) t.x[nb][r] = (r < rows && 16 * nb < keys) ? p[r * ldb + 16 * nb] : 0.f;
  }
}

// dK/dV kernel, the transpose: lane (c, g) holds keys 4 g + r of the wave's 16 keys and query rows 16 nb + c of the tile, so
// a lane's four r are four consecutive keys of one query row: one 16-byte load when `vec` (the plan's vec_b: every row of
// every item starts 16-byte aligned, and a lane's first key is a multiple of 4) and the four keys are all inside the
// problem, element loads otherwise.  `p` is the lane's element (0, 0), `rows` and `keys` what is left from there.
__device__ __forceinline__ void load_bias_t(BiasTile& t, const float* __restrict__ p, long ldb, long rows, long keys, bool vec) {
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (16 * nb < rows && keys > 0) {
      const float* const q = p + 16 * nb * ldb;
      if (vec && keys >= 4) {
        v = *reinterpret_cast<const f32x4*>(q);
      } else {
        v[0] = q[0];
        if (keys > 1) v[1] = q[1];
        if (keys > 2) v[2] = q[2];
        if (keys > 3) v[3] = q[3];
      }
    }
    t.x[nb] = v;
  }
}

// ---- what the CAUSAL kernels visit (eg_attention_causal, eg_attention_causal_grad; attention_plan.hpp has the bounds) ------------
// Each is the unmasked kernel's value without CAUSAL, and `a` has an offset only with it.
// The block's item and row tile: the forward and dQ blocks of a causal item take the row tiles in descending order, because a
// late row tile walks up to tiles times the key tiles of the first and the longest loops should be issued first.
template <bool CAUSAL>
__device__ __forceinline__ BlockItem causal_block_item(const Items& it) {
  BlockItem b = block_item(it);
#ifndef EG_ATTENTION_CAUSAL_NATURAL_ORDER   // the other order, for tools/bench_attention_causal.py
  if constexpr (CAUSAL) b.tile = it.tiles - 1 - b.tile;
#endif
  return b;
}

// Forward and dQ: the keys that are loaded, and the key tiles of the loop of the block of rows [i0, i0 + 64).
template <bool CAUSAL, class Args>
__device__ __forceinline__ long causal_loaded_keys(const Args& a) {
  if constexpr (CAUSAL)
    return causal_visible_keys(a.I, a.offset, a.J);
  else
    return a.J;
}
template <bool CAUSAL, class Args>
__device__ __forceinline__ long causal_loop_tiles(const Args& a, long i0, long keys) {
  if constexpr (CAUSAL)
    return causal_key_tiles(i0, a.offset, keys);
  else
    return (a.J + TILE_J - 1) / TILE_J;
}

// dK/dV: the first row tile of the loop of the block of keys [j0, j0 + 64); nt, an empty loop, when no row sees them.
template <bool CAUSAL, class Args>
__device__ __forceinline__ long causal_loop_start(const Args& a, long j0, long nt) {
  if constexpr (CAUSAL)
    return j0 < causal_visible_keys(a.I, a.offset, a.J) ? causal_first_row_tile(j0, a.offset) : nt;
  else
    return 0;
}

// What one wave wrote to its own LDS rows becomes visible to its other lanes: no block barrier.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- a row maximum over a DPP row (the kernels with a running maximum: attention_stable_f32.hip, attention_split_f32.hip) ----
// The value of the lane N places on in its DPP row of 16, wrapping round (row_ror:N); through the LDS crossbar where the
// compiler has no DPP builtin.
template <int N>
__device__ __forceinline__ float row_rotate(float v) {
#if __has_builtin(__builtin_amdgcn_update_dpp)
  const int b = __builtin_bit_cast(int, v);
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(b, b, 0x120 + N, 0xF, 0xF, false));
#else
  return __shfl_xor(v, N);   // another partner, the same maximum after the four steps
#endif
}

// The maximum over the 16 lanes of a DPP row, in every one of them.
__device__ __forceinline__ float row_max16(float v) {
  v = fmaxf(v, row_rotate<8>(v));
  v = fmaxf(v, row_rotate<4>(v));
  v = fmaxf(v, row_rotate<2>(v));
  v = fmaxf(v, row_rotate<1>(v));
  return v;
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
