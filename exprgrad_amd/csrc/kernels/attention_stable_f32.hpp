// The kernel of the fused attention forward with a running row maximum and its launch, as a template: attention_stable_f32.hip
// has the formulas, the special values and the 18 instantiations of eg_attention_stable, attention_causal_f32.hip the 18 of
// eg_attention_causal (CAUSAL), a translation unit of its own so that the two sets compile side by side.
#pragma once

#include "attention_tile.hpp"   // kernel operands, tiles, the MFMA loops, the launcher

#include <cmath>

namespace eg {
namespace attention {

struct StableArgs {
  In q, k, v;
  Out o;
  Out st;      // Stats: row 0 the maxima, row 1 (st.v.ld floats on) the sums; p may be NULL
  long I, J;
  int K, D;
  float scale;
  int accumulate;
  Items items;
};

struct StableBiasArgs : StableArgs {
  In b;
};

// The CAUSAL kernels take these with or without BIAS: key j is visible to row i iff j <= i + offset, 0 <= offset <= J.
struct StableCausalArgs : StableBiasArgs {
  long offset;
};

template <bool BIAS, bool CAUSAL>
using StableArgsOf = std::conditional_t<CAUSAL, StableCausalArgs, std::conditional_t<BIAS, StableBiasArgs, StableArgs>>;

// One launch of the CAUSAL kernel (attention_causal_f32.hip), BIAS where args.b.p is not NULL.
int launch_stable_causal(eg_ctx* ctx, unsigned grid, const Plan& p, const StableCausalArgs& args);

}  // namespace attention
}  // namespace eg

namespace {

using eg::gemm::f32x4;
using namespace eg::attention;

// CAUSAL: which key tiles the block visits and how the diagonal is cut (attention_plan.hpp has the bounds).  A compile-time
// flag: every line of it is under `if constexpr`, and the instantiations without it are the kernels they were.
//   - the block's row tile is tiles - 1 - b.tile: the row tiles with the most key tiles are issued first;
//   - the loop, and with it the prefetch of K, V and the bias, stops at causal_key_tiles; no key at or beyond the item's
//     causal_visible_keys is loaded (its rows of the K and V tiles are zeros);
//   - on a cut tile (causal_tile_cut) the select that turns keys j >= J into -Inf also takes j > i + offset, from the lane's own
//     row i0 + 16 w + 4 g + r and key j0 + 16 nb + c: lim[r] is the lane's last visible key of the tile, 63 or J - 1 - j0 on an
//     interior tile, where the select is the unmasked kernel's;
//   - a wave whose 16 rows all lie above a cut tile skips both products and the softmax: every term would be expf(-Inf) = 0, the
//     maximum would not move (key 0 is visible to every row, so it is finite after tile 0) and E * V would add zeros.  The skip
//     is wave-uniform and comes after the two block barriers.
template <int KP, int DP, bool BIAS, bool CAUSAL = false>
__global__ __launch_bounds__(THREADS) void attention_stable_f32_kernel(StableArgsOf<BIAS, CAUSAL> a) {
  constexpr int KS = KP + 4, VS = DP + 16;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const Ks = lds;                      // [64][KS]; the Q tile first
  float* const Vs = Ks + TILE_J * KS;         // [64][VS]
  float* const Es = Vs + TILE_J * VS;         // [4][16][ES]

  const BlockItem b = causal_block_item<CAUSAL>(a.items);
  const long i0 = (long)b.tile * TILE_I;
  const long ldq = a.q.v.ld, ldk = a.k.v.ld, ldv = a.v.v.ld;
  const float* const Q = item_base(a.q, b.outer, b.inner) + i0 * ldq;
  const float* const Kk = item_base(a.k, b.outer, b.inner);
  const float* const V = item_base(a.v, b.outer, b.inner);
  float* const O = item_base(a.o, b.outer, b.inner);

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  float* const Ew = Es + w * 16 * ES;

  // Q rows of the wave as A operands of every k step, for the whole loop
  float q[KP / 4];
  {
    TileRegs<KP> tq;
    load_rows<KP>(tq, Q, ldq, a.I - i0, a.K, a.q.vec != 0, tid);
    store_rows<KP, KS>(tq, Ks, tid);
    __syncthreads();
    read_a_rows<KP, KS>(Ks, w, c, g, q);
  }

  f32x4 o[DP / 16];
#pragma unroll
  for (int nb = 0; nb < DP / 16; ++nb) o[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
  float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};   // the same value in the 16 lanes of a row

  TileRegs<KP> tk;
  TileRegs<DP> tv;
  // the lane's bias: rows 4 g + r of the wave's, keys c + 16 nb of a tile; `next` is a tile ahead
  [[maybe_unused]] BiasTile bias, bias_next;
  [[maybe_unused]] const long bias_rows = a.I - i0 - w * 16 - 4 * g;
  [[maybe_unused]] long ldb = 0;
  [[maybe_unused]] const float* Bl = nullptr;
  if constexpr (BIAS) {
    ldb = a.b.v.ld;
    Bl = item_base(a.b, b.outer, b.inner) + (i0 + w * 16 + 4 * g) * ldb + c;
  }
  // the keys that are loaded, and the tiles that hold those the block's rows see
  const long keys = causal_loaded_keys<CAUSAL>(a);
  const long nt = causal_loop_tiles<CAUSAL>(a, i0, keys);
  if (nt > 0) {
    load_rows<KP>(tk, Kk, ldk, keys, a.K, a.k.vec != 0, tid);
    load_rows<DP>(tv, V, ldv, keys, a.D, a.v.vec != 0, tid);
    if constexpr (BIAS) load_bias(bias_next, Bl, ldb, bias_rows, keys - c);
  }
  for (long t = 0; t < nt; ++t) {
    const long j0 = t * TILE_J;
    __syncthreads();   // every wave is done with the tiles in LDS (the first time: with the Q tile)
    store_rows<KP, KS>(tk, Ks, tid);
    store_rows<DP, VS>(tv, Vs, tid);
    __syncthreads();
    if constexpr (BIAS) bias = bias_next;
    if (t + 1 < nt) {   // in flight during this tile's MFMAs
      load_rows<KP>(tk, Kk + (j0 + TILE_J) * ldk, ldk, keys - j0 - TILE_J, a.K, a.k.vec != 0, tid);
      load_rows<DP>(tv, V + (j0 + TILE_J) * ldv, ldv, keys - j0 - TILE_J, a.D, a.v.vec != 0, tid);
      if constexpr (BIAS) load_bias(bias_next, Bl + j0 + TILE_J, ldb, bias_rows, keys - j0 - TILE_J - c);
    }

    // CAUSAL: the lane's last visible key of this tile for each of its four rows, relative to j0
    [[maybe_unused]] int lim[4];
    if constexpr (CAUSAL) {
      const long left = a.J - 1 - j0;   // >= 0: j0 < keys <= J
      const int in_problem = left < TILE_J - 1 ? (int)left : TILE_J - 1;
      // row i0 against key j0: above -64 on a visited tile and below 63 on a cut one
      const int d0 = causal_tile_cut(i0, j0, a.offset, a.J) ? (int)(i0 + a.offset - j0) : 2 * TILE_J;
      if (d0 + __builtin_amdgcn_readfirstlane(w) * 16 + 15 < 0) continue;   // the wave's last row does not see key j0
#pragma unroll
      for (int r = 0; r < 4; ++r) lim[r] = min(in_problem, d0 + w * 16 + 4 * g + r);
    }

    f32x4 s[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) s[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    mma_nt<KP, KS>(q, Ks, c, g, s);

    // the scores, in place; a key outside the problem is -Inf by a select, whatever its score: its term is exactly 0
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      [[maybe_unused]] const bool live = j0 + nb * 16 + c < a.J;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x = s[nb][r] * a.scale;
        if constexpr (BIAS) x = x + bias.x[nb][r];
        if constexpr (CAUSAL)
          s[nb][r] = nb * 16 + c <= lim[r] ? x : -INFINITY;
        else
          s[nb][r] = live ? x : -INFINITY;
      }
    }

    // the running maximum and the subtrahend of each of the lane's four rows
    float m_new[4], sub[4];
    bool raised = false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float tile_max = row_max16(fmaxf(fmaxf(s[0][r], s[1][r]), fmaxf(s[2][r], s[3][r])));
      m_new[r] = fmaxf(m[r], tile_max);   // never NaN: m starts at -Inf and fmaxf drops a NaN operand
      sub[r] = m_new[r] == -INFINITY ? 0.f : m_new[r];
      raised |= m_new[r] > m[r];
    }
    if (__any(raised)) {   // wave-uniform; a row that did not move would be multiplied by 1.0f
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float alpha = expf(m[r] - sub[r]);
        sum[r] *= alpha;
#pragma unroll
        for (int nb = 0; nb < DP / 16; ++nb) o[nb][r] *= alpha;
        m[r] = m_new[r];   // equal to m[r] wherever nothing was raised
      }
    }

#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = expf(s[nb][r] - sub[r]);
        sum[r] += e;
        Ew[(4 * g + r) * ES + nb * 16 + c] = e;
      }
    }
    wave_sync();

    mma_nn<DP, VS, ES>(Ew, Vs, c, g, o);
    wave_sync();   // the wave's E rows are read before its next tile overwrites them
  }

  // Row sums: the 16 lanes of a group hold the columns = c (mod 16) of rows 4g + r.  L <= J: no overflow to look for.
  const bool empty = a.J == 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float t = sum[r];
    t += __shfl_xor(t, 1);
    t += __shfl_xor(t, 2);
    t += __shfl_xor(t, 4);
    t += __shfl_xor(t, 8);
    sum[r] = t;
  }
  if (a.st.p) {
    // from the lane that holds column 0 of its group's rows; without keys the maximum is -Inf and the sum 0
    float* const St = item_base(a.st, b.outer, b.inner);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long row = i0 + w * 16 + 4 * g + r;
      if (c == 0 && row < a.I) {
        St[row] = m[r];
        St[a.st.v.ld + row] = sum[r];
      }
    }
  }
  if (empty && a.accumulate) return;   // an empty sum adds nothing to O
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long row = i0 + w * 16 + 4 * g + r;
    if (row >= a.I) continue;
#pragma unroll
    for (int nb = 0; nb < DP / 16; ++nb) {
      const int col = nb * 16 + c;
      if (col >= a.D) continue;
      const float v = empty ? 0.f : o[nb][r] / sum[r];
      float* const p = O + row * a.o.v.ld + col;
      *p = a.accumulate ? *p + v : v;
    }
  }
}

template <auto KERNEL, class Args, int KP, int DP>
int launch(eg_ctx* ctx, unsigned grid, const Plan& p, const Args& args) {
  const int rc = dynamic_lds_once<KERNEL>(ctx, {lds_bytes_for(KP, DP)});
  if (rc) return rc;
  hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(p.block), (size_t)p.lds_bytes, ctx->stream, args);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}

}  // namespace
