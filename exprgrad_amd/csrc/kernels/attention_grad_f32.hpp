// The two kernels of the fused float32 attention backward and their launch, as templates: attention_grad_f32.hip has the
// formulas, the LDS rows and the instantiations of eg_attention_grad and eg_attention_bias_grad, attention_grad_stable_f32.hip
// those of eg_attention_stable_grad (STABLE), a translation unit of its own so that the two sets compile side by side, and
// attention_grad_causal_f32.hip and attention_grad_causal_bias_f32.hip those of eg_attention_causal_grad (STABLE and CAUSAL).
#pragma once

#include "attention_tile.hpp"        // kernel operands, tiles, the MFMA loops, the launcher
#include "attention_grad_tile.hpp"   // O parts, delta, 1 / L, the accumulators' way out

#include <cmath>

namespace eg {
namespace attention {

struct GradArgs {
  In q, k, v, o, s, dout;
  Out dq, dk, dv;
  long I, J;
  int K, D;
  float scale;
  int acc_dq, acc_dk, acc_dv;          // that output is added to
  int put_dk, put_dv;                  // the dK/dV kernel stores that output
  Items items;
};

// eg_attention_bias_grad: the forward's score bias.  Arguments of their own for the BIAS kernels, so that the others take the
// arguments they took.
struct GradBiasArgs : GradArgs {
  In b;
};
// The STABLE kernels (eg_attention_stable_grad) take GradBiasArgs with or without BIAS: `s` is the forward's Stats, row 0
// the maxima and row 1, s.v.ld floats on, the sums.
// The CAUSAL kernels (eg_attention_causal_grad; STABLE too) take these with or without BIAS: key j is visible to row i iff
// j <= i + offset, 0 <= offset <= J.
struct GradCausalArgs : GradBiasArgs {
  long offset;
};
template <bool BIAS, bool STABLE, bool CAUSAL = false>
using ArgsOf = std::conditional_t<CAUSAL, GradCausalArgs, std::conditional_t<BIAS || STABLE, GradBiasArgs, GradArgs>>;

// One launch of the STABLE dQ kernel or dK/dV kernel (attention_grad_stable_f32.hip), BIAS where args.b.p is not NULL.
int launch_grad_stable(eg_ctx* ctx, bool dkv, unsigned grid, const GradPlan& p, const GradBiasArgs& args);
// The same of the CAUSAL kernels: without a bias (attention_grad_causal_f32.hip) and with one (attention_grad_causal_bias_f32.hip).
int launch_grad_causal(eg_ctx* ctx, bool dkv, unsigned grid, const GradPlan& p, const GradCausalArgs& args);
int launch_grad_causal_bias(eg_ctx* ctx, bool dkv, unsigned grid, const GradPlan& p, const GradCausalArgs& args);

}  // namespace attention
}  // namespace eg

namespace {

using eg::gemm::f32x4;
using namespace eg::attention;

constexpr int TILE = 64;

// BIAS (both kernels): p_ij = expf(scale * s_ij + bias_ij) / L_i, the bias an operand with a view of its own whose ld and
// strides may each be 0; a compile-time flag, and the instantiations without it are the kernels they were.  One
// multiplication, one addition, not fused: what the forward computes, so that L is the sum of these very terms.  The dQ kernel
// holds the wave's 16 x 64 bias tile in accumulator layout, as the forward does; the dK/dV kernel holds its transpose, where
// a lane's four elements are four consecutive keys of one query row: one 16-byte load per nb when the plan's vec_b allows it.
// Both load a tile ahead, with the other operands' next tiles, straight into registers: no LDS.  No gradient of the bias.
// STABLE (both kernels): p_ij = expf(x_ij - m_i) / L_i with m and L from eg_attention_stable's Stats: the rows' small LDS array
// holds the maximum as a third column and the exponent gets one subtraction.  Again a compile-time flag: every line of it is
// under `if constexpr`, and the instantiations without it are the kernels they were.
// CAUSAL (both kernels, with STABLE): which tiles of the other axis a block visits, and the cut of the diagonal; the third
// compile-time flag of the same kind (attention_plan.hpp has the bounds).  A masked pair's x is -Inf by a select where the bias
// is added, so p and dS are the zeros that a Bias of -Inf gives, and the tiles that are not visited would have added zeros.
//   dQ     the row tile is tiles - 1 - b.tile (the longest loops first); the loop over key tiles and its prefetch stop at
//          causal_key_tiles, and no key at or beyond causal_visible_keys is loaded; on a cut tile lim[r] is the last visible key
//          of the lane's row r, relative to j0; a wave whose 16 rows all lie above a cut tile skips its three products;
//   dK/dV  the loop over row tiles and its prefetch start at causal_first_row_tile; the layout is the transpose, a lane's four
//          r are four consecutive keys of one row, so on a cut tile first[r] is the first row that sees the lane's key r,
//          relative to i0.
template <int KP, int DP, bool BIAS, bool STABLE = false, bool CAUSAL = false>
__global__ __launch_bounds__(THREADS) void attention_dq_kernel(ArgsOf<BIAS, STABLE, CAUSAL> a) {
  static_assert(STABLE || !CAUSAL, "the causal kernels read the stable forward's Stats");
  constexpr int KS = KP + GRAD_PAD_BOTH, VS = DP + GRAD_PAD_NT, SW = STABLE ? 3 : 2;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const Ks = lds;                  // [64][KS]: the Q tile first, dQ last
  float* const Vs = Ks + TILE * KS;       // [64][VS]: the dO tile first
  float* const Es = Vs + TILE * VS;       // [4][16][ES]
  float* const St = Es + 4 * 16 * ES;     // [64][SW]: 1 / L, delta, and under STABLE the maximum

  const BlockItem b = causal_block_item<CAUSAL>(a.items);
  const long i0 = (long)b.tile * TILE;
  const long rows = a.I - i0;
  const long read_rows = a.J > 0 ? rows : 0;   // without keys nothing is read: dQ is zeros
  const long ldk = a.k.v.ld, ldv = a.v.v.ld;
  const float* const Q = item_base(a.q, b.outer, b.inner) + i0 * a.q.v.ld;
  const float* const dO = item_base(a.dout, b.outer, b.inner) + i0 * a.dout.v.ld;
  const float* const O = item_base(a.o, b.outer, b.inner) + i0 * a.o.v.ld;
  const float* const M = item_base(a.s, b.outer, b.inner) + i0;   // STABLE: the maxima, the sums a row on
  const float* const S = STABLE ? M + a.s.v.ld : M;
  const float* const Kk = item_base(a.k, b.outer, b.inner);
  const float* const V = item_base(a.v, b.outer, b.inner);
  float* const dQ = item_base(a.dq, b.outer, b.inner) + i0 * a.dq.v.ld;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  float* const Ew = Es + w * 16 * ES;

  TileRegs<KP> tk;
  TileRegs<DP> tv;
  // the wave's Q rows and dO rows as A operands for the whole loop; 1 / L and delta of its accumulator rows
  float q[KP / 4], dout[DP / 4], inv[4], delta[4];
  [[maybe_unused]] float mx[4];
  {
    OPart<DP> po;
    load_rows<KP>(tk, Q, a.q.v.ld, read_rows, a.K, a.q.vec != 0, tid);
    load_rows<DP>(tv, dO, a.dout.v.ld, read_rows, a.D, a.dout.vec != 0, tid);
    load_o_part<DP>(po, O, a.o.v.ld, read_rows, a.D, a.o.vec != 0, tid);
    const f32x4 sums = load_sums(S, read_rows, a.s.vec != 0, tid);
    store_rows<KP, KS>(tk, Ks, tid);
    store_rows<DP, VS>(tv, Vs, tid);
    store_inverse_sums<SW>(sums, St, rows, tid);
    if constexpr (STABLE) store_maxima<SW>(load_sums(M, read_rows, a.s.vec != 0, tid), St, tid);
    __syncthreads();
    read_a_rows<KP, KS>(Ks, w, c, g, q);
    read_a_rows<DP, VS>(Vs, w, c, g, dout);
    const float d = row_delta<DP>(Vs, VS, po, tid);
    if ((tid & 3) == 0) St[SW * (tid >> 2) + 1] = d;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      inv[r] = St[SW * (w * 16 + 4 * g + r)];
      delta[r] = St[SW * (w * 16 + 4 * g + r) + 1];
      if constexpr (STABLE) mx[r] = St[SW * (w * 16 + 4 * g + r) + 2];
    }
  }

  f32x4 dq[KP / 16];
#pragma unroll
  for (int nb = 0; nb < KP / 16; ++nb) dq[nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the lane's bias: rows 4 g + r of the wave's, keys c + 16 nb of a tile; `next` is a tile ahead
  [[maybe_unused]] BiasTile bias, bias_next;
  [[maybe_unused]] const long bias_rows = rows - w * 16 - 4 * g;
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
    const long j0 = t * TILE;
    __syncthreads();   // every wave is done with the tiles in LDS (the first time: with the Q and dO tiles)
    store_rows<KP, KS>(tk, Ks, tid);
    store_rows<DP, VS>(tv, Vs, tid);
    __syncthreads();
    if constexpr (BIAS) bias = bias_next;
    if (t + 1 < nt) {   // in flight during this tile's MFMAs
      load_rows<KP>(tk, Kk + (j0 + TILE) * ldk, ldk, keys - j0 - TILE, a.K, a.k.vec != 0, tid);
      load_rows<DP>(tv, V + (j0 + TILE) * ldv, ldv, keys - j0 - TILE, a.D, a.v.vec != 0, tid);
      if constexpr (BIAS) load_bias(bias_next, Bl + j0 + TILE, ldb, bias_rows, keys - j0 - TILE - c);
    }

    [[maybe_unused]] int lim[4];
    if constexpr (CAUSAL) {
      // row i0 against key j0: above -64 on a visited tile and below 63 on a cut one
      const int d0 = causal_tile_cut(i0, j0, a.offset, a.J) ? (int)(i0 + a.offset - j0) : 2 * TILE;
      if (d0 + __builtin_amdgcn_readfirstlane(w) * 16 + 15 < 0) continue;   // the wave's last row does not see key j0
#pragma unroll
      for (int r = 0; r < 4; ++r) lim[r] = d0 + w * 16 + 4 * g + r;
    }

    f32x4 s[4], dp[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) s[nb] = dp[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KP / 4; ++kk) {
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) s[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(q[kk], Ks[(nb * 16 + c) * KS + 4 * kk + g], s[nb], 0, 0, 0);
    }
#pragma unroll
    for (int dd = 0; dd < DP / 4; ++dd) {
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) dp[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(dout[dd], Vs[(nb * 16 + c) * VS + 4 * dd + g], dp[nb], 0, 0, 0);
    }

#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      const bool live = j0 + nb * 16 + c < a.J;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x = s[nb][r] * a.scale;
        if constexpr (BIAS) x = x + bias.x[nb][r];
        if constexpr (CAUSAL) x = nb * 16 + c <= lim[r] ? x : -INFINITY;
        if constexpr (STABLE) x = x - mx[r];
        const float p = expf(x) * inv[r];
        const float ds = (a.scale * p) * (dp[nb][r] - delta[r]);
        Ew[(4 * g + r) * ES + nb * 16 + c] = live ? ds : 0.f;   // a select: a key outside the problem adds exactly 0
      }
    }
    wave_sync();

#pragma unroll
    for (int jj = 0; jj < TILE / 4; ++jj) {
      const float e = Ew[c * ES + 4 * jj + g];
#pragma unroll
      for (int nb = 0; nb < KP / 16; ++nb) dq[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(e, Ks[(4 * jj + g) * KS + nb * 16 + c], dq[nb], 0, 0, 0);
    }
    wave_sync();   // the wave's rows are read before its next tile overwrites them
  }

  __syncthreads();   // every wave is done with the K tile
  stage_acc<KP, KS>(dq, Ks, w, c, g);
  __syncthreads();
  store_out<KP, KS>(Ks, dQ, a.dq.v.ld, rows, a.K, a.dq.vec != 0, a.acc_dq != 0, tid);
}

template <int KP, int DP, bool BIAS, bool STABLE = false, bool CAUSAL = false>
__global__ __launch_bounds__(THREADS) void attention_dkv_kernel(ArgsOf<BIAS, STABLE, CAUSAL> a) {
  static_assert(STABLE || !CAUSAL, "the causal kernels read the stable forward's Stats");
  constexpr int QS = KP + GRAD_PAD_BOTH, DS = DP + GRAD_PAD_BOTH, SW = STABLE ? 3 : 2;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const Qs = lds;                  // [64][QS]: the K tile first, dK last
  float* const Ds = Qs + TILE * QS;       // [64][DS]: the V tile first, dV last
  float* const Es = Ds + TILE * DS;       // [4][16][ES]
  float* const St = Es + 4 * 16 * ES;     // [64][SW]: 1 / L, delta and under STABLE the maximum of the query tile's rows

  const BlockItem b = block_item(a.items);
  const long j0 = (long)b.tile * TILE;
  const long keys = a.J - j0;
  const long read_keys = a.I > 0 ? keys : 0;   // without query rows nothing is read: dK and dV are zeros
  const long ldq = a.q.v.ld, lddo = a.dout.v.ld, ldo = a.o.v.ld;
  const float* const Q = item_base(a.q, b.outer, b.inner);
  const float* const dO = item_base(a.dout, b.outer, b.inner);
  const float* const O = item_base(a.o, b.outer, b.inner);
  const float* const M = item_base(a.s, b.outer, b.inner);   // STABLE: the maxima, the sums a row on
  const float* const S = STABLE ? M + a.s.v.ld : M;
  const float* const Kk = item_base(a.k, b.outer, b.inner) + j0 * a.k.v.ld;
  const float* const V = item_base(a.v, b.outer, b.inner) + j0 * a.v.v.ld;
  float* const dK = item_base(a.dk, b.outer, b.inner) + j0 * a.dk.v.ld;
  float* const dV = item_base(a.dv, b.outer, b.inner) + j0 * a.dv.v.ld;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  float* const Ew = Es + w * 16 * ES;

  TileRegs<KP> tq;
  TileRegs<DP> td;
  OPart<DP> po;
  f32x4 sums = {1.f, 1.f, 1.f, 1.f};
  [[maybe_unused]] f32x4 maxs = {1.f, 1.f, 1.f, 1.f};
  // the wave's K rows and V rows as A operands for the whole loop
  float kreg[KP / 4], vreg[DP / 4];
  load_rows<KP>(tq, Kk, a.k.v.ld, read_keys, a.K, a.k.vec != 0, tid);
  load_rows<DP>(td, V, a.v.v.ld, read_keys, a.D, a.v.vec != 0, tid);
  store_rows<KP, QS>(tq, Qs, tid);
  store_rows<DP, DS>(td, Ds, tid);
  __syncthreads();
  read_a_rows<KP, QS>(Qs, w, c, g, kreg);
  read_a_rows<DP, DS>(Ds, w, c, g, vreg);

  f32x4 dk[KP / 16], dv[DP / 16];
#pragma unroll
  for (int nb = 0; nb < KP / 16; ++nb) dk[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int nb = 0; nb < DP / 16; ++nb) dv[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  bool klive[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) klive[r] = w * 16 + 4 * g + r < keys;

  // the lane's bias, transposed: keys 4 g + r of the wave's, query rows c + 16 nb of a tile; `next` is a tile ahead
  [[maybe_unused]] BiasTile bias, bias_next;
  [[maybe_unused]] const long bias_keys = keys - w * 16 - 4 * g;
  [[maybe_unused]] long ldb = 0;
  [[maybe_unused]] const float* Bl = nullptr;
  [[maybe_unused]] bool vec_b = false;
  if constexpr (BIAS) {
    ldb = a.b.v.ld, vec_b = a.b.vec != 0;
    Bl = item_base(a.b, b.outer, b.inner) + c * ldb + j0 + w * 16 + 4 * g;
  }
  const long nt = (a.I + TILE - 1) / TILE;
  const long t0 = causal_loop_start<CAUSAL>(a, j0, nt);   // the first row tile with a row that sees key j0
  if (t0 < nt) {
    const long f0 = t0 * TILE;
    load_rows<KP>(tq, Q + f0 * ldq, ldq, a.I - f0, a.K, a.q.vec != 0, tid);
    load_rows<DP>(td, dO + f0 * lddo, lddo, a.I - f0, a.D, a.dout.vec != 0, tid);
    load_o_part<DP>(po, O + f0 * ldo, ldo, a.I - f0, a.D, a.o.vec != 0, tid);
    sums = load_sums(S + f0, a.I - f0, a.s.vec != 0, tid);
    if constexpr (STABLE) maxs = load_sums(M + f0, a.I - f0, a.s.vec != 0, tid);
    if constexpr (BIAS) load_bias_t(bias_next, Bl + f0 * ldb, ldb, a.I - f0 - c, bias_keys, vec_b);
  }
  for (long t = t0; t < nt; ++t) {
    const long i0 = t * TILE;
    __syncthreads();   // every wave is done with the tiles in LDS (the first time: with the K and V tiles)
    store_rows<KP, QS>(tq, Qs, tid);
    store_rows<DP, DS>(td, Ds, tid);
    store_inverse_sums<SW>(sums, St, a.I - i0, tid);
    if constexpr (STABLE) store_maxima<SW>(maxs, St, tid);
    __syncthreads();
    {
      const float d = row_delta<DP>(Ds, DS, po, tid);
      if ((tid & 3) == 0) St[SW * (tid >> 2) + 1] = d;
    }
    if constexpr (BIAS) bias = bias_next;
    if (t + 1 < nt) {   // in flight during this tile's MFMAs
      const long n0 = i0 + TILE;
      load_rows<KP>(tq, Q + n0 * ldq, ldq, a.I - n0, a.K, a.q.vec != 0, tid);
      load_rows<DP>(td, dO + n0 * lddo, lddo, a.I - n0, a.D, a.dout.vec != 0, tid);
      load_o_part<DP>(po, O + n0 * ldo, ldo, a.I - n0, a.D, a.o.vec != 0, tid);
      sums = load_sums(S + n0, a.I - n0, a.s.vec != 0, tid);
      if constexpr (STABLE) maxs = load_sums(M + n0, a.I - n0, a.s.vec != 0, tid);
      if constexpr (BIAS) load_bias_t(bias_next, Bl + n0 * ldb, ldb, a.I - n0 - c, bias_keys, vec_b);
    }
    __syncthreads();   // delta of every row is in St

    [[maybe_unused]] int first[4];
    if constexpr (CAUSAL) {
      // key j0 against row i0: at most 63 on a visited tile and above -63 on a cut one
      const int d0 = causal_tile_cut(i0, j0, a.offset, a.J) ? (int)(j0 - a.offset - i0) : -2 * TILE;
#pragma unroll
      for (int r = 0; r < 4; ++r) first[r] = d0 + w * 16 + 4 * g + r;
    }

    // S^T and dP^T: rows are the wave's keys, columns the tile's query rows
    f32x4 s[4], dp[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) s[nb] = dp[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KP / 4; ++kk) {
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) s[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(kreg[kk], Qs[(nb * 16 + c) * QS + 4 * kk + g], s[nb], 0, 0, 0);
    }
#pragma unroll
    for (int dd = 0; dd < DP / 4; ++dd) {
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) dp[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(vreg[dd], Ds[(nb * 16 + c) * DS + 4 * dd + g], dp[nb], 0, 0, 0);
    }

    // p^T to the wave's rows, dS^T kept in s for the second pass; a row outside the problem or a key outside it is exactly
    // 0 by a select
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      const int col = nb * 16 + c;
      const bool qlive = i0 + col < a.I;
      const float inv = St[SW * col], delta = St[SW * col + 1];
      [[maybe_unused]] float mx = 0.f;
      if constexpr (STABLE) mx = St[SW * col + 2];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool live = qlive && klive[r];
        float x = s[nb][r] * a.scale;
        if constexpr (BIAS) x = x + bias.x[nb][r];
        if constexpr (CAUSAL) x = col >= first[r] ? x : -INFINITY;
        if constexpr (STABLE) x = x - mx;
        const float p = expf(x) * inv;
        const float ds = (a.scale * p) * (dp[nb][r] - delta);
        Ew[(4 * g + r) * ES + col] = live ? p : 0.f;
        s[nb][r] = live ? ds : 0.f;
      }
    }
    wave_sync();
#pragma unroll
    for (int ii = 0; ii < TILE / 4; ++ii) {
      const float e = Ew[c * ES + 4 * ii + g];
#pragma unroll
      for (int nb = 0; nb < DP / 16; ++nb) dv[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(e, Ds[(4 * ii + g) * DS + nb * 16 + c], dv[nb], 0, 0, 0);
    }
    wave_sync();   // p^T is read before dS^T takes its place
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) Ew[(4 * g + r) * ES + nb * 16 + c] = s[nb][r];
    }
    wave_sync();
#pragma unroll
    for (int ii = 0; ii < TILE / 4; ++ii) {
      const float e = Ew[c * ES + 4 * ii + g];
#pragma unroll
      for (int nb = 0; nb < KP / 16; ++nb) dk[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(e, Qs[(4 * ii + g) * QS + nb * 16 + c], dk[nb], 0, 0, 0);
    }
    wave_sync();
  }

  __syncthreads();   // every wave is done with the Q and dO tiles
  stage_acc<KP, QS>(dk, Qs, w, c, g);
  stage_acc<DP, DS>(dv, Ds, w, c, g);
  __syncthreads();
  if (a.put_dk) store_out<KP, QS>(Qs, dK, a.dk.v.ld, keys, a.K, a.dk.vec != 0, a.acc_dk != 0, tid);
  if (a.put_dv) store_out<DP, DS>(Ds, dV, a.dv.v.ld, keys, a.D, a.dv.vec != 0, a.acc_dv != 0, tid);
}

// One launch of one of the two kernels; the attributes of both are set together, once per device and instantiation.
template <auto DQ_KERNEL, auto DKV_KERNEL, class Args, int KP, int DP, bool STABLE = false>
int launch(eg_ctx* ctx, bool dkv, unsigned grid, const GradPlan& p, const Args& args) {
  const int rc = dynamic_lds_once<DQ_KERNEL, DKV_KERNEL>(ctx, {grad_dq_lds_bytes(KP, DP, STABLE), grad_dkv_lds_bytes(KP, DP, STABLE)});
  if (rc) return rc;
  if (dkv)
    hipLaunchKernelGGL(DKV_KERNEL, dim3(grid), dim3(p.block), (size_t)p.dkv.lds_bytes, ctx->stream, args);
  else
    hipLaunchKernelGGL(DQ_KERNEL, dim3(grid), dim3(p.block), (size_t)p.dq.lds_bytes, ctx->stream, args);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}

}  // namespace
