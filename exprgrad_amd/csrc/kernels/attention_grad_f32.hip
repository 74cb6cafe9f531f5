// Fused attention backward, exact f32 on the matrix cores.  Per item, with s_ij = q_i . k_j, e_ij = expf(scale * s_ij),
// L_i = sum_j e_ij (eg_attention_sums' output), p_ij = e_ij / L_i and o_i = sum_j p_ij v_j (the forward's result):
//   delta_i = dO_i . o_i          dP_ij = dO_i . v_j          dS_ij = scale * p_ij * (dP_ij - delta_i)
//   dV_j = sum_i p_ij dO_i        dQ_i = sum_j dS_ij k_j      dK_j = sum_i dS_ij q_i
// Nothing of size I x J is stored: both kernels recompute the probabilities tile by tile, as the forward computes them.
// No atomics, no workspace, every sum in a fixed order: two calls give the same bits.
//
// attention_dq_kernel: one block owns one item and 64 query rows, a wave 16 of them.  The wave's Q rows and dO rows stay in
// registers as A operands; 1 / L_i and delta_i of the block's rows are computed once.  Per tile of 64 keys:
//   S  = Q_rows * K_tile^T, dP = dO_rows * V_tile^T    both tiles read as NT operands, 4 + 4 accumulators;
//   dS = scale * (expf(scale * S) / L) * (dP - delta)  in registers, keys j >= J zeroed with a select, then through the
//        wave's own [16][64] LDS rows (accumulator layout -> A-operand layout);
//   dQ_acc += dS * K_tile                              the K tile read a second time, as an NN operand.
// attention_dkv_kernel: the transpose.  One block owns 64 keys, a wave 16 of them; its K rows and V rows stay in registers
// as A operands.  Per tile of 64 query rows, with the Q tile and the dO tile in LDS and 1 / L_i, delta_i of the tile's rows
// in a small LDS array (delta recomputed from the dO tile and O, by the same function as in the dQ kernel: same bits):
//   S^T = K_rows * Q_tile^T, dP^T = V_rows * dO_tile^T;
//   p^T and dS^T take 1 / L and delta per column; rows i >= I and keys j >= J are zeroed with a select;
//   dV_acc += p^T * dO_tile, dK_acc += dS^T * Q_tile   both through the wave's LDS rows, both tiles read as NN operands.
// Both kernels load the next tile into registers during the MFMAs of the current one, and both write their accumulators
// through LDS so that whole rows leave in 16-byte stores where the output allows them.
//
// LDS rows.  ds_read_b32 serves a wave in two halves of 32 lanes over 32 banks.  An NT read (lane (c, g) takes
// tile[16 nb + c][4 kk + g]) wants c * stride + g spread out, an NN read (tile[4 jj + g][16 nb + c]) wants g * stride + c
// spread out.  A stride = 4 (mod 32), the forward's, is as good as an aligned stride gets for NT (c and c + 8 share a bank)
// and poor for NN (rows g and g + 1 overlap in 12 of 16 banks); = 20 (mod 32) keeps NT where it was and leaves NN four
// shared banks.  Tiles read both ways have rows of width + 20 floats, tiles read NT only of width + 4.
#include "gemm_plan.hpp"        // batched2_c_distinct
#include "attention.hpp"        // the internal entry
#include "attention_tile.hpp"   // kernel operands, tiles, the MFMA loops, the launcher

#include <cmath>

namespace {

using eg::gemm::f32x4;
using namespace eg::attention;

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

constexpr int TILE = 64;

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

// St[2 * row] = 1 / L of the tile's rows, 0 for rows outside the problem
__device__ __forceinline__ void store_inverse_sums(const f32x4& v, float* __restrict__ St, long rows, int tid) {
  if (tid < 16) {
#pragma unroll
    for (int e = 0; e < 4; ++e) St[2 * (4 * tid + e)] = 4 * tid + e < rows ? 1.f / v[e] : 0.f;
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

template <int KP, int DP>
__global__ __launch_bounds__(THREADS) void attention_dq_kernel(GradArgs a) {
  constexpr int KS = KP + GRAD_PAD_BOTH, VS = DP + GRAD_PAD_NT;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const Ks = lds;                  // [64][KS]: the Q tile first, dQ last
  float* const Vs = Ks + TILE * KS;       // [64][VS]: the dO tile first
  float* const Es = Vs + TILE * VS;       // [4][16][ES]
  float* const St = Es + 4 * 16 * ES;     // [64][2]: 1 / L, delta

  const BlockItem b = block_item(a.items);
  const long i0 = (long)b.tile * TILE;
  const long rows = a.I - i0;
  const long read_rows = a.J > 0 ? rows : 0;   // without keys nothing is read: dQ is zeros
  const long ldk = a.k.v.ld, ldv = a.v.v.ld;
  const float* const Q = item_base(a.q, b.outer, b.inner) + i0 * a.q.v.ld;
  const float* const dO = item_base(a.dout, b.outer, b.inner) + i0 * a.dout.v.ld;
  const float* const O = item_base(a.o, b.outer, b.inner) + i0 * a.o.v.ld;
  const float* const S = item_base(a.s, b.outer, b.inner) + i0;
  const float* const Kk = item_base(a.k, b.outer, b.inner);
  const float* const V = item_base(a.v, b.outer, b.inner);
  float* const dQ = item_base(a.dq, b.outer, b.inner) + i0 * a.dq.v.ld;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  float* const Ew = Es + w * 16 * ES;

  TileRegs<KP> tk;
  TileRegs<DP> tv;
  // the wave's Q rows and dO rows as A operands for the whole loop; 1 / L and delta of its accumulator rows
  float q[KP / 4], dout[DP / 4], inv[4], delta[4];
  {
    OPart<DP> po;
    load_rows<KP>(tk, Q, a.q.v.ld, read_rows, a.K, a.q.vec != 0, tid);
    load_rows<DP>(tv, dO, a.dout.v.ld, read_rows, a.D, a.dout.vec != 0, tid);
    load_o_part<DP>(po, O, a.o.v.ld, read_rows, a.D, a.o.vec != 0, tid);
    const f32x4 sums = load_sums(S, read_rows, a.s.vec != 0, tid);
    store_rows<KP, KS>(tk, Ks, tid);
    store_rows<DP, VS>(tv, Vs, tid);
    store_inverse_sums(sums, St, rows, tid);
    __syncthreads();
    read_a_rows<KP, KS>(Ks, w, c, g, q);
    read_a_rows<DP, VS>(Vs, w, c, g, dout);
    const float d = row_delta<DP>(Vs, VS, po, tid);
    if ((tid & 3) == 0) St[2 * (tid >> 2) + 1] = d;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      inv[r] = St[2 * (w * 16 + 4 * g + r)];
      delta[r] = St[2 * (w * 16 + 4 * g + r) + 1];
    }
  }

  f32x4 dq[KP / 16];
#pragma unroll
  for (int nb = 0; nb < KP / 16; ++nb) dq[nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  const long nt = (a.J + TILE - 1) / TILE;
  if (nt > 0) {
    load_rows<KP>(tk, Kk, ldk, a.J, a.K, a.k.vec != 0, tid);
    load_rows<DP>(tv, V, ldv, a.J, a.D, a.v.vec != 0, tid);
  }
  for (long t = 0; t < nt; ++t) {
    const long j0 = t * TILE;
    __syncthreads();   // every wave is done with the tiles in LDS (the first time: with the Q and dO tiles)
    store_rows<KP, KS>(tk, Ks, tid);
    store_rows<DP, VS>(tv, Vs, tid);
    __syncthreads();
    if (t + 1 < nt) {   // in flight during this tile's MFMAs
      load_rows<KP>(tk, Kk + (j0 + TILE) * ldk, ldk, a.J - j0 - TILE, a.K, a.k.vec != 0, tid);
      load_rows<DP>(tv, V + (j0 + TILE) * ldv, ldv, a.J - j0 - TILE, a.D, a.v.vec != 0, tid);
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
        const float p = expf(s[nb][r] * a.scale) * inv[r];
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

template <int KP, int DP>
__global__ __launch_bounds__(THREADS) void attention_dkv_kernel(GradArgs a) {
  constexpr int QS = KP + GRAD_PAD_BOTH, DS = DP + GRAD_PAD_BOTH;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const Qs = lds;                  // [64][QS]: the K tile first, dK last
  float* const Ds = Qs + TILE * QS;       // [64][DS]: the V tile first, dV last
  float* const Es = Ds + TILE * DS;       // [4][16][ES]
  float* const St = Es + 4 * 16 * ES;     // [64][2]: 1 / L, delta of the query tile's rows

  const BlockItem b = block_item(a.items);
  const long j0 = (long)b.tile * TILE;
  const long keys = a.J - j0;
  const long read_keys = a.I > 0 ? keys : 0;   // without query rows nothing is read: dK and dV are zeros
  const long ldq = a.q.v.ld, lddo = a.dout.v.ld, ldo = a.o.v.ld;
  const float* const Q = item_base(a.q, b.outer, b.inner);
  const float* const dO = item_base(a.dout, b.outer, b.inner);
  const float* const O = item_base(a.o, b.outer, b.inner);
  const float* const S = item_base(a.s, b.outer, b.inner);
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

  const long nt = (a.I + TILE - 1) / TILE;
  if (nt > 0) {
    load_rows<KP>(tq, Q, ldq, a.I, a.K, a.q.vec != 0, tid);
    load_rows<DP>(td, dO, lddo, a.I, a.D, a.dout.vec != 0, tid);
    load_o_part<DP>(po, O, ldo, a.I, a.D, a.o.vec != 0, tid);
    sums = load_sums(S, a.I, a.s.vec != 0, tid);
  }
  for (long t = 0; t < nt; ++t) {
    const long i0 = t * TILE;
    __syncthreads();   // every wave is done with the tiles in LDS (the first time: with the K and V tiles)
    store_rows<KP, QS>(tq, Qs, tid);
    store_rows<DP, DS>(td, Ds, tid);
    store_inverse_sums(sums, St, a.I - i0, tid);
    __syncthreads();
    {
      const float d = row_delta<DP>(Ds, DS, po, tid);
      if ((tid & 3) == 0) St[2 * (tid >> 2) + 1] = d;
    }
    if (t + 1 < nt) {   // in flight during this tile's MFMAs
      const long n0 = i0 + TILE;
      load_rows<KP>(tq, Q + n0 * ldq, ldq, a.I - n0, a.K, a.q.vec != 0, tid);
      load_rows<DP>(td, dO + n0 * lddo, lddo, a.I - n0, a.D, a.dout.vec != 0, tid);
      load_o_part<DP>(po, O + n0 * ldo, ldo, a.I - n0, a.D, a.o.vec != 0, tid);
      sums = load_sums(S + n0, a.I - n0, a.s.vec != 0, tid);
    }
    __syncthreads();   // delta of every row is in St

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
      const float inv = St[2 * col], delta = St[2 * col + 1];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool live = qlive && klive[r];
        const float p = expf(s[nb][r] * a.scale) * inv;
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
template <int KP, int DP>
int launch(eg_ctx* ctx, bool dkv, unsigned grid, const GradPlan& p, const GradArgs& args) {
  const int rc = dynamic_lds_once<&attention_dq_kernel<KP, DP>, &attention_dkv_kernel<KP, DP>>(ctx, {grad_dq_lds_bytes(KP, DP), grad_dkv_lds_bytes(KP, DP)});
  if (rc) return rc;
  if (dkv)
    hipLaunchKernelGGL((attention_dkv_kernel<KP, DP>), dim3(grid), dim3(p.block), (size_t)p.dkv.lds_bytes, ctx->stream, args);
  else
    hipLaunchKernelGGL((attention_dq_kernel<KP, DP>), dim3(grid), dim3(p.block), (size_t)p.dq.lds_bytes, ctx->stream, args);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}

}  // namespace

namespace eg {
namespace attention {

int attention_grad(eg_ctx* ctx, const Extents& e, float scale, const float* Q, View q, const float* Kk, View k, const float* V, View v,
                   const float* O, View o, const float* Sums, View s, const float* dO, View dout, float* dQ, View dq, float* dK, View dk, float* dV,
                   View dv, int accumulate) {
  const long batch0 = e.batch0, batch1 = e.batch1, I = e.I, J = e.J, K = e.K, D = e.D;
  EG_REQUIRE(ctx, EG_ERR_INVALID, "eg_attention_grad: ctx is NULL");
  EG_REQUIRE(batch0 >= 0 && batch1 >= 0 && I >= 0 && J >= 0 && K >= 0 && D >= 0, EG_ERR_INVALID, "eg_attention_grad: negative extent");
  EG_REQUIRE(batch0 < (1L << 31) && batch1 < (1L << 31), EG_ERR_INVALID, "eg_attention_grad: a batch extent of 2^31 or more");
  EG_REQUIRE(q.stride0 >= 0 && q.stride1 >= 0 && k.stride0 >= 0 && k.stride1 >= 0 && v.stride0 >= 0 && v.stride1 >= 0 && o.stride0 >= 0 &&
                 o.stride1 >= 0 && s.stride0 >= 0 && s.stride1 >= 0 && dout.stride0 >= 0 && dout.stride1 >= 0,
             EG_ERR_INVALID, "eg_attention_grad: negative stride");
  EG_REQUIRE((accumulate & ~7) == 0, EG_ERR_INVALID, "eg_attention_grad: accumulate has bits other than 1 (dQ), 2 (dK) and 4 (dV)");
  if (batch0 == 0 || batch1 == 0) return EG_OK;
  const bool want_dq = I > 0 && K > 0, want_dk = J > 0 && K > 0, want_dv = J > 0 && D > 0;   // the outputs that have elements
  if (!want_dq && !want_dk && !want_dv) return EG_OK;
  EG_REQUIRE((!want_dq || dQ) && (!want_dk || dK) && (!want_dv || dV), EG_ERR_INVALID, "eg_attention_grad: NULL output");
  if (I > 0 && J > 0) {
    EG_REQUIRE(Sums, EG_ERR_INVALID, "eg_attention_grad: NULL operand (Sums)");
    EG_REQUIRE(K == 0 || (Q && Kk), EG_ERR_INVALID, "eg_attention_grad: NULL operand (Q or Kk)");
    EG_REQUIRE(D == 0 || (V && O && dO), EG_ERR_INVALID, "eg_attention_grad: NULL operand (V, O or dO)");
  }
  EG_REQUIRE(q.ld >= K && k.ld >= K && dq.ld >= K && dk.ld >= K && v.ld >= D && o.ld >= D && dout.ld >= D && dv.ld >= D, EG_ERR_INVALID,
             "eg_attention_grad: leading dimension smaller than the row length");
  EG_REQUIRE(!want_dq || eg::gemm::batched2_c_distinct(batch0, dq.stride0, batch1, dq.stride1, I, dq.ld, K), EG_ERR_INVALID,
             "eg_attention_grad: lddq, stride_dq0 and stride_dq1 make elements of dQ share an address");
  EG_REQUIRE(!want_dk || eg::gemm::batched2_c_distinct(batch0, dk.stride0, batch1, dk.stride1, J, dk.ld, K), EG_ERR_INVALID,
             "eg_attention_grad: lddk, stride_dk0 and stride_dk1 make elements of dK share an address");
  EG_REQUIRE(!want_dv || eg::gemm::batched2_c_distinct(batch0, dv.stride0, batch1, dv.stride1, J, dv.ld, D), EG_ERR_INVALID,
             "eg_attention_grad: lddv, stride_dv0 and stride_dv1 make elements of dV share an address");
  EG_REQUIRE(K <= MAX_HEAD, EG_ERR_UNSUPPORTED, "eg_attention_grad: K = %ld is above the limit of %d", K, MAX_HEAD);
  EG_REQUIRE(D <= MAX_HEAD, EG_ERR_UNSUPPORTED, "eg_attention_grad: D = %ld is above the limit of %d", D, MAX_HEAD);

  // An output that is all zeros (an empty sum) is written as zeros when its bit is clear and left alone otherwise.
  const bool acc_dq = accumulate & 1, acc_dk = accumulate & 2, acc_dv = accumulate & 4;
  const bool run_dq = want_dq && !((J == 0 || D == 0) && acc_dq);
  const bool put_dk = want_dk && !((I == 0 || D == 0) && acc_dk);
  const bool put_dv = want_dv && !(I == 0 && acc_dv);
  if (!run_dq && !put_dk && !put_dv) return EG_OK;
  int rc = eg::set_device(ctx);
  if (rc) return rc;

  GradProblem pr;
  static_cast<Extents&>(pr) = e;
  pr.q = {q, aligned16(Q)}, pr.k = {k, aligned16(Kk)}, pr.v = {v, aligned16(V)}, pr.o = {o, aligned16(O)}, pr.s = {s, aligned16(Sums)};
  pr.dout = {dout, aligned16(dO)}, pr.dq = {dq, aligned16(dQ)}, pr.dk = {dk, aligned16(dK)}, pr.dv = {dv, aligned16(dV)};
  pr.cus = ctx->compute_units;
  const GradPlan p = plan_attention_grad(pr);
  EG_REQUIRE(p.supported, EG_ERR_UNSUPPORTED, "eg_attention_grad: %s", p.reason);

  GradArgs args = {};
  args.q = {Q, q, p.vec_q}, args.k = {Kk, k, p.vec_k}, args.v = {V, v, p.vec_v}, args.o = {O, o, p.vec_o}, args.s = {Sums, s, p.vec_s};
  args.dout = {dO, dout, p.vec_do}, args.dq = {dQ, dq, p.vec_dq}, args.dk = {dK, dk, p.vec_dk}, args.dv = {dV, dv, p.vec_dv};
  args.I = I, args.J = J, args.K = (int)K, args.D = (int)D;
  args.scale = scale;
  args.acc_dq = acc_dq, args.acc_dk = acc_dk, args.acc_dv = acc_dv;
  args.put_dk = put_dk, args.put_dv = put_dv;
  // 9 instantiations of each kernel: the padded K x the padded D
  auto run = [&](bool dkv, const GradKernel& kernel) {
    return for_each_launch("eg_attention_grad", p.items, kernel, batch1, [&](const Items& items, unsigned grid) {
      args.items = items;
      return dispatch_heads(p.kp, p.dp, [&](auto KP, auto DP) { return launch<KP(), DP()>(ctx, dkv, grid, p, args); });
    });
  };
  if (run_dq) rc = run(false, p.dq);
  if (!rc && (put_dk || put_dv)) rc = run(true, p.dkv);
  return rc;
}

}  // namespace attention
}  // namespace eg

extern "C" int eg_attention_grad(eg_ctx* ctx, int64_t batch0, int64_t batch1, int64_t I, int64_t J, int64_t K, int64_t D, float scale,
                                 const float* Q, int64_t ldq, int64_t stride_q0, int64_t stride_q1,
                                 const float* Kk, int64_t ldk, int64_t stride_k0, int64_t stride_k1,
                                 const float* V, int64_t ldv, int64_t stride_v0, int64_t stride_v1,
                                 const float* O, int64_t ldo, int64_t stride_o0, int64_t stride_o1,
                                 const float* Sums, int64_t stride_s0, int64_t stride_s1,
                                 const float* dO, int64_t lddo, int64_t stride_do0, int64_t stride_do1,
                                 float* dQ, int64_t lddq, int64_t stride_dq0, int64_t stride_dq1,
                                 float* dK, int64_t lddk, int64_t stride_dk0, int64_t stride_dk1,
                                 float* dV, int64_t lddv, int64_t stride_dv0, int64_t stride_dv1, int accumulate) {
  return eg::attention::attention_grad(ctx, {batch0, batch1, I, J, K, D}, scale, Q, {ldq, stride_q0, stride_q1}, Kk, {ldk, stride_k0, stride_k1}, V,
                                       {ldv, stride_v0, stride_v1}, O, {ldo, stride_o0, stride_o1}, Sums, {0, stride_s0, stride_s1}, dO,
                                       {lddo, stride_do0, stride_do1}, dQ, {lddq, stride_dq0, stride_dq1}, dK, {lddk, stride_dk0, stride_dk1}, dV,
                                       {lddv, stride_dv0, stride_dv1}, accumulate);
}
