// Fused attention backward in float64 on the matrix cores: the formulas of attention_grad_f32.hip in doubles.  Per item, with
// s_ij = q_i . k_j, e_ij = exp(scale * s_ij) (the double exp, as in attention_f64.hip), L_i = sum_j e_ij
// (eg_attention_sums_f64's output), p_ij = e_ij / L_i and o_i = sum_j p_ij v_j (the forward's result):
//   delta_i = dO_i . o_i          dP_ij = dO_i . v_j          dS_ij = scale * p_ij * (dP_ij - delta_i)
//   dV_j = sum_i p_ij dO_i        dQ_i = sum_j dS_ij k_j      dK_j = sum_i dS_ij q_i
// Nothing of size I x J is stored.  No atomics, no workspace, every sum in a fixed order: two calls give the same bits, and an
// item has the same bits whatever batch it is part of.
//
// attention_dq_f64_kernel: one block owns one item and 64 query rows, a wave 16 of them.  The wave's Q rows and dO rows stay
// in registers as A operands; 1 / L_i (one IEEE division per row) and delta_i of the block's rows are computed once.  Per tile
// of TJ keys (attention_plan.hpp, grad_dq_step_f64: 64, or 32 where 64 do not fit the LDS):
//   S  = Q_rows * K_tile^T, dP = dO_rows * V_tile^T    both tiles read as NT operands, TJ / 16 accumulators each;
//   dS = scale * (exp(scale * S) / L) * (dP - delta)   in registers, keys j >= J zeroed with a select, then through the wave's
//        own [16][TJ] LDS rows (accumulator layout -> A-operand layout, wave-private);
//   dQ_acc += dS * K_tile                              the K tile read a second time, as an NN operand.
// attention_dkv_f64_kernel: the transpose.  One block owns 64 keys, a wave 16 of them; its K rows and V rows stay in registers
// as A operands.  Per tile of TI query rows (grad_dkv_step_f64), with the Q tile and the dO tile in LDS and 1 / L_i, delta_i of
// the tile's rows in a small LDS array (delta from the dO tile and O by row_delta, the dQ kernel's function: the same bits):
//   S^T = K_rows * Q_tile^T, dP^T = V_rows * dO_tile^T;
//   p^T and dS^T take 1 / L and delta per column; rows i >= I and keys j >= J are zeroed with a select;
//   dV_acc += p^T * dO_tile, dK_acc += dS^T * Q_tile   both through the wave's LDS rows, both tiles read as NN operands.
// Both kernels load the next tile into registers during the MFMAs of the current one.  The block's own 64 rows pass through
// the front of the same LDS before the loop, and its accumulators leave through it afterwards, in whole rows and 16-byte
// stores where the output allows them — one operand after the other where two [64][...] tiles do not fit at once.
//
// The instruction (attention_f64.hip, gemm_f64_mfma.hip): lane (c, g) = (lane & 15, lane >> 4) gives A[row c][k = g] and
// B[k = g][col c] and receives D[row g + 4 r][col c] in element r — a lane's four rows are 4 apart.  Everything indexed by an
// accumulator's row follows that map: the writes of dS, p^T and dS^T to the wave's rows, 1 / L and delta by row in the dQ
// kernel, the live keys by row in the dK/dV kernel, and the rows of the epilogue.  The LDS row steps are
// attention_plan.hpp's (GRAD_F64_PAD_*).
#include "gemm_plan.hpp"            // batched2_c_distinct
#include "attention.hpp"            // the internal entry
#include "attention_tile_f64.hpp"   // kernel operands, tiles in doubles, the two MFMA loops, the launcher

#include <cmath>

namespace {

using namespace eg::attention;

struct GradArgsD {
  InD q, k, v, o, s, dout;
  OutD dq, dk, dv;
  long I, J;
  int K, D;
  double scale;
  int acc_dq, acc_dk, acc_dv;          // that output is added to
  int put_dk, put_dv;                  // the dK/dV kernel stores that output
  Items items;
};

constexpr int TILE = 64;   // the block's own rows

// The thread index as a value the compiler cannot follow.  A tile's loads address row * ld + col per chunk; computed from the
// plain index these are loop invariants, and the compiler keeps two registers per chunk of the look-ahead tile alive across
// the whole loop — the registers that then spill.  Computed from this copy they are a few instructions per tile.
__device__ __forceinline__ int opaque(int tid) {
  asm volatile("" : "+v"(tid));
  return tid;
}

// ---- delta -----------------------------------------------------------------------------------------------------------------
// A row of O is cut into eight parts: part p holds columns 16 n + 2 p + {0, 1}.  TPR threads share a row (4 where the tile
// has 64 rows, 8 where it has 32) and thread tid holds the 8 / TPR parts (tid % TPR) * U + u of row tid / TPR.  Zero outside
// rows x D, where nothing is read.
template <int DP, int TPR>
struct OPartD {
  static constexpr int U = 8 / TPR;
  d2 r[DP / 16][U];
};

template <int DP, int TPR>
__device__ __forceinline__ void load_o_part(OPartD<DP, TPR>& o, const double* __restrict__ base, long ld, long rows, int width, bool vec, int tid) {
  constexpr int U = OPartD<DP, TPR>::U;
  const int row = tid / TPR, part = tid % TPR;
#pragma unroll
  for (int n = 0; n < DP / 16; ++n) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int col = 16 * n + 2 * (part * U + u);
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
      o.r[n][u] = v;
    }
  }
}

// delta of row tid / TPR of a dO tile in LDS (row step `stride`, even) against the thread's parts of O.  Each of the row's
// eight parts adds its columns in ascending order with fused multiply-adds; the parts then fold by xor 1, 2 and 4 of the part
// index — a thread's own two first where it holds two.  An addition gives the same bits whichever side an operand is on, so the
// one summation order serves both kernels at either TPR: the same dO and O rows give the same bits.
template <int DP, int TPR>
__device__ __forceinline__ double row_delta(const double* __restrict__ dOs, int stride, const OPartD<DP, TPR>& o, int tid) {
  constexpr int U = OPartD<DP, TPR>::U;
  const double* const d = dOs + (tid / TPR) * stride + 2 * U * (tid % TPR);
  double acc[U];
#pragma unroll
  for (int u = 0; u < U; ++u) acc[u] = 0.0;
#pragma unroll
  for (int n = 0; n < DP / 16; ++n) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const d2 x = *reinterpret_cast<const d2*>(d + 16 * n + 2 * u);
      acc[u] = __fma_rn(x[0], o.r[n][u][0], acc[u]);
      acc[u] = __fma_rn(x[1], o.r[n][u][1], acc[u]);
    }
  }
  double t = acc[0];
  if constexpr (U == 2) t += acc[1];
  t += __shfl_xor(t, 1);
  t += __shfl_xor(t, 2);
  if constexpr (TPR == 8) t += __shfl_xor(t, 4);
  return t;
}

// The row sums of a tile's ROWS rows: threads 0 .. ROWS / 2 - 1 hold two each.  Rows outside the problem are not read.
template <int ROWS>
__device__ __forceinline__ d2 load_sums(const double* __restrict__ S, long rows, bool vec, int tid) {
  d2 v = {1.0, 1.0};
  const int r0 = 2 * tid;
  if (tid < ROWS / 2 && r0 < rows) {
    if (vec && r0 + 2 <= rows) {
      v = *reinterpret_cast<const d2*>(S + r0);
    } else {
      v[0] = S[r0];
      if (r0 + 1 < rows) v[1] = S[r0 + 1];
    }
  }
  return v;
}

// St[2 * row] = 1 / L of the tile's rows (one IEEE division each), 0 for rows outside the problem
template <int ROWS>
__device__ __forceinline__ void store_inverse_sums(const d2& v, double* __restrict__ St, long rows, int tid) {
  if (tid < ROWS / 2) {
#pragma unroll
    for (int e = 0; e < 2; ++e) St[2 * (2 * tid + e)] = 2 * tid + e < rows ? 1.0 / v[e] : 0.0;
  }
}

// Rows 16 w .. 16 w + 15 of a [64][STRIDE] LDS tile of width W as the A operands of every k step.
template <int W, int STRIDE>
__device__ __forceinline__ void read_a_rows(const double* tile, int w, int c, int g, double (&regs)[W / 4]) {
  const double* const p = tile + (w * 16 + c) * STRIDE + g;
#pragma unroll
  for (int kk = 0; kk < W / 4; ++kk) regs[kk] = p[4 * kk];
}

// ---- the epilogue ------------------------------------------------------------------------------------------------------------
// The wave's accumulators (rows g + 4 r of its 16, columns 16 nb + c) into a [64][STRIDE] LDS tile
template <int WP, int STRIDE>
__device__ __forceinline__ void stage_acc(const d4 (&acc)[WP / 16], double* __restrict__ lds, int w, int c, int g) {
#pragma unroll
  for (int nb = 0; nb < WP / 16; ++nb) {
#pragma unroll
    for (int r = 0; r < 4; ++r) lds[(w * 16 + g + 4 * r) * STRIDE + nb * 16 + c] = acc[nb][r];
  }
}

// Rows [0, rows) x columns [0, width) of a [64][STRIDE] LDS tile to `base` (row step ld), chunk by chunk as load_rows reads:
// whole chunks as 16-byte stores when `vec`, everything else element by element; nothing outside is written, and nothing is
// read unless `accumulate`.
template <int WP, int STRIDE>
__device__ __forceinline__ void store_out(const double* __restrict__ lds, double* __restrict__ base, long ld, long rows, int width, bool vec,
                                          bool accumulate, int tid) {
  static_assert(STRIDE % 2 == 0, "16-byte LDS reads");
  constexpr int CPR = WP / 2;
#pragma unroll
  for (int i = 0; i < TILE * WP / (2 * THREADS); ++i) {
    const int idx = tid + i * THREADS;
    const int row = idx / CPR, col = (idx % CPR) * 2;
    if (row < rows && col < width) {
      const d2 v = *reinterpret_cast<const d2*>(&lds[row * STRIDE + col]);
      double* const p = base + (long)row * ld + col;
      if (vec && col + 2 <= width) {
        d2 x = v;
        if (accumulate) x = *reinterpret_cast<const d2*>(p) + v;
        *reinterpret_cast<d2*>(p) = x;
      } else {
        p[0] = accumulate ? p[0] + v[0] : v[0];
        if (col + 1 < width) p[1] = accumulate ? p[1] + v[1] : v[1];
      }
    }
  }
}

// ---- dQ ------------------------------------------------------------------------------------------------------------------------
template <int KP, int DP, int TJ>
__global__ __launch_bounds__(THREADS) void attention_dq_f64_kernel(GradArgsD a) {
  constexpr int KS = KP + GRAD_F64_PAD_BOTH, VS = DP + GRAD_F64_PAD_NT, ES = TJ + GRAD_F64_PAD_E;
  constexpr int FRONT = TJ * KS + TJ * VS + 4 * 16 * ES;   // doubles in front of 1 / L and delta
  // The block's Q tile [64][KS] and dO tile [64][VS] pass through the front before the loop, and dQ [64][KS] after it: side
  // by side where both fit, else one after the other.
  constexpr bool BOTH = TILE * KS + TILE * VS <= FRONT;
  static_assert(TILE * KS <= FRONT && TILE * VS <= FRONT, "each of the block's own tiles fits the LDS of the loop's tiles");
  extern __shared__ __attribute__((aligned(16))) double lds_d[];
  double* const Ks = lds_d;               // [TJ][KS]
  double* const Vs = Ks + TJ * KS;        // [TJ][VS]
  double* const Es = Vs + TJ * VS;        // [4][16][ES]
  double* const St = lds_d + FRONT;       // [64][2]: 1 / L, delta
  double* const dOs = BOTH ? lds_d + TILE * KS : lds_d;

  const BlockItem b = block_item(a.items);
  const long i0 = (long)b.tile * TILE;
  const long rows = a.I - i0;
  const long read_rows = a.J > 0 ? rows : 0;   // without keys nothing is read: dQ is zeros
  const long ldk = a.k.v.ld, ldv = a.v.v.ld;
  const double* const Q = item_base(a.q, b.outer, b.inner) + i0 * a.q.v.ld;
  const double* const dO = item_base(a.dout, b.outer, b.inner) + i0 * a.dout.v.ld;
  const double* const O = item_base(a.o, b.outer, b.inner) + i0 * a.o.v.ld;
  const double* const S = item_base(a.s, b.outer, b.inner) + i0;
  const double* const Kk = item_base(a.k, b.outer, b.inner);
  const double* const V = item_base(a.v, b.outer, b.inner);
  double* const dQ = item_base(a.dq, b.outer, b.inner) + i0 * a.dq.v.ld;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  double* const Ew = Es + w * 16 * ES;

  // the wave's Q rows and dO rows as A operands for the whole loop; 1 / L and delta of its accumulator rows g + 4 r
  double q[KP / 4], dout[DP / 4], inv[4], delta[4];
  {
    TileRegsD<TILE, KP> tq;
    TileRegsD<TILE, DP> td;
    OPartD<DP, 4> po;
    load_rows<TILE, KP>(tq, Q, a.q.v.ld, read_rows, a.K, a.q.vec != 0, tid);
    load_rows<TILE, DP>(td, dO, a.dout.v.ld, read_rows, a.D, a.dout.vec != 0, tid);
    load_o_part<DP, 4>(po, O, a.o.v.ld, read_rows, a.D, a.o.vec != 0, tid);
    const d2 sums = load_sums<TILE>(S, read_rows, a.s.vec != 0, tid);
    store_rows<TILE, KP, KS>(tq, lds_d, tid);
    if constexpr (BOTH) store_rows<TILE, DP, VS>(td, dOs, tid);
    store_inverse_sums<TILE>(sums, St, rows, tid);
    __syncthreads();
    read_a_rows<KP, KS>(lds_d, w, c, g, q);
    if constexpr (!BOTH) {
      __syncthreads();   // the Q tile is read before the dO tile takes its place
      store_rows<TILE, DP, VS>(td, dOs, tid);
      __syncthreads();
    }
    read_a_rows<DP, VS>(dOs, w, c, g, dout);
    const double d = row_delta<DP, 4>(dOs, VS, po, tid);
    if ((tid & 3) == 0) St[2 * (tid >> 2) + 1] = d;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      inv[r] = St[2 * (w * 16 + g + 4 * r)];
      delta[r] = St[2 * (w * 16 + g + 4 * r) + 1];
    }
  }

  d4 dq[KP / 16];
#pragma unroll
  for (int nb = 0; nb < KP / 16; ++nb) dq[nb] = d4{0.0, 0.0, 0.0, 0.0};

  TileRegsD<TJ, KP> tk;
  TileRegsD<TJ, DP> tv;
  const long nt = (a.J + TJ - 1) / TJ;
  if (nt > 0) {
    load_rows<TJ, KP>(tk, Kk, ldk, a.J, a.K, a.k.vec != 0, tid);
    load_rows<TJ, DP>(tv, V, ldv, a.J, a.D, a.v.vec != 0, tid);
  }
  for (long t = 0; t < nt; ++t) {
    const long j0 = t * TJ;
    __syncthreads();   // every wave is done with the tiles in LDS (the first time: with the Q and dO tiles)
    store_rows<TJ, KP, KS>(tk, Ks, tid);
    store_rows<TJ, DP, VS>(tv, Vs, tid);
    __syncthreads();
    if (t + 1 < nt) {   // in flight during this tile's MFMAs
      const int lt = opaque(tid);
      load_rows<TJ, KP>(tk, Kk + (j0 + TJ) * ldk, ldk, a.J - j0 - TJ, a.K, a.k.vec != 0, lt);
      load_rows<TJ, DP>(tv, V + (j0 + TJ) * ldv, ldv, a.J - j0 - TJ, a.D, a.v.vec != 0, lt);
    }

    d4 s[TJ / 16], dp[TJ / 16];
#pragma unroll
    for (int nb = 0; nb < TJ / 16; ++nb) s[nb] = dp[nb] = d4{0.0, 0.0, 0.0, 0.0};
    mma_nt<KP, KS, TJ>(q, Ks, c, g, s);
    mma_nt<DP, VS, TJ>(dout, Vs, c, g, dp);

#pragma unroll
    for (int nb = 0; nb < TJ / 16; ++nb) {
      const bool live = j0 + nb * 16 + c < a.J;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double p = exp(s[nb][r] * a.scale) * inv[r];
        const double ds = (a.scale * p) * (dp[nb][r] - delta[r]);
        Ew[(g + 4 * r) * ES + nb * 16 + c] = live ? ds : 0.0;   // a select: a key outside the problem adds exactly 0
      }
    }
    wave_sync();

    mma_nn<KP, KS, ES, TJ>(Ew, Ks, c, g, dq);
    wave_sync();   // the wave's rows are read before its next tile overwrites them
  }

  __syncthreads();   // every wave is done with the K tile
  stage_acc<KP, KS>(dq, lds_d, w, c, g);
  __syncthreads();
  store_out<KP, KS>(lds_d, dQ, a.dq.v.ld, rows, a.K, a.dq.vec != 0, a.acc_dq != 0, tid);
}

// ---- dK and dV -----------------------------------------------------------------------------------------------------------------
// AHEAD: the next query tile is loaded into registers during this tile's MFMAs; without it (where the registers do not hold
// it: attention_plan.hpp, grad_dkv_ahead_f64) each tile is loaded at the top of its own pass.
template <int KP, int DP, int TI, bool AHEAD>
__global__ __launch_bounds__(THREADS) void attention_dkv_f64_kernel(GradArgsD a) {
  constexpr int QS = KP + GRAD_F64_PAD_BOTH, DS = DP + GRAD_F64_PAD_BOTH, ES = TI + GRAD_F64_PAD_E;
  constexpr int TPR = THREADS / TI;   // threads per row of the query tile's O
  constexpr int FRONT = TI * QS + TI * DS + 4 * 16 * ES;
  // The block's K tile [64][QS] and V tile [64][DS] pass through the front before the loop, dK and dV after it: side by side
  // where both fit, else one after the other.
  constexpr bool BOTH = TILE * QS + TILE * DS <= FRONT;
  static_assert(TILE * QS <= FRONT && TILE * DS <= FRONT, "each of the block's own tiles fits the LDS of the loop's tiles");
  extern __shared__ __attribute__((aligned(16))) double lds_d[];
  double* const Qs = lds_d;               // [TI][QS]
  double* const Ds = Qs + TI * QS;        // [TI][DS]
  double* const Es = Ds + TI * DS;        // [4][16][ES]
  double* const St = lds_d + FRONT;       // [TI][2]: 1 / L, delta of the query tile's rows
  double* const Vf = BOTH ? lds_d + TILE * QS : lds_d;   // the V tile before the loop, dV after it

  const BlockItem b = block_item(a.items);
  const long j0 = (long)b.tile * TILE;
  const long keys = a.J - j0;
  const long read_keys = a.I > 0 ? keys : 0;   // without query rows nothing is read: dK and dV are zeros
  const long ldq = a.q.v.ld, lddo = a.dout.v.ld, ldo = a.o.v.ld;
  const double* const Q = item_base(a.q, b.outer, b.inner);
  const double* const dO = item_base(a.dout, b.outer, b.inner);
  const double* const O = item_base(a.o, b.outer, b.inner);
  const double* const S = item_base(a.s, b.outer, b.inner);
  const double* const Kk = item_base(a.k, b.outer, b.inner) + j0 * a.k.v.ld;
  const double* const V = item_base(a.v, b.outer, b.inner) + j0 * a.v.v.ld;
  double* const dK = item_base(a.dk, b.outer, b.inner) + j0 * a.dk.v.ld;
  double* const dV = item_base(a.dv, b.outer, b.inner) + j0 * a.dv.v.ld;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  double* const Ew = Es + w * 16 * ES;

  // the wave's K rows and V rows as A operands for the whole loop
  double kreg[KP / 4], vreg[DP / 4];
  {
    TileRegsD<TILE, KP> tk;
    TileRegsD<TILE, DP> tv;
    load_rows<TILE, KP>(tk, Kk, a.k.v.ld, read_keys, a.K, a.k.vec != 0, tid);
    load_rows<TILE, DP>(tv, V, a.v.v.ld, read_keys, a.D, a.v.vec != 0, tid);
    store_rows<TILE, KP, QS>(tk, lds_d, tid);
    if constexpr (BOTH) store_rows<TILE, DP, DS>(tv, Vf, tid);
    __syncthreads();
    read_a_rows<KP, QS>(lds_d, w, c, g, kreg);
    if constexpr (!BOTH) {
      __syncthreads();   // the K tile is read before the V tile takes its place
      store_rows<TILE, DP, DS>(tv, Vf, tid);
      __syncthreads();
    }
    read_a_rows<DP, DS>(Vf, w, c, g, vreg);
  }

  d4 dk[KP / 16], dv[DP / 16];
#pragma unroll
  for (int nb = 0; nb < KP / 16; ++nb) dk[nb] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int nb = 0; nb < DP / 16; ++nb) dv[nb] = d4{0.0, 0.0, 0.0, 0.0};
  bool klive[4];   // the keys of the accumulators' rows g + 4 r
#pragma unroll
  for (int r = 0; r < 4; ++r) klive[r] = w * 16 + g + 4 * r < keys;

  TileRegsD<TI, KP> tq;
  TileRegsD<TI, DP> td;
  OPartD<DP, TPR> po;
  d2 sums = {1.0, 1.0};
  const long nt = (a.I + TI - 1) / TI;
  const auto fetch = [&](long n0) {   // the query tile that starts at row n0
    const int lt = opaque(tid);
    load_rows<TI, KP>(tq, Q + n0 * ldq, ldq, a.I - n0, a.K, a.q.vec != 0, lt);
    load_rows<TI, DP>(td, dO + n0 * lddo, lddo, a.I - n0, a.D, a.dout.vec != 0, lt);
    load_o_part<DP, TPR>(po, O + n0 * ldo, ldo, a.I - n0, a.D, a.o.vec != 0, lt);
    sums = load_sums<TI>(S + n0, a.I - n0, a.s.vec != 0, lt);
  };
  if (AHEAD && nt > 0) fetch(0);
  for (long t = 0; t < nt; ++t) {
    const long i0 = t * TI;
    if (!AHEAD) fetch(i0);
    __syncthreads();   // every wave is done with the tiles in LDS (the first time: with the K and V tiles)
    store_rows<TI, KP, QS>(tq, Qs, tid);
    store_rows<TI, DP, DS>(td, Ds, tid);
    store_inverse_sums<TI>(sums, St, a.I - i0, tid);
    __syncthreads();
    {
      const double d = row_delta<DP, TPR>(Ds, DS, po, tid);
      if (tid % TPR == 0) St[2 * (tid / TPR) + 1] = d;
    }
    if (AHEAD && t + 1 < nt) fetch(i0 + TI);   // in flight during this tile's MFMAs
    __syncthreads();   // delta of every row is in St

    // S^T and dP^T: rows are the wave's keys, columns the tile's query rows
    d4 s[TI / 16], dp[TI / 16];
#pragma unroll
    for (int nb = 0; nb < TI / 16; ++nb) s[nb] = dp[nb] = d4{0.0, 0.0, 0.0, 0.0};
    mma_nt<KP, QS, TI>(kreg, Qs, c, g, s);
    mma_nt<DP, DS, TI>(vreg, Ds, c, g, dp);

    // p^T to the wave's rows, dS^T kept in s for the second pass; a row outside the problem or a key outside it is exactly
    // 0 by a select
#pragma unroll
    for (int nb = 0; nb < TI / 16; ++nb) {
      const int col = nb * 16 + c;
      const bool qlive = i0 + col < a.I;
      const double inv = St[2 * col], delta = St[2 * col + 1];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool live = qlive && klive[r];
        const double p = exp(s[nb][r] * a.scale) * inv;
        const double ds = (a.scale * p) * (dp[nb][r] - delta);
        Ew[(g + 4 * r) * ES + col] = live ? p : 0.0;
        s[nb][r] = live ? ds : 0.0;
      }
    }
    wave_sync();
    mma_nn<DP, DS, ES, TI>(Ew, Ds, c, g, dv);
    wave_sync();   // p^T is read before dS^T takes its place
#pragma unroll
    for (int nb = 0; nb < TI / 16; ++nb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) Ew[(g + 4 * r) * ES + nb * 16 + c] = s[nb][r];
    }
    wave_sync();
    mma_nn<KP, QS, ES, TI>(Ew, Qs, c, g, dk);
    wave_sync();
  }

  __syncthreads();   // every wave is done with the Q and dO tiles
  stage_acc<KP, QS>(dk, lds_d, w, c, g);
  if constexpr (BOTH) stage_acc<DP, DS>(dv, Vf, w, c, g);
  __syncthreads();
  if (a.put_dk) store_out<KP, QS>(lds_d, dK, a.dk.v.ld, keys, a.K, a.dk.vec != 0, a.acc_dk != 0, tid);
  if constexpr (!BOTH) {
    __syncthreads();   // dK has left before dV takes its place
    stage_acc<DP, DS>(dv, Vf, w, c, g);
    __syncthreads();
  }
  if (a.put_dv) store_out<DP, DS>(Vf, dV, a.dv.v.ld, keys, a.D, a.dv.vec != 0, a.acc_dv != 0, tid);
}

// One launch of one of the two kernels, each instantiated on the planner's step; the attributes of both are set together, once
// per device and instantiation.
template <int KP, int DP>
int launch(eg_ctx* ctx, bool dkv, unsigned grid, const GradPlan& p, const GradArgsD& args) {
  constexpr int TJ = grad_dq_step_f64(KP, DP), TI = grad_dkv_step_f64(KP, DP);
  constexpr bool AHEAD = grad_dkv_ahead_f64(KP, DP);
  static_assert((TJ == 64 || TJ == 32) && (TI == 64 || TI == 32), "steps that fit");
  constexpr long DQ_LDS = grad_dq_lds_bytes_f64(KP, DP, TJ), DKV_LDS = grad_dkv_lds_bytes_f64(KP, DP, TI);
  EG_REQUIRE(p.dq.step == TJ && p.dkv.step == TI && p.dq.lds_bytes == DQ_LDS && p.dkv.lds_bytes == DKV_LDS, EG_ERR_INVALID,
             "eg_attention_grad_f64: the plan and the kernels disagree on a step");
  const int rc = dynamic_lds_once<&attention_dq_f64_kernel<KP, DP, TJ>, &attention_dkv_f64_kernel<KP, DP, TI, AHEAD>>(ctx, {DQ_LDS, DKV_LDS});
  if (rc) return rc;
  if (dkv)
    hipLaunchKernelGGL((attention_dkv_f64_kernel<KP, DP, TI, AHEAD>), dim3(grid), dim3(p.block), (size_t)DKV_LDS, ctx->stream, args);
  else
    hipLaunchKernelGGL((attention_dq_f64_kernel<KP, DP, TJ>), dim3(grid), dim3(p.block), (size_t)DQ_LDS, ctx->stream, args);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}

}  // namespace

namespace eg {
namespace attention {

// The checks are attention_grad's (attention_grad_f32.hip), word for word.
int attention_grad_f64(eg_ctx* ctx, const Extents& e, double scale, const double* Q, View q, const double* Kk, View k, const double* V, View v,
                       const double* O, View o, const double* Sums, View s, const double* dO, View dout, double* dQ, View dq, double* dK, View dk,
                       double* dV, View dv, int accumulate) {
  const long batch0 = e.batch0, batch1 = e.batch1, I = e.I, J = e.J, K = e.K, D = e.D;
  EG_REQUIRE(ctx, EG_ERR_INVALID, "eg_attention_grad_f64: ctx is NULL");
  EG_REQUIRE(batch0 >= 0 && batch1 >= 0 && I >= 0 && J >= 0 && K >= 0 && D >= 0, EG_ERR_INVALID, "eg_attention_grad_f64: negative extent");
  EG_REQUIRE(batch0 < (1L << 31) && batch1 < (1L << 31), EG_ERR_INVALID, "eg_attention_grad_f64: a batch extent of 2^31 or more");
  EG_REQUIRE(q.stride0 >= 0 && q.stride1 >= 0 && k.stride0 >= 0 && k.stride1 >= 0 && v.stride0 >= 0 && v.stride1 >= 0 && o.stride0 >= 0 &&
                 o.stride1 >= 0 && s.stride0 >= 0 && s.stride1 >= 0 && dout.stride0 >= 0 && dout.stride1 >= 0,
             EG_ERR_INVALID, "eg_attention_grad_f64: negative stride");
  EG_REQUIRE((accumulate & ~7) == 0, EG_ERR_INVALID, "eg_attention_grad_f64: accumulate has bits other than 1 (dQ), 2 (dK) and 4 (dV)");
  if (batch0 == 0 || batch1 == 0) return EG_OK;
  const bool want_dq = I > 0 && K > 0, want_dk = J > 0 && K > 0, want_dv = J > 0 && D > 0;   // the outputs that have elements
  if (!want_dq && !want_dk && !want_dv) return EG_OK;
  EG_REQUIRE((!want_dq || dQ) && (!want_dk || dK) && (!want_dv || dV), EG_ERR_INVALID, "eg_attention_grad_f64: NULL output");
  if (I > 0 && J > 0) {
    EG_REQUIRE(Sums, EG_ERR_INVALID, "eg_attention_grad_f64: NULL operand (Sums)");
    EG_REQUIRE(K == 0 || (Q && Kk), EG_ERR_INVALID, "eg_attention_grad_f64: NULL operand (Q or Kk)");
    EG_REQUIRE(D == 0 || (V && O && dO), EG_ERR_INVALID, "eg_attention_grad_f64: NULL operand (V, O or dO)");
  }
  EG_REQUIRE(q.ld >= K && k.ld >= K && dq.ld >= K && dk.ld >= K && v.ld >= D && o.ld >= D && dout.ld >= D && dv.ld >= D, EG_ERR_INVALID,
             "eg_attention_grad_f64: leading dimension smaller than the row length");
  EG_REQUIRE(!want_dq || eg::gemm::batched2_c_distinct(batch0, dq.stride0, batch1, dq.stride1, I, dq.ld, K), EG_ERR_INVALID,
             "eg_attention_grad_f64: lddq, stride_dq0 and stride_dq1 make elements of dQ share an address");
  EG_REQUIRE(!want_dk || eg::gemm::batched2_c_distinct(batch0, dk.stride0, batch1, dk.stride1, J, dk.ld, K), EG_ERR_INVALID,
             "eg_attention_grad_f64: lddk, stride_dk0 and stride_dk1 make elements of dK share an address");
  EG_REQUIRE(!want_dv || eg::gemm::batched2_c_distinct(batch0, dv.stride0, batch1, dv.stride1, J, dv.ld, D), EG_ERR_INVALID,
             "eg_attention_grad_f64: lddv, stride_dv0 and stride_dv1 make elements of dV share an address");
  EG_REQUIRE(K <= MAX_HEAD, EG_ERR_UNSUPPORTED, "eg_attention_grad_f64: K = %ld is above the limit of %d", K, MAX_HEAD);
  EG_REQUIRE(D <= MAX_HEAD, EG_ERR_UNSUPPORTED, "eg_attention_grad_f64: D = %ld is above the limit of %d", D, MAX_HEAD);

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
  const GradPlan p = plan_attention_grad_f64(pr);
  EG_REQUIRE(p.supported, EG_ERR_UNSUPPORTED, "eg_attention_grad_f64: %s", p.reason);

  GradArgsD args = {};
  args.q = {Q, q, p.vec_q}, args.k = {Kk, k, p.vec_k}, args.v = {V, v, p.vec_v}, args.o = {O, o, p.vec_o}, args.s = {Sums, s, p.vec_s};
  args.dout = {dO, dout, p.vec_do}, args.dq = {dQ, dq, p.vec_dq}, args.dk = {dK, dk, p.vec_dk}, args.dv = {dV, dv, p.vec_dv};
  args.I = I, args.J = J, args.K = (int)K, args.D = (int)D;
  args.scale = scale;
  args.acc_dq = acc_dq, args.acc_dk = acc_dk, args.acc_dv = acc_dv;
  args.put_dk = put_dk, args.put_dv = put_dv;
  // 9 instantiations of each kernel: the padded K x the padded D, each on its step
  auto run = [&](bool dkv, const GradKernel& kernel) {
    return for_each_launch("eg_attention_grad_f64", p.items, kernel, batch1, [&](const Items& items, unsigned grid) {
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

extern "C" int eg_attention_grad_f64(eg_ctx* ctx, int64_t batch0, int64_t batch1, int64_t I, int64_t J, int64_t K, int64_t D, double scale,
                                     const double* Q, int64_t ldq, int64_t stride_q0, int64_t stride_q1,
                                     const double* Kk, int64_t ldk, int64_t stride_k0, int64_t stride_k1,
                                     const double* V, int64_t ldv, int64_t stride_v0, int64_t stride_v1,
                                     const double* O, int64_t ldo, int64_t stride_o0, int64_t stride_o1,
                                     const double* Sums, int64_t stride_s0, int64_t stride_s1,
                                     const double* dO, int64_t lddo, int64_t stride_do0, int64_t stride_do1,
                                     double* dQ, int64_t lddq, int64_t stride_dq0, int64_t stride_dq1,
                                     double* dK, int64_t lddk, int64_t stride_dk0, int64_t stride_dk1,
                                     double* dV, int64_t lddv, int64_t stride_dv0, int64_t stride_dv1, int accumulate) {
  return eg::attention::attention_grad_f64(ctx, {batch0, batch1, I, J, K, D}, scale, Q, {ldq, stride_q0, stride_q1}, Kk, {ldk, stride_k0, stride_k1},
                                           V, {ldv, stride_v0, stride_v1}, O, {ldo, stride_o0, stride_o1}, Sums, {0, stride_s0, stride_s1}, dO,
                                           {lddo, stride_do0, stride_do1}, dQ, {lddq, stride_dq0, stride_dq1}, dK, {lddk, stride_dk0, stride_dk1}, dV,
                                           {lddv, stride_dv0, stride_dv1}, accumulate);
}
