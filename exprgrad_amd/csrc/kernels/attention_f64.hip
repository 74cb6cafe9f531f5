// Fused attention forward in float64 on the matrix cores: attention_f32.hip's algorithm in doubles,
//   O_{o,i1}[i,:] (+)= (sum_j exp(scale * q_i . k_j) * V[j,:]) / (sum_j exp(scale * q_i . k_j))
// for every item (o, i1) of batch0 x batch1 — what a compile[float64] model runs between its two multi-head products, as
// written, without a row maximum: one pass with a running numerator and a running denominator, nothing of size I x J stored.
//
// One block owns one item and a tile of 64 query rows; its four waves own 16 whole rows each and keep them in registers as
// A operands.  The loop over tiles of TJ keys (64, or 32 where 64 do not fit the LDS: attention_plan.hpp, key_tile_f64):
//   stage  K tile [TJ][K] and V tile [TJ][D] into LDS (loaded into registers one tile ahead, during the MFMAs of the tile
//          before; rows j >= J and columns k >= K, d >= D are zero-filled, never read);
//   S      = Q_rows * K_tile^T   16 x TJ per wave: TJ / 16 accumulators of v_mfma_f64_16x16x4_f64, Q from registers;
//   e      = exp(S * scale)      one multiplication, then the double exp, as the generated float64 kernels emit it; keys
//          j >= J are zeroed with a select; e is added into four per-lane row sums and written to the wave's own [16][TJ]
//          LDS rows (accumulator layout -> A-operand layout: wave-private, no block barrier);
//   O_acc += E * V_tile          16 x D per wave, D / 16 accumulators.
// After the last tile the row sums are folded across the 16 lanes that share a row (xor shuffles 1, 2, 4, 8: a fixed order),
// a sum that is +Inf becomes NaN, the accumulators are divided (IEEE double division) and the rows stored.  No atomics, no
// workspace, no k-slices: two runs give the same bits, and an item has the same bits whatever batch it is part of.
//
// Operand conventions of the instruction (gemm_f64_mfma.hip has them): lane l gives A[row l & 15][k = l >> 4] and
// B[k = l >> 4][col l & 15]; it receives D[row (l >> 4) + 4 r][col l & 15] in element r — the rows of a lane's four elements
// are 4 apart, not neighbours as in the f32 16x16x4 form.  The LDS row steps are attention_plan.hpp's (F64_PAD_*).
#include "gemm_plan.hpp"        // batched2_c_distinct
#include "attention.hpp"        // the internal entry
#include "attention_tile.hpp"   // kernel operands, the item grid, the launcher
#include "gemm_f64_tile.hpp"    // d4, d2

#include <cmath>

namespace {

using eg::f64tile::d2;
using eg::f64tile::d4;
using namespace eg::attention;

using InD = Arg<const double>;
using OutD = Arg<double>;

struct AttnArgsD {
  InD q, k, v;
  OutD o;
  OutD s;   // eg_attention_sums_f64: the row sums, I doubles per item (SUMS instantiations only)
  long I, J;
  int K, D;
  double scale;
  int accumulate;
  Items items;
};

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

// SUMS: also store each row's denominator (eg_attention_sums_f64); a compile-time flag in the epilogue.
template <int KP, int DP, int TJ, bool SUMS>
__global__ __launch_bounds__(THREADS) void attention_f64_kernel(AttnArgsD a) {
  constexpr int KS = KP + F64_PAD_K, VS = DP + F64_PAD_V, ES = TJ + F64_PAD_E;
  // the Q tile [64][KS] passes through the front of the block's LDS before the loop
  static_assert(TILE_I * KS <= TJ * KS + TJ * VS + 4 * 16 * ES, "the Q tile fits the LDS of the three tiles");
  extern __shared__ __attribute__((aligned(16))) double lds_d[];
  double* const Ks = lds_d;                   // [TJ][KS]
  double* const Vs = Ks + TJ * KS;            // [TJ][VS]
  double* const Es = Vs + TJ * VS;            // [4][16][ES]

  const BlockItem b = block_item(a.items);
  const long i0 = (long)b.tile * TILE_I;
  const long ldq = a.q.v.ld, ldk = a.k.v.ld, ldv = a.v.v.ld;
  const double* const Q = item_base(a.q, b.outer, b.inner) + i0 * ldq;
  const double* const Kk = item_base(a.k, b.outer, b.inner);
  const double* const V = item_base(a.v, b.outer, b.inner);
  double* const O = item_base(a.o, b.outer, b.inner);

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  double* const Ew = Es + w * 16 * ES;

  // Q rows of the wave as A operands of every k step, for the whole loop
  double q[KP / 4];
  {
    TileRegsD<TILE_I, KP> tq;
    load_rows<TILE_I, KP>(tq, Q, ldq, a.I - i0, a.K, a.q.vec != 0, tid);
    store_rows<TILE_I, KP, KS>(tq, lds_d, tid);
    __syncthreads();
    const double* const p = lds_d + (w * 16 + c) * KS + g;
#pragma unroll
    for (int kk = 0; kk < KP / 4; ++kk) q[kk] = p[4 * kk];
  }

  d4 o[DP / 16];
#pragma unroll
  for (int nb = 0; nb < DP / 16; ++nb) o[nb] = d4{0.0, 0.0, 0.0, 0.0};
  double sum[4] = {0.0, 0.0, 0.0, 0.0};

  TileRegsD<TJ, KP> tk;
  TileRegsD<TJ, DP> tv;
  const long nt = (a.J + TJ - 1) / TJ;
  if (nt > 0) {
    load_rows<TJ, KP>(tk, Kk, ldk, a.J, a.K, a.k.vec != 0, tid);
    load_rows<TJ, DP>(tv, V, ldv, a.J, a.D, a.v.vec != 0, tid);
  }
  for (long t = 0; t < nt; ++t) {
    const long j0 = t * TJ;
    __syncthreads();   // every wave is done with the tiles in LDS (the first time: with the Q tile)
    store_rows<TJ, KP, KS>(tk, Ks, tid);
    store_rows<TJ, DP, VS>(tv, Vs, tid);
    __syncthreads();
    if (t + 1 < nt) {   // in flight during this tile's MFMAs
      load_rows<TJ, KP>(tk, Kk + (j0 + TJ) * ldk, ldk, a.J - j0 - TJ, a.K, a.k.vec != 0, tid);
      load_rows<TJ, DP>(tv, V + (j0 + TJ) * ldv, ldv, a.J - j0 - TJ, a.D, a.v.vec != 0, tid);
    }

    d4 s[TJ / 16];
#pragma unroll
    for (int nb = 0; nb < TJ / 16; ++nb) s[nb] = d4{0.0, 0.0, 0.0, 0.0};
    mma_nt<KP, KS, TJ>(q, Ks, c, g, s);

#pragma unroll
    for (int nb = 0; nb < TJ / 16; ++nb) {
      const bool live = j0 + nb * 16 + c < a.J;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double x = s[nb][r] * a.scale;
        double e = exp(x);
        e = live ? e : 0.0;   // a select: a key outside the problem adds exactly 0, whatever its score
        sum[r] += e;
        Ew[(g + 4 * r) * ES + nb * 16 + c] = e;
      }
    }
    wave_sync();

    mma_nn<DP, VS, ES, TJ>(Ew, Vs, c, g, o);
    wave_sync();   // the wave's E rows are read before its next tile overwrites them
  }

  // Row sums: the 16 lanes of a group hold the columns = c (mod 16) of rows g + 4 r.  A sum that overflowed is NaN, not
  // Inf: a row is NaN whenever its denominator is not finite (the header has the one case where the program differs).
  const bool empty = a.J == 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double t = sum[r];
    t += __shfl_xor(t, 1);
    t += __shfl_xor(t, 2);
    t += __shfl_xor(t, 4);
    t += __shfl_xor(t, 8);
    sum[r] = t == (double)INFINITY ? (double)NAN : t;
  }
  if constexpr (SUMS) {
    // the value row i is divided by, from the lane that holds column 0 of its group's rows; 0 when there are no keys
    double* const S = item_base(a.s, b.outer, b.inner);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long row = i0 + w * 16 + g + 4 * r;
      if (c == 0 && row < a.I) S[row] = sum[r];
    }
    if (empty && a.accumulate) return;   // an empty sum adds nothing to O
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long row = i0 + w * 16 + g + 4 * r;
    if (row >= a.I) continue;
#pragma unroll
    for (int nb = 0; nb < DP / 16; ++nb) {
      const int col = nb * 16 + c;
      if (col >= a.D) continue;
      const double v = empty ? 0.0 : o[nb][r] / sum[r];
      double* const p = O + row * a.o.v.ld + col;
      *p = a.accumulate ? *p + v : v;
    }
  }
}

template <int KP, int DP, bool SUMS>
int launch(eg_ctx* ctx, const char* name, unsigned grid, const Plan& p, const AttnArgsD& args) {
  constexpr int TJ = key_tile_f64(KP, DP);   // the planner's choice, as a template argument
  static_assert(TJ == 64 || TJ == 32, "a key tile that fits");
  EG_REQUIRE(p.tile_j == TJ && p.lds_bytes == lds_bytes_for_f64(KP, DP, TJ), EG_ERR_INVALID, "%s: the plan and the kernel disagree on the key tile", name);
  const int rc = dynamic_lds_once<&attention_f64_kernel<KP, DP, TJ, SUMS>>(ctx, {lds_bytes_for_f64(KP, DP, TJ)});
  if (rc) return rc;
  hipLaunchKernelGGL((attention_f64_kernel<KP, DP, TJ, SUMS>), dim3(grid), dim3(p.block), (size_t)p.lds_bytes, ctx->stream, args);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}

}  // namespace

namespace eg {
namespace attention {

// The one launcher: eg_attention_f64 and a float64 model's attention launches (host/run.cpp) come here with Sums == NULL,
// eg_attention_sums_f64 with the row sums' view.  The checks are attention_forward's, word for word.
int attention_forward_f64(eg_ctx* ctx, const Extents& e, double scale, const double* Q, View q, const double* Kk, View k, const double* V, View v,
                          double* O, View o, int accumulate, double* Sums, View s) {
  const char* const name = Sums ? "eg_attention_sums_f64" : "eg_attention_f64";   // the entry the messages speak of
  const long batch0 = e.batch0, batch1 = e.batch1, I = e.I, J = e.J, K = e.K, D = e.D;
  EG_REQUIRE(ctx, EG_ERR_INVALID, "%s: ctx is NULL", name);
  EG_REQUIRE(batch0 >= 0 && batch1 >= 0 && I >= 0 && J >= 0 && K >= 0 && D >= 0, EG_ERR_INVALID, "%s: negative extent", name);
  EG_REQUIRE(batch0 < (1L << 31) && batch1 < (1L << 31), EG_ERR_INVALID, "%s: a batch extent of 2^31 or more", name);
  EG_REQUIRE(q.stride0 >= 0 && q.stride1 >= 0 && k.stride0 >= 0 && k.stride1 >= 0 && v.stride0 >= 0 && v.stride1 >= 0, EG_ERR_INVALID,
             "%s: negative stride", name);
  if (batch0 == 0 || batch1 == 0 || I == 0 || (D == 0 && !Sums)) return EG_OK;
  EG_REQUIRE(D == 0 || O, EG_ERR_INVALID, "%s: O is NULL", name);
  EG_REQUIRE(J == 0 || D == 0 || V, EG_ERR_INVALID, "%s: NULL operand", name);
  EG_REQUIRE(J == 0 || K == 0 || (Q && Kk), EG_ERR_INVALID, "%s: NULL operand", name);
  EG_REQUIRE(q.ld >= K && k.ld >= K && v.ld >= D, EG_ERR_INVALID, "%s: leading dimension smaller than the row length", name);
  EG_REQUIRE(D == 0 || eg::gemm::batched2_c_distinct(batch0, o.stride0, batch1, o.stride1, I, o.ld, D), EG_ERR_INVALID,
             "%s: ldo, stride_o0 and stride_o1 make elements of O share an address", name);
  // the row sums: one row of I columns per item
  EG_REQUIRE(!Sums || eg::gemm::batched2_c_distinct(batch0, s.stride0, batch1, s.stride1, 1, I, I), EG_ERR_INVALID,
             "%s: stride_s0 and stride_s1 make elements of Sums share an address", name);
  EG_REQUIRE(K <= MAX_HEAD, EG_ERR_UNSUPPORTED, "%s: K = %ld is above the limit of %d", name, K, MAX_HEAD);
  EG_REQUIRE(D <= MAX_HEAD, EG_ERR_UNSUPPORTED, "%s: D = %ld is above the limit of %d", name, D, MAX_HEAD);
  if (J == 0 && accumulate && !Sums) return EG_OK;   // an empty sum adds nothing
  const int rc = eg::set_device(ctx);
  if (rc) return rc;

  Problem pr;
  static_cast<Extents&>(pr) = e;
  pr.q = {q, aligned16(Q)}, pr.k = {k, aligned16(Kk)}, pr.v = {v, aligned16(V)}, pr.o = {o, aligned16(O)};
  pr.sums = Sums != nullptr;
  pr.cus = ctx->compute_units;
  const Plan p = plan_attention_f64(pr);
  EG_REQUIRE(p.supported, EG_ERR_UNSUPPORTED, "%s: %s", name, p.reason);

  AttnArgsD args = {};
  args.q = {Q, q, p.vec_q}, args.k = {Kk, k, p.vec_k}, args.v = {V, v, p.vec_v};
  args.o = {O, o, 0}, args.s = {Sums, s, 0};
  args.I = I, args.J = J, args.K = (int)K, args.D = (int)D;
  args.scale = scale;
  args.accumulate = accumulate;
  // 9 kernels: the padded K x the padded D, each on its key tile; 9 more that store the row sums
  return for_each_launch(name, p.items, p.cut(), batch1, [&](const Items& items, unsigned grid) {
    args.items = items;
    return dispatch_heads(p.kp, p.dp, [&](auto KP, auto DP) {
      return Sums ? launch<KP(), DP(), true>(ctx, name, grid, p, args) : launch<KP(), DP(), false>(ctx, name, grid, p, args);
    });
  });
}

}  // namespace attention
}  // namespace eg

extern "C" int eg_attention_f64(eg_ctx* ctx, int64_t batch0, int64_t batch1, int64_t I, int64_t J, int64_t K, int64_t D, double scale, const double* Q,
                                int64_t ldq, int64_t stride_q0, int64_t stride_q1, const double* Kk, int64_t ldk, int64_t stride_k0,
                                int64_t stride_k1, const double* V, int64_t ldv, int64_t stride_v0, int64_t stride_v1, double* O, int64_t ldo,
                                int64_t stride_o0, int64_t stride_o1, int accumulate) {
  return eg::attention::attention_forward_f64(ctx, {batch0, batch1, I, J, K, D}, scale, Q, {ldq, stride_q0, stride_q1}, Kk, {ldk, stride_k0, stride_k1},
                                              V, {ldv, stride_v0, stride_v1}, O, {ldo, stride_o0, stride_o1}, accumulate);
}

extern "C" int eg_attention_sums_f64(eg_ctx* ctx, int64_t batch0, int64_t batch1, int64_t I, int64_t J, int64_t K, int64_t D, double scale,
                                     const double* Q, int64_t ldq, int64_t stride_q0, int64_t stride_q1, const double* Kk, int64_t ldk,
                                     int64_t stride_k0, int64_t stride_k1, const double* V, int64_t ldv, int64_t stride_v0, int64_t stride_v1,
                                     double* O, int64_t ldo, int64_t stride_o0, int64_t stride_o1, int accumulate, double* Sums, int64_t stride_s0,
                                     int64_t stride_s1) {
  return eg::attention::attention_forward_f64(ctx, {batch0, batch1, I, J, K, D}, scale, Q, {ldq, stride_q0, stride_q1}, Kk, {ldk, stride_k0, stride_k1},
                                              V, {ldv, stride_v0, stride_v1}, O, {ldo, stride_o0, stride_o1}, accumulate, Sums,
                                              {0, stride_s0, stride_s1});
}
