// Fused attention forward with a running row maximum, exact f32 on the matrix cores (eg_attention_stable):
//   x_ij = scale * q_i . k_j (+ bias_ij)     m_i = max_j x_ij     L_i = sum_j expf(x_ij - m_i)
//   O_{o,i1}[i,:] (+)= (sum_j expf(x_ij - m_i) * V[j,:]) / L_i,   Stats = (m, L)
// The softmax a library user expects: finite for finite scores of any magnitude, where attention_f32.hip computes the
// program's expf(x) as written and is NaN outside a window of about [-103, 88.7].  The DSL has no maximum reduction, so this is
// a library kernel and not a generated one.
//
// The block, the LDS tiles, the prefetch and the two barriers per key tile are attention_f32_kernel's (its header has the
// operand maps and the bank arithmetic): one block per item and 64 query rows, four waves of 16 whole rows, K tile [64][KP + 4],
// V tile [64][DP + 16], a wave's own E rows [16][68], K, V and the bias loaded a tile ahead.  lds_bytes_for and plan_attention
// serve both.  What differs is between the two products of a key tile.  Lane (c, g) holds rows 4 g + r and keys 16 nb + c of
// S = Q_rows * K_tile^T in s[nb][r], and the same rows of O in o[nb][r]: everything per row is lane-local in r.
//   scores   x = s * scale, x = x + bias (two roundings, as in the as-written kernels); keys j >= J become -Inf by a select;
//   tile max the lane's four nb, then the 16 lanes that share g: those are one DPP row, so four row rotations (8, 4, 2, 1) on
//            the vector ALU, no trip through the LDS crossbar.  A maximum has the same bits in any order;
//   running  m_new = max(m, tile max); the subtrahend is m_new, or 0 while m_new is still -Inf (so that -Inf - -Inf never
//            appears and a masked key adds expf(-Inf) = 0);
//   correct  alpha = expf(m - subtrahend), o[nb][r] *= alpha[r], sum[r] *= alpha[r] — only when some row of the wave raised its
//            maximum: a wave-uniform branch on a ballot.  A row that did not move has alpha = 1.0f exactly (or holds zeros
//            or NaNs that alpha leaves what they are), so skipping is the same bits as multiplying.  With scores that do not
//            grow along j most waves skip it after the first tiles: DP / 4 + 4 multiplications and four expf saved per lane;
//   terms    e = expf(x - subtrahend), added into the lane's row sum, written to the wave's E rows; O_acc += E * V_tile.
// The epilogue folds the row sums over the 16 lanes (xor 1, 2, 4, 8: a fixed order), divides, stores O, and stores Stats when
// the pointer is not NULL: a runtime test outside the loop, so there are 18 kernels (KP x DP x BIAS), not 36.
//
// Special values.  e <= 1 and L <= J: the denominator cannot overflow, and the as-written kernel's NaN-for-Inf step is gone.
//   - only finite scores: O is finite whatever their magnitude; some term is expf(0) = 1, so L >= 1;
//   - a -Inf score (a masked key) adds exactly 0;
//   - every key -Inf: m = -Inf, L = 0, O = 0 / 0 = NaN (the rule of the other entries);
//   - a NaN score: O and L NaN, m unspecified (v_max_f32 drops a NaN operand);
//   - a +Inf score: m = +Inf, its term is expf(Inf - Inf) = NaN: O and L NaN;
//   - J == 0: O = 0 (left alone when accumulating), L = 0, m = -Inf.
// No atomics, no workspace: two runs give the same bits.
#include "gemm_plan.hpp"        // batched2_c_distinct
#include "attention.hpp"        // the internal entry
#include "attention_tile.hpp"   // kernel operands, tiles, the MFMA loops, the launcher

#include <cmath>

namespace {

using eg::gemm::f32x4;
using namespace eg::attention;

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

template <int KP, int DP, bool BIAS>
__global__ __launch_bounds__(THREADS) void attention_stable_f32_kernel(std::conditional_t<BIAS, StableBiasArgs, StableArgs> a) {
  constexpr int KS = KP + 4, VS = DP + 16;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const Ks = lds;                      // [64][KS]; the Q tile first
  float* const Vs = Ks + TILE_J * KS;         // [64][VS]
  float* const Es = Vs + TILE_J * VS;         // [4][16][ES]

  const BlockItem b = block_item(a.items);
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
  const long nt = (a.J + TILE_J - 1) / TILE_J;
  if (nt > 0) {
    load_rows<KP>(tk, Kk, ldk, a.J, a.K, a.k.vec != 0, tid);
    load_rows<DP>(tv, V, ldv, a.J, a.D, a.v.vec != 0, tid);
    if constexpr (BIAS) load_bias(bias_next, Bl, ldb, bias_rows, a.J - c);
  }
  for (long t = 0; t < nt; ++t) {
    const long j0 = t * TILE_J;
    __syncthreads();   // every wave is done with the tiles in LDS (the first time: with the Q tile)
    store_rows<KP, KS>(tk, Ks, tid);
    store_rows<DP, VS>(tv, Vs, tid);
    __syncthreads();
    if constexpr (BIAS) bias = bias_next;
    if (t + 1 < nt) {   // in flight during this tile's MFMAs
      load_rows<KP>(tk, Kk + (j0 + TILE_J) * ldk, ldk, a.J - j0 - TILE_J, a.K, a.k.vec != 0, tid);
      load_rows<DP>(tv, V + (j0 + TILE_J) * ldv, ldv, a.J - j0 - TILE_J, a.D, a.v.vec != 0, tid);
      if constexpr (BIAS) load_bias(bias_next, Bl + j0 + TILE_J, ldb, bias_rows, a.J - j0 - TILE_J - c);
    }

    f32x4 s[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) s[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    mma_nt<KP, KS>(q, Ks, c, g, s);

    // the scores, in place; a key outside the problem is -Inf by a select, whatever its score: its term is exactly 0
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      const bool live = j0 + nb * 16 + c < a.J;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x = s[nb][r] * a.scale;
        if constexpr (BIAS) x = x + bias.x[nb][r];
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

namespace eg {
namespace attention {

int attention_stable_check(eg_ctx* ctx, const Extents& e, const float* Q, View q, const float* Kk, View k, const float* V, View v, float* O, View o,
                           int accumulate, float* Stats, View st, const float* Bias, View bv, const char* name, bool* nothing) {
  *nothing = true;
  const long batch0 = e.batch0, batch1 = e.batch1, I = e.I, J = e.J, K = e.K, D = e.D;
  EG_REQUIRE(ctx, EG_ERR_INVALID, "%s: ctx is NULL", name);
  EG_REQUIRE(batch0 >= 0 && batch1 >= 0 && I >= 0 && J >= 0 && K >= 0 && D >= 0, EG_ERR_INVALID, "%s: negative extent", name);
  EG_REQUIRE(batch0 < (1L << 31) && batch1 < (1L << 31), EG_ERR_INVALID, "%s: a batch extent of 2^31 or more", name);
  EG_REQUIRE(q.stride0 >= 0 && q.stride1 >= 0 && k.stride0 >= 0 && k.stride1 >= 0 && v.stride0 >= 0 && v.stride1 >= 0, EG_ERR_INVALID,
             "%s: negative stride", name);
  EG_REQUIRE(!Stats || (st.stride0 >= 0 && st.stride1 >= 0), EG_ERR_INVALID, "%s: negative stride of Stats", name);
  EG_REQUIRE(!Stats || st.ld >= I, EG_ERR_INVALID, "%s: lds is smaller than I", name);
  EG_REQUIRE(!Bias || (bv.stride0 >= 0 && bv.stride1 >= 0), EG_ERR_INVALID, "%s: negative stride of Bias", name);
  EG_REQUIRE(!Bias || bv.ld == 0 || bv.ld >= J, EG_ERR_INVALID, "%s: ldb is neither 0 nor at least J", name);
  if (batch0 == 0 || batch1 == 0 || I == 0 || (D == 0 && !Stats)) return EG_OK;
  EG_REQUIRE(D == 0 || O, EG_ERR_INVALID, "%s: O is NULL", name);
  EG_REQUIRE(J == 0 || D == 0 || V, EG_ERR_INVALID, "%s: NULL operand", name);
  EG_REQUIRE(J == 0 || K == 0 || (Q && Kk), EG_ERR_INVALID, "%s: NULL operand", name);
  EG_REQUIRE(q.ld >= K && k.ld >= K && v.ld >= D, EG_ERR_INVALID, "%s: leading dimension smaller than the row length", name);
  EG_REQUIRE(D == 0 || eg::gemm::batched2_c_distinct(batch0, o.stride0, batch1, o.stride1, I, o.ld, D), EG_ERR_INVALID,
             "%s: ldo, stride_o0 and stride_o1 make elements of O share an address", name);
  // the stats: two rows of I columns per item, lds apart
  EG_REQUIRE(!Stats || eg::gemm::batched2_c_distinct(batch0, st.stride0, batch1, st.stride1, 2, st.ld, I), EG_ERR_INVALID,
             "%s: lds, stride_s0 and stride_s1 make elements of Stats share an address", name);
  EG_REQUIRE(K <= MAX_HEAD, EG_ERR_UNSUPPORTED, "%s: K = %ld is above the limit of %d", name, K, MAX_HEAD);
  EG_REQUIRE(D <= MAX_HEAD, EG_ERR_UNSUPPORTED, "%s: D = %ld is above the limit of %d", name, D, MAX_HEAD);
  if (J == 0 && accumulate && !Stats) return EG_OK;   // an empty sum adds nothing
  *nothing = false;
  return EG_OK;
}

int attention_stable(eg_ctx* ctx, const Extents& e, float scale, const float* Q, View q, const float* Kk, View k, const float* V, View v, float* O,
                     View o, int accumulate, float* Stats, View st, const float* Bias, View bv, const char* entry) {
  const char* const name = entry ? entry : "eg_attention_stable";
  const long batch1 = e.batch1, I = e.I, J = e.J, K = e.K, D = e.D;
  bool nothing = false;
  int rc = attention_stable_check(ctx, e, Q, q, Kk, k, V, v, O, o, accumulate, Stats, st, Bias, bv, name, &nothing);
  if (rc || nothing) return rc;
  rc = eg::set_device(ctx);
  if (rc) return rc;

  Problem pr;
  static_cast<Extents&>(pr) = e;
  pr.q = {q, aligned16(Q)}, pr.k = {k, aligned16(Kk)}, pr.v = {v, aligned16(V)}, pr.o = {o, aligned16(O)};
  pr.sums = Stats != nullptr;   // D == 0 still has the stats to store; the tiles and the cut are eg_attention_sums'
  pr.has_bias = Bias != nullptr;
  pr.bias = {bv, aligned16(Bias)};
  pr.cus = ctx->compute_units;
  const Plan p = plan_attention(pr);
  EG_REQUIRE(p.supported, EG_ERR_UNSUPPORTED, "%s: %s", name, p.reason);

  StableBiasArgs args = {};
  args.q = {Q, q, p.vec_q}, args.k = {Kk, k, p.vec_k}, args.v = {V, v, p.vec_v};
  args.o = {O, o, 0}, args.st = {Stats, st, 0}, args.b = {Bias, bv, p.vec_b};
  args.I = I, args.J = J, args.K = (int)K, args.D = (int)D;
  args.scale = scale;
  args.accumulate = accumulate;
  // 18 kernels: the padded K x the padded D, with and without a bias
  return for_each_launch(name, p.items, p.cut(), batch1, [&](const Items& items, unsigned grid) {
    args.items = items;
    return dispatch_heads(p.kp, p.dp, [&](auto KP, auto DP) {
      constexpr int kp = KP(), dp = DP();
      return Bias ? launch<&attention_stable_f32_kernel<kp, dp, true>, StableBiasArgs, kp, dp>(ctx, grid, p, args)
                  : launch<&attention_stable_f32_kernel<kp, dp, false>, StableArgs, kp, dp>(ctx, grid, p, args);
    });
  });
}

}  // namespace attention
}  // namespace eg

extern "C" int eg_attention_stable(eg_ctx* ctx, int64_t batch0, int64_t batch1, int64_t I, int64_t J, int64_t K, int64_t D, float scale, const float* Q,
                                   int64_t ldq, int64_t stride_q0, int64_t stride_q1, const float* Kk, int64_t ldk, int64_t stride_k0,
                                   int64_t stride_k1, const float* V, int64_t ldv, int64_t stride_v0, int64_t stride_v1, float* O, int64_t ldo,
                                   int64_t stride_o0, int64_t stride_o1, int accumulate, float* Stats, int64_t lds, int64_t stride_s0,
                                   int64_t stride_s1, const float* Bias, int64_t ldb, int64_t stride_b0, int64_t stride_b1) {
  return eg::attention::attention_stable(ctx, {batch0, batch1, I, J, K, D}, scale, Q, {ldq, stride_q0, stride_q1}, Kk, {ldk, stride_k0, stride_k1}, V,
                                         {ldv, stride_v0, stride_v1}, O, {ldo, stride_o0, stride_o1}, accumulate, Stats, {lds, stride_s0, stride_s1}, Bias,
                                         {ldb, stride_b0, stride_b1});
}
