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
#include "attention_stable_f32.hpp"   // the kernel template and its launch

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
                     View o, int accumulate, float* Stats, View st, const float* Bias, View bv, const char* entry, long causal_offset) {
  const char* const name = entry ? entry : "eg_attention_stable";
  const bool causal = causal_offset >= 0;
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

  StableCausalArgs args = {};
  args.offset = causal_offset < J ? causal_offset : J;   // an offset of J - 1 or more masks nothing
  args.q = {Q, q, p.vec_q}, args.k = {Kk, k, p.vec_k}, args.v = {V, v, p.vec_v};
  args.o = {O, o, 0}, args.st = {Stats, st, 0}, args.b = {Bias, bv, p.vec_b};
  args.I = I, args.J = J, args.K = (int)K, args.D = (int)D;
  args.scale = scale;
  args.accumulate = accumulate;
  // 18 kernels: the padded K x the padded D, with and without a bias; 18 more that are CAUSAL
  return for_each_launch(name, p.items, p.cut(), batch1, [&](const Items& items, unsigned grid) {
    args.items = items;
    if (causal) return launch_stable_causal(ctx, grid, p, args);
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
