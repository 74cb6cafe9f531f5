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
//
// The kernels themselves are templates in attention_grad_f32.hpp; this file instantiates them for eg_attention_grad and
// eg_attention_bias_grad, attention_grad_stable_f32.hip for eg_attention_stable_grad, and attention_grad_causal_f32.hip and
// attention_grad_causal_bias_f32.hip for eg_attention_causal_grad.
#include "gemm_plan.hpp"        // batched2_c_distinct
#include "attention.hpp"        // the internal entry
#include "attention_grad_f32.hpp"   // the two kernels and their launch

namespace eg {
namespace attention {

int attention_grad(eg_ctx* ctx, const Extents& e, float scale, const float* Q, View q, const float* Kk, View k, const float* V, View v,
                   const float* O, View o, const float* Sums, View s, const float* dO, View dout, float* dQ, View dq, float* dK, View dk, float* dV,
                   View dv, int accumulate, const float* Bias, View bv, const char* entry, bool stable, long causal_offset) {
  const bool causal = causal_offset >= 0;   // eg_attention_causal_grad, which is `stable` too
  const char* const name = entry ? entry : "eg_attention_grad";   // the entry the messages speak of
  const long batch0 = e.batch0, batch1 = e.batch1, I = e.I, J = e.J, K = e.K, D = e.D;
  EG_REQUIRE(ctx, EG_ERR_INVALID, "%s: ctx is NULL", name);
  EG_REQUIRE(batch0 >= 0 && batch1 >= 0 && I >= 0 && J >= 0 && K >= 0 && D >= 0, EG_ERR_INVALID, "%s: negative extent", name);
  EG_REQUIRE(batch0 < (1L << 31) && batch1 < (1L << 31), EG_ERR_INVALID, "%s: a batch extent of 2^31 or more", name);
  EG_REQUIRE(q.stride0 >= 0 && q.stride1 >= 0 && k.stride0 >= 0 && k.stride1 >= 0 && v.stride0 >= 0 && v.stride1 >= 0 && o.stride0 >= 0 &&
                 o.stride1 >= 0 && s.stride0 >= 0 && s.stride1 >= 0 && dout.stride0 >= 0 && dout.stride1 >= 0,
             EG_ERR_INVALID, "%s: negative stride", name);
  EG_REQUIRE(!Bias || (bv.stride0 >= 0 && bv.stride1 >= 0), EG_ERR_INVALID, "%s: negative stride of Bias", name);
  EG_REQUIRE(!Bias || bv.ld == 0 || bv.ld >= J, EG_ERR_INVALID, "%s: ldb is neither 0 nor at least J", name);
  // eg_attention_stable_grad: s is the view of the forward's Stats, two rows of I floats, s.ld apart
  EG_REQUIRE(!stable || s.ld >= I, EG_ERR_INVALID, "%s: lds is smaller than I", name);
  EG_REQUIRE(!stable || eg::gemm::batched2_c_distinct(batch0, s.stride0, batch1, s.stride1, 2, s.ld, I), EG_ERR_INVALID,
             "%s: lds, stride_s0 and stride_s1 make elements of Stats share an address", name);
  EG_REQUIRE((accumulate & ~7) == 0, EG_ERR_INVALID, "%s: accumulate has bits other than 1 (dQ), 2 (dK) and 4 (dV)", name);
  if (batch0 == 0 || batch1 == 0) return EG_OK;
  const bool want_dq = I > 0 && K > 0, want_dk = J > 0 && K > 0, want_dv = J > 0 && D > 0;   // the outputs that have elements
  if (!want_dq && !want_dk && !want_dv) return EG_OK;
  EG_REQUIRE((!want_dq || dQ) && (!want_dk || dK) && (!want_dv || dV), EG_ERR_INVALID, "%s: NULL output", name);
  if (I > 0 && J > 0) {
    EG_REQUIRE(Sums, EG_ERR_INVALID, "%s: NULL operand (%s)", name, stable ? "Stats" : "Sums");
    EG_REQUIRE(K == 0 || (Q && Kk), EG_ERR_INVALID, "%s: NULL operand (Q or Kk)", name);
    EG_REQUIRE(D == 0 || (V && O && dO), EG_ERR_INVALID, "%s: NULL operand (V, O or dO)", name);
  }
  EG_REQUIRE(q.ld >= K && k.ld >= K && dq.ld >= K && dk.ld >= K && v.ld >= D && o.ld >= D && dout.ld >= D && dv.ld >= D, EG_ERR_INVALID,
             "%s: leading dimension smaller than the row length", name);
  EG_REQUIRE(!want_dq || eg::gemm::batched2_c_distinct(batch0, dq.stride0, batch1, dq.stride1, I, dq.ld, K), EG_ERR_INVALID,
             "%s: lddq, stride_dq0 and stride_dq1 make elements of dQ share an address", name);
  EG_REQUIRE(!want_dk || eg::gemm::batched2_c_distinct(batch0, dk.stride0, batch1, dk.stride1, J, dk.ld, K), EG_ERR_INVALID,
             "%s: lddk, stride_dk0 and stride_dk1 make elements of dK share an address", name);
  EG_REQUIRE(!want_dv || eg::gemm::batched2_c_distinct(batch0, dv.stride0, batch1, dv.stride1, J, dv.ld, D), EG_ERR_INVALID,
             "%s: lddv, stride_dv0 and stride_dv1 make elements of dV share an address", name);
  EG_REQUIRE(K <= MAX_HEAD, EG_ERR_UNSUPPORTED, "%s: K = %ld is above the limit of %d", name, K, MAX_HEAD);
  EG_REQUIRE(D <= MAX_HEAD, EG_ERR_UNSUPPORTED, "%s: D = %ld is above the limit of %d", name, D, MAX_HEAD);

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
  pr.has_bias = Bias != nullptr;
  pr.bias = {bv, aligned16(Bias)};
  pr.stable = stable;
  pr.cus = ctx->compute_units;
  const GradPlan p = plan_attention_grad(pr);
  EG_REQUIRE(p.supported, EG_ERR_UNSUPPORTED, "%s: %s", name, p.reason);

  GradCausalArgs args = {};
  args.offset = causal_offset < J ? causal_offset : J;   // an offset of J - 1 or more masks nothing
  args.q = {Q, q, p.vec_q}, args.k = {Kk, k, p.vec_k}, args.v = {V, v, p.vec_v}, args.o = {O, o, p.vec_o}, args.s = {Sums, s, p.vec_s};
  args.dout = {dO, dout, p.vec_do}, args.dq = {dQ, dq, p.vec_dq}, args.dk = {dK, dk, p.vec_dk}, args.dv = {dV, dv, p.vec_dv};
  args.b = {Bias, bv, p.vec_b};
  args.I = I, args.J = J, args.K = (int)K, args.D = (int)D;
  args.scale = scale;
  args.acc_dq = acc_dq, args.acc_dk = acc_dk, args.acc_dv = acc_dv;
  args.put_dk = put_dk, args.put_dv = put_dv;
  // 9 instantiations of each kernel: the padded K x the padded D; as many again that add the bias
  auto run = [&](bool dkv, const GradKernel& kernel) {
    return for_each_launch(name, p.items, kernel, batch1, [&](const Items& items, unsigned grid) {
      args.items = items;
      return dispatch_heads(p.kp, p.dp, [&](auto KP, auto DP) {
        constexpr int kp = KP(), dp = DP();
        if (causal) return Bias ? launch_grad_causal_bias(ctx, dkv, grid, p, args) : launch_grad_causal(ctx, dkv, grid, p, args);
        if (stable) return launch_grad_stable(ctx, dkv, grid, p, args);
        return Bias ? launch<&attention_dq_kernel<kp, dp, true>, &attention_dkv_kernel<kp, dp, true>, GradBiasArgs, kp, dp>(ctx, dkv, grid, p, args)
                    : launch<&attention_dq_kernel<kp, dp, false>, &attention_dkv_kernel<kp, dp, false>, GradArgs, kp, dp>(ctx, dkv, grid, p, args);
      });
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

extern "C" int eg_attention_bias_grad(eg_ctx* ctx, int64_t batch0, int64_t batch1, int64_t I, int64_t J, int64_t K, int64_t D, float scale,
                                      const float* Q, int64_t ldq, int64_t stride_q0, int64_t stride_q1,
                                      const float* Kk, int64_t ldk, int64_t stride_k0, int64_t stride_k1,
                                      const float* V, int64_t ldv, int64_t stride_v0, int64_t stride_v1,
                                      const float* O, int64_t ldo, int64_t stride_o0, int64_t stride_o1,
                                      const float* Sums, int64_t stride_s0, int64_t stride_s1,
                                      const float* dO, int64_t lddo, int64_t stride_do0, int64_t stride_do1,
                                      float* dQ, int64_t lddq, int64_t stride_dq0, int64_t stride_dq1,
                                      float* dK, int64_t lddk, int64_t stride_dk0, int64_t stride_dk1,
                                      float* dV, int64_t lddv, int64_t stride_dv0, int64_t stride_dv1, int accumulate,
                                      const float* Bias, int64_t ldb, int64_t stride_b0, int64_t stride_b1) {
  return eg::attention::attention_grad(ctx, {batch0, batch1, I, J, K, D}, scale, Q, {ldq, stride_q0, stride_q1}, Kk, {ldk, stride_k0, stride_k1}, V,
                                       {ldv, stride_v0, stride_v1}, O, {ldo, stride_o0, stride_o1}, Sums, {0, stride_s0, stride_s1}, dO,
                                       {lddo, stride_do0, stride_do1}, dQ, {lddq, stride_dq0, stride_dq1}, dK, {lddk, stride_dk0, stride_dk1}, dV,
                                       {lddv, stride_dv0, stride_dv1}, accumulate, Bias, {ldb, stride_b0, stride_b1}, "eg_attention_bias_grad");
}

extern "C" int eg_attention_stable_grad(eg_ctx* ctx, int64_t batch0, int64_t batch1, int64_t I, int64_t J, int64_t K, int64_t D, float scale,
                                        const float* Q, int64_t ldq, int64_t stride_q0, int64_t stride_q1,
                                        const float* Kk, int64_t ldk, int64_t stride_k0, int64_t stride_k1,
                                        const float* V, int64_t ldv, int64_t stride_v0, int64_t stride_v1,
                                        const float* O, int64_t ldo, int64_t stride_o0, int64_t stride_o1,
                                        const float* Stats, int64_t lds, int64_t stride_s0, int64_t stride_s1,
                                        const float* dO, int64_t lddo, int64_t stride_do0, int64_t stride_do1,
                                        float* dQ, int64_t lddq, int64_t stride_dq0, int64_t stride_dq1,
                                        float* dK, int64_t lddk, int64_t stride_dk0, int64_t stride_dk1,
                                        float* dV, int64_t lddv, int64_t stride_dv0, int64_t stride_dv1, int accumulate,
                                        const float* Bias, int64_t ldb, int64_t stride_b0, int64_t stride_b1) {
  return eg::attention::attention_grad(ctx, {batch0, batch1, I, J, K, D}, scale, Q, {ldq, stride_q0, stride_q1}, Kk, {ldk, stride_k0, stride_k1}, V,
                                       {ldv, stride_v0, stride_v1}, O, {ldo, stride_o0, stride_o1}, Stats, {lds, stride_s0, stride_s1}, dO,
                                       {lddo, stride_do0, stride_do1}, dQ, {lddq, stride_dq0, stride_dq1}, dK, {lddk, stride_dk0, stride_dk1}, dV,
                                       {lddv, stride_dv0, stride_dv1}, accumulate, Bias, {ldb, stride_b0, stride_b1}, "eg_attention_stable_grad",
                                       true);
}

extern "C" int eg_attention_causal_grad(eg_ctx* ctx, int64_t batch0, int64_t batch1, int64_t I, int64_t J, int64_t K, int64_t D, float scale,
                                        const float* Q, int64_t ldq, int64_t stride_q0, int64_t stride_q1,
                                        const float* Kk, int64_t ldk, int64_t stride_k0, int64_t stride_k1,
                                        const float* V, int64_t ldv, int64_t stride_v0, int64_t stride_v1,
                                        const float* O, int64_t ldo, int64_t stride_o0, int64_t stride_o1,
                                        const float* Stats, int64_t lds, int64_t stride_s0, int64_t stride_s1,
                                        const float* dO, int64_t lddo, int64_t stride_do0, int64_t stride_do1,
                                        float* dQ, int64_t lddq, int64_t stride_dq0, int64_t stride_dq1,
                                        float* dK, int64_t lddk, int64_t stride_dk0, int64_t stride_dk1,
                                        float* dV, int64_t lddv, int64_t stride_dv0, int64_t stride_dv1, int accumulate,
                                        const float* Bias, int64_t ldb, int64_t stride_b0, int64_t stride_b1, int64_t offset) {
  EG_REQUIRE(offset >= 0, EG_ERR_INVALID, "eg_attention_causal_grad: offset is negative: the first rows would see no key");
  return eg::attention::attention_grad(ctx, {batch0, batch1, I, J, K, D}, scale, Q, {ldq, stride_q0, stride_q1}, Kk, {ldk, stride_k0, stride_k1}, V,
                                       {ldv, stride_v0, stride_v1}, O, {ldo, stride_o0, stride_o1}, Stats, {lds, stride_s0, stride_s1}, dO,
                                       {lddo, stride_do0, stride_do1}, dQ, {lddq, stride_dq0, stride_dq1}, dK, {lddk, stride_dk0, stride_dk1}, dV,
                                       {lddv, stride_dv0, stride_dv1}, accumulate, Bias, {ldb, stride_b0, stride_b1}, "eg_attention_causal_grad",
                                       true, offset);
}
