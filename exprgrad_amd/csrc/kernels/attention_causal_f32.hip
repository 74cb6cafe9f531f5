// Causal attention forward (eg_attention_causal): eg_attention_stable where key j is visible to query row i iff j <= i + offset,
// on the kernel of attention_stable_f32.hpp under CAUSAL.  A causal mask as a Bias table of -Inf is computed tile by tile and
// adds zeros; here the block of rows [i0, i0 + 64) walks only the key tiles that hold a visible key (causal_key_tiles,
// attention_plan.hpp), takes the unmasked kernel's path on the interior ones and cuts the one or two on the diagonal with a
// lane-local select.  With I = J and offset = 0 that is tiles_i (tiles_i + 1) / 2 of tiles_i^2 tile visits, the diagonal
// included.  The tiles are walked in ascending order with the products and sums of the unmasked kernel, a masked term is
// exactly 0 and a skipped tile adds zeros: O and Stats have the bits of eg_attention_stable on a Bias of -Inf where
// j > i + offset (finite V).  The 18 instantiations live here so that they compile beside attention_stable_f32.hip's, and that
// file's kernels stay the ones they were.
#include "attention.hpp"              // the internal entry
#include "attention_stable_f32.hpp"   // the kernel template and its launch

namespace eg {
namespace attention {

// attention_stable (attention_stable_f32.hip) has made and checked the plan and filled the arguments.
int launch_stable_causal(eg_ctx* ctx, unsigned grid, const Plan& p, const StableCausalArgs& args) {
  return dispatch_heads(p.kp, p.dp, [&](auto KP, auto DP) {
    constexpr int kp = KP(), dp = DP();
    return args.b.p ? launch<&attention_stable_f32_kernel<kp, dp, true, true>, StableCausalArgs, kp, dp>(ctx, grid, p, args)
                    : launch<&attention_stable_f32_kernel<kp, dp, false, true>, StableCausalArgs, kp, dp>(ctx, grid, p, args);
  });
}

}  // namespace attention
}  // namespace eg

extern "C" int eg_attention_causal(eg_ctx* ctx, int64_t batch0, int64_t batch1, int64_t I, int64_t J, int64_t K, int64_t D, float scale, const float* Q,
                                   int64_t ldq, int64_t stride_q0, int64_t stride_q1, const float* Kk, int64_t ldk, int64_t stride_k0,
                                   int64_t stride_k1, const float* V, int64_t ldv, int64_t stride_v0, int64_t stride_v1, float* O, int64_t ldo,
                                   int64_t stride_o0, int64_t stride_o1, int accumulate, float* Stats, int64_t lds, int64_t stride_s0,
                                   int64_t stride_s1, const float* Bias, int64_t ldb, int64_t stride_b0, int64_t stride_b1, int64_t offset) {
  EG_REQUIRE(offset >= 0, EG_ERR_INVALID, "eg_attention_causal: offset is negative: the first rows would see no key");
  return eg::attention::attention_stable(ctx, {batch0, batch1, I, J, K, D}, scale, Q, {ldq, stride_q0, stride_q1}, Kk, {ldk, stride_k0, stride_k1}, V,
                                         {ldv, stride_v0, stride_v1}, O, {ldo, stride_o0, stride_o1}, accumulate, Stats, {lds, stride_s0, stride_s1}, Bias,
                                         {ldb, stride_b0, stride_b1}, "eg_attention_causal", offset);
}
