// The backward of eg_attention_stable (eg_attention_stable_grad): the two kernels of attention_grad_f32.hpp under STABLE,
//   p_ij = expf(x_ij - m_i) / L_i,   x_ij = scale * q_i . k_j (+ bias_ij),   (m, L) the forward's Stats,
// and everything else eg_attention_grad's: delta, dP, dS, the three sums, the tiles, the look-ahead, the way out through LDS.
// Their instantiations, with and without BIAS, live here so that they compile beside attention_grad_f32.hip's, and that
// file's kernels stay the ones they were.  A row whose L is 0 or whose stats are not finite is NaN and poisons dK and dV, as
// in eg_attention_bias_grad: a fully masked row has m = -Inf, L = 0 and p = expf(x + Inf) * Inf.
#include "attention_grad_f32.hpp"

namespace eg {
namespace attention {

// attention_grad (attention_grad_f32.hip) has made and checked the plan and filled the arguments.
int launch_grad_stable(eg_ctx* ctx, bool dkv, unsigned grid, const GradPlan& p, const GradBiasArgs& args) {
  return dispatch_heads(p.kp, p.dp, [&](auto KP, auto DP) {
    constexpr int kp = KP(), dp = DP();
    return args.b.p ? launch<&attention_dq_kernel<kp, dp, true, true>, &attention_dkv_kernel<kp, dp, true, true>, GradBiasArgs, kp, dp, true>(
                          ctx, dkv, grid, p, args)
                    : launch<&attention_dq_kernel<kp, dp, false, true>, &attention_dkv_kernel<kp, dp, false, true>, GradBiasArgs, kp, dp, true>(
                          ctx, dkv, grid, p, args);
  });
}

}  // namespace attention
}  // namespace eg
