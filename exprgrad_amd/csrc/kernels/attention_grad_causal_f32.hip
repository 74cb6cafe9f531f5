// The backward of eg_attention_causal (eg_attention_causal_grad): the two kernels of attention_grad_f32.hpp under STABLE and
// CAUSAL, without a score bias.  The dQ kernel walks the key tiles the forward walked; the dK/dV kernel starts at the first row tile
// that sees its keys; both cut the diagonal tiles with a lane-local select where the bias is added.  Ascending tiles, the same
// products and sums: dQ, dK and dV have the bits of eg_attention_stable_grad on a Bias of -Inf where j > i + offset (finite
// operands).  The 18 instantiations with a bias are attention_grad_causal_bias_f32.hip's: two units
// that compile side by side.
#include "attention_grad_f32.hpp"

namespace eg {
namespace attention {

// attention_grad (attention_grad_f32.hip) has made and checked the plan and filled the arguments.
int launch_grad_causal(eg_ctx* ctx, bool dkv, unsigned grid, const GradPlan& p, const GradCausalArgs& args) {
  return dispatch_heads(p.kp, p.dp, [&](auto KP, auto DP) {
    constexpr int kp = KP(), dp = DP();
    return launch<&attention_dq_kernel<kp, dp, false, true, true>, &attention_dkv_kernel<kp, dp, false, true, true>, GradCausalArgs, kp, dp, true>(ctx, dkv, grid,
                                                                                                                                           p, args);
  });
}

}  // namespace attention
}  // namespace eg
