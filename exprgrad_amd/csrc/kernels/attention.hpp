// The fused attention kernels' internal entries: what the C ABI (eg_attention, eg_attention_sums, eg_attention_grad) and
// the model layer's attention launches (host/run.cpp) call.  Every operand is a pointer to item (0, 0) and its View
// (attention_plan.hpp); the row sums' view has no leading dimension.
#pragma once

#include "../eg_internal.hpp"
#include "attention_plan.hpp"

namespace eg {
namespace attention {

// The forward over batch0 x batch1 items (attention_f32.hip).  With Sums the row sums are stored too, one row of I floats
// per item: the forward launch of the model layer's fit route (host/plan_attention.cpp, form_attention_fit_groups).
int attention_forward(eg_ctx* ctx, const Extents& e, float scale, const float* Q, View q, const float* Kk, View k, const float* V, View v, float* O,
                      View o, int accumulate, float* Sums = nullptr, View s = {});

// The float64 forward (attention_f64.hip): eg_attention_f64, eg_attention_sums_f64 and the attention launches of a float64
// model under eg_model_fuse_attention_f64.  The same contract in doubles; the scale is a double end to end.
int attention_forward_f64(eg_ctx* ctx, const Extents& e, double scale, const double* Q, View q, const double* Kk, View k, const double* V, View v,
                          double* O, View o, int accumulate, double* Sums = nullptr, View s = {});

// The backward over what that launch left (attention_grad_f32.hip); accumulate: bits 1 (dQ), 2 (dK) and 4 (dV).
int attention_grad(eg_ctx* ctx, const Extents& e, float scale, const float* Q, View q, const float* Kk, View k, const float* V, View v,
                   const float* O, View o, const float* Sums, View s, const float* dO, View dout, float* dQ, View dq, float* dK, View dk, float* dV,
                   View dv, int accumulate);

}  // namespace attention
}  // namespace eg
