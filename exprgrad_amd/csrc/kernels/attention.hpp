// The fused attention kernels' internal entries: what the C ABI (eg_attention, eg_attention_sums, eg_attention_grad and their _f64 forms) and
// the model layer's attention launches (host/run.cpp) call.  Every operand is a pointer to item (0, 0) and its View
// (attention_plan.hpp); the row sums' view has no leading dimension.
#pragma once

#include "../eg_internal.hpp"
#include "attention_plan.hpp"

namespace eg {
namespace attention {

// The forward over batch0 x batch1 items (attention_f32.hip).  With Sums the row sums are stored too, one row of I floats
// per item: the forward launch of the model layer's fit route (host/plan_attention.cpp, form_attention_fit_groups).  With Bias
// e_ij = expf(scale * s_ij + Bias[i * bv.ld + j]): eg_attention_bias and a model's biased chain; bv.ld and both strides may
// each be 0, and `entry` is the name the messages speak of.  A NULL Bias is the call without one.
int attention_forward(eg_ctx* ctx, const Extents& e, float scale, const float* Q, View q, const float* Kk, View k, const float* V, View v, float* O,
                      View o, int accumulate, float* Sums = nullptr, View s = {}, const float* Bias = nullptr, View bv = {},
                      const char* entry = nullptr);

// The float64 forward (attention_f64.hip): eg_attention_f64, eg_attention_sums_f64 and the attention launches of a float64
// model under eg_model_fuse_attention_f64.  The same contract in doubles; the scale is a double end to end.
int attention_forward_f64(eg_ctx* ctx, const Extents& e, double scale, const double* Q, View q, const double* Kk, View k, const double* V, View v,
                          double* O, View o, int accumulate, double* Sums = nullptr, View s = {});

// The backward over what that launch left (attention_grad_f32.hip); accumulate: bits 1 (dQ), 2 (dK) and 4 (dV).  With Bias
// (eg_attention_bias_grad) the probabilities are those of the biased forward; no gradient of the bias is produced.
int attention_grad(eg_ctx* ctx, const Extents& e, float scale, const float* Q, View q, const float* Kk, View k, const float* V, View v,
                   const float* O, View o, const float* Sums, View s, const float* dO, View dout, float* dQ, View dq, float* dK, View dk, float* dV,
                   View dv, int accumulate, const float* Bias = nullptr, View bv = {}, const char* entry = nullptr, bool stable = false,
                   long causal_offset = -1);

// The forward with a running row maximum (attention_stable_f32.hip): eg_attention_stable and a model's forward attention
// launches under eg_model_fuse_attention_stable.  e_ij = expf(x_ij - m_i); Stats, when not NULL, takes two rows of I floats per
// item, st.ld apart: the maxima m and the sums L.  Its backward is attention_grad with `stable`, Sums that Stats and s its view
// (s.ld the step between the two rows): p_ij = expf(x_ij - m_i) / L_i, the STABLE kernels of attention_grad_stable_f32.hip.
// causal_offset >= 0 (eg_attention_causal, attention_causal_f32.hip): key j is visible to row i iff j <= i + causal_offset, and
// key tiles without a visible key are not visited; the same bits as a Bias of -Inf there.  attention_grad takes the same offset.
int attention_stable(eg_ctx* ctx, const Extents& e, float scale, const float* Q, View q, const float* Kk, View k, const float* V, View v, float* O,
                     View o, int accumulate, float* Stats = nullptr, View st = {}, const float* Bias = nullptr, View bv = {},
                     const char* entry = nullptr, long causal_offset = -1);
// What that entry refuses, under the name `name`; *nothing: valid, and nothing to compute or store.
int attention_stable_check(eg_ctx* ctx, const Extents& e, const float* Q, View q, const float* Kk, View k, const float* V, View v, float* O, View o,
                           int accumulate, float* Stats, View st, const float* Bias, View bv, const char* name, bool* nothing);

// The same forward split over the keys (attention_split_f32.hip, eg_attention_stable_split): `splits` blocks per item and row
// tile leave partial results in the context's workspace and one more launch combines them; up to 16 query rows the four waves
// of a block split the keys of a tile.  splits == 0: plan_attention_split chooses.  Stats serve attention_grad with `stable`.
int attention_stable_split(eg_ctx* ctx, const Extents& e, float scale, const float* Q, View q, const float* Kk, View k, const float* V, View v,
                           float* O, View o, int accumulate, float* Stats, View st, const float* Bias, View bv, int splits);

// The causal forward cut into chunks of key tiles (attention_causal_split_f32.hip, eg_attention_causal_split): every 64-row tile's
// visible key tiles go to ceil(n / chunk) blocks; a row tile with one piece is finished by its block with attention_stable's
// causal bits, the others through the workspace and a combine launch.  chunk == 0: plan_attention_causal_split chooses.
int attention_causal_split(eg_ctx* ctx, const Extents& e, float scale, const float* Q, View q, const float* Kk, View k, const float* V, View v,
                           float* O, View o, int accumulate, float* Stats, View st, const float* Bias, View bv, long offset, int chunk);

// The gradient of that bias (attention_dbias_f32.hip): eg_attention_bias_dbias, over what attention_forward left with Sums and
// the same Bias.  dBias (+)= the sum of p * (dP - delta) over every index whose step in `db` is 0; db.ld and both its strides
// are 0 exactly where bv's are.
int attention_dbias(eg_ctx* ctx, const Extents& e, float scale, const float* Q, View q, const float* Kk, View k, const float* V, View v,
                    const float* O, View o, const float* Sums, View s, const float* dO, View dout, const float* Bias, View bv, float* dBias,
                    View db, int accumulate);

// The float64 backward (attention_grad_f64.hip): eg_attention_grad_f64, over what attention_forward_f64 left with Sums.
int attention_grad_f64(eg_ctx* ctx, const Extents& e, double scale, const double* Q, View q, const double* Kk, View k, const double* V, View v,
                       const double* O, View o, const double* Sums, View s, const double* dO, View dout, double* dQ, View dq, double* dK, View dk,
                       double* dV, View dv, int accumulate);

}  // namespace attention
}  // namespace eg
