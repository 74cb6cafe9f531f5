// Pattern matching of lowered kernels against the hand-written library (match.cpp).  No HIP header: kernel descriptions only.
#pragma once
#include "kd.hpp"

namespace eg {
namespace model {

using namespace eg::kd;

struct GemmMatch {
  int a_read = 0, b_read = 0;  // indices into k.reads
  bool trans_a = false, trans_b = false;
  int li = 0, lj = 0, lk = 0;  // loop indices of m, n, k
};

struct ConvMatch {
  // which operand plays which part: -1 = the written tensor, 0 / 1 = k.reads[i]
  int out_op = -1, img_op = 0, flt_op = 1;
  bool batched = true;
  enum Role { Forward, GradImage, GradFilter } role = Forward;
};

// A `++=` product with a leading batch index (match_batched_gemm).
//   batched:   write and both reads rank 3, the batch register first in each — one product per g
//              (out[g,i,j] ++= a[g,i,k] * b[g,k,j] and its two derived gradients): trans_a / trans_b as for GemmMatch
//   collapsed: exactly one operand is rank 2 (a weight shared by every g) and the product is a plain one once (g, i) is read
//              as one index of the dense row-major rank-3 tensors:
//                row_k = false: out[g,i,n] ++= a[g,i,k] * w(k,n)   M = G * I, A = a untransposed, trans_b from w
//                row_k = true:  gw[m,n] ++= a[g,i,m] * b[g,i,n]    K = G * I, TN
struct BatchedGemmMatch {
  bool collapsed = false, row_k = false;
  int a_read = 0, b_read = 0;  // indices into k.reads
  bool trans_a = false, trans_b = false;
  int lg = 0, li = 0, lj = 0, lk = 0;  // loop indices of g, m, n, k (collapsed: lg, and li (row_k: lk), are the two collapsed loops)
};

// A `++=` product with two batch indices anywhere but last (match_batched2_gemm): five loops, the write and both reads of
// rank 4 over bare registers.  Two registers are in all three operands (the batch registers), m is in the write and A, n in
// the write and B, k in both reads; every operand ends in one of its two matrix registers, the write in n:
//   s[b,h,i,j] ++= q[b,i,h,k] * kk[b,j,h,k]   NT        o[b,i,h,d] ++= p[b,h,i,j] * v[b,j,h,d]   NN
// trans_a / trans_b as for GemmMatch.  Operands are indexed 0 = A, 1 = B, 2 = the write.
struct Batched2GemmMatch {
  int a_read = 0, b_read = 0;  // indices into k.reads
  bool trans_a = false, trans_b = false;
  int lb[2] = {0, 0};          // loop indices of the batch registers, in the order the write names them
  int li = 0, lj = 0, lk = 0;  // loop indices of m, n, k
  int batch_dim[3][2] = {};    // per operand: the dimensions that lb[0] and lb[1] index
  int row_dim[3] = {};         // per operand: the dimension of its matrix register that is not the last one
};

// The forward attention chain over consecutive live kernels of a target (match_attention.cpp):
//   [0]       scores[b,h,i,j]  ++= q[..] * kk[..]              a product match_batched2_gemm takes as NT
//   [1]       scaled[b,h,i,j]  ++= scores[b,h,i,j] * literal   optional, either operand order; absent: scale 1
//   [n - 3]   sums[b,h,i]      ++= exp(e[b,h,i,j])             e: scaled, or scores without a scale map
//   [n - 2]   softmax[b,h,i,j] ++= exp(e[b,h,i,j]) / sums[b,h,i]
//   [n - 1]   context[..]      ++= softmax[b,h,i,j] * v[..]    a product match_batched2_gemm takes as NN, softmax its A
// with every register of the three middle kernels bare and in the positions of the scores, no loop bounds, and every
// intermediate tensor (scores, scaled, sums, softmax) a Result that exactly one live kernel of the target writes, no live
// kernel outside the chain reads, and that is not the target's output.  (Gradient-bucket membership is the planner's check.)
struct AttentionMatch {
  int n = 0;                           // kernels of the chain: 5 with a scale map, 4 without
  std::vector<int> at;                 // their live positions: p, p + 1, ... (match_attention_chain with gaps: ascending)
  float scale = 1.f;
  double scale_f64 = 1.0;              // the literal as written: what a float64 model multiplies by
  Batched2GemmMatch scores, context;   // of kernels [0] and [n - 1]
  int t_scores = 0, t_scaled = 0, t_sums = 0, t_softmax = 0;   // t_scaled: 0 without a scale map
  int t_q = 0, t_k = 0, t_v = 0, t_out = 0;
};
// The chain at live positions [p, p + m.n) of `t`?  why (optional): the reason of a refusal, a constant string.
bool match_attention(const Program& prog, const Target& t, int p, AttentionMatch& m, const char** why = nullptr);

// The two halves of match_attention, shared with match_attention_fit (match_attention_grad.cpp):
//   the kernels' structure at [p, p + m.n), nothing about who else touches the tensors (gaps: kernels that touch none of the
//   chain's four intermediates may stand between its members — a projection of v between the softmax and the context);
bool match_attention_chain(const Target& t, int p, AttentionMatch& m, const char** why = nullptr, bool gaps = false);
//   and the privacy of tensors: every xs[i] (0: skipped) is a Result, not the target's output, none of `operands`, read by
//   no live kernel outside `members` (live positions; `read_outside` is the refusal's reason) and written by exactly
//   writers[i] live kernels.
bool attention_private(const Program& prog, const Target& t, const std::vector<int>& xs, const std::vector<int>& writers, const std::vector<int>& operands,
                       const std::vector<int>& members, const char* read_outside, const char** why);
// every dimension of `op` a single bare loop register of `k`, all different: those registers
bool bare_regs(const Kernel& k, const Op& op, std::vector<int>& regs);
// `loops` loops without bounds, no setup, no computed indices
bool plain_loops(const Kernel& k, size_t loops);

// A training step over the chain (match_attention_grad.cpp): the forward chain at live position p and the gradient kernels
// that the library's own derive (kd.cpp) makes of it, anywhere behind it in the target —
//   dsoftmax[b,h,i,j] ++= dcontext[..] * v[..]                  NT product          dv[..] ++= softmax[b,h,i,j] * dcontext[..]
//   de[b,h,i,j]       ++= dsoftmax / sums * exp(e)              map                 dsums[b,h,i] ++= -exp(e) * (dsoftmax / (sums * sums))
//   de[b,h,i,j]       ++= dsums[b,h,i] * exp(e)                 map                 dscores[b,h,i,j] ++= de[b,h,i,j] * literal (with a scale map)
//   dq[..]            ++= dscores[b,h,i,j] * kk[..]             product             dk[..] ++= dscores[b,h,i,j] * q[..]
// — eight with a scale map, seven without: what eg_attention_sums and eg_attention_grad compute in three launches.  Found by
// the tensors they read and write, held to the registers' positions that the forward products fix and to the instructions
// derive emits; where derive recorded a kernel's origin (Kernel::derived_from) that has to agree too.  The scores, the scaled
// scores, the softmax and the four gradients between the products are `hidden`: Results that the members alone read and
// write and that are not the target's output.  The sums and the context are ordinary tensors: the backward reads them.
struct AttentionFitMatch {
  AttentionMatch fwd;
  int t_do = 0, t_dq = 0, t_dk = 0, t_dv = 0;
  int t_dsoftmax = 0, t_dsums = 0, t_de = 0, t_dscores = 0;   // without a scale map de is dscores: t_de == t_dscores
  // live positions of the gradient kernels, in the order above (dscale: -1 without a scale map)
  int p_dsoftmax = -1, p_dv = -1, p_de = -1, p_dsums = -1, p_de_sums = -1, p_dscale = -1, p_dq = -1, p_dk = -1;
  Batched2GemmMatch dsoftmax, dv, dq, dk;
  std::vector<int> forward, backward;   // live positions of the members, ascending
  std::vector<int> hidden;
};
bool match_attention_fit(const Program& prog, const Target& t, int p, AttentionFitMatch& m, const char** why = nullptr);

bool bare2(const Op& op, int& r0, int& r1);
int loop_index(const Kernel& k, int reg);
bool match_gemm(const Kernel& k, GemmMatch& m);
bool match_batched_gemm(const Kernel& k, BatchedGemmMatch& m);
bool match_batched2_gemm(const Kernel& k, Batched2GemmMatch& m);
bool match_bias(const Kernel& k, int tensor);
bool match_conv(const Kernel& k, ConvMatch& m);

}  // namespace model
}  // namespace eg
