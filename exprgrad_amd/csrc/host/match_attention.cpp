// The forward attention chain (match.hpp, AttentionMatch): scores product, optional scale by a literal, row sum of exp,
// exp / sums, context product — what eg_attention (kernels/attention_f32.hip) computes in one launch.  Structure only:
// shapes, loop extents and the switches are the planner's business (plan_groups.cpp, form_attention_groups).
// Refused, each with its reason: a mask (`select`), bounded column loops, a transposed row operand, rank 3 or 5 (the
// products then do not match), a scale by a tensor or by division, a softmax or scores tensor with a second consumer or that
// is the target's output — which includes every `fit` target, whose gradient kernels read them.
#include "match.hpp"

#include <vector>

namespace eg {
namespace model {

// every dimension a single bare register, all different, each a loop register
bool bare_regs(const Kernel& k, const Op& op, std::vector<int>& regs) {
  regs.clear();
  if (op.raw) return false;
  for (auto& d : op.dims) {
    const int r = d.only_register();
    if (!r || loop_index(k, r) < 0) return false;
    for (int s : regs)
      if (s == r) return false;
    regs.push_back(r);
  }
  return true;
}

// `loops` unbounded loops, no setup, no computed indices
bool plain_loops(const Kernel& k, size_t loops) {
  if (!k.index_instrs.empty() || !k.setup.empty() || k.loops.size() != loops) return false;
  for (auto& lp : k.loops)
    if (lp.has_bounds) return false;
  return true;
}

namespace {

// a map or a row sum over the scores
bool plain_rank4(const Kernel& k) { return plain_loops(k, 4); }

bool fail(const char** why, const char* reason) {
  if (why) *why = reason;
  return false;
}

}  // namespace

bool match_attention_chain(const Target& t, int p, AttentionMatch& out, const char** why, bool gaps) {
  const int n_live = (int)t.live.size();
  if (p < 0 || p + 4 > n_live) return fail(why, "fewer than four kernels");
  AttentionMatch m;
  auto kernel = [&](int q) -> const Kernel& { return t.all[t.live[q]]; };

  // [0] the scores
  const Kernel& k0 = kernel(p);
  if (!match_batched2_gemm(k0, m.scores) || m.scores.trans_a || !m.scores.trans_b) return fail(why, "the first kernel is not an NT product with two batch indices");
  for (int q = 0; q < 2; ++q)
    if (m.scores.batch_dim[2][q] > 1) return fail(why, "the scores do not lead with their batch indices");
  if (m.scores.row_dim[2] != 2) return fail(why, "the scores do not lead with their batch indices");
  m.t_scores = k0.write.tensor;
  m.t_q = k0.reads[m.scores.a_read].tensor;
  m.t_k = k0.reads[m.scores.b_read].tensor;
  m.at.push_back(p);
  const char* const ends = "the chain ends behind the target's last kernel";
  // gaps: the next member from `from` on, over kernels that touch none of the chain's tensors
  auto next = [&](int from) {
    while (gaps && from < n_live) {
      const Kernel& k = kernel(from);
      bool touches = false;
      for (int x : {m.t_scores, m.t_scaled, m.t_sums, m.t_softmax}) {
        if (!x) continue;
        touches = touches || k.write.tensor == x;
        for (auto& rd : k.reads) touches = touches || rd.tensor == x;
      }
      if (touches) break;
      ++from;
    }
    return from;
  };

  // [1] the optional scale map: scaled = scores * literal, either order
  int at = next(p + 1);
  if (at >= n_live) return fail(why, ends);
  int e = m.t_scores;   // what the softmax reads
  {
    const Kernel& k = kernel(at);
    std::vector<int> r, w;
    const bool map_shape = plain_rank4(k) && k.reads.size() == 1 && k.reads[0].tensor == m.t_scores && bare_regs(k, k.reads[0], r) &&
                           bare_regs(k, k.write, w) && r.size() == 4 && r == w;
    const bool is_sum = k.write.dims.size() == 3;
    if (!is_sum) {
      if (!map_shape) return fail(why, "the kernel behind the scores is neither a scale map over them nor the row sum");
      if (k.instrs.size() != 2) return fail(why, "the scale is not one multiplication by a literal");
      const Instr* lit = nullptr;
      const Instr* mul = nullptr;
      for (auto& ins : k.instrs) {
        if (ins.kind == IK::Scalar) lit = &ins;
        if (ins.kind == IK::Mul) mul = &ins;
      }
      if (!lit || !mul || mul->args.size() != 2 || k.result != mul->res) return fail(why, "the scale is not one multiplication by a literal");
      const int x = k.reads[0].reg;
      if (!((mul->args[0] == x && mul->args[1] == lit->res) || (mul->args[1] == x && mul->args[0] == lit->res)))
        return fail(why, "the scale is not one multiplication by a literal");
      m.scale = (float)lit->lit;
      m.scale_f64 = lit->lit;
      m.t_scaled = k.write.tensor;
      e = m.t_scaled;
      m.at.push_back(at);
      at = next(at + 1);
    }
  }
  if (at >= n_live || (!gaps && at + 3 > n_live)) return fail(why, ends);

  // [n - 3] the row sum of exp over the last axis
  {
    const Kernel& k = kernel(at);
    std::vector<int> r, w;
    if (!plain_rank4(k)) return fail(why, "the row sum has loop bounds, computed indices or another rank");
    if (k.reads.size() != 1 || k.reads[0].tensor != e || !bare_regs(k, k.reads[0], r) || r.size() != 4) return fail(why, "the row sum does not read the scaled scores alone");
    if (k.instrs.size() != 1 || k.instrs[0].kind != IK::Exp || k.instrs[0].args.size() != 1 || k.instrs[0].args[0] != k.reads[0].reg ||
        k.result != k.instrs[0].res)
      return fail(why, "the row sum is not a sum of exp alone");
    if (!bare_regs(k, k.write, w) || w.size() != 3 || w[0] != r[0] || w[1] != r[1] || w[2] != r[2]) return fail(why, "the row sum does not run over the last axis");
    m.t_sums = k.write.tensor;
    m.at.push_back(at);
    at = next(at + 1);
    if (at >= n_live) return fail(why, ends);
  }

  // [n - 2] exp(e) / sums
  {
    const Kernel& k = kernel(at);
    std::vector<int> w;
    if (!plain_rank4(k)) return fail(why, "the softmax has loop bounds, computed indices or another rank");
    if (k.reads.size() != 2) return fail(why, "the softmax does not read the scaled scores and the sums alone");
    int re = -1, rs = -1;
    for (int i = 0; i < 2; ++i) {
      if (k.reads[i].tensor == e) re = i;
      if (k.reads[i].tensor == m.t_sums) rs = i;
    }
    std::vector<int> er, sr;
    if (re < 0 || rs < 0 || !bare_regs(k, k.reads[re], er) || !bare_regs(k, k.reads[rs], sr) || er.size() != 4 || sr.size() != 3)
      return fail(why, "the softmax does not read the scaled scores and the sums alone");
    if (!bare_regs(k, k.write, w) || w != er || sr[0] != er[0] || sr[1] != er[1] || sr[2] != er[2])
      return fail(why, "a register of the softmax is not in the position of the scores");
    const Instr* ex = nullptr;
    const Instr* dv = nullptr;
    if (k.instrs.size() == 2) {
      for (auto& ins : k.instrs) {
        if (ins.kind == IK::Exp) ex = &ins;
        if (ins.kind == IK::Div) dv = &ins;
      }
    }
    if (!ex || !dv || ex->args.size() != 1 || ex->args[0] != k.reads[re].reg || dv->args.size() != 2 || dv->args[0] != ex->res ||
        dv->args[1] != k.reads[rs].reg || k.result != dv->res)
      return fail(why, "the softmax is not exp / sums alone");
    m.t_softmax = k.write.tensor;
    m.at.push_back(at);
    at = next(at + 1);
    if (at >= n_live) return fail(why, ends);
  }

  // [n - 1] the context
  {
    const Kernel& k = kernel(at);
    if (!match_batched2_gemm(k, m.context) || m.context.trans_a || m.context.trans_b) return fail(why, "the last kernel is not an NN product with two batch indices");
    if (k.reads[m.context.a_read].tensor != m.t_softmax) return fail(why, "the softmax is not the A operand of the context product");
    for (int q = 0; q < 2; ++q)
      if (m.context.batch_dim[0][q] > 1) return fail(why, "the context product does not read the softmax in the positions of the scores");
    if (m.context.row_dim[0] != 2) return fail(why, "the context product does not read the softmax in the positions of the scores");
    m.t_v = k.reads[m.context.b_read].tensor;
    m.t_out = k.write.tensor;
    m.at.push_back(at);
  }
  m.n = (int)m.at.size();

  out = m;
  return true;
}

bool attention_private(const Program& prog, const Target& t, const std::vector<int>& xs, const std::vector<int>& writers, const std::vector<int>& operands,
                       const std::vector<int>& members, const char* read_outside, const char** why) {
  const int n_live = (int)t.live.size();
  std::vector<char> member((size_t)n_live, 0);
  for (int q : members) member[(size_t)q] = 1;
  for (size_t i = 0; i < xs.size(); ++i) {
    const int x = xs[i];
    if (!x) continue;
    if (x < 1 || x >= (int)prog.tensors.size() || prog.tensors[x].kind != TK::Result) return fail(why, "an intermediate is not a result tensor");
    if (x == t.output) return fail(why, "an intermediate is the target's output");
    for (int o : operands)
      if (x == o) return fail(why, "an intermediate is an operand of the chain");
    int n_writers = 0;
    for (int q = 0; q < n_live; ++q) {
      const Kernel& k = t.all[t.live[q]];
      if (k.write.tensor == x) ++n_writers;
      if (member[(size_t)q]) continue;
      for (auto& rd : k.reads)
        if (rd.tensor == x) return fail(why, read_outside);
    }
    if (n_writers != writers[i]) return fail(why, "an intermediate has another writer");
  }
  return true;
}

bool match_attention(const Program& prog, const Target& t, int p, AttentionMatch& out, const char** why) {
  AttentionMatch m;
  if (!match_attention_chain(t, p, m, why)) return false;
  // the intermediates exist for the chain alone
  if (!attention_private(prog, t, {m.t_scores, m.t_scaled, m.t_sums, m.t_softmax}, {1, 1, 1, 1}, {m.t_out, m.t_q, m.t_k, m.t_v}, m.at,
                         "an intermediate is read outside the chain", why))
    return false;
  out = m;
  return true;
}

}  // namespace model
}  // namespace eg
