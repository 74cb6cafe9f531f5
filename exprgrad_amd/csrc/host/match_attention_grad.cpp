// A training step over the attention chain (match.hpp, AttentionFitMatch): the forward chain of match_attention.cpp with its
// intermediates read by the gradient kernels too, and those gradient kernels themselves — what eg_attention_sums and
// eg_attention_grad (kernels/attention_f32.hip, kernels/attention_grad_f32.hip) compute in three launches.  Structure only:
// shapes, loop extents, the switches and the model's setting are the planner's business (plan_attention.cpp,
// form_attention_fit_groups).  No HIP header.
//
// A gradient kernel is looked for by the tensors it reads (the one kernel outside the chain that reads the softmax is dv's,
// the readers of the scores' gradient are dq's and dk's, ...), never by its name or its place in the list, and then held to
//   - the positions of its registers: a register's role (the four positions of the scores, k, d) follows from the scores'
//     gradient or the softmax it reads, and every operand has to show the roles the forward products gave it;
//   - the instructions derive (kd.cpp, derive_instrs) emits for the forward kernel, dead code removed;
//   - derive's own record of where the kernel came from, where there is one.
// Refused, each with its reason: a missing gradient kernel (v an input: no dv), an intermediate or a gradient between the
// products that somebody else reads or writes or that is the target's output, two of dq, dk, dv in one tensor (q and kk one
// tensor: eg_attention_grad leaves aliasing outputs undefined), one of them an operand, operands out of position, other
// arithmetic, and everything match_attention_chain refuses.
#include "match.hpp"

#include <algorithm>
#include <map>
#include <set>

namespace eg {
namespace model {

namespace {

const char* const MISSING = "a gradient kernel of the chain is missing";
const char* const TWICE = "a gradient kernel of the chain is there twice";
const char* const POSITIONS = "a gradient kernel does not read its operands in the positions the forward products fix";
const char* const ARITHMETIC = "a gradient kernel does not compute what derive makes of the chain";
const char* const ORIGIN = "a gradient kernel was derived from another kernel or operand";
const char* const OUTSIDE = "an intermediate or its gradient is read outside the chain and its gradient kernels";

enum Role { ROLE_K = 4, ROLE_D = 5 };   // 0..3: the positions of the scores
using Roles = std::map<int, int>;       // register -> role
using Pattern = std::vector<int>;       // role per dimension of an operand

// The dimensions of `op` show `want`: a register with a role stands where `want` has that role, one without takes the role
// `want` has there if no other register holds it.
bool dims_as(const Kernel& k, const Op& op, Roles& role, const Pattern& want) {
  std::vector<int> regs;
  if (!bare_regs(k, op, regs) || regs.size() != want.size()) return false;
  for (size_t d = 0; d < regs.size(); ++d) {
    auto it = role.find(regs[d]);
    if (it != role.end()) {
      if (it->second != want[d]) return false;
      continue;
    }
    for (auto& kv : role)
      if (kv.second == want[d]) return false;
    role[regs[d]] = want[d];
  }
  return true;
}

Pattern pattern_of(const Op& op, const Roles& role) {
  Pattern out;
  for (auto& d : op.dims) {
    auto it = role.find(d.only_register());
    out.push_back(it == role.end() ? -1 : it->second);
  }
  return out;
}

const Instr* def_of(const Kernel& k, int reg) {
  for (auto& ins : k.instrs)
    if (ins.res == reg) return &ins;
  return nullptr;
}

bool is_op(const Instr* ins, IK kind, size_t args) { return ins && ins->kind == kind && ins->args.size() == args; }

// ins = a * b in either order
bool is_mul_of(const Instr* ins, int a, int b) {
  return is_op(ins, IK::Mul, 2) && ((ins->args[0] == a && ins->args[1] == b) || (ins->args[0] == b && ins->args[1] == a));
}

int read_of(const Kernel& k, int tensor) {
  int found = -1;
  for (size_t i = 0; i < k.reads.size(); ++i)
    if (k.reads[i].tensor == tensor) found = found < 0 ? (int)i : -2;
  return found;   // -1: none, -2: more than one
}

bool origin_ok(const Kernel& k, int from, int read) { return k.derived_from < 0 || (k.derived_from == from && k.derived_read == read); }

struct Finder {
  const Target& t;
  std::vector<char> forward;   // live position -> member of the forward chain
  const char* reason = "";

  const Kernel& kernel(int q) const { return t.all[t.live[q]]; }
  // live positions outside the forward chain whose kernels read every tensor of `tensors`
  std::vector<int> readers(std::initializer_list<int> tensors) const {
    std::vector<int> out;
    for (int q = 0; q < (int)t.live.size(); ++q) {
      if (forward[(size_t)q]) continue;
      bool all = true;
      for (int x : tensors) all = all && read_of(kernel(q), x) != -1;
      if (all) out.push_back(q);
    }
    return out;
  }
  // the one candidate that passes `test` (which names the reason of its refusal); -1 with `reason` set
  template <class Test>
  int pick(const std::vector<int>& cands, Test test) {
    if (cands.empty()) {
      reason = MISSING;
      return -1;
    }
    int found = -1;
    const char* last = MISSING;
    for (int q : cands) {
      const char* why = nullptr;
      if (test(kernel(q), &why)) {
        if (found >= 0) {
          reason = TWICE;
          return -1;
        }
        found = q;
      } else if (why) {
        last = why;
      }
    }
    if (found < 0) reason = last;
    return found;
  }
};

// W[pw] ++= X[px] * Y[py], X the read of tensor tx and Y the other read: five unbounded loops, one multiplication.
// *ty: the tensor of Y (in: 0 = any); *tw: the written tensor.
bool product_as(const Kernel& k, int tx, const Pattern& px, int* ty, const Pattern& py, const Pattern& pw, int* tw, const char** why) {
  *why = ARITHMETIC;
  if (!plain_loops(k, 5) || k.reads.size() != 2 || k.instrs.size() != 1) return false;
  const int x = read_of(k, tx);
  if (x < 0) return false;
  const Op& X = k.reads[(size_t)x];
  const Op& Y = k.reads[(size_t)(1 - x)];
  if (*ty && Y.tensor != *ty) return false;
  if (!is_mul_of(&k.instrs[0], X.reg, Y.reg) || k.result != k.instrs[0].res) return false;
  *why = POSITIONS;
  Roles role;
  if (!dims_as(k, X, role, px) || !dims_as(k, Y, role, py) || !dims_as(k, k.write, role, pw)) return false;
  *ty = Y.tensor;
  *tw = k.write.tensor;
  return true;
}

// A map or the row sum among the gradients between the products: four unbounded loops, every rank-4 operand over the same
// four registers, every rank-3 operand over the first three of them, the write of rank `write_rank`.
bool rows_as(const Kernel& k, size_t reads, size_t write_rank, const char** why) {
  *why = ARITHMETIC;
  if (!plain_loops(k, 4) || k.reads.size() != reads) return false;
  *why = POSITIONS;
  std::vector<int> four, r;
  for (auto& rd : k.reads)
    if (rd.dims.size() == 4 && four.empty() && !bare_regs(k, rd, four)) return false;
  if (four.size() != 4) return false;
  auto in_place = [&](const Op& op) {
    if (!bare_regs(k, op, r) || (r.size() != 4 && r.size() != 3)) return false;
    for (size_t d = 0; d < r.size(); ++d)
      if (r[d] != four[d]) return false;
    return true;
  };
  for (auto& rd : k.reads)
    if (!in_place(rd)) return false;
  return in_place(k.write) && k.write.dims.size() == write_rank;
}

}  // namespace

bool match_attention_fit(const Program& prog, const Target& t, int p, AttentionFitMatch& out, const char** why) {
  auto fail = [&](const char* reason) {
    if (why) *why = reason;
    return false;
  };
  AttentionFitMatch m;
  const char* fwd_why = "";
  if (!match_attention_chain(t, p, m.fwd, &fwd_why, true)) return fail(fwd_why);
  const AttentionMatch& f = m.fwd;
  const int n_live = (int)t.live.size(), last = f.at.back();
  Finder find{t, std::vector<char>((size_t)n_live, 0)};
  m.forward = f.at;
  for (int q : m.forward) find.forward[(size_t)q] = 1;
  const Kernel& k0 = t.all[t.live[p]];
  const Kernel& k4 = t.all[t.live[last]];
  const int e = f.t_scaled ? f.t_scaled : f.t_scores;   // what the softmax reads
  const int p_sums = f.at[(size_t)f.n - 3], p_softmax = f.at[(size_t)f.n - 2];

  // the roles the forward products give their operands
  const Pattern scores = {0, 1, 2, 3};
  Roles r0, r4;
  for (int d = 0; d < 4; ++d) r0[k0.write.dims[(size_t)d].only_register()] = d;
  r0[k0.loops[(size_t)f.scores.lk].reg] = ROLE_K;
  for (int d = 0; d < 4; ++d) r4[k4.reads[(size_t)f.context.a_read].dims[(size_t)d].only_register()] = d;
  r4[k4.loops[(size_t)f.context.lj].reg] = ROLE_D;
  const Pattern pq = pattern_of(k0.reads[(size_t)f.scores.a_read], r0), pk = pattern_of(k0.reads[(size_t)f.scores.b_read], r0);
  const Pattern pv = pattern_of(k4.reads[(size_t)f.context.b_read], r4), po = pattern_of(k4.write, r4);

  // dv: the one kernel outside the chain that reads the softmax; its other operand is the context's gradient
  m.p_dv = find.pick(find.readers({f.t_softmax}), [&](const Kernel& k, const char** w) {
    int ty = 0, tw = 0;
    if (!product_as(k, f.t_softmax, scores, &ty, po, pv, &tw, w)) return false;
    m.t_do = ty, m.t_dv = tw;
    return true;
  });
  if (m.p_dv < 0) return fail(find.reason);
  // dsoftmax: reads the context's gradient and v
  m.p_dsoftmax = find.pick(find.readers({m.t_do, f.t_v}), [&](const Kernel& k, const char** w) {
    int ty = f.t_v, tw = 0;
    if (!product_as(k, m.t_do, po, &ty, pv, scores, &tw, w)) return false;
    m.t_dsoftmax = tw;
    return true;
  });
  if (m.p_dsoftmax < 0) return fail(find.reason);

  // the softmax's two gradients: de ++= dsoftmax / sums * exp(e) and dsums ++= -exp(e) * (dsoftmax / (sums * sums))
  auto softmax_grad = [&](bool sums_side) {
    return [&, sums_side](const Kernel& k, const char** w) {
      if ((k.write.dims.size() == 3) != sums_side) return false;
      if (!rows_as(k, 3, sums_side ? 3 : 4, w)) return false;
      *w = ARITHMETIC;
      const int re = read_of(k, e), rs = read_of(k, f.t_sums), rg = read_of(k, m.t_dsoftmax);
      if (re < 0 || rs < 0 || rg < 0 || k.reads[(size_t)re].dims.size() != 4 || k.reads[(size_t)rs].dims.size() != 3 || k.reads[(size_t)rg].dims.size() != 4)
        return false;
      const int x = k.reads[(size_t)re].reg, s = k.reads[(size_t)rs].reg, g = k.reads[(size_t)rg].reg;
      const Instr* top = def_of(k, k.result);
      if (!is_op(top, IK::Mul, 2)) return false;
      if (!sums_side) {
        const Instr* a = def_of(k, top->args[0]);
        const Instr* ex = def_of(k, top->args[1]);
        return k.instrs.size() == 3 && is_op(a, IK::Div, 2) && a->args[0] == g && a->args[1] == s && is_op(ex, IK::Exp, 1) && ex->args[0] == x;
      }
      const Instr* neg = def_of(k, top->args[0]);
      const Instr* dg = def_of(k, top->args[1]);
      if (k.instrs.size() != 5 || !is_op(neg, IK::Negate, 1) || !is_op(dg, IK::Div, 2) || dg->args[0] != g) return false;
      const Instr* ex = def_of(k, neg->args[0]);
      return is_op(ex, IK::Exp, 1) && ex->args[0] == x && is_mul_of(def_of(k, dg->args[1]), s, s);
    };
  };
  m.p_de = find.pick(find.readers({e, f.t_sums, m.t_dsoftmax}), softmax_grad(false));
  if (m.p_de < 0) return fail(find.reason);
  m.t_de = find.kernel(m.p_de).write.tensor;
  m.p_dsums = find.pick(find.readers({e, f.t_sums, m.t_dsoftmax}), softmax_grad(true));
  if (m.p_dsums < 0) return fail(find.reason);
  m.t_dsums = find.kernel(m.p_dsums).write.tensor;
  // the row sum's gradient: de ++= dsums * exp(e)
  m.p_de_sums = find.pick(find.readers({e, m.t_dsums}), [&](const Kernel& k, const char** w) {
    if (!rows_as(k, 2, 4, w)) return false;
    *w = ARITHMETIC;
    const int re = read_of(k, e), rg = read_of(k, m.t_dsums);
    if (re < 0 || rg < 0 || k.reads[(size_t)re].dims.size() != 4 || k.reads[(size_t)rg].dims.size() != 3 || k.instrs.size() != 2) return false;
    const Instr* top = def_of(k, k.result);
    if (!is_op(top, IK::Mul, 2) || top->args[0] != k.reads[(size_t)rg].reg) return false;
    const Instr* ex = def_of(k, top->args[1]);
    return is_op(ex, IK::Exp, 1) && ex->args[0] == k.reads[(size_t)re].reg && k.write.tensor == m.t_de;
  });
  if (m.p_de_sums < 0) return fail(find.reason);
  // the scale map's gradient: dscores ++= de * the same literal
  m.t_dscores = m.t_de;
  if (f.t_scaled) {
    m.p_dscale = find.pick(find.readers({m.t_de}), [&](const Kernel& k, const char** w) {
      if (!rows_as(k, 1, 4, w)) return false;
      *w = ARITHMETIC;
      if (k.instrs.size() != 2) return false;
      const Instr* top = def_of(k, k.result);
      if (!is_op(top, IK::Mul, 2) || top->args[0] != k.reads[0].reg) return false;
      const Instr* lit = def_of(k, top->args[1]);
      return is_op(lit, IK::Scalar, 0) && (float)lit->lit == f.scale;
    });
    if (m.p_dscale < 0) return fail(find.reason);
    m.t_dscores = find.kernel(m.p_dscale).write.tensor;
  }
  // dq and dk: the two readers of the scores' gradient
  m.p_dq = find.pick(find.readers({m.t_dscores, f.t_k}), [&](const Kernel& k, const char** w) {
    int ty = f.t_k, tw = 0;
    if (!product_as(k, m.t_dscores, scores, &ty, pk, pq, &tw, w)) return false;
    m.t_dq = tw;
    return true;
  });
  if (m.p_dq < 0) return fail(find.reason);
  m.p_dk = find.pick(find.readers({m.t_dscores, f.t_q}), [&](const Kernel& k, const char** w) {
    int ty = f.t_q, tw = 0;
    if (!product_as(k, m.t_dscores, scores, &ty, pq, pk, &tw, w)) return false;
    m.t_dk = tw;
    return true;
  });
  if (m.p_dk < 0) return fail(find.reason);

  for (int q : {m.p_dsoftmax, m.p_dv, m.p_de, m.p_dsums, m.p_de_sums, m.p_dscale, m.p_dq, m.p_dk})
    if (q >= 0) m.backward.push_back(q);
  std::sort(m.backward.begin(), m.backward.end());
  if (std::adjacent_find(m.backward.begin(), m.backward.end()) != m.backward.end()) return fail(TWICE);
  if (m.backward.front() <= last) return fail(MISSING);   // a gradient kernel in front of the chain it differentiates
  // the four products as the library's launches know them (the planner's plan_batched2)
  if (!match_batched2_gemm(find.kernel(m.p_dsoftmax), m.dsoftmax) || !match_batched2_gemm(find.kernel(m.p_dv), m.dv) ||
      !match_batched2_gemm(find.kernel(m.p_dq), m.dq) || !match_batched2_gemm(find.kernel(m.p_dk), m.dk))
    return fail(ARITHMETIC);

  // derive's record, where there is one
  const int a0 = t.live[p], a4 = t.live[last];
  bool origin = origin_ok(find.kernel(m.p_dq), a0, f.scores.a_read) && origin_ok(find.kernel(m.p_dk), a0, f.scores.b_read) &&
                origin_ok(find.kernel(m.p_dsoftmax), a4, f.context.a_read) && origin_ok(find.kernel(m.p_dv), a4, f.context.b_read) &&
                origin_ok(find.kernel(m.p_de), t.live[p_softmax], read_of(t.all[t.live[p_softmax]], e)) &&
                origin_ok(find.kernel(m.p_dsums), t.live[p_softmax], read_of(t.all[t.live[p_softmax]], f.t_sums)) &&
                origin_ok(find.kernel(m.p_de_sums), t.live[p_sums], 0);
  if (m.p_dscale >= 0) origin = origin && origin_ok(find.kernel(m.p_dscale), t.live[f.at[1]], 0);
  if (!origin) return fail(ORIGIN);

  // the outputs: three tensors, none of them an operand
  if (m.t_dq == m.t_dk || m.t_dq == m.t_dv || m.t_dk == m.t_dv) return fail("two of the gradients of q, kk and v are one tensor");
  for (int g : {m.t_dq, m.t_dk, m.t_dv})
    for (int x : {f.t_q, f.t_k, f.t_v, f.t_out, f.t_sums, m.t_do})
      if (g == x) return fail("a gradient tensor is an operand of the chain");

  // the tensors between the products, forward and backward, exist for the members alone
  std::vector<int> members = m.forward;
  members.insert(members.end(), m.backward.begin(), m.backward.end());
  std::vector<int> xs = {f.t_scores, f.t_scaled, f.t_sums, f.t_softmax, m.t_dsoftmax, m.t_dsums, m.t_de};
  std::vector<int> writers = {1, 1, 1, 1, 1, 1, 2};
  if (f.t_scaled) {
    xs.push_back(m.t_dscores);
    writers.push_back(1);
  }
  const char* priv = "";
  if (!attention_private(prog, t, xs, writers, {f.t_q, f.t_k, f.t_v, f.t_out, m.t_do, m.t_dq, m.t_dk, m.t_dv}, members, OUTSIDE, &priv)) return fail(priv);
  for (int x : xs)
    if (x && x != f.t_sums) m.hidden.push_back(x);
  out = m;
  return true;
}

}  // namespace model
}  // namespace eg
