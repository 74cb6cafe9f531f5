// Pattern matching of lowered kernels against the hand-written library: contraction, bias add,
// convolution and its two gradients.
#include "match.hpp"

#include <set>
#include <vector>

namespace eg {
namespace model {

bool bare2(const Op& op, int& r0, int& r1) {
  if (op.raw || op.dims.size() != 2) return false;
  r0 = op.dims[0].only_register();
  r1 = op.dims[1].only_register();
  return r0 && r1 && r0 != r1;
}

int loop_index(const Kernel& k, int reg) {
  for (size_t l = 0; l < k.loops.size(); ++l)
    if (k.loops[l].reg == reg) return (int)l;
  return -1;
}

// c[i,j] += a(i,k) * b(k,j)      base.nim:27-28 and its two derived forms (passes.nim:519-549)
bool match_gemm(const Kernel& k, GemmMatch& m) {
  if (!k.index_instrs.empty()) return false;
  if (k.instrs.size() != 1 || k.instrs[0].kind != IK::Mul || k.result != k.instrs[0].res) return false;
  if (k.reads.size() != 2 || k.loops.size() != 3 || !k.setup.empty()) return false;
  for (auto& lp : k.loops)
    if (lp.has_bounds) return false;
  const std::vector<int>& args = k.instrs[0].args;
  if (!((args[0] == k.reads[0].reg && args[1] == k.reads[1].reg) || (args[0] == k.reads[1].reg && args[1] == k.reads[0].reg)))
    return false;
  int wi, wj;
  if (!bare2(k.write, wi, wj)) return false;
  int kk = 0;
  for (auto& lp : k.loops)
    if (lp.reg != wi && lp.reg != wj) kk = lp.reg;
  if (!kk || loop_index(k, wi) < 0 || loop_index(k, wj) < 0) return false;
  int r[2][2];
  if (!bare2(k.reads[0], r[0][0], r[0][1]) || !bare2(k.reads[1], r[1][0], r[1][1])) return false;
  auto is = [](const int* p, int x, int y) { return (p[0] == x && p[1] == y) || (p[0] == y && p[1] == x); };
  for (int a = 0; a < 2; ++a) {
    const int b = 1 - a;
    if (is(r[a], wi, kk) && is(r[b], kk, wj)) {
      m.a_read = a;
      m.b_read = b;
      m.trans_a = r[a][0] == kk;
      m.trans_b = r[b][0] == wj;
      m.li = loop_index(k, wi);
      m.lj = loop_index(k, wj);
      m.lk = loop_index(k, kk);
      return true;
    }
  }
  return false;
}

namespace {
// every dimension a single bare register, all different
bool bare_dims(const Op& op, std::vector<int>& regs) {
  regs.clear();
  if (op.raw) return false;
  std::set<int> seen;
  for (auto& d : op.dims) {
    const int r = d.only_register();
    if (!r || !seen.insert(r).second) return false;
    regs.push_back(r);
  }
  return true;
}
}  // namespace

// out[g,i,j] += a[g,i,k] * b[g,k,j], its two derived forms, and the shared-weight forms that collapse to a plain product
// (match.hpp), in either scalar type.  Anything else — the batch index elsewhere, a bounded loop — is not a match.
bool match_batched_gemm(const Kernel& k, BatchedGemmMatch& m) {
  if (!k.index_instrs.empty()) return false;
  if (k.instrs.size() != 1 || k.instrs[0].kind != IK::Mul || k.result != k.instrs[0].res) return false;
  if (k.reads.size() != 2 || k.loops.size() != 4 || !k.setup.empty()) return false;
  for (auto& lp : k.loops)
    if (lp.has_bounds) return false;
  const std::vector<int>& args = k.instrs[0].args;
  if (!((args[0] == k.reads[0].reg && args[1] == k.reads[1].reg) || (args[0] == k.reads[1].reg && args[1] == k.reads[0].reg)))
    return false;
  std::vector<int> w, r[2];
  if (!bare_dims(k.write, w) || !bare_dims(k.reads[0], r[0]) || !bare_dims(k.reads[1], r[1])) return false;
  for (const std::vector<int>* regs : {&w, &r[0], &r[1]}) {
    if (regs->size() != 2 && regs->size() != 3) return false;
    for (int reg : *regs)
      if (loop_index(k, reg) < 0) return false;
  }
  const int rank2 = (w.size() == 2) + (r[0].size() == 2) + (r[1].size() == 2);
  auto is = [](int p, int q, int x, int y) { return (p == x && q == y) || (p == y && q == x); };
  BatchedGemmMatch out;
  if (rank2 == 0) {
    const int g = w[0], wi = w[1], wj = w[2];
    int kk = 0;
    for (auto& lp : k.loops)
      if (lp.reg != g && lp.reg != wi && lp.reg != wj) kk = lp.reg;
    if (!kk || r[0][0] != g || r[1][0] != g) return false;
    for (int a = 0; a < 2; ++a) {
      const int b = 1 - a;
      if (is(r[a][1], r[a][2], wi, kk) && is(r[b][1], r[b][2], kk, wj)) {
        out.a_read = a;
        out.b_read = b;
        out.trans_a = r[a][1] == kk;
        out.trans_b = r[b][1] == wj;
        out.lg = loop_index(k, g);
        out.li = loop_index(k, wi);
        out.lj = loop_index(k, wj);
        out.lk = loop_index(k, kk);
        m = out;
        return true;
      }
    }
    return false;
  }
  if (rank2 != 1) return false;
  out.collapsed = true;
  if (w.size() == 3) {
    // out[g,i,n] += a[g,i,k] * w(k,n): the rank-3 read has the write's two leading registers and k last
    const int g = w[0], i = w[1], n = w[2];
    const int a = r[0].size() == 3 ? 0 : 1, b = 1 - a;
    if (r[a][0] != g || r[a][1] != i) return false;
    const int kk = r[a][2];
    if (kk == n || !is(r[b][0], r[b][1], kk, n)) return false;
    out.a_read = a;
    out.b_read = b;
    out.trans_b = r[b][0] == n;
    out.lg = loop_index(k, g);
    out.li = loop_index(k, i);
    out.lj = loop_index(k, n);
    out.lk = loop_index(k, kk);
    m = out;
    return true;
  }
  // gw[m,n] += a[g,i,m] * b[g,i,n]: both reads share their two leading registers, which the write does not name
  const int g = r[0][0], i = r[0][1];
  if (r[1][0] != g || r[1][1] != i || g == w[0] || g == w[1] || i == w[0] || i == w[1]) return false;
  for (int a = 0; a < 2; ++a) {
    const int b = 1 - a;
    if (r[a][2] == w[0] && r[b][2] == w[1]) {
      out.row_k = true;
      out.a_read = a;
      out.b_read = b;
      out.trans_a = true;
      out.lg = loop_index(k, g);
      out.lk = loop_index(k, i);
      out.li = loop_index(k, w[0]);
      out.lj = loop_index(k, w[1]);
      m = out;
      return true;
    }
  }
  return false;
}

// s[b,h,i,j] += q[b,i,h,k] * kk[b,j,h,k], o[b,i,h,d] += p[b,h,i,j] * v[b,j,h,d] and their derived forms (match.hpp): two
// batch registers in any position but the last.  An operand that ends in a batch register has no unit-stride matrix axis
// and is not a match.
bool match_batched2_gemm(const Kernel& k, Batched2GemmMatch& m) {
  if (!k.index_instrs.empty()) return false;
  if (k.instrs.size() != 1 || k.instrs[0].kind != IK::Mul || k.result != k.instrs[0].res) return false;
  if (k.reads.size() != 2 || k.loops.size() != 5 || !k.setup.empty()) return false;
  for (auto& lp : k.loops)
    if (lp.has_bounds) return false;
  const std::vector<int>& args = k.instrs[0].args;
  if (!((args[0] == k.reads[0].reg && args[1] == k.reads[1].reg) || (args[0] == k.reads[1].reg && args[1] == k.reads[0].reg)))
    return false;
  std::vector<int> w, r[2];
  if (!bare_dims(k.write, w) || !bare_dims(k.reads[0], r[0]) || !bare_dims(k.reads[1], r[1])) return false;
  for (const std::vector<int>* regs : {&w, &r[0], &r[1]}) {
    if (regs->size() != 4) return false;
    for (int reg : *regs)
      if (loop_index(k, reg) < 0) return false;
  }
  auto pos = [](const std::vector<int>& regs, int reg) {
    for (int d = 0; d < 4; ++d)
      if (regs[d] == reg) return d;
    return -1;
  };
  // the write's registers: in both reads (batch), or in exactly one (m, n); n is the last one
  std::vector<int> batch;
  int mm = 0;
  const int n = w[3];
  for (int reg : w) {
    const bool in0 = pos(r[0], reg) >= 0, in1 = pos(r[1], reg) >= 0;
    if (in0 && in1) batch.push_back(reg);
    else if (in0 != in1 && reg != n) mm = reg;
    else if (in0 == in1) return false;
  }
  if (batch.size() != 2 || !mm || n == batch[0] || n == batch[1]) return false;
  const int b = pos(r[0], n) >= 0 ? 0 : 1, a = 1 - b;   // the read that names n is B: the product commutes
  if (pos(r[a], mm) < 0) return false;
  int kk = 0;
  for (auto& lp : k.loops)
    if (pos(w, lp.reg) < 0) kk = lp.reg;
  if (!kk || pos(r[a], kk) < 0 || pos(r[b], kk) < 0) return false;
  if ((r[a][3] != mm && r[a][3] != kk) || (r[b][3] != n && r[b][3] != kk)) return false;
  Batched2GemmMatch out;
  out.a_read = a;
  out.b_read = b;
  out.trans_a = r[a][3] == mm;
  out.trans_b = r[b][3] == kk;
  out.li = loop_index(k, mm);
  out.lj = loop_index(k, n);
  out.lk = loop_index(k, kk);
  const std::vector<int>* ops[3] = {&r[a], &r[b], &w};
  const int rows[3] = {out.trans_a ? kk : mm, out.trans_b ? n : kk, mm};
  for (int o = 0; o < 3; ++o) {
    for (int q = 0; q < 2; ++q) {
      out.lb[q] = loop_index(k, batch[q]);
      out.batch_dim[o][q] = pos(*ops[o], batch[q]);
    }
    out.row_dim[o] = pos(*ops[o], rows[o]);
  }
  m = out;
  return true;
}

// out[y,x] += bias[x] on the tensor the preceding contraction wrote   dnn.nim:22-24
bool match_bias(const Kernel& k, int tensor) {
  if (!k.index_instrs.empty()) return false;
  if (!k.instrs.empty() || k.reads.size() != 1 || k.result != k.reads[0].reg || k.write.tensor != tensor) return false;
  if (k.loops.size() != 2 || !k.setup.empty()) return false;
  for (auto& lp : k.loops)
    if (lp.has_bounds) return false;
  int wi, wj;
  if (!bare2(k.write, wi, wj)) return false;
  const Op& b = k.reads[0];
  return !b.raw && b.dims.size() == 1 && b.dims[0].only_register() == wj;
}

// out[n,y,x,f] += img[n,y+dy,x+dx,c] * flt[f,dy,dx,c]   dnn.nim:45-49 (4-D) / conv2.nim:128-132 (3-D)
// and the two kernels derive (passes.nim:383-549) makes of it, which are the same loop nest with
// another of the three tensors written:
//   gimg[n,y+dy,x+dx,c] += gout[n,y,x,f] * flt[f,dy,dx,c]      gflt[f,dy,dx,c] += gout[n,y,x,f] * img[n,y+dy,x+dx,c]
bool match_conv(const Kernel& k, ConvMatch& m) {
  if (!k.index_instrs.empty()) return false;
  if (k.instrs.size() != 1 || k.instrs[0].kind != IK::Mul || k.result != k.instrs[0].res || k.reads.size() != 2) return false;
  if (!k.setup.empty() || k.write.raw || k.reads[0].raw || k.reads[1].raw) return false;
  const std::vector<int>& args = k.instrs[0].args;
  if (!((args[0] == k.reads[0].reg && args[1] == k.reads[1].reg) || (args[0] == k.reads[1].reg && args[1] == k.reads[0].reg)))
    return false;
  for (auto& lp : k.loops)
    if (lp.has_bounds) return false;
  const Op* ops[3] = {&k.write, &k.reads[0], &k.reads[1]};  // operand index + 1
  static const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  for (auto& pm : perms) {
    const Op& out = *ops[pm[0]];
    const Op& img = *ops[pm[1]];
    const Op& flt = *ops[pm[2]];
    const size_t nd = out.dims.size();
    if ((nd != 4 && nd != 3) || img.dims.size() != nd || flt.dims.size() != 4) continue;
    const bool batched = nd == 4;
    if (k.loops.size() != (batched ? 7u : 6u)) continue;
    std::vector<int> w;
    for (auto& d : out.dims) w.push_back(d.only_register());
    const int off = batched ? 1 : 0;
    const int n = batched ? w[0] : 0, y = w[off], x = w[off + 1], f = w[off + 2];
    if (!y || !x || !f || (batched && !n)) continue;
    const int ff = flt.dims[0].only_register(), dy = flt.dims[1].only_register(), dx = flt.dims[2].only_register(),
              c = flt.dims[3].only_register();
    if (ff != f || !dy || !dx || !c) continue;
    std::set<int> all = {y, x, f, dy, dx, c};
    if (batched) all.insert(n);
    if (all.size() != (batched ? 7u : 6u)) continue;
    auto pair_sum = [](const Lin& l, int p, int q) {
      return l.constant == 0 && l.factors.size() == 2 && l.factor_of(p) == 1 && l.factor_of(q) == 1;
    };
    if (batched && img.dims[0].only_register() != n) continue;
    if (!pair_sum(img.dims[off], y, dy) || !pair_sum(img.dims[off + 1], x, dx) || img.dims[off + 2].only_register() != c)
      continue;
    m.out_op = pm[0] - 1;
    m.img_op = pm[1] - 1;
    m.flt_op = pm[2] - 1;
    m.batched = batched;
    m.role = pm[0] == 0 ? ConvMatch::Forward : (pm[1] == 0 ? ConvMatch::GradImage : ConvMatch::GradFilter);
    return true;
  }
  return false;
}

}  // namespace model
}  // namespace eg
