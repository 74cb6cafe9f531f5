// Attention groups of a plan: a forward attention chain (match_attention) becomes ONE launch of eg_attention's internal
// entry (kernels/attention_f32.hip) — scores, scale, row sums and softmax live in the registers of its blocks and get no
// arena storage.  Formed before every other group, only when
//   - row fusion and the batched products are both enabled (EG_NO_ROWFUSE, EG_NO_BATCHED_GEMM: the plan is then the unfused one);
//   - the model does not keep values (eg_model_keep_values) and computes in float32 (make_plan calls this under `fuse`), or
//     computes in float64 and asks for it (eg_model_fuse_attention_f64: the launch is kernels/attention_f64.hip's, and the
//     chain's products are two-index products only under eg_model_batched2_f64, so the group needs that setting too);
//   - plan_batched2's checks pass for both products (loops from 0, extents at least 1, rank-4 dense shapes covered by the loops);
//   - the three kernels between them run over exactly the scores' shape, which the products' loops cover exactly;
//   - no intermediate is a gradient-bucket member, and the chain does not straddle the backward | update boundary;
//   - plan_attention (kernels/attention_plan.cpp) supports the shape: K and D at most 128.
// Anything else keeps the plan it had: two eg_bgemm2 launches around a collapsed wide row group, or generated kernels.
//
// Fit groups (form_attention_fit_groups, only under eg_model_fuse_attention_fit): a training step over the chain
// (match_attention_fit) becomes two launches — the forward one as above, which stores the row sums too, and one
// StepKind::AttentionGrad for the seven or eight gradient kernels (eg_attention_grad's internal entry: two kernels).  The
// conditions above hold for both halves: all six products pass plan_batched2, the gradient maps and the row sum run over
// exactly the scores' shape, no member is absorbed, inlined or grouped, neither half straddles the boundary, and both
// plan_attention and plan_attention_grad support the shape.  Further:
//   - no hidden tensor is a gradient-bucket member, and a model whose gradient bucket is bound to a caller's buffer
//     (eg_model_bind_grad_bucket: the data-parallel step) keeps the unfused plan when dq, dk or dv lies in it;
//   - where the launches stand.  The chain's members need not be neighbours (a projection of v sits between the softmax and
//     the context; the projection's gradient sits between dv and the softmax's gradients).  The forward launch stands at the
//     chain's last kernel: a kernel between its members may not write q or kk nor touch the context.  The backward launch
//     stands at the FIRST gradient kernel — everything it reads (q, kk, v, the context, the sums, the context's gradient)
//     is complete there, and a consumer of dv between the members finds dv written.  Between the first and the last gradient
//     kernel no other kernel may write one of those six operands, and none may touch dq, dk or dv in front of the member that
//     writes it.
// The sums and the context are ordinary tensors of such a plan; scores, scaled scores, softmax and the four gradients
// between the products are Plan::attn_hidden.
#include "../kernels/attention_plan.hpp"
#include "model_types.hpp"

namespace eg {
namespace model {

namespace {

long stride_of(const std::vector<long>& dims, int d) {
  long st = 1;
  for (size_t e = (size_t)d + 1; e < dims.size(); ++e) st *= dims[e];
  return st;
}

// A map or a row sum of a group at live position s runs over exactly the scores' shape S: its rank-4 operands have that
// shape with the loops covering it, its rank-3 operands the shape's first three extents.
bool rows_cover(const Target& t, const std::vector<KernelInfo>& infos, const Shapes& shapes, int s, const std::vector<long>& S) {
  const Kernel& k = t.all[t.live[s]];
  const KernelInfo& info = infos[t.live[s]];
  bool ok = info.ok;
  const Op* e = nullptr;   // the rank-4 read: all four registers in the positions of the scores
  for (auto& rd : k.reads)
    if (rd.dims.size() == 4) e = &rd;
  ok = ok && e;
  for (int d = 0; ok && d < 4; ++d) {
    const int l = loop_index(k, e->dims[d].only_register());
    ok = l >= 0 && info.bounds[l].first == 0 && info.bounds[l].second == S[d];
  }
  for (auto& rd : k.reads) {
    auto sh = shapes.find(rd.tensor);
    ok = ok && sh != shapes.end() && sh->second == (rd.dims.size() == 4 ? S : std::vector<long>(S.begin(), S.begin() + 3));
  }
  auto ws = shapes.find(k.write.tensor);
  return ok && ws != shapes.end() && ws->second == (k.write.dims.size() == 4 ? S : std::vector<long>(S.begin(), S.begin() + 3));
}

// The forward chain `am` (members at am.at) as one launch: every check of the header that concerns its kernels and shapes.
// outer_pos: the position among the scores' dimensions (0 or 1) of the batch index that is the launch's outer one.
bool plan_chain(eg_model* m, TargetState& ts, const Plan& plan, const std::vector<KernelInfo>& infos, const std::vector<int>& group_of,
                const AttentionMatch& am, Launch& L, int& outer_pos) {
  const Target& t = *ts.target;
  const Shapes& shapes = plan.shapes;
  const int p = am.at.front(), last = am.at.back();
  bool ok = ts.lowered[p].two_batch && ts.lowered[last].two_batch;
  for (int s : am.at) ok = ok && group_of[s] == -1 && !ts.lowered[s].absorbed && !ts.lowered[s].inlined;
  ok = ok && !(t.first_update > p && t.first_update <= last);
  if (!ok) return false;
  const Kernel& k0 = t.all[t.live[p]];
  const Kernel& k4 = t.all[t.live[last]];
  const KernelInfo& i0 = infos[t.live[p]];
  const KernelInfo& i4 = infos[t.live[last]];
  Launch L0, L4;
  if (!plan_batched2(am.scores, k0, i0, shapes, L0) || !plan_batched2(am.context, k4, i4, shapes, L4)) return false;
  const Batched2GemmMatch& g0 = am.scores;
  const Batched2GemmMatch& g4 = am.context;
  // the scores' shape [x0, x1, I, J]: covered exactly by both products and by every kernel between them
  const std::vector<long>& S = shapes.at(am.t_scores);
  ok = S.size() == 4 && L0.M == L4.M && L0.N == L4.K && S[2] == L0.M && S[3] == L0.N;
  for (int q = 0; ok && q < 2; ++q)
    ok = S[g0.batch_dim[2][q]] == i0.bounds[g0.lb[q]].second && S[g4.batch_dim[0][q]] == i4.bounds[g4.lb[q]].second;
  for (size_t s = 1; ok && s + 1 < am.at.size(); ++s) ok = rows_cover(t, infos, shapes, am.at[s], S);
  if (!ok) return false;
  // The context's batch register with the larger stride in its output is the outer index (as plan_batched2 has it); the
  // scores' batch register at the same position of the scores is its partner.
  const std::vector<long>& Qs = shapes.at(am.t_q);
  const std::vector<long>& Ks = shapes.at(am.t_k);
  const std::vector<long>& Vs = shapes.at(am.t_v);
  const std::vector<long>& Os = shapes.at(am.t_out);
  const int outer4 = stride_of(Os, g4.batch_dim[2][0]) >= stride_of(Os, g4.batch_dim[2][1]) ? 0 : 1, inner4 = 1 - outer4;
  auto partner = [&](int q4) {
    for (int r = 0; r < 2; ++r)
      if (g0.batch_dim[2][r] == g4.batch_dim[0][q4]) return r;
    return -1;
  };
  const int outer0 = partner(outer4), inner0 = partner(inner4);
  if (outer0 < 0 || inner0 < 0 || outer0 == inner0) return false;
  outer_pos = g4.batch_dim[0][outer4];
  L = Launch();
  L.kind = StepKind::Attention;
  L.lowered = p;
  L.standalone = true;
  Launch::Attn& A = L.attn;
  A.e = {i4.bounds[g4.lb[outer4]].second, i4.bounds[g4.lb[inner4]].second, L0.M, L0.N, L0.K, L4.N};
  if (A.e.batch0 != i0.bounds[g0.lb[outer0]].second || A.e.batch1 != i0.bounds[g0.lb[inner0]].second) return false;
  A.scale = am.scale;
  A.scale_f64 = am.scale_f64;
  A.q = {am.t_q, {L0.lda, stride_of(Qs, g0.batch_dim[0][outer0]), stride_of(Qs, g0.batch_dim[0][inner0])}};
  A.k = {am.t_k, {L0.ldb, stride_of(Ks, g0.batch_dim[1][outer0]), stride_of(Ks, g0.batch_dim[1][inner0])}};
  A.v = {am.t_v, {L4.ldb, stride_of(Vs, g4.batch_dim[1][outer4]), stride_of(Vs, g4.batch_dim[1][inner4])}};
  A.o = {am.t_out, {L4.ldc, stride_of(Os, g4.batch_dim[2][outer4]), stride_of(Os, g4.batch_dim[2][inner4])}};
  A.members = am.at;
  return true;
}

// A view as the planner takes it: the arena's tensors start 16-byte aligned.
eg::attention::Operand operand(const Launch::Attn::Operand& x) { return {x.view, true}; }

eg::attention::Problem problem_of(eg_model* m, const Launch::Attn& A) {
  eg::attention::Problem pr;
  static_cast<eg::attention::Extents&>(pr) = A.e;
  pr.q = operand(A.q), pr.k = operand(A.k), pr.v = operand(A.v), pr.o = operand(A.o);
  pr.sums = A.sums.tensor != 0;
  pr.cus = m->ctx->compute_units;
  return pr;
}

// (a float64 model: only under eg_model_fuse_attention_f64, and — plan_chain's two_batch check — only where
// eg_model_batched2_f64 has lowered the chain's products as two-index products)
bool enabled(eg_model* m) {
  return row_fusion_enabled() && !eg::sw::on(eg::Sw::NO_BATCHED_GEMM) && !m->keep_values && (!m->f64 || m->fuse_attention_f64);
}

// The kernel's own planner for the model's scalar type: K and D at most 128.
bool kernel_supports(eg_model* m, const Launch::Attn& A) {
  return m->f64 ? eg::attention::plan_attention_f64(problem_of(m, A)).supported : eg::attention::plan_attention(problem_of(m, A)).supported;
}

}  // namespace

int form_attention_groups(eg_model* m, TargetState& ts, Plan& plan, const std::vector<KernelInfo>& infos, const std::map<int, int>& first_writer,
                          std::vector<int>& group_of) {
  (void)first_writer;
  if (!enabled(m)) return EG_OK;
  const Target& t = *ts.target;
  const int n = (int)t.live.size();
  for (int p = 0; p + 4 <= n; ++p) {
    AttentionMatch am;
    if (group_of[p] != -1 || !match_attention(m->prog, t, p, am)) continue;
    const int last = p + am.n - 1;
    bool ok = true;
    for (int x : {am.t_scores, am.t_scaled, am.t_sums, am.t_softmax}) ok = ok && (!x || !ts.bucket_offset.count(x));
    Launch L;
    int outer_pos = 0;
    if (!ok || !plan_chain(m, ts, plan, infos, group_of, am, L, outer_pos)) continue;
    if (!kernel_supports(m, L.attn)) continue;   // K or D above 128: the unfused plan
    for (int s = p; s <= last; ++s) group_of[s] = ATTENTION_GROUP_CODE;
    for (int x : {am.t_scores, am.t_scaled, am.t_sums, am.t_softmax})
      if (x) plan.attn_hidden.insert(x);
    plan.attn_groups[p] = L;
    p = last;
  }
  return EG_OK;
}

int form_attention_fit_groups(eg_model* m, TargetState& ts, Plan& plan, const std::vector<KernelInfo>& infos, const std::map<int, int>& first_writer,
                              std::vector<int>& group_of) {
  (void)first_writer;
  if (!m->fuse_attention_fit || m->f64 || !enabled(m)) return EG_OK;   // (the fit route is float32-only)
  const Target& t = *ts.target;
  const Shapes& shapes = plan.shapes;
  const int n = (int)t.live.size();
  for (int p = 0; p + 4 <= n; ++p) {
    AttentionFitMatch fm;
    if (group_of[p] != -1 || !match_attention_fit(m->prog, t, p, fm)) continue;
    const AttentionMatch& am = fm.fwd;
    bool ok = true;
    for (int x : fm.hidden) ok = ok && !ts.bucket_offset.count(x);
    ok = ok && !ts.bucket_offset.count(am.t_sums);
    if (!ts.bucket_owned)   // the data-parallel step exchanges the bucket: its plans stay as they were
      for (int x : {fm.t_dq, fm.t_dk, fm.t_dv}) ok = ok && !ts.bucket_offset.count(x);
    Launch F;
    int outer_pos = 0;
    if (!ok || !plan_chain(m, ts, plan, infos, group_of, am, F, outer_pos)) continue;
    const eg::attention::Extents& E = F.attn.e;
    const std::vector<long>& S = shapes.at(am.t_scores);

    // ---- the gradient kernels: not grouped, on one side of the boundary, behind the chain
    const int first = fm.backward.front(), last = fm.backward.back();
    for (int s : fm.backward) ok = ok && group_of[s] == -1 && !ts.lowered[s].absorbed && !ts.lowered[s].inlined;
    ok = ok && !(t.first_update > first && t.first_update <= last);
    for (int s : {fm.p_de, fm.p_dsums, fm.p_de_sums, fm.p_dscale})
      if (s >= 0) ok = ok && rows_cover(t, infos, shapes, s, S);
    if (!ok) continue;
    // the four products: plan_batched2's checks, the chain's extents, and each operand's view in the launch's batch order
    struct Product {
      int pos;
      const Batched2GemmMatch* g;
      int like_scores;   // the tensor of the operand that is shaped like the scores
      long M, N, K;
    };
    const Product products[4] = {{fm.p_dsoftmax, &fm.dsoftmax, fm.t_dsoftmax, E.I, E.J, E.D},
                                 {fm.p_dv, &fm.dv, am.t_softmax, E.J, E.D, E.I},
                                 {fm.p_dq, &fm.dq, fm.t_dscores, E.I, E.K, E.J},
                                 {fm.p_dk, &fm.dk, fm.t_dscores, E.J, E.K, E.I}};
    std::map<int, eg::attention::View> views;   // tensor -> its view, from the product that names it
    for (const Product& pr : products) {
      const Kernel& k = t.all[t.live[pr.pos]];
      const KernelInfo& info = infos[t.live[pr.pos]];
      const Batched2GemmMatch& g = *pr.g;
      Launch P;
      ok = ok && ts.lowered[pr.pos].two_batch && plan_batched2(g, k, info, shapes, P) && P.M == pr.M && P.N == pr.N && P.K == pr.K;
      if (!ok) break;
      const Op* ops[3] = {&k.reads[g.a_read], &k.reads[g.b_read], &k.write};
      int os = -1;
      for (int o = 0; o < 3; ++o)
        if (ops[o]->tensor == pr.like_scores) os = o;
      ok = os >= 0 && g.batch_dim[os][0] <= 1 && g.batch_dim[os][1] <= 1 && g.batch_dim[os][0] != g.batch_dim[os][1];
      if (!ok) break;
      const int q_outer = g.batch_dim[os][0] == outer_pos ? 0 : 1, q_inner = 1 - q_outer;
      ok = info.bounds[g.lb[q_outer]].second == E.batch0 && info.bounds[g.lb[q_inner]].second == E.batch1;
      for (int o = 0; ok && o < 3; ++o) {
        if (o == os) continue;
        const std::vector<long>& dims = shapes.at(ops[o]->tensor);
        const eg::attention::View v = {stride_of(dims, g.row_dim[o]), stride_of(dims, g.batch_dim[o][q_outer]), stride_of(dims, g.batch_dim[o][q_inner])};
        auto seen = views.find(ops[o]->tensor);
        if (seen != views.end()) ok = seen->second == v;
        views[ops[o]->tensor] = v;
      }
    }
    if (!ok) continue;
    // q, kk and v as the gradient products see them are what the forward launch has
    auto same = [&](const Launch::Attn::Operand& x) {
      auto v = views.find(x.tensor);
      return v != views.end() && v->second == x.view;
    };
    if (!same(F.attn.q) || !same(F.attn.k) || !same(F.attn.v)) continue;
    if (!views.count(fm.t_do) || !views.count(fm.t_dq) || !views.count(fm.t_dk) || !views.count(fm.t_dv)) continue;
    if (shapes.at(fm.t_do) != shapes.at(am.t_out)) continue;

    // ---- where the launches stand (header): the forward at the chain's last kernel, the backward at the first gradient kernel
    auto touches = [&](const Kernel& k, int x, bool reads_too) {
      if (k.write.tensor == x) return true;
      for (auto& rd : k.reads)
        if (reads_too && rd.tensor == x) return true;
      return false;
    };
    std::set<int> members(fm.forward.begin(), fm.forward.end());
    members.insert(fm.backward.begin(), fm.backward.end());
    for (int s = am.at.front(); ok && s <= am.at.back(); ++s) {
      if (members.count(s)) continue;
      const Kernel& k = t.all[t.live[s]];
      ok = !touches(k, am.t_q, false) && !touches(k, am.t_k, false) && !touches(k, am.t_out, true);
    }
    const std::pair<int, int> outputs[3] = {{fm.t_dq, fm.p_dq}, {fm.t_dk, fm.p_dk}, {fm.t_dv, fm.p_dv}};
    for (int s = first; ok && s <= last; ++s) {
      if (members.count(s)) continue;
      const Kernel& k = t.all[t.live[s]];
      for (int x : {am.t_q, am.t_k, am.t_v, am.t_out, am.t_sums, fm.t_do}) ok = ok && !touches(k, x, false);
      for (auto& out : outputs)
        if (s < out.second) ok = ok && !touches(k, out.first, true);
    }
    if (!ok) continue;

    // ---- both launches
    F.attn.sums = {am.t_sums, outer_pos == 0 ? eg::attention::View{0, S[1] * S[2], S[2]} : eg::attention::View{0, S[2], S[1] * S[2]}};
    if (!eg::attention::plan_attention(problem_of(m, F.attn)).supported) continue;
    Launch G = F;
    G.kind = StepKind::AttentionGrad;
    G.lowered = first;
    Launch::Attn& A = G.attn;
    A.members = fm.backward;
    A.dout = {fm.t_do, views[fm.t_do]};
    A.dq = {fm.t_dq, views[fm.t_dq]};
    A.dk = {fm.t_dk, views[fm.t_dk]};
    A.dv = {fm.t_dv, views[fm.t_dv]};
    eg::attention::GradProblem gp;
    static_cast<eg::attention::Extents&>(gp) = A.e;
    gp.q = operand(A.q), gp.k = operand(A.k), gp.v = operand(A.v), gp.o = operand(A.o), gp.s = operand(A.sums);
    gp.dout = operand(A.dout), gp.dq = operand(A.dq), gp.dk = operand(A.dk), gp.dv = operand(A.dv);
    gp.cus = m->ctx->compute_units;
    if (!eg::attention::plan_attention_grad(gp).supported) continue;
    for (int s : members) group_of[s] = ATTENTION_GROUP_CODE;
    for (int x : fm.hidden) plan.attn_hidden.insert(x);
    plan.attn_groups[am.at.back()] = F;
    plan.attn_grad_groups[first] = G;
  }
  return EG_OK;
}

}  // namespace model
}  // namespace eg
