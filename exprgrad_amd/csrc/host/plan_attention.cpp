// Attention groups of a plan: a forward attention chain (match_attention) becomes ONE launch of eg_attention's internal
// entry (kernels/attention_f32.hip) — scores, scale, row sums and softmax live in the registers of its blocks and get no
// arena storage.  Formed before every other group, only when
//   - row fusion and the batched products are both enabled (EG_NO_ROWFUSE, EG_NO_BATCHED_GEMM: the plan is then the unfused one);
//   - the model does not keep values (eg_model_keep_values) and computes in float32 (make_plan calls this under `fuse`);
//   - plan_batched2's checks pass for both products (loops from 0, extents at least 1, rank-4 dense shapes covered by the loops);
//   - the three kernels between them run over exactly the scores' shape, which the products' loops cover exactly;
//   - no intermediate is a gradient-bucket member, and the chain does not straddle the backward | update boundary;
//   - plan_attention (kernels/attention_plan.cpp) supports the shape: K and D at most 128.
// Anything else keeps the plan it had: two eg_bgemm2 launches around a collapsed wide row group, or generated kernels.
#include "../kernels/attention_plan.hpp"
#include "model_types.hpp"

namespace eg {
namespace model {

int form_attention_groups(eg_model* m, TargetState& ts, Plan& plan, const std::vector<KernelInfo>& infos, const std::map<int, int>& first_writer,
                          std::vector<int>& group_of) {
  (void)first_writer;
  plan.attn_groups.clear();
  plan.attn_hidden.clear();
  if (!row_fusion_enabled() || eg::sw::on(eg::Sw::NO_BATCHED_GEMM) || m->keep_values || m->f64) return EG_OK;
  const Target& t = *ts.target;
  const Shapes& shapes = plan.shapes;
  const int n = (int)t.live.size();
  auto stride = [](const std::vector<long>& dims, int d) {
    long st = 1;
    for (size_t e = (size_t)d + 1; e < dims.size(); ++e) st *= dims[e];
    return st;
  };
  for (int p = 0; p + 4 <= n; ++p) {
    AttentionMatch am;
    if (group_of[p] != -1 || !match_attention(m->prog, t, p, am)) continue;
    const int last = p + am.n - 1;
    bool ok = ts.lowered[p].two_batch && ts.lowered[last].two_batch;
    for (int s = p; s <= last; ++s) ok = ok && group_of[s] == -1 && !ts.lowered[s].absorbed && !ts.lowered[s].inlined;
    ok = ok && !(t.first_update > p && t.first_update <= last);
    for (int x : {am.t_scores, am.t_scaled, am.t_sums, am.t_softmax}) ok = ok && (!x || !ts.bucket_offset.count(x));
    if (!ok) continue;
    const Kernel& k0 = t.all[t.live[p]];
    const Kernel& k4 = t.all[t.live[last]];
    const KernelInfo& i0 = infos[t.live[p]];
    const KernelInfo& i4 = infos[t.live[last]];
    Launch L0, L4;
    if (!plan_batched2(am.scores, k0, i0, shapes, L0) || !plan_batched2(am.context, k4, i4, shapes, L4)) continue;
    const Batched2GemmMatch& g0 = am.scores;
    const Batched2GemmMatch& g4 = am.context;
    // the scores' shape [x0, x1, I, J]: covered exactly by both products and by every kernel between them
    const std::vector<long>& S = shapes.at(am.t_scores);
    ok = S.size() == 4 && L0.M == L4.M && L0.N == L4.K && S[2] == L0.M && S[3] == L0.N;
    for (int q = 0; ok && q < 2; ++q)
      ok = S[g0.batch_dim[2][q]] == i0.bounds[g0.lb[q]].second && S[g4.batch_dim[0][q]] == i4.bounds[g4.lb[q]].second;
    for (int s = p + 1; ok && s < last; ++s) {
      const Kernel& k = t.all[t.live[s]];
      const KernelInfo& info = infos[t.live[s]];
      ok = info.ok;
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
      ok = ok && ws != shapes.end() && ws->second == (k.write.dims.size() == 4 ? S : std::vector<long>(S.begin(), S.begin() + 3));
    }
    if (!ok) continue;
    // The context's batch register with the larger stride in its output is the outer index (as plan_batched2 has it); the
    // scores' batch register at the same position of the scores is its partner.
    const std::vector<long>& Qs = shapes.at(am.t_q);
    const std::vector<long>& Ks = shapes.at(am.t_k);
    const std::vector<long>& Vs = shapes.at(am.t_v);
    const std::vector<long>& Os = shapes.at(am.t_out);
    const int outer4 = stride(Os, g4.batch_dim[2][0]) >= stride(Os, g4.batch_dim[2][1]) ? 0 : 1, inner4 = 1 - outer4;
    auto partner = [&](int q4) {
      for (int r = 0; r < 2; ++r)
        if (g0.batch_dim[2][r] == g4.batch_dim[0][q4]) return r;
      return -1;
    };
    const int outer0 = partner(outer4), inner0 = partner(inner4);
    if (outer0 < 0 || inner0 < 0 || outer0 == inner0) continue;
    Launch L;
    L.kind = StepKind::Attention;
    L.lowered = p;
    L.standalone = true;
    L.a_tensor = am.t_q;
    L.b_tensor = am.t_k;
    L.v_tensor = am.t_v;
    L.c_tensor = am.t_out;
    L.batch = i4.bounds[g4.lb[outer4]].second;
    L.batch1 = i4.bounds[g4.lb[inner4]].second;
    if (L.batch != i0.bounds[g0.lb[outer0]].second || L.batch1 != i0.bounds[g0.lb[inner0]].second) continue;
    L.M = L0.M;
    L.N = L0.N;
    L.K = L0.K;
    L.attn_d = L4.N;
    L.attn_scale = am.scale;
    L.lda = L0.lda;
    L.ldb = L0.ldb;
    L.ldv = L4.ldb;
    L.ldc = L4.ldc;
    L.stride_a = stride(Qs, g0.batch_dim[0][outer0]);
    L.stride_a1 = stride(Qs, g0.batch_dim[0][inner0]);
    L.stride_b = stride(Ks, g0.batch_dim[1][outer0]);
    L.stride_b1 = stride(Ks, g0.batch_dim[1][inner0]);
    L.stride_v = stride(Vs, g4.batch_dim[1][outer4]);
    L.stride_v1 = stride(Vs, g4.batch_dim[1][inner4]);
    L.stride_c = stride(Os, g4.batch_dim[2][outer4]);
    L.stride_c1 = stride(Os, g4.batch_dim[2][inner4]);
    eg::attention::Problem pr;
    pr.batch0 = L.batch, pr.batch1 = L.batch1, pr.I = L.M, pr.J = L.N, pr.K = L.K, pr.D = L.attn_d;
    pr.q = {L.lda, L.stride_a, L.stride_a1, true};
    pr.k = {L.ldb, L.stride_b, L.stride_b1, true};
    pr.v = {L.ldv, L.stride_v, L.stride_v1, true};
    pr.o = {L.ldc, L.stride_c, L.stride_c1, true};
    pr.cus = m->ctx->compute_units;
    if (!eg::attention::plan_attention(pr).supported) continue;   // K or D above 128: the unfused plan
    for (int s = p; s <= last; ++s) {
      group_of[s] = ATTENTION_GROUP_CODE;
      L.attn_members.push_back(s);
    }
    for (int x : {am.t_scores, am.t_scaled, am.t_sums, am.t_softmax})
      if (x) plan.attn_hidden.insert(x);
    plan.attn_groups[p] = L;
    p = last;
  }
  return EG_OK;
}

}  // namespace model
}  // namespace eg
