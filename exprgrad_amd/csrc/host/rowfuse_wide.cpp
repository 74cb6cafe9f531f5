// Wide row groups: one WAVE per sample (rowfuse.hpp).
#include "rowfuse_internal.hpp"

namespace eg::kd {

long wide_width_of(const Kernel& k, const Shapes& shapes, long B, std::vector<long>* lead) {
  auto width = [&](const Op& op) -> long {
    auto it = shapes.find(op.tensor);
    return it != shapes.end() && it->second.size() == 2 && it->second[0] == B ? it->second[1] : 0;
  };
  long w = 0;
  for (auto& rd : k.reads)
    if (!w) w = width(rd);
  if (!w) w = width(k.write);
  if (!lead) return w;
  lead->clear();
  if (w) {  // a [B, W] tensor decides, as without `lead`
    lead->push_back(B);
    return w;
  }
  // collapsed leading axes: the first operand of the highest rank among 3 and 4 (a per-row operand has one dimension less)
  const std::vector<long>* best = nullptr;
  for (const Op* op : ops_of(k)) {
    auto it = shapes.find(op->tensor);
    if (it == shapes.end() || it->second.size() < 3 || it->second.size() > 4) continue;
    if (!best || it->second.size() > best->size()) best = &it->second;
  }
  if (!best) return 0;
  lead->assign(best->begin(), best->end() - 1);
  return best->back();
}

// A wide row kernel over collapsed leading axes (rowfuse.hpp): `lead` are the extents d0 .. d(r-2), W the row's width.
static WideKernelInfo analyse_collapsed_kernel(const Program& prog, const Kernel& k, const KernelInfo& info, const Shapes& shapes,
                                               const std::vector<long>& lead, long W) {
  WideKernelInfo r;
  const long R = prodv(lead);
  const size_t nlead = lead.size();
  if (nlead < 2 || nlead > 3 || R <= 0) return r;
  const std::vector<const Op*> ops = ops_of(k);
  for (const Op* op : ops)
    if (!shapes.count(op->tensor)) return r;
  auto state = [&](const Op* op) {
    const TK kind = prog.tensors[op->tensor].kind;
    return kind == TK::Param || kind == TK::Cache;
  };
  auto single = [&](const Op* op) {  // one element, addressed by constants
    for (auto& d : op->dims)
      if (!d.factors.empty()) return false;
    return prodv(shapes.at(op->tensor)) == 1;
  };
  auto used_as_value = [&](int reg) {
    for (auto& ins : k.instrs)
      for (int a : ins.args)
        if (a == reg) return true;
    return false;
  };
  if (!k.setup.empty() || k.loops.empty() || k.loops.size() > nlead + 1) return r;
  for (auto& l : k.loops)
    if (l.has_bounds) return r;
  std::vector<long> row_shape = lead;
  row_shape.push_back(W);
  bool any_raw = false;
  for (const Op* op : ops) any_raw = any_raw || (op->raw && !single(op));
  if (any_raw) {
    // a raw map over R * W elements: it = row * W + x
    if (k.loops.size() != 1 || info.bounds[0].first != 0 || info.bounds[0].second != R * W) return r;
    const int it = k.loops[0].reg;
    if (used_as_value(it)) return r;
    for (const Op* op : ops) {
      if (single(op)) continue;
      if (!op->raw || op->dims.size() != 1 || op->dims[0].only_register() != it || state(op) || shapes.at(op->tensor) != row_shape) return r;
    }
    r.ok = true;
    r.raw = true;
    r.row_loop = 0;
    r.row_loops = {0};
    r.kind = single(&k.write) ? WideKernelInfo::AllRed : WideKernelInfo::Map;
    return r;
  }
  // The registers by POSITION: the first row or per-row operand names them, every other one must agree.  Extents decide
  // nothing (I == J, a leading extent equal to W): a [lead.., W] tensor has rank r, a [lead..] tensor rank r - 1 >= 2, a [W]
  // tensor rank 1.
  std::vector<int> regs(nlead, 0);
  int x = 0;
  bool named = false;
  std::vector<int> kinds(ops.size(), 0);  // per op: 0 single element, 1 row tensor, 2 per-row tensor, 3 [W]
  for (size_t o = 0; o < ops.size(); ++o) {
    const Op* op = ops[o];
    if (single(op)) {
      kinds[o] = 0;
      continue;
    }
    const std::vector<long>& shp = shapes.at(op->tensor);
    if (op->raw || op->dims.size() != shp.size()) return r;
    std::vector<int> at(op->dims.size());
    for (size_t d = 0; d < op->dims.size(); ++d)
      if (!(at[d] = op->dims[d].only_register())) return r;  // bare registers only
    if (shp == row_shape || shp == lead) {
      if (state(op)) return r;
      kinds[o] = shp == row_shape ? 1 : 2;
      for (size_t d = 0; d < nlead; ++d) {
        if (named && regs[d] != at[d]) return r;  // another register at this position
        regs[d] = at[d];
      }
      named = true;
      if (kinds[o] == 1) {
        if (x && x != at[nlead]) return r;
        x = at[nlead];
      }
    } else if (shp.size() == 1 && shp[0] == W) {
      kinds[o] = 3;
      if (x && x != at[0]) return r;
      x = at[0];
    } else {
      return r;
    }
  }
  if (!named) return r;  // nothing indexed by the row
  for (size_t d = 0; d < nlead; ++d) {
    if (regs[d] == x) return r;
    for (size_t e = 0; e < d; ++e)
      if (regs[d] == regs[e]) return r;  // one register at two positions
  }
  // every loop is one of those registers, over its tensor extent; a loop no operand uses can only be x
  r.row_loops.assign(nlead, -1);
  for (size_t l = 0; l < k.loops.size(); ++l) {
    const int reg = k.loops[l].reg;
    if (used_as_value(reg)) return WideKernelInfo();
    size_t d = 0;
    while (d < nlead && regs[d] != reg) ++d;
    const long extent = d < nlead ? lead[d] : W;
    if (info.bounds[l].first != 0 || info.bounds[l].second != extent) return WideKernelInfo();
    if (d < nlead) {
      r.row_loops[d] = (int)l;
    } else {
      if ((x && x != reg) || r.col_loop >= 0) return WideKernelInfo();
      r.col_loop = (int)l;
    }
  }
  for (int l : r.row_loops)
    if (l < 0) return WideKernelInfo();
  if (x && r.col_loop < 0) return WideKernelInfo();
  r.ok = true;
  r.row_loop = r.row_loops[0];
  const int wk = kinds[ops.size() - 1];  // (ops_of: the write is last)
  r.kind = wk == 1 ? WideKernelInfo::Map : wk == 2 ? WideKernelInfo::RowRed : wk == 3 ? WideKernelInfo::ColRed : WideKernelInfo::AllRed;
  return r;
}

WideKernelInfo analyse_wide_kernel(const Program& prog, const Kernel& k, const KernelInfo& info, const Shapes& shapes, long B, long W,
                                   const std::vector<long>* lead) {
  WideKernelInfo r;
  if (!info.ok || B <= 0 || W < WIDE_MIN_W || W > WIDE_MAX_W || !k.index_instrs.empty() || k.f64) return r;
  if (lead && lead->size() >= 2 && !k.is_seed) return prodv(*lead) == B ? analyse_collapsed_kernel(prog, k, info, shapes, *lead, W) : r;
  const std::vector<const Op*> ops = ops_of(k);
  for (const Op* op : ops)
    if (!shapes.count(op->tensor)) return r;
  auto state = [&](const Op* op) {
    const TK kind = prog.tensors[op->tensor].kind;
    return kind == TK::Param || kind == TK::Cache;
  };
  auto single = [&](const Op* op) {  // one element, addressed by constants
    for (auto& d : op->dims)
      if (!d.factors.empty()) return false;
    return prodv(shapes.at(op->tensor)) == 1;
  };
  auto used_as_value = [&](int reg) {
    for (auto& ins : k.instrs)
      for (int a : ins.args)
        if (a == reg) return true;
    return false;
  };
  if (k.is_seed) {  // gradLoss{i} = 1 over one element: every lane keeps the value
    if (k.loops.size() <= 1 && single_extent(info) && prodv(shapes.at(k.write.tensor)) == 1 && k.reads.empty()) {
      r.ok = true;
      r.seed = true;
    }
    return r;
  }
  if (!k.setup.empty() || k.loops.empty() || k.loops.size() > 2) return r;
  for (auto& l : k.loops)
    if (l.has_bounds) return r;
  const std::vector<long> row_shape = {B, W};
  bool any_raw = false;
  for (const Op* op : ops) any_raw = any_raw || (op->raw && !single(op));
  if (any_raw) {
    // a raw map over B * W elements: it = y * W + x
    if (k.loops.size() != 1 || info.bounds[0].first != 0 || info.bounds[0].second != B * W) return r;
    const int it = k.loops[0].reg;
    if (used_as_value(it)) return r;
    for (const Op* op : ops) {
      if (single(op)) continue;
      if (!op->raw || op->dims.size() != 1 || op->dims[0].only_register() != it || state(op) || shapes.at(op->tensor) != row_shape) return r;
    }
    r.ok = true;
    r.raw = true;
    r.row_loop = 0;
    r.kind = single(&k.write) ? WideKernelInfo::AllRed : WideKernelInfo::Map;
    return r;
  }
  // y (and x): with B == W the [B, W] operands tell the two apart; a kernel without one takes its only loop for y
  for (size_t ly = 0; ly < k.loops.size(); ++ly) {
    const int lx = k.loops.size() == 2 ? 1 - (int)ly : -1;
    if (info.bounds[ly].first != 0 || info.bounds[ly].second != B) continue;
    if (lx >= 0 && (info.bounds[lx].first != 0 || info.bounds[lx].second != W)) continue;
    const int y = k.loops[ly].reg, x = lx >= 0 ? k.loops[lx].reg : 0;
    if (used_as_value(y) || (x && used_as_value(x))) continue;
    bool ok = true, by_row = false;
    auto kind_of = [&](const Op* op) {  // 0 single element, 1 [B, W], 2 [B], 3 [W], -1 none of them
      if (single(op)) return 0;
      const std::vector<long>& shp = shapes.at(op->tensor);
      if (op->raw || op->dims.size() != shp.size()) return -1;
      if (shp.size() == 2 && x && op->dims[0].only_register() == y && op->dims[1].only_register() == x && shp == row_shape && !state(op)) return 1;
      if (shp.size() == 1 && op->dims[0].only_register() == y && shp[0] == B && !state(op)) return 2;
      if (shp.size() == 1 && x && op->dims[0].only_register() == x && shp[0] == W) return 3;
      return -1;
    };
    for (const Op* op : ops) {
      const int kd = kind_of(op);
      ok = ok && kd >= 0;
      by_row = by_row || kd == 1 || kd == 2;
    }
    if (!ok || !by_row) continue;
    r.ok = true;
    r.row_loop = (int)ly;
    r.col_loop = lx;
    const int wk = kind_of(&k.write);
    r.kind = wk == 1 ? WideKernelInfo::Map : wk == 2 ? WideKernelInfo::RowRed : wk == 3 ? WideKernelInfo::ColRed : WideKernelInfo::AllRed;
    return r;
  }
  return r;
}

int generate_wide_group(const std::vector<Kernel>& all, const Shapes& shapes, RowGroup& g) {
  const long W = g.W, NJ = (W + 63) / 64;
  const std::string WL = std::to_string(W) + "L", NJs = std::to_string(NJ);
  auto role_of = [&](int t) -> const RowGroupTensor& { return g.tensors.at(t); };
  g.single_block = false;
  g.in_kernel_finalize = false;
  g.tail_kernels.clear();
  g.tail_ptr_args.clear();
  set_pointer_args(g);
  // two waves per SIMD at least (at most 256 registers): the next block's loads run under this one's arithmetic
  std::string sig = "extern \"C\" __global__ void __launch_bounds__(256, 2) " + g.name + "(float* __restrict__ partial";
  for (int t : g.ptr_args)
    sig += (role_of(t).role == RowGroupTensor::RowLocal ? ", float* __restrict__ t" : ", const float* __restrict__ t") + std::to_string(t);
  sig += ", long B, float GS, long EP)";

  std::string c;
  // (the wave index as a scalar: the sample, its row offset and the [B] operands stay in scalar registers)
  c += "  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));\n";
  for (auto& kv : g.tensors) {  // batch totals: once per lane
    if (kv.second.role != RowGroupTensor::Reduction) continue;
    const std::string id = std::to_string(kv.first);
    if (kv.second.inner == 1) c += "  float A" + id + " = 0.0f;\n";
    else c += "  float C" + id + "[" + NJs + "];\n  _Pragma(\"unroll\") for (int j = 0; j < " + NJs + "; ++j) C" + id + "[j] = 0.0f;\n";
  }
  c += "  auto one_sample = [&](const long y) {\n";
  c += "    const long row = y * " + WL + " + lane;\n";
  const std::string in_row = "(lane + 64 * j < " + std::to_string(W) + ")";
  for (auto& kv : g.tensors) {
    const RowGroupTensor& t = kv.second;
    const std::string id = std::to_string(kv.first);
    const bool mem = std::find(g.ptr_args.begin(), g.ptr_args.end(), kv.first) != g.ptr_args.end();
    if ((t.role == RowGroupTensor::RowLocal || t.role == RowGroupTensor::RowExternal) && t.inner == W && mem)
      c += std::string("    ") + (t.role == RowGroupTensor::RowLocal ? "float* const p" : "const float* const p") + id + " = t" + id + " + row;\n";
    if (t.role == RowGroupTensor::RowLocal && t.inner == W) {
      c += "    float L" + id + "[" + NJs + "];\n    _Pragma(\"unroll\") for (int j = 0; j < " + NJs + "; ++j) L" + id + "[j] = ";
      c += t.load_first ? "p" + id + "[" + in_row + " ? 64 * j : 0];\n" : "0.0f;\n";
    } else if (t.role == RowGroupTensor::RowLocal) {
      c += "    float V" + id + " = " + (t.load_first ? "t" + id + "[y]" : std::string("0.0f")) + ";\n";
    } else if (t.role == RowGroupTensor::SmallLocal) {
      c += "    float S" + id + " = 0.0f;\n";
    }
  }
  // text of the element a tensor op refers to, for column lane + 64 * j
  auto element = [&](const Op& op) {
    const RowGroupTensor& gt = role_of(op.tensor);
    const std::string id = std::to_string(op.tensor);
    switch (gt.role) {
      case RowGroupTensor::RowLocal: return gt.inner == W ? "L" + id + "[j]" : "V" + id;
      case RowGroupTensor::RowExternal: return gt.inner == W ? "p" + id + "[in ? 64 * j : 0]" : "t" + id + "[y]";
      case RowGroupTensor::SmallExternal: return gt.inner == W ? "t" + id + "[lane + (in ? 64 * j : 0)]" : "t" + id + "[0]";
      case RowGroupTensor::SmallLocal: return "S" + id;
      case RowGroupTensor::Reduction: return gt.inner == W ? "C" + id + "[j]" : "A" + id;
    }
    return std::string();
  };
  for (size_t i = 0; i < g.kernel_index.size(); ++i) {
    const Kernel& k = all[g.kernel_index[i]];
    const WideKernelInfo& wi = g.wide[i];
    const std::vector<Ty> ty = infer_types(k);
    c += "    {  // kernel " + std::to_string(i) + ": " + to_text(k).substr(0, 90) + "\n";
    if (wi.seed) {
      c += "      S" + std::to_string(k.write.tensor) + " = S" + std::to_string(k.write.tensor) + " + GS;\n    }\n";
      continue;
    }
    const bool columns = wi.raw || wi.col_loop >= 0;
    const bool row_sum = wi.kind == WideKernelInfo::RowRed && columns;
    if (row_sum) c += "      float acc = 0.0f;\n";
    if (columns) c += "      _Pragma(\"unroll\") for (int j = 0; j < " + NJs + "; ++j) {\n        const bool in = " + in_row + ";\n";
    else if (wi.kind == WideKernelInfo::AllRed) c += "      if (lane == 0) {\n";   // one term per sample
    else c += "      {\n";
    for (auto& rd : k.reads) c += "        const float r" + std::to_string(rd.reg) + " = " + element(rd) + ";\n";
    for (auto& ins : k.instrs) c += instr_line(k, ins, ty, shapes, "        ");
    // Lanes beyond the row's end (the last j only) run the same instructions on column `lane` of their row (a load that
    // is always in bounds, no branch in the body: the loads of a sample are issued together) and their values are
    // dropped: they add nothing to a sum and are not stored.
    const std::string w = row_sum ? std::string("acc") : element(k.write);
    const bool sum_of_lanes = columns && (row_sum || wi.kind == WideKernelInfo::AllRed);
    const std::string term = "r" + std::to_string(k.result);
    c += "        " + w + " = " + w + " + " + (sum_of_lanes ? "(in ? " + term + " : 0.0f)" : term) + ";\n      }\n";
    if (row_sum) {  // the lanes' sums -> the row's, the same value in every lane
      for (int off = 32; off >= 1; off >>= 1) c += "      acc += eg_xor_lane<" + std::to_string(off) + ">(acc);\n";
      const std::string v = element(k.write);
      c += "      " + v + " = " + v + " + acc;\n";
    }
    c += "    }\n";
  }
  for (auto& kv : g.tensors) {  // rows that are needed after the group
    const RowGroupTensor& t = kv.second;
    if (t.role != RowGroupTensor::RowLocal || !t.store) continue;
    const std::string id = std::to_string(kv.first);
    if (t.inner == W) c += "    _Pragma(\"unroll\") for (int j = 0; j < " + NJs + "; ++j) if " + in_row + " p" + id + "[64 * j] = L" + id + "[j];\n";
    else c += "    if (lane == 0) t" + id + "[y] = V" + id + ";\n";
  }
  c += "  };\n";
  c += "  for (long y = (long)blockIdx.x * 4 + wave; y < B; y += (long)gridDim.x * 4) one_sample(y);\n";
  // batch reductions: the four waves' accumulators through LDS, one partial row per block (row_finalize_kernel adds the blocks)
  if (g.red_total > 0) {
    const std::string E = std::to_string(g.red_total), ES = std::to_string(g.red_stride());
    c += "  __shared__ float red[4 * " + E + "];\n";
    for (auto& kv : g.tensors) {
      const RowGroupTensor& t = kv.second;
      if (t.role != RowGroupTensor::Reduction) continue;
      const std::string id = std::to_string(kv.first), off = std::to_string(t.red_offset);
      if (t.inner == W) {
        c += "  _Pragma(\"unroll\") for (int j = 0; j < " + NJs + "; ++j) if " + in_row + " red[wave * " + E + " + " + off + " + lane + 64 * j] = C" + id + "[j];\n";
      } else {
        for (int o = 32; o >= 1; o >>= 1) c += "  A" + id + " += eg_xor_lane<" + std::to_string(o) + ">(A" + id + ");\n";
        c += "  if (lane == 0) red[wave * " + E + " + " + off + "] = A" + id + ";\n";
      }
    }
    c += "  __syncthreads();\n";
    c += "  for (int e = threadIdx.x; e < " + E + "; e += 256) {\n";
    c += "    const float total = (red[e] + red[" + E + " + e]) + (red[2 * " + E + " + e] + red[3 * " + E + " + e]);\n";
    c += "    partial[(long)blockIdx.x * " + ES + " + e] = total;\n  }\n";
  }
  g.source = xor_lane_prelude() + sig + " {\n" + c + "}\n";
  return EG_OK;
}

}  // namespace eg::kd
