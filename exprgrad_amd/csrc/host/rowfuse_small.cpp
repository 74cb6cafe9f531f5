// Small groups and map groups (rowfuse.hpp): runs of kernels over small tensors, or of elementwise maps, as one launch.
#include "rowfuse_internal.hpp"

namespace eg::kd {

bool is_small_kernel(const Program& prog, const Kernel& k, const KernelInfo& info, const Shapes& shapes) {
  if (!info.ok || !k.index_instrs.empty()) return false;
  if (!k.setup.empty() && !k.is_seed) return false;
  const std::vector<const Op*> ops = ops_of(k);
  for (const Op* op : ops) {
    auto it = shapes.find(op->tensor);
    if (it == shapes.end() || prodv(it->second) > SMALL_MAX) return false;
  }
  long work = 1;
  for (size_t l = 0; l < k.loops.size(); ++l) work *= std::max(0L, info.bounds[l].second - info.bounds[l].first);
  if (work > 65536) return false;
  std::vector<int> indep, red;
  bool scatter;
  split_loops(k, indep, red, scatter);
  return !scatter;
}

std::string small_kernel_body(const Kernel& k, const KernelInfo& info, const Shapes& shapes, const std::string& prefix,
                                     int serial, bool barrier) {
  std::string c;
  {
    const std::vector<Ty> ty = infer_types(k);
    std::vector<int> indep, red;
    bool scatter;
    split_loops(k, indep, red, scatter);
    long total = 1;
    for (int l : indep) total *= std::max(0L, info.bounds[l].second - info.bounds[l].first);
    auto element = [&](const Op& op) { return literal_element(op, shapes, prefix + std::to_string(op.tensor)); };
    c += "  // kernel " + std::to_string(serial) + ": " + to_text(k).substr(0, 90) + "\n";
    c += "  for (long idx = threadIdx.x; idx < " + std::to_string(total) + "L; idx += 256) {\n";
    for (auto& s : k.setup) c += "    const long r" + std::to_string(s.res) + " = " + std::to_string(info.vals.at(s.res)) + "L;\n";
    c += "    long rem = idx;\n";
    for (size_t i = indep.size(); i-- > 0;) {
      const int l = indep[i];
      const long ext = info.bounds[l].second - info.bounds[l].first;
      c += "    const long r" + std::to_string(k.loops[l].reg) + " = " + std::to_string(info.bounds[l].first) + "L + rem % " +
           std::to_string(ext) + "L; rem /= " + std::to_string(ext) + "L;\n";
    }
    c += "    float acc = 0.0f;\n";
    for (int l : red) {
      const std::string r = "r" + std::to_string(k.loops[l].reg);
      c += "    for (long " + r + " = " + std::to_string(info.bounds[l].first) + "L; " + r + " < " +
           std::to_string(info.bounds[l].second) + "L; ++" + r + ") {\n";
    }
    for (auto& rd : k.reads) c += "      const float r" + std::to_string(rd.reg) + " = " + element(rd) + ";\n";
    for (auto& ins : k.instrs) c += instr_line(k, ins, ty, shapes, "      ");
    c += "      acc = acc + r" + std::to_string(k.result) + ";\n";
    for (size_t i = 0; i < red.size(); ++i) c += "    }\n";
    const std::string w = element(k.write);
    c += "    " + w + " = " + w + " + acc;\n  }\n";
    if (barrier) c += "  __syncthreads();\n";
  }
  return c;
}

// the pointer arguments (every tensor of `touched`; g.ptr_args) and the head of the signature: `... name(t<ids>..., float GS, long EP`
static std::string small_signature(SmallGroup& g, const std::set<int>& written, const std::set<int>& touched) {
  g.ptr_args.assign(touched.begin(), touched.end());
  std::string sig = "extern \"C\" __global__ void __launch_bounds__(256) " + g.name + "(";
  for (size_t i = 0; i < g.ptr_args.size(); ++i) {
    const int t = g.ptr_args[i];
    sig += (i ? ", " : "") + std::string(written.count(t) ? "float* t" : "const float* t") + std::to_string(t);
  }
  return sig + std::string(g.ptr_args.empty() ? "" : ", ") + "float GS, long EP";
}

int generate_small_group(const std::vector<Kernel>& all, const std::vector<KernelInfo>& infos,
                         const Shapes& shapes, SmallGroup& g) {
  std::set<int> written, touched;
  for (int ki : g.kernel_index) {
    written.insert(all[ki].write.tensor);
    touched.insert(all[ki].write.tensor);
    for (auto& rd : all[ki].reads) touched.insert(rd.tensor);
  }
  const std::string sig = small_signature(g, written, touched) + ")";
  std::string c;
  for (size_t gi = 0; gi < g.kernel_index.size(); ++gi)
    c += small_kernel_body(all[g.kernel_index[gi]], infos[g.kernel_index[gi]], shapes, "t", (int)gi);
  g.source = sig + " {\n" + c + "}\n";
  return EG_OK;
}

bool is_map_kernel(const Program& prog, const Kernel& k, const KernelInfo& info, const Shapes& shapes, long& count) {
  (void)prog;
  if (!info.ok || !k.index_instrs.empty() || k.loops.size() != 1 || k.gen != Gen::None) return false;
  if (!k.setup.empty() && !k.is_seed) return false;
  const int it = k.loops[0].reg;
  const std::vector<const Op*> ops = ops_of(k);
  auto ws = shapes.find(k.write.tensor);
  if (ws == shapes.end()) return false;
  count = prodv(ws->second);
  if (count <= 0 || info.bounds[0].first != 0 || info.bounds[0].second != count) return false;
  for (const Op* op : ops) {
    auto sh = shapes.find(op->tensor);
    if (sh == shapes.end() || prodv(sh->second) != count) return false;
    if (!op->raw || op->dims.size() != 1 || op->dims[0].only_register() != it) return false;
  }
  return true;
}

int generate_map_group(const Program& prog, const std::vector<Kernel>& all, const std::vector<KernelInfo>& infos,
                       const Shapes& shapes, SmallGroup& g) {
  std::set<int> written, touched;
  std::vector<long> counts;  // distinct element counts, in order of first appearance = the segments
  std::vector<long> of_kernel;
  for (int ki : g.kernel_index) {
    long n = 0;
    if (!is_map_kernel(prog, all[ki], infos[ki], shapes, n)) {
      set_error("internal: kernel %d is not an elementwise map", ki);
      return EG_ERR_INVALID;
    }
    of_kernel.push_back(n);
    if (std::find(counts.begin(), counts.end(), n) == counts.end()) counts.push_back(n);
    written.insert(all[ki].write.tensor);
    touched.insert(all[ki].write.tensor);
    for (auto& rd : all[ki].reads) touched.insert(rd.tensor);
  }
  for (auto& f : g.fold_offset) written.insert(f.first);  // (the folded total is stored where the gradient lives)
  std::string sig = small_signature(g, written, touched);
  if (!g.fold_offset.empty()) sig += ", const float* __restrict__ slab, long FOLD";
  sig += ")";
  std::string c = "  const long block = blockIdx.x;\n";
  long first_block = 0;
  for (size_t seg = 0; seg < counts.size(); ++seg) {
    const long n = counts[seg], nblocks = (n + 255) / 256;
    c += std::string(seg ? "  else if" : "  if") + " (block < " + std::to_string(first_block + nblocks) + "L) {  // " +
         std::to_string(n) + " elements\n";
    c += "    const long idx = (block - " + std::to_string(first_block) + "L) * 256 + threadIdx.x;\n";
    c += "    if (idx < " + std::to_string(n) + "L) {\n";
    for (auto& f : g.fold_offset) {
      if (prodv(shapes.at(f.first)) != n || !touched.count(f.first)) continue;
      bool in_segment = false;
      for (size_t gi = 0; gi < g.kernel_index.size(); ++gi)
        if (of_kernel[gi] == n)
          for (auto& rd : all[g.kernel_index[gi]].reads) in_segment = in_segment || rd.tensor == f.first;
      if (!in_segment) continue;
      c += "      if (FOLD) {  // this element's sum over the batch: the samples' contributions in sample order\n";
      c += "        float total = 0.0f;\n";
      c += "        for (long s = 0; s < " + std::to_string(g.fold_rows) + "L; ++s) total = total + slab[s * " + std::to_string(g.fold_row_floats) +
           "L + " + std::to_string(f.second) + "L + idx];\n";
      c += "        t" + std::to_string(f.first) + "[idx] = total;\n      }\n";
    }
    for (size_t gi = 0; gi < g.kernel_index.size(); ++gi) {
      if (of_kernel[gi] != n) continue;
      const Kernel& k = all[g.kernel_index[gi]];
      const KernelInfo& info = infos[g.kernel_index[gi]];
      const std::vector<Ty> ty = infer_types(k);
      c += "      {  // " + to_text(k).substr(0, 100) + "\n";
      for (auto& s : k.setup) c += "        const long r" + std::to_string(s.res) + " = " + std::to_string(info.vals.at(s.res)) + "L;\n";
      c += "        const long r" + std::to_string(k.loops[0].reg) + " = idx;\n";
      for (auto& rd : k.reads) c += "        const float r" + std::to_string(rd.reg) + " = t" + std::to_string(rd.tensor) + "[idx];\n";
      for (auto& ins : k.instrs) c += instr_line(k, ins, ty, shapes, "        ");
      const std::string w = "t" + std::to_string(k.write.tensor) + "[idx]";
      c += "        " + w + " = " + w + " + (0.0f + r" + std::to_string(k.result) + ");\n      }\n";
    }
    c += "    }\n  }\n";
    first_block += nblocks;
  }
  g.blocks = first_block;
  g.source = sig + " {\n" + c + "}\n";
  return EG_OK;
}

}  // namespace eg::kd
