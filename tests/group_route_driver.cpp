// Host-only driver of the fusion groups' analyses and of the sample generator's member record (tests/test_group_cases_cpu.py):
// built with the host compiler against host/kd.cpp, host/codegen.cpp, host/match.cpp, host/rowfuse_*.cpp, switches.cpp and
// error.cpp, which shows that none of them needs HIP.
//   group_route_driver FILE TARGET NAME=d0xd1x... ...     the kernel-description file, a target, the shape of every input
// One line per live kernel of the target:
//   pos=<n> write=<tensor name or t<id>> row=<0|1> row_raw= row_small= row_work= ww=<W> wide=<0|1> wide_kind=map|rowsum|colsum|total|seed
//   wide_raw= wide_col=<0|1> sample=<0|1> sample_raw= sample_reduced= sample_seed= sample_work= member=<the entry, blanks as '_'>
// W is the width a wide group over the target would have: wide_width_of the first live kernel that has one (a [B] or
// single-element member has none of its own and is analysed at its group's width, as form_wide_groups does).
// `member` is the record (SampleMemberRoute) of the kernel emitted alone in a one-member sample group of 512 threads, in the
// words of eg_model_launch_text; `-` for a kernel analyse_sample_kernel refuses.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "exprgrad_hip.h"
#include "../exprgrad_amd/csrc/host/rowfuse.hpp"

using namespace eg::kd;

static std::string member_entry(const SampleMemberRoute& r) {
  std::string s;
  switch (r.kind) {
    case SampleMemberRoute::Seed: s = "seed"; break;
    case SampleMemberRoute::Raw: s = "raw"; break;
    case SampleMemberRoute::Items: s = "items"; break;
    case SampleMemberRoute::Scatter: s = "scatter"; break;
    case SampleMemberRoute::Split: s = "split_T=" + std::to_string(r.T); break;
    case SampleMemberRoute::Gather: s = "gather"; break;
    case SampleMemberRoute::Conv: s = "conv"; break;
  }
  if (r.kind == SampleMemberRoute::Split && r.ragged > 0) s += "_ragged=" + std::to_string(r.ragged);
  if (r.R > 1) s += "_R=" + std::to_string(r.R);
  if (r.trips >= 0) s += "_trips=" + std::to_string(r.trips) + (r.ragged_trip ? "_+ragged" : "");
  if (r.rolled) s += "_rolled";
  if (r.slab) s += r.slab == 1 ? "_slab" : "_slab+";
  return s;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: group_route_driver FILE TARGET NAME=d0xd1... ...\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  std::stringstream text;
  text << in.rdbuf();
  Program prog;
  if (parse(text.str().c_str(), prog) || compile_program(prog)) {
    fprintf(stderr, "%s: %s\n", argv[1], eg_last_error());
    return 2;
  }
  Target* t = prog.find_target(argv[2]);
  if (!t) {
    fprintf(stderr, "no target %s\n", argv[2]);
    return 2;
  }
  Shapes shapes;
  long B = 0;
  for (int a = 3; a < argc; ++a) {
    const std::string arg = argv[a];
    const size_t eq = arg.find('=');
    auto it = eq == std::string::npos ? prog.inputs.end() : prog.inputs.find(arg.substr(0, eq));
    if (it == prog.inputs.end()) {
      fprintf(stderr, "no input %s\n", arg.c_str());
      return 2;
    }
    std::vector<long> shp;
    std::stringstream dims(arg.substr(eq + 1));
    for (std::string d; std::getline(dims, d, 'x');) shp.push_back(atol(d.c_str()));
    shapes[it->second] = shp;
  }
  // the batch as the planner takes it: dimension 0 of the first bound input in tensor order
  for (auto& kv : shapes)
    if (!kv.second.empty()) {
      B = kv.second[0];
      break;
    }
  for (size_t i = 1; i < prog.tensors.size(); ++i)
    if (prog.tensors[i].kind == TK::Param) shapes[(int)i] = prog.tensors[i].shape;
  std::vector<KernelInfo> infos(t->all.size());
  for (size_t i = 0; i < t->all.size(); ++i) {
    const Kernel& k = t->all[i];
    bool ready = true;
    for (auto& r : k.reads) ready = ready && shapes.count(r.tensor);
    for (auto& s : k.setup) ready = ready && !(s.tensor && s.tensor != k.write.tensor && !shapes.count(s.tensor));
    if (ready && infer_kernel(prog, k, shapes, 0, infos[i])) {
      fprintf(stderr, "kernel %zu: %s\n", i, eg_last_error());
      return 2;
    }
  }
  long ww = 0;
  for (size_t p = 0; p < t->live.size() && !ww; ++p) ww = wide_width_of(t->all[t->live[p]], shapes, B);
  for (size_t p = 0; p < t->live.size(); ++p) {
    const int ki = t->live[p];
    const Kernel& k = t->all[ki];
    const RowKernelInfo ri = analyse_row_kernel(prog, k, infos[ki], shapes, B);
    const WideKernelInfo wi = analyse_wide_kernel(prog, k, infos[ki], shapes, B, ww);
    const SampleKernelInfo si = analyse_sample_kernel(prog, k, infos[ki], shapes, B);
    std::string member = "-";
    if (si.ok) {
      SampleGroup g;
      g.B = B;
      g.kernel_index = {ki};
      g.infos = {si};
      g.overwrite = {1};
      g.threads = 512;
      g.name = "probe";
      if (si.reduced) {
        long n = 1;
        for (long d : shapes.at(k.write.tensor)) n *= d;
        g.slab_offset[k.write.tensor] = 0;
        g.slab_floats = (n + 3) & ~3L;
      }
      if (generate_sample_group(t->all, infos, shapes, g)) {
        fprintf(stderr, "member %zu: %s\n", p, eg_last_error());
        return 2;
      }
      member = member_entry(g.routes.at(0));
    }
    const std::string& nm = prog.tensors[k.write.tensor].name;
    const char* const kinds[] = {"map", "rowsum", "colsum", "total"};
    printf("pos=%zu write=%s row=%d row_raw=%d row_small=%d row_work=%ld ww=%ld wide=%d wide_kind=%s wide_raw=%d wide_col=%d sample=%d sample_raw=%d "
           "sample_reduced=%d sample_seed=%d sample_work=%ld member=%s\n",
           p, nm.empty() || nm == "-" ? ("t" + std::to_string(k.write.tensor)).c_str() : nm.c_str(), (int)ri.ok, (int)ri.raw, (int)ri.small_only, ri.work,
           ww, (int)wi.ok, wi.seed ? "seed" : kinds[(int)wi.kind], (int)wi.raw, (int)(wi.col_loop >= 0), (int)si.ok, (int)si.raw, (int)si.reduced,
           (int)si.seed, si.work, member.c_str());
  }
  return 0;
}
