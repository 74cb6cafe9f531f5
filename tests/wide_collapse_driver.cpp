// Host-only driver of the wide row analysis over collapsed leading axes (tests/test_wide_collapse_cpu.py): built with the host
// compiler against host/kd.cpp, host/codegen.cpp, host/match.cpp, host/rowfuse_*.cpp, switches.cpp and error.cpp, which shows
// that the analysis needs no HIP.
//   wide_collapse_driver collapsed FILE TARGET NAME=d0xd1x... ...   the kernel-description file, a target, the shape of every input
//   wide_collapse_driver rank2     FILE TARGET NAME=d0xd1x... ...
// One line per live kernel of the target.
//   collapsed: pos=<n> write=<tensor name or t<id>> ok=<0|1> kind=map|rowsum|colsum|total|seed|- R=<rows> W=<width> rows=<d0xd1..|->
//     A kernel is analysed as the planner does it: at the rows and the width of the run it continues (a per-row or
//     single-element member has none of its own), else at those wide_width_of reports for the kernel itself.
//   rank2: pos=<n> write=.. ww=<W> ok=<0|1> kind=.. raw=<0|1> col=<0|1>
//     The [B, W] analysis exactly as the planner's second pass calls it (no `lead`), at the width of the run a kernel
//     continues, else at its own.  This mode uses nothing newer than the first wide row groups, so the same file built against an
//     older checkout with -DWIDE_COLLAPSE_RANK2_ONLY prints that checkout's decisions: tests/golden/wide_rank2_parent.txt
//     was made so from the commit before collapsed rows existed.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "exprgrad_hip.h"
#include "../exprgrad_amd/csrc/host/rowfuse.hpp"

using namespace eg::kd;

static const char* kind_name(const WideKernelInfo& wi) {
  const char* const kinds[] = {"map", "rowsum", "colsum", "total"};
  return !wi.ok ? "-" : wi.seed ? "seed" : kinds[(int)wi.kind];
}

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: wide_collapse_driver collapsed|rank2 FILE TARGET NAME=d0xd1... ...\n");
    return 2;
  }
  const std::string mode = argv[1];
  std::ifstream in(argv[2]);
  std::stringstream text;
  text << in.rdbuf();
  Program prog;
  if (parse(text.str().c_str(), prog) || compile_program(prog)) {
    fprintf(stderr, "%s: %s\n", argv[2], eg_last_error());
    return 2;
  }
  Target* t = prog.find_target(argv[3]);
  if (!t) {
    fprintf(stderr, "no target %s\n", argv[3]);
    return 2;
  }
  Shapes shapes;
  for (int a = 4; a < argc; ++a) {
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
  long B = 0;
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
  auto name_of = [&](const Kernel& k) {
    const std::string& nm = prog.tensors[k.write.tensor].name;
    return nm.empty() || nm == "-" ? "t" + std::to_string(k.write.tensor) : nm;
  };
  if (mode == "rank2") {
    long run_w = 0;  // the width of the run being continued
    for (size_t p = 0; p < t->live.size(); ++p) {
      const int ki = t->live[p];
      const Kernel& k = t->all[ki];
      long ww = run_w;
      WideKernelInfo wi;
      if (run_w) wi = analyse_wide_kernel(prog, k, infos[ki], shapes, B, run_w);
      if (!wi.ok) {
        ww = wide_width_of(k, shapes, B);
        wi = analyse_wide_kernel(prog, k, infos[ki], shapes, B, ww);
      }
      run_w = wi.ok ? ww : 0;
#ifndef WIDE_COLLAPSE_RANK2_ONLY
      // with `lead` a [B, W] tensor still decides: the same width, the rows {B}, the same analysis
      std::vector<long> lead;
      const long own = wide_width_of(k, shapes, B), with_lead = wide_width_of(k, shapes, B, &lead);
      if (own && (with_lead != own || lead != std::vector<long>{B})) {
        fprintf(stderr, "kernel at %zu: wide_width_of with lead disagrees (%ld against %ld)\n", p, with_lead, own);
        return 3;
      }
      const std::vector<long> rows = {B};
      const WideKernelInfo again = analyse_wide_kernel(prog, k, infos[ki], shapes, B, ww, &rows);
      if (again.ok != wi.ok || again.kind != wi.kind || again.raw != wi.raw || again.col_loop != wi.col_loop || again.row_loop != wi.row_loop) {
        fprintf(stderr, "kernel at %zu: the analysis with rows {B} disagrees\n", p);
        return 3;
      }
#endif
      printf("pos=%zu write=%s ww=%ld ok=%d kind=%s raw=%d col=%d\n", p, name_of(k).c_str(), ww, (int)wi.ok, kind_name(wi), (int)wi.raw,
             (int)(wi.col_loop >= 0));
    }
    return 0;
  }
#ifndef WIDE_COLLAPSE_RANK2_ONLY
  if (mode == "collapsed") {
    std::vector<long> run_lead;  // the run being continued
    long run_w = 0;
    for (size_t p = 0; p < t->live.size(); ++p) {
      const int ki = t->live[p];
      const Kernel& k = t->all[ki];
      auto rows_of = [](const std::vector<long>& lead) {
        long r = 1;
        for (long d : lead) r *= d;
        return r;
      };
      WideKernelInfo wi;
      std::vector<long> lead = run_lead;
      long W = run_w;
      if (run_w) wi = analyse_wide_kernel(prog, k, infos[ki], shapes, rows_of(run_lead), run_w, &run_lead);
      if (!wi.ok) {
        W = wide_width_of(k, shapes, B, &lead);
        if (W && lead.size() >= 2) wi = analyse_wide_kernel(prog, k, infos[ki], shapes, rows_of(lead), W, &lead);
        else wi = WideKernelInfo();
      }
      if (wi.ok) {
        run_lead = lead;
        run_w = W;
      } else {
        run_lead.clear();
        run_w = 0;
      }
      std::string rows;
      for (size_t d = 0; d < lead.size(); ++d) rows += (d ? "x" : "") + std::to_string(lead[d]);
      printf("pos=%zu write=%s ok=%d kind=%s R=%ld W=%ld rows=%s\n", p, name_of(k).c_str(), (int)wi.ok, kind_name(wi), lead.empty() ? 0 : rows_of(lead), W,
             rows.empty() ? "-" : rows.c_str());
    }
    return 0;
  }
#endif
  fprintf(stderr, "unknown mode %s\n", mode.c_str());
  return 2;
}
