// Host-only driver of the batched contraction's matcher and planner (tests/test_batched_match_cpu.py): built with the host
// compiler against host/kd.cpp, host/match.cpp and kernels/gemm_plan.cpp, which shows that none of them needs HIP.
//   batched_match_driver match FILE...   every live kernel of every target of the kernel-description files:
//                                        file=<name> target=<name> pos=<n> loops=<n> match=0|1 collapsed= row_k= ta= tb=
//   batched_match_driver plan            stdin lines `batch M N K ta tb lda ldb ldc aligned`: plan_gemm_batched, twice
//   batched_match_driver route           stdin lines `M N K ta tb lda ldb ldc a b c bias` (1 = 16-byte aligned / present and
//                                        aligned, 2 = not aligned, bias 0 = none): plan_gemm as eg_sgemm's exact path
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "exprgrad_hip.h"
#include "../exprgrad_amd/csrc/host/match.hpp"
#include "../exprgrad_amd/csrc/kernels/gemm_plan.hpp"

using namespace eg::gemm;

static const char* route_name(Route r) {
  static const char* const names[] = {"small", "skinny", "kw8", "t96", "streamk", "remainder", "extra_rows", "bk32", "pair", "generic"};
  return names[(int)r];
}

static const char* second_name(Second s) {
  static const char* const names[] = {"none", "split_reduce", "tail_reduce", "streamk_fixup", "tree"};
  return names[(int)s];
}

static void print_plan(const GemmPlan& p) {
  printf("route=%s bm=%d bn=%d kb=%d vec=%d edge=%d tiles_m=%d tiles_n=%d splits=%d k_per_split=%ld edge_splits=%d tail_tiles=%d grid=%ld "
         "block=%d second=%s workspace_floats=%ld\n",
         route_name(p.route), p.bm, p.bn, p.kb, p.vec, (int)p.edge, p.tiles_m, p.tiles_n, p.splits, p.k_per_split, p.edge_splits, p.tail_tiles,
         p.grid, p.block, second_name(p.second), p.workspace_floats);
}

static GemmProblem problem(long M, long N, long K, int ta, int tb, long lda, long ldb, long ldc, int a, int b, int c, int bias) {
  GemmProblem p;
  p.M = M;
  p.N = N;
  p.K = K;
  p.a_kc = !ta;
  p.b_kc = tb != 0;
  p.lda = lda;
  p.ldb = ldb;
  p.ldc = ldc;
  p.a_aligned = a == 1;
  p.b_aligned = b == 1;
  p.c_aligned = c == 1;
  p.has_bias = bias != 0;
  p.bias_aligned = bias != 2;
  p.cus = 256;
  const bool vec_a = operand_vec(lda, p.a_kc ? K : M, p.a_aligned), vec_b = operand_vec(ldb, p.b_kc ? K : N, p.b_aligned);
  p.vec_ok = vec_a && vec_b;
  p.a_vec_only = vec_a && !vec_b;
  return p;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "match") {
    for (int f = 2; f < argc; ++f) {
      std::ifstream in(argv[f]);
      std::stringstream text;
      text << in.rdbuf();
      eg::kd::Program prog;
      if (eg::kd::parse(text.str().c_str(), prog) || eg::kd::compile_program(prog)) {
        fprintf(stderr, "%s: %s\n", argv[f], eg_last_error());
        return 2;
      }
      for (const eg::kd::Target& t : prog.targets)
        for (size_t p = 0; p < t.live.size(); ++p) {
          const eg::kd::Kernel& k = t.all[t.live[p]];
          eg::model::BatchedGemmMatch m;
          const bool hit = eg::model::match_batched_gemm(k, m);
          printf("file=%s target=%s pos=%zu loops=%zu match=%d collapsed=%d row_k=%d ta=%d tb=%d\n", argv[f], t.name.c_str(), p, k.loops.size(),
                 (int)hit, (int)(hit && m.collapsed), (int)(hit && m.row_k), (int)(hit && m.trans_a), (int)(hit && m.trans_b));
        }
    }
    return 0;
  }
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    if (mode == "plan") {
      long batch, M, N, K, lda, ldb, ldc;
      int ta, tb, aligned;
      if (!(in >> batch >> M >> N >> K >> ta >> tb >> lda >> ldb >> ldc >> aligned)) return 2;
      const int al = aligned ? 1 : 2;
      const GemmProblem p = problem(M, N, K, ta, tb, lda, ldb, ldc, al, al, al, 0);
      print_plan(plan_gemm_batched(p, batch, GemmSwitches()));
      print_plan(plan_gemm_batched(p, batch, GemmSwitches()));
    } else if (mode == "route") {
      long M, N, K, lda, ldb, ldc;
      int ta, tb, a, b, c, bias;
      if (!(in >> M >> N >> K >> ta >> tb >> lda >> ldb >> ldc >> a >> b >> c >> bias)) return 2;
      print_plan(plan_gemm(problem(M, N, K, ta, tb, lda, ldb, ldc, a, b, c, bias), GemmSwitches()));
    } else {
      fprintf(stderr, "usage: batched_match_driver match FILE... | plan | route\n");
      return 2;
    }
  }
  return 0;
}
