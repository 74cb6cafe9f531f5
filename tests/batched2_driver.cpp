// Host-only driver of the matcher and the C rule of the products with two batch indices (tests/test_batched2_cpu.py): built
// with the host compiler against host/kd.cpp, host/match.cpp, kernels/gemm_plan.cpp and error.cpp, which shows that none of
// them needs HIP.
//   batched2_driver match FILE...   every live kernel of every target of the kernel-description files:
//                                   file= target= pos= loops= match=0|1 ta= tb= a= b= (tensor names of the A and B reads) and,
//                                   per operand x in a b c, x_batch=<dim>,<dim> x_row=<dim>
//   batched2_driver crule           stdin lines `batch0 stride_c0 batch1 stride_c1 M ldc N`: ok=0|1 (batched2_c_distinct)
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "exprgrad_hip.h"
#include "../exprgrad_amd/csrc/host/match.hpp"
#include "../exprgrad_amd/csrc/kernels/gemm_plan.hpp"

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
          eg::model::Batched2GemmMatch m;
          const bool hit = eg::model::match_batched2_gemm(k, m);
          printf("file=%s target=%s pos=%zu loops=%zu match=%d", argv[f], t.name.c_str(), p, k.loops.size(), (int)hit);
          if (hit) {
            printf(" ta=%d tb=%d a=%s b=%s", (int)m.trans_a, (int)m.trans_b, prog.tensors[k.reads[m.a_read].tensor].name.c_str(),
                   prog.tensors[k.reads[m.b_read].tensor].name.c_str());
            const char* names[3] = {"a", "b", "c"};
            for (int o = 0; o < 3; ++o) printf(" %s_batch=%d,%d %s_row=%d", names[o], m.batch_dim[o][0], m.batch_dim[o][1], names[o], m.row_dim[o]);
          }
          printf("\n");
        }
    }
    return 0;
  }
  if (mode != "crule") {
    fprintf(stderr, "usage: batched2_driver match FILE... | crule\n");
    return 2;
  }
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    long b0, s0, b1, s1, M, ldc, N;
    if (!(in >> b0 >> s0 >> b1 >> s1 >> M >> ldc >> N)) return 2;
    printf("ok=%d\n", (int)eg::gemm::batched2_c_distinct(b0, s0, b1, s1, M, ldc, N));
  }
  return 0;
}
