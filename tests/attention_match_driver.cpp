// Host-only driver of the forward attention chain's matcher (tests/test_attention_match_cpu.py): built with the host compiler
// against host/kd.cpp, host/match.cpp, host/match_attention.cpp and error.cpp, which shows that none of them needs HIP.
//   attention_match_driver FILE...   every live position of every target of the kernel-description files:
//     target=<name> pos=<n> match=1 n=<kernels> scale=<%g> q=<name> kk=<name> v=<name> out=<name> scores=<name> scaled=<name|-> sums=<name> softmax=<name>
//     target=<name> pos=<n> match=0 why=<reason with _ for spaces>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "exprgrad_hip.h"
#include "../exprgrad_amd/csrc/host/match.hpp"

int main(int argc, char** argv) {
  for (int f = 1; f < argc; ++f) {
    std::ifstream in(argv[f]);
    std::stringstream text;
    text << in.rdbuf();
    eg::kd::Program prog;
    if (eg::kd::parse(text.str().c_str(), prog) || eg::kd::compile_program(prog)) {
      fprintf(stderr, "%s: %s\n", argv[f], eg_last_error());
      return 2;
    }
    auto name = [&](int t) { return t ? prog.tensors[t].name.c_str() : "-"; };
    for (const eg::kd::Target& t : prog.targets)
      for (size_t p = 0; p < t.live.size(); ++p) {
        eg::model::AttentionMatch m;
        const char* why = "";
        if (eg::model::match_attention(prog, t, (int)p, m, &why)) {
          printf("target=%s pos=%zu match=1 n=%d scale=%g q=%s kk=%s v=%s out=%s scores=%s scaled=%s sums=%s softmax=%s\n", t.name.c_str(), p, m.n,
                 (double)m.scale, name(m.t_q), name(m.t_k), name(m.t_v), name(m.t_out), name(m.t_scores), name(m.t_scaled), name(m.t_sums),
                 name(m.t_softmax));
        } else {
          std::string w = why;
          for (char& c : w)
            if (c == ' ') c = '_';
          printf("target=%s pos=%zu match=0 why=%s\n", t.name.c_str(), p, w.c_str());
        }
      }
  }
  return 0;
}
