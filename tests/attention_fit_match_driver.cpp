// Host-only driver of the attention training step's matcher (tests/test_attention_fit_match_cpu.py): built with the host
// compiler against host/kd.cpp, host/match.cpp, host/match_attention.cpp, host/match_attention_grad.cpp and error.cpp, which
// shows that none of them needs HIP.
//   attention_fit_match_driver FILE...   every live position of every target of the kernel-description files, two lines each:
//     fit target=<name> pos=<n> match=1 scale=<%g> q= kk= v= out= sums= do= dq= dk= dv= members=<n> forward=<p,p,..> backward=<p,p,..> hidden=<name,name,..>
//     fit target=<name> pos=<n> match=0 why=<reason with _ for spaces>
//     fwd target=<name> pos=<n> match=<0|1> why=<reason, - for a match>        (match_attention, as tests/attention_match_driver.cpp has it)
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "exprgrad_hip.h"
#include "../exprgrad_amd/csrc/host/match.hpp"

static std::string underscored(const char* why) {
  std::string w = why;
  for (char& c : w)
    if (c == ' ') c = '_';
  return w;
}

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
    // unnamed tensors (the gradients) print as #<id>
    auto name = [&](int t) {
      if (!t) return std::string("-");
      const std::string& n = prog.tensors[t].name;
      return n.empty() || n == "-" || n == "grad" ? "#" + std::to_string(t) : n;
    };
    auto list = [](const std::vector<int>& v) {
      std::string s;
      for (int x : v) s += (s.empty() ? "" : ",") + std::to_string(x);
      return s;
    };
    for (const eg::kd::Target& t : prog.targets)
      for (size_t p = 0; p < t.live.size(); ++p) {
        eg::model::AttentionFitMatch m;
        const char* why = "";
        if (eg::model::match_attention_fit(prog, t, (int)p, m, &why)) {
          std::string hidden;
          for (int x : m.hidden) hidden += (hidden.empty() ? "" : ",") + name(x);
          printf("fit target=%s pos=%zu match=1 scale=%g q=%s kk=%s v=%s out=%s sums=%s do=%s dq=%s dk=%s dv=%s members=%zu forward=%s backward=%s hidden=%s\n",
                 t.name.c_str(), p, (double)m.fwd.scale, name(m.fwd.t_q).c_str(), name(m.fwd.t_k).c_str(), name(m.fwd.t_v).c_str(),
                 name(m.fwd.t_out).c_str(), name(m.fwd.t_sums).c_str(), name(m.t_do).c_str(), name(m.t_dq).c_str(), name(m.t_dk).c_str(),
                 name(m.t_dv).c_str(), m.forward.size() + m.backward.size(), list(m.forward).c_str(), list(m.backward).c_str(), hidden.c_str());
        } else {
          printf("fit target=%s pos=%zu match=0 why=%s\n", t.name.c_str(), p, underscored(why).c_str());
        }
        eg::model::AttentionMatch fm;
        why = "-";
        const bool hit = eg::model::match_attention(prog, t, (int)p, fm, &why);
        printf("fwd target=%s pos=%zu match=%d why=%s\n", t.name.c_str(), p, hit ? 1 : 0, hit ? "-" : underscored(why).c_str());
      }
  }
  return 0;
}
