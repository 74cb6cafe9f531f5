// Prints the plans of exprgrad_amd/csrc/kernels/gemm_plan.cpp for the cases on stdin (tests/test_gemm_plan_cpu.py).
// One case per line:  mode M N K ta tb lda ldb ldc a b c bias vec switches
//   mode      exact (eg_sgemm's exact path), ones (the virtual row of ones, M without it), conv1 / conv2 (implicit GEMM),
//             single (exact_single_launch), fused (the generic tile of a fused launch)
//   a b c     base pointer of A / B / C: 1 = 16-byte aligned, 2 = not;  bias: 0 = none, 1 / 2 as above
//   vec       conv1 / conv2: the operands qualify for 16-byte loads
//   switches  "-" or a comma list: no_pair, force_tile=128x128, force_splits=4, streamk_blocks=3, ...
// One output line per case: key=value pairs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../exprgrad_amd/csrc/kernels/gemm_plan.hpp"

using namespace eg::gemm;

static GemmSwitches parse_switches(const std::string& list) {
  GemmSwitches s;
  std::stringstream ss(list);
  std::string item;
  while (std::getline(ss, item, ',')) {
    const size_t eq = item.find('=');
    const std::string name = item.substr(0, eq), value = eq == std::string::npos ? "" : item.substr(eq + 1);
    if (name == "-") continue;
    else if (name == "no_small") s.no_small = true;
    else if (name == "no_skinny") s.no_skinny = true;
    else if (name == "no_pair") s.no_pair = true;
    else if (name == "no_t96") s.no_t96 = true;
    else if (name == "no_streamk") s.no_streamk = true;
    else if (name == "no_xrow") s.no_xrow = true;
    else if (name == "no_bk32") s.no_bk32 = true;
    else if (name == "no_wide_store") s.no_wide_store = true;
    else if (name == "no_skew") s.no_skew = true;
    else if (name == "old_tile_model") s.old_tile_model = true;
    else if (name == "small_bk32") s.small_bk32 = true;
    else if (name == "force_tile") {
      s.force_tile = true;
      sscanf(value.c_str(), "%dx%d", &s.force_bm, &s.force_bn);
    } else if (name == "force_splits") {
      s.force_splits = true;
      s.force_splits_n = atoi(value.c_str());
    } else if (name == "streamk_blocks") {
      s.streamk_blocks = true;
      s.streamk_blocks_per_cu = atol(value.c_str());
    } else if (name == "streamk_min_ratio") {
      s.streamk_min_ratio = atof(value.c_str());
    } else {
      fprintf(stderr, "unknown switch %s\n", name.c_str());
      exit(2);
    }
  }
  return s;
}

static const char* route_name(Route r) {
  switch (r) {
    case Route::Small: return "small";
    case Route::Skinny: return "skinny";
    case Route::Kw8: return "kw8";
    case Route::T96: return "t96";
    case Route::StreamK: return "streamk";
    case Route::Remainder: return "remainder";
    case Route::ExtraRows: return "extra_rows";
    case Route::Bk32: return "bk32";
    case Route::Pair: return "pair";
    case Route::Generic: return "generic";
  }
  return "?";
}

static const char* second_name(Second s) {
  switch (s) {
    case Second::None: return "none";
    case Second::SplitReduce: return "split_reduce";
    case Second::TailReduce: return "tail_reduce";
    case Second::StreamKFixup: return "streamk_fixup";
    case Second::Tree: return "tree";
  }
  return "?";
}

static void print_plan(const GemmPlan& p) {
  printf("route=%s bm=%d bn=%d kb=%d wm=%d wn=%d minb=%d vec=%d edge=%d tiles_m=%d tiles_n=%d splits=%d k_per_split=%ld "
         "edge_splits=%d k_per_split_edge=%ld tail_tiles=%d tail_splits=%d tail_k_per_split=%ld x_rows=%d wide_store=%d nt_store=%d "
         "no_skew=%d grid=%ld block=%d second=%s workspace_floats=%ld parts=",
         route_name(p.route), p.bm, p.bn, p.kb, p.waves.wm, p.waves.wn, p.waves.minb, p.vec, (int)p.edge, p.tiles_m, p.tiles_n, p.splits, p.k_per_split,
         p.edge_splits, p.k_per_split_edge, p.tail_tiles, p.tail_splits, p.tail_k_per_split, p.x_rows, (int)p.wide_store, (int)p.nt_store,
         (int)p.no_skew, p.grid, p.block, second_name(p.second), p.workspace_floats);
  for (int i = 0; i < p.nparts; ++i)
    printf("%s%ld:%ld:%ld:%ld", i ? "/" : "", p.parts[i].row0, p.parts[i].col0, p.parts[i].M, p.parts[i].N);
  printf("\n");
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string mode, sw;
    long M, N, K, lda, ldb, ldc;
    int ta, tb, a, b, c, bias, vec;
    if (!(in >> mode >> M >> N >> K >> ta >> tb >> lda >> ldb >> ldc >> a >> b >> c >> bias >> vec >> sw)) {
      fprintf(stderr, "bad case: %s\n", line.c_str());
      return 2;
    }
    GemmProblem p;
    p.M = mode == "ones" ? M + 1 : M;
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
    if (mode == "conv1" || mode == "conv2") {
      p.conv = mode == "conv1" ? 1 : 2;
      p.vec_ok = vec != 0;
    } else if (mode == "ones") {
      p.ones_row = true;
      p.vec_ok = true;
    } else {   // as eg_sgemm: both operands 16-byte, or A alone
      const bool vec_a = operand_vec(lda, p.a_kc ? K : M, p.a_aligned), vec_b = operand_vec(ldb, p.b_kc ? K : N, p.b_aligned);
      p.vec_ok = vec_a && vec_b;
      p.a_vec_only = vec_a && !vec_b && mode != "fused";
    }
    const GemmSwitches s = parse_switches(sw);
    if (mode == "single") {
      printf("single=%d\n", (int)exact_single_launch(plan_gemm(p, s)));
    } else if (mode == "fused") {
      const GemmPlan t = generic_tile(p, s, true);
      printf("bm=%d bn=%d kb=%d wm=%d wn=%d minb=%d splits=%d edge=%d vec=%d wide_store=%d\n", t.bm, t.bn, t.kb, t.waves.wm, t.waves.wn, t.waves.minb, t.splits,
             (int)t.edge, t.vec, (int)wide_store_ok(p, s, false, true));
    } else {
      print_plan(plan_gemm(p, s));
    }
  }
  return 0;
}
