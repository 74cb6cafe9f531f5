// Prints plan_attention_f64 and, for the same problem, plan_attention (csrc/kernels/attention_plan.cpp, the only unit linked)
// for tests/test_attention_f64_plan_cpu.py.
//   attention_f64_plan_driver batch0 batch1 I J K D  ldq sq0 sq1 aq  ldk sk0 sk1 ak  ldv sv0 sv1 av
// One line "f64 key=value ..." and one line "f32 key=value ..." for the two plans, then one line per launch of the float64
// plan: "launch first items grid".  "fits64" and "fits32": whether a key tile of 64 or of 32 keys fits the LDS of a CU.
#include <cstdio>
#include <cstdlib>

#include "kernels/attention_plan.hpp"

using namespace eg::attention;

static void print(const char* which, const Plan& r) {
  std::printf("%s supported=%d tile_i=%d tile_j=%d kp=%d dp=%d vec_q=%d vec_k=%d vec_v=%d tiles_i=%ld items=%ld grid=%ld items_per_launch=%ld launches=%ld block=%d lds=%ld max_blocks=%ld",
              which, (int)r.supported, r.tile_i, r.tile_j, r.kp, r.dp, (int)r.vec_q, (int)r.vec_k, (int)r.vec_v, r.tiles_i, r.items, r.grid,
              r.items_per_launch, r.launches, r.block, r.lds_bytes, eg::gemm::BATCHED_MAX_BLOCKS);
  if (r.kp && r.dp)
    std::printf(" lds64=%ld lds32=%ld key_tile=%d", lds_bytes_for_f64(r.kp, r.dp, 64), lds_bytes_for_f64(r.kp, r.dp, 32), key_tile_f64(r.kp, r.dp));
  std::printf(" reason=%s\n", r.reason);
}

int main(int argc, char** argv) {
  if (argc != 19) {
    std::fprintf(stderr, "expected 18 arguments\n");
    return 2;
  }
  long a[18];
  for (int i = 0; i < 18; ++i) a[i] = std::atol(argv[i + 1]);
  Problem p;
  p.batch0 = a[0], p.batch1 = a[1], p.I = a[2], p.J = a[3], p.K = a[4], p.D = a[5];
  p.q = {a[6], a[7], a[8], a[9] != 0};
  p.k = {a[10], a[11], a[12], a[13] != 0};
  p.v = {a[14], a[15], a[16], a[17] != 0};
  const Plan r = plan_attention_f64(p);
  print("f64", r);
  print("f32", plan_attention(p));
  if (r.supported && r.launches <= 64)
    for (long n = 0; n < r.launches; ++n) {
      const Launch l = plan_launch(r, n);
      std::printf("launch %ld %ld %ld\n", l.first, l.items, l.grid);
    }
  return 0;
}
