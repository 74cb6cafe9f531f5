// Prints plan_attention_grad (csrc/kernels/attention_plan.cpp, the only unit linked) for tests/test_attention_grad_plan_cpu.py.
//   attention_grad_plan_driver batch0 batch1 I J K D  then (ld stride0 stride1 aligned) of q k v o s dO dQ dK dV
// One line "key=value ..." for the plan, then one line per launch of each kernel: "dq first items grid" / "dkv first items grid".
// With the single argument "lds": one line "kp dp dq_bytes dkv_bytes" per instantiation.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "kernels/attention_plan.hpp"

using namespace eg::attention;

static void launches(const char* name, const GradPlan& r, const GradKernel& k) {
  if (k.launches > 64) return;
  for (long n = 0; n < k.launches; ++n) {
    const Launch l = plan_grad_launch(r, k, n);
    std::printf("%s %ld %ld %ld\n", name, l.first, l.items, l.grid);
  }
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "lds")) {
    for (int kp : {32, 64, 128})
      for (int dp : {32, 64, 128}) std::printf("%d %d %ld %ld\n", kp, dp, grad_dq_lds_bytes(kp, dp), grad_dkv_lds_bytes(kp, dp));
    return 0;
  }
  if (argc != 43) {
    std::fprintf(stderr, "expected 42 arguments\n");
    return 2;
  }
  long a[42];
  for (int i = 0; i < 42; ++i) a[i] = std::atol(argv[i + 1]);
  GradProblem p;
  p.batch0 = a[0], p.batch1 = a[1], p.I = a[2], p.J = a[3], p.K = a[4], p.D = a[5];
  Operand* ops[9] = {&p.q, &p.k, &p.v, &p.o, &p.s, &p.dout, &p.dq, &p.dk, &p.dv};
  for (int i = 0; i < 9; ++i) *ops[i] = {a[6 + 4 * i], a[7 + 4 * i], a[8 + 4 * i], a[9 + 4 * i] != 0};
  const GradPlan r = plan_attention_grad(p);
  std::printf("supported=%d kp=%d dp=%d vec_q=%d vec_k=%d vec_v=%d vec_o=%d vec_s=%d vec_do=%d vec_dq=%d vec_dk=%d vec_dv=%d items=%ld block=%d "
              "dq_tile=%d dq_tiles=%ld dq_grid=%ld dq_items_per_launch=%ld dq_launches=%ld dq_lds=%ld "
              "dkv_tile=%d dkv_tiles=%ld dkv_grid=%ld dkv_items_per_launch=%ld dkv_launches=%ld dkv_lds=%ld max_blocks=%ld reason=%s\n",
              (int)r.supported, r.kp, r.dp, (int)r.vec_q, (int)r.vec_k, (int)r.vec_v, (int)r.vec_o, (int)r.vec_s, (int)r.vec_do, (int)r.vec_dq,
              (int)r.vec_dk, (int)r.vec_dv, r.items, r.block, r.dq.tile, r.dq.tiles, r.dq.grid, r.dq.items_per_launch, r.dq.launches, r.dq.lds_bytes,
              r.dkv.tile, r.dkv.tiles, r.dkv.grid, r.dkv.items_per_launch, r.dkv.launches, r.dkv.lds_bytes, eg::gemm::BATCHED_MAX_BLOCKS, r.reason);
  if (r.supported) {
    launches("dq", r, r.dq);
    launches("dkv", r, r.dkv);
  }
  return 0;
}
