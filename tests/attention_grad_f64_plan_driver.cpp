// Prints plan_attention_grad_f64 (csrc/kernels/attention_plan.cpp, the only unit linked) for
// tests/test_attention_grad_f64_plan_cpu.py, with the arguments and in the format of attention_grad_plan_driver.cpp; the
// constexpr functions' steps and LDS bytes stand beside the plan's, and the launches are not listed.
#include <cstdio>
#include <cstdlib>

#include "kernels/attention_plan.hpp"

using namespace eg::attention;

int main(int argc, char** argv) {
  if (argc != 43) return 2;
  long a[42];
  for (int i = 0; i < 42; ++i) a[i] = std::atol(argv[i + 1]);
  GradProblem p;
  p.batch0 = a[0], p.batch1 = a[1], p.I = a[2], p.J = a[3], p.K = a[4], p.D = a[5];
  Operand* ops[9] = {&p.q, &p.k, &p.v, &p.o, &p.s, &p.dout, &p.dq, &p.dk, &p.dv};
  for (int i = 0; i < 9; ++i) *ops[i] = {a[6 + 4 * i], a[7 + 4 * i], a[8 + 4 * i], a[9 + 4 * i] != 0};
  const GradPlan r = plan_attention_grad_f64(p);
  std::printf("supported=%d kp=%d dp=%d vec_q=%d vec_k=%d vec_v=%d vec_o=%d vec_s=%d vec_do=%d vec_dq=%d vec_dk=%d vec_dv=%d items=%ld block=%d "
              "dq_tile=%d dq_step=%d dq_tiles=%ld dq_grid=%ld dq_items_per_launch=%ld dq_launches=%ld dq_lds=%ld "
              "dkv_tile=%d dkv_step=%d dkv_tiles=%ld dkv_grid=%ld dkv_items_per_launch=%ld dkv_launches=%ld dkv_lds=%ld max_blocks=%ld",
              (int)r.supported, r.kp, r.dp, (int)r.vec_q, (int)r.vec_k, (int)r.vec_v, (int)r.vec_o, (int)r.vec_s, (int)r.vec_do, (int)r.vec_dq,
              (int)r.vec_dk, (int)r.vec_dv, r.items, r.block, r.dq.tile, r.dq.step, r.dq.tiles, r.dq.grid, r.dq.items_per_launch, r.dq.launches,
              r.dq.lds_bytes, r.dkv.tile, r.dkv.step, r.dkv.tiles, r.dkv.grid, r.dkv.items_per_launch, r.dkv.launches, r.dkv.lds_bytes,
              eg::gemm::BATCHED_MAX_BLOCKS);
  if (r.kp && r.dp) {
    const int tj = grad_dq_step_f64(r.kp, r.dp), ti = grad_dkv_step_f64(r.kp, r.dp);
    std::printf(" fn_dq_step=%d fn_dkv_step=%d fn_dq_lds=%ld fn_dkv_lds=%ld dq_lds64=%ld dkv_lds64=%ld", tj, ti, grad_dq_lds_bytes_f64(r.kp, r.dp, tj),
                grad_dkv_lds_bytes_f64(r.kp, r.dp, ti), grad_dq_lds_bytes_f64(r.kp, r.dp, 64), grad_dkv_lds_bytes_f64(r.kp, r.dp, 64));
  }
  std::printf(" reason=%s\n", r.reason);
  return 0;
}
