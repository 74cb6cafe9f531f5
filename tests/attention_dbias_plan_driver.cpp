// Prints plan_attention_dbias (csrc/kernels/attention_plan.cpp, the only unit linked) for tests/test_attention_dbias_plan_cpu.py.
//   attention_dbias_plan_driver batch0 batch1 I J K D  then (ld stride0 stride1 aligned) of q k v o s dO bias dBias
// One line "key=value ..." for the plan, then one line "launch first items grid" per launch.
#include <cstdio>
#include <cstdlib>

#include "kernels/attention_plan.hpp"

using namespace eg::attention;

int main(int argc, char** argv) {
  if (argc != 39) {
    std::fprintf(stderr, "expected 38 arguments\n");
    return 2;
  }
  long a[38];
  for (int i = 0; i < 38; ++i) a[i] = std::atol(argv[i + 1]);
  DbiasProblem p;
  p.batch0 = a[0], p.batch1 = a[1], p.I = a[2], p.J = a[3], p.K = a[4], p.D = a[5];
  Operand* ops[8] = {&p.q, &p.k, &p.v, &p.o, &p.s, &p.dout, &p.bias, &p.dbias};
  for (int i = 0; i < 8; ++i) *ops[i] = {a[6 + 4 * i], a[7 + 4 * i], a[8 + 4 * i], a[9 + 4 * i] != 0};
  const DbiasPlan r = plan_attention_dbias(p);
  std::printf("supported=%d kp=%d dp=%d vec_q=%d vec_k=%d vec_v=%d vec_o=%d vec_s=%d vec_do=%d vec_db=%d row_fold=%d cells0=%ld cells1=%ld "
              "cells=%ld sum0=%ld sum1=%ld tiles_i=%ld tiles_j=%ld tiles=%ld grid=%ld items_per_launch=%ld launches=%ld ahead=%d block=%d lds=%ld "
              "max_blocks=%ld reason=%s\n",
              (int)r.supported, r.kp, r.dp, (int)r.vec_q, (int)r.vec_k, (int)r.vec_v, (int)r.vec_o, (int)r.vec_s, (int)r.vec_do, (int)r.vec_db,
              (int)r.row_fold, r.cells0, r.cells1, r.cells, r.sum0, r.sum1, r.tiles_i, r.tiles_j, r.cut.tiles, r.cut.grid, r.cut.items_per_launch,
              r.cut.launches, (int)r.ahead, r.block, r.lds_bytes, eg::gemm::BATCHED_MAX_BLOCKS, r.reason);
  if (r.supported && r.cut.launches <= 64) {
    for (long n = 0; n < r.cut.launches; ++n) {
      const Launch l = plan_dbias_launch(r, n);
      std::printf("launch %ld %ld %ld\n", l.first, l.items, l.grid);
    }
  }
  return 0;
}
