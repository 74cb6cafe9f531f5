// Prints plan_attention_split (csrc/kernels/attention_plan.cpp, the only unit linked) for tests/test_attention_split_plan_cpu.py.
//   attention_split_plan_driver batch0 batch1 I J K D cus splits
// One line "key=value ..." for the plan, then one line "range first last" per split.  Operands are dense and aligned.
#include <cstdio>
#include <cstdlib>

#include "kernels/attention_plan.hpp"

using namespace eg::attention;

int main(int argc, char** argv) {
  if (argc != 9) {
    std::fprintf(stderr, "expected 8 arguments\n");
    return 2;
  }
  long a[8];
  for (int i = 0; i < 8; ++i) a[i] = std::atol(argv[i + 1]);
  Problem p;
  p.batch0 = a[0], p.batch1 = a[1], p.I = a[2], p.J = a[3], p.K = a[4], p.D = a[5], p.cus = (int)a[6];
  p.q.ld = p.k.ld = a[4], p.v.ld = p.o.ld = a[5];
  const SplitPlan r = plan_attention_split(p, (int)a[7]);
  std::printf("supported=%d rows16=%d forward=%d nt=%ld splits=%d rows_pad=%ld stats_offset=%ld workspace=%ld tiles=%ld grid=%ld launches=%ld "
              "combine_rows=%ld combine_rows_per_block=%d combine_grid=%ld lds=%ld lds64=%ld dp=%d tiles_i=%ld items=%ld max_blocks=%ld reason=%s\n",
              (int)r.supported, (int)r.rows16, (int)r.forward, r.nt, r.splits, r.rows_pad, r.stats_offset, r.workspace_bytes, r.partial.tiles,
              r.partial.grid, r.partial.launches, r.combine_rows, r.combine_rows_per_block, r.combine_grid, r.lds_bytes,
              lds_bytes_for(r.base.kp, r.base.dp), r.base.dp, r.base.tiles_i, r.base.items, eg::gemm::BATCHED_MAX_BLOCKS, r.reason);
  if (r.supported && r.splits <= 4096)
    for (int s = 0; s < r.splits; ++s) std::printf("range %ld %ld\n", split_first(r.nt, r.splits, s), split_first(r.nt, r.splits, s + 1));
  return 0;
}
