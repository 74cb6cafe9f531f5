// Host-only driver of the batched float64 product's planner (tests/test_dgemm_batched_plan_cpu.py): built with the host
// compiler against kernels/gemm_plan.cpp alone, which shows that the planner needs no HIP.
//   stdin lines `batch M N K lda ldb stride_a stride_b a_aligned b_aligned cus`; per line one `plan` line
//     plan loop= vec= tiles_m= tiles_n= tiles= items_per_launch= launches= max_blocks= dgemm_vec= item_config= item_splits=
//          item_workspace_doubles=
//   (dgemm_vec: the plain product's rule on the same operands; item_*: the plain plan of one item of a looping batch)
//   followed by one line per launch
//     launch index= first= items= grid= remap=
#include <cstdio>

#include "../exprgrad_amd/csrc/kernels/gemm_plan.hpp"

using namespace eg::gemm;

int main() {
  DgemmBatchedProblem p;
  int a = 1, b = 1;
  while (scanf("%ld %ld %ld %ld %ld %ld %ld %ld %d %d %d", &p.batch, &p.M, &p.N, &p.K, &p.lda, &p.ldb, &p.stride_a, &p.stride_b, &a, &b, &p.cus) == 11) {
    p.a_aligned = a != 0;
    p.b_aligned = b != 0;
    const DgemmBatchedPlan plan = plan_dgemm_batched(p);
    if (plan.loop != dgemm_batched_runs_as_loop(p.M, p.N, p.K, p.cus)) return 2;
    printf("plan loop=%d vec=%d tiles_m=%d tiles_n=%d tiles=%ld items_per_launch=%ld launches=%ld max_blocks=%ld dgemm_vec=%d item_config=%d "
           "item_splits=%d item_workspace_doubles=%ld\n",
           (int)plan.loop, (int)plan.vec, plan.tiles_m, plan.tiles_n, plan.tiles, plan.items_per_launch, plan.launches, BATCHED_MAX_BLOCKS,
           (int)dgemm_vec(p.lda, p.ldb, p.a_aligned, p.b_aligned), plan.item.config, plan.item.splits, plan.item.workspace_doubles);
    for (long i = 0; i < plan.launches; ++i) {
      const DgemmBatchedLaunch l = dgemm_batched_launch(plan, p.batch, i);
      printf("launch index=%ld first=%ld items=%ld grid=%ld remap=%d\n", i, l.first, l.items, l.grid, (int)l.remap);
    }
  }
  return 0;
}
