// Host-only driver of the float64 batched planner with two batch indices (tests/test_dgemm_batched2_plan_cpu.py): built with
// the host compiler against kernels/gemm_plan.cpp alone.
//   stdin lines `batch0 batch1 M N K lda ldb stride_a0 stride_a1 stride_b0 stride_b1 a_aligned b_aligned cus`; per line
//     plan loop= vec= tiles_m= tiles_n= tiles= items_per_launch= launches= max_blocks= dgemm_vec=
//   followed by one line per launch: the items [first, first + items) of the flattened (outer, inner) range, and the item
//   the launch starts at as the kernel's argument names it (for_each_launch, kernels/item_launch.hpp: first / batch1 and
//   first % batch1 — restated here, that header needs HIP)
//     launch index= first= items= grid= first_outer= first_inner=
#include <cstdio>

#include "../exprgrad_amd/csrc/kernels/gemm_plan.hpp"

using namespace eg::gemm;

int main() {
  DgemmBatchedProblem p;
  int a = 1, b = 1;
  while (scanf("%ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %d %d %d", &p.batch, &p.batch1, &p.M, &p.N, &p.K, &p.lda, &p.ldb, &p.stride_a, &p.stride_a1,
               &p.stride_b, &p.stride_b1, &a, &b, &p.cus) == 14) {
    p.a_aligned = a != 0;
    p.b_aligned = b != 0;
    const DgemmBatchedPlan plan = plan_dgemm_batched(p);
    if (plan.loop != dgemm_batched_runs_as_loop(p.M, p.N, p.K, p.cus)) return 2;
    if (!plan.loop && plan.vec != dgemm_batched_vec(p)) return 3;
    printf("plan loop=%d vec=%d tiles_m=%d tiles_n=%d tiles=%ld items_per_launch=%ld launches=%ld max_blocks=%ld dgemm_vec=%d\n", (int)plan.loop,
           (int)plan.vec, plan.tiles_m, plan.tiles_n, plan.tiles, plan.items_per_launch, plan.launches, BATCHED_MAX_BLOCKS,
           (int)dgemm_vec(p.lda, p.ldb, p.a_aligned, p.b_aligned));
    const long items = p.batch * p.batch1;
    const eg::Cut cut = eg::cut_items(items, plan.tiles);
    if (!plan.loop && (cut.launches != plan.launches || cut.items_per_launch != plan.items_per_launch)) return 4;
    for (long i = 0; i < plan.launches; ++i) {
      const eg::Launch l = eg::plan_launch(items, cut, i);
      const DgemmBatchedLaunch d = dgemm_batched_launch(plan, items, i);
      if (d.first != l.first || d.items != l.items || d.grid != l.grid) return 5;
      printf("launch index=%ld first=%ld items=%ld grid=%ld first_outer=%ld first_inner=%ld\n", i, l.first, l.items, l.grid, l.first / p.batch1,
             l.first % p.batch1);
    }
  }
  return 0;
}
