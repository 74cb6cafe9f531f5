// Host-only driver of the batched float64 product's planner (tests/test_dgemm_batched_plan_cpu.py): built with the host
// compiler against kernels/gemm_plan.cpp alone, which shows that the planner needs no HIP.
//   stdin lines `batch M N K lda ldb stride_a stride_b a_aligned b_aligned cus`; per line one `plan` line
//     plan loop= vec= tiles_m= tiles_n= tiles= items_per_launch= launches= max_blocks= dgemm_vec= item_config= item_splits=
//          item_workspace_doubles=
//   (dgemm_vec: the plain product's rule on the same operands; item_*: the plain plan of one item of a looping batch)
//   followed by one line per launch
//     launch index= first= items= grid= remap=
// With the argument `cut`: the item grid's cut (kernels/item_grid.hpp: cut_items, plan_launch) beside the float64 planner's.
//   stdin lines `items tiles_m tiles_n`; per line one line
//     cut tiles= items_per_launch= launches= max_blocks= d_loop= d_tiles= d_items_per_launch= d_launches=
//   (d_*: plan_dgemm_batched of `items` products of 64 tiles_m x 64 tiles_n, forced to one launch where an item fits one; where
//   none does the planner loops (d_loop=1), and the launches below are dgemm_batched_launch on a plan that holds the cut's figures)
//   followed by one line per launch
//     launch index= first= items= grid= d_first= d_items= d_grid=
#include <cstdio>
#include <cstring>

#include "../exprgrad_amd/csrc/kernels/gemm_plan.hpp"

using namespace eg::gemm;

int cuts() {
  long items = 0, tiles_m = 0, tiles_n = 0;
  while (scanf("%ld %ld %ld", &items, &tiles_m, &tiles_n) == 3) {
    const eg::Cut cut = eg::cut_items(items, tiles_m * tiles_n);
    DgemmBatchedProblem p;
    p.batch = items, p.M = DGEMM_BATCHED_TILE * tiles_m, p.N = DGEMM_BATCHED_TILE * tiles_n, p.K = 8, p.lda = p.K, p.ldb = p.N;
    p.force = 1;
    DgemmBatchedPlan plan = plan_dgemm_batched(p);
    printf("cut tiles=%ld items_per_launch=%ld launches=%ld max_blocks=%ld d_loop=%d d_tiles=%ld d_items_per_launch=%ld d_launches=%ld\n", cut.tiles,
           cut.items_per_launch, cut.launches, eg::BATCHED_MAX_BLOCKS, (int)plan.loop, plan.tiles, plan.items_per_launch, plan.launches);
    if (plan.loop) plan.tiles = cut.tiles, plan.items_per_launch = cut.items_per_launch, plan.launches = cut.launches;
    for (long i = 0; i < cut.launches; ++i) {
      const eg::Launch l = eg::plan_launch(items, cut, i);
      const DgemmBatchedLaunch d = dgemm_batched_launch(plan, items, i);
      printf("launch index=%ld first=%ld items=%ld grid=%ld d_first=%ld d_items=%ld d_grid=%ld\n", i, l.first, l.items, l.grid, d.first, d.items, d.grid);
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "cut") == 0) return cuts();
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
