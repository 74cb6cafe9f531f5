// Host-only driver of the plain float64 product's planner (tests/test_dgemm_plan_cpu.py): built with the host compiler
// against kernels/gemm_plan.cpp alone, which shows that the planner needs no HIP.
//   stdin lines `M N K lda ldb a_aligned b_aligned cus force_config force_splits` (-1 and 0: the model's choice); per line
//     config= bm= bn= wr= wc= vec= splits= k_per_split= tiles_m= tiles_n= remap= grid= workspace_doubles= reduce=
#include <cstdio>

#include "../exprgrad_amd/csrc/kernels/gemm_plan.hpp"

using namespace eg::gemm;

int main() {
  DgemmProblem p;
  int a = 1, b = 1;
  while (scanf("%ld %ld %ld %ld %ld %d %d %d %d %ld", &p.M, &p.N, &p.K, &p.lda, &p.ldb, &a, &b, &p.cus, &p.force_config, &p.force_splits) == 10) {
    p.a_aligned = a != 0;
    p.b_aligned = b != 0;
    const DgemmPlan r = plan_dgemm(p);
    printf("config=%d bm=%d bn=%d wr=%d wc=%d vec=%d splits=%d k_per_split=%ld tiles_m=%d tiles_n=%d remap=%d grid=%ldx%ld workspace_doubles=%ld reduce=%d\n",
           r.config, r.bm, r.bn, r.wr, r.wc, (int)r.vec, r.splits, r.k_per_split, r.tiles_m, r.tiles_n, (int)r.remap, r.grid_x, r.grid_y,
           r.workspace_doubles, (int)r.reduce);
  }
  return 0;
}
