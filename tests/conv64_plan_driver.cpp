// Host-only driver of the float64 convolution planner (tests/test_conv64_plan_cpu.py): built with the host compiler against
// kernels/gemm_plan.cpp alone, which shows that the planner needs no HIP.
//   stdin lines `role N H W C F FH FW img_aligned flt_aligned gout_aligned cus` (role 1 forward, 2 image gradient, 3 filter
//   gradient); per line one line
//     plan ok= M= N= K= config= bm= bn= wr= wc= vec_a= vec_b= tiles_m= tiles_n= remap= grid_x= grid_y= slices=
//          pixels_per_slice= workspace_doubles= reduce= aux_doubles= max_index=
#include <cstdio>

#include "../exprgrad_amd/csrc/kernels/gemm_plan.hpp"

using namespace eg::gemm;

int main() {
  Conv64Problem p;
  int role = 1, ia = 1, fa = 1, ga = 1;
  while (scanf("%d %ld %ld %ld %ld %ld %ld %ld %d %d %d %d", &role, &p.N, &p.H, &p.W, &p.C, &p.F, &p.FH, &p.FW, &ia, &fa, &ga, &p.cus) == 12) {
    p.role = static_cast<Conv64Role>(role);
    p.img_aligned = ia != 0;
    p.flt_aligned = fa != 0;
    p.gout_aligned = ga != 0;
    const Conv64Plan r = plan_conv64(p);
    printf("plan ok=%d M=%ld N=%ld K=%ld config=%d bm=%d bn=%d wr=%d wc=%d vec_a=%d vec_b=%d tiles_m=%d tiles_n=%d remap=%d grid_x=%ld grid_y=%ld "
           "slices=%d pixels_per_slice=%ld workspace_doubles=%ld reduce=%d aux_doubles=%ld max_index=%ld\n",
           (int)r.ok, r.M, r.Ncols, r.K, r.config, r.bm, r.bn, r.wr, r.wc, (int)r.vec_a, (int)r.vec_b, r.tiles_m, r.tiles_n, (int)r.remap, r.grid_x,
           r.grid_y, r.slices, r.pixels_per_slice, r.workspace_doubles, (int)r.reduce, r.aux_doubles, CONV64_MAX_INDEX);
  }
  return 0;
}
