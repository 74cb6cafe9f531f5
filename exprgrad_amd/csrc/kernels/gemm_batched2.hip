// Batched f32 contraction with two batch indices: C_{o,i}[m,n] (+)= sum_k opA_{o,i}(m,k) * opB_{o,i}(k,n) (+ bias[n]) for
// o in [0, batch0), i in [0, batch1), X_{o,i} = X + o * stride_x0 + i * stride_x1, in ONE launch of batch0 x batch1 x tiles_m x
// tiles_n blocks.
//
// The multi-head products — s[b,h,i,j] ++= q[b,i,h,k] * kk[b,j,h,k], o[b,i,h,d] ++= p[b,h,i,j] * v[b,j,h,d] and their derived
// gradients — keep the head index inside the activation's row: the items of an operand interleave, and two strides per
// operand address them.  Everything else is gemm_batched.hip: every block runs the tile body of the plain product
// (gemm_block_at, gemm_f32_mfma.hpp) on a copy of the arguments whose three pointers are advanced to its item, on the 64 x 64
// tile of plan_gemm_batched.  No k-slices, no second pass, no workspace, no atomics, never the split-bf16 route: every output
// element is one k-ascending chain of the f32 matrix instruction, the same as in eg_sgemm_batched.
#include "gemm_f32_mfma.hpp"
#include "gemm_fused.hpp"
#include "gemm_layout.hpp"
#include "gemm_plan.hpp"

#include <algorithm>
#include <type_traits>

#include "../eg_internal.hpp"

namespace {

using namespace eg::gemm;

struct Batched2Args {
  GemmArgs item;   // item (0, 0); tiles_m x tiles_n tiles, unsliced
  long stride_a0, stride_a1, stride_b0, stride_b1, stride_c0, stride_c1;   // floats per step of the outer / inner index
  unsigned batch1;                     // extent of the inner index
  unsigned first_outer, first_inner;   // the item the launch starts at: launches cut the flattened (o, i) range
  int tiles;                           // blocks per item
};

// Block id -> (outer, inner, tile).  As in gemm_batched_kernel the items are folded into grid x and xcd_remap keeps the tiles
// of one item in one L2.  All of it is block-uniform 32-bit arithmetic (first_inner < batch1 < 2^31 and fewer than 2^22 items
// per launch: the sum stays below 2^32); only the three pointer offsets are 64-bit.
template <int BM, int BN, int BK, int WM, int WN, int MINB, bool A_KC, bool B_KC, int VEC, bool EDGE>
__global__ __launch_bounds__((Geometry<BM, BN, WM, WN>::NT), (WavesPerSimd<BM, BN, WM, WN, MINB, EDGE, VEC>::value)) void
gemm_batched2_kernel(Batched2Args b) {
  const int work = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int local = work / b.tiles;
  const int tile = work - local * b.tiles;
  unsigned inner = b.first_inner + (unsigned)local;
  const unsigned outer = b.first_outer + inner / b.batch1;
  inner %= b.batch1;
  GemmArgs a = b.item;
  a.A += (long)outer * b.stride_a0 + (long)inner * b.stride_a1;
  a.B += (long)outer * b.stride_b0 + (long)inner * b.stride_b1;
  a.C += (long)outer * b.stride_c0 + (long)inner * b.stride_c1;
  gemm_block_at<BM, BN, BK, WM, WN, A_KC, B_KC, VEC, EDGE, 0, 0, (VEC == 4), EpiNone>(a, tile);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

constexpr int TILE = 64;   // the one tile of plan_gemm_batched

template <bool AKC, bool BKC, int V, bool E>
void launch_tile(eg_ctx* ctx, unsigned grid, const GemmPlan& p, const Batched2Args& args) {
  constexpr TileWaves w = tile_waves(TILE, TILE);
  hipLaunchKernelGGL((gemm_batched2_kernel<TILE, TILE, BK, w.wm, w.wn, w.minb, AKC, BKC, V, E>), dim3(grid), dim3(p.block), 0, ctx->stream, args);
}

// 12 kernels: four layouts x (whole tiles | ragged with 16-byte loads | ragged with element loads)
void launch_config(eg_ctx* ctx, unsigned grid, bool a_kc, bool b_kc, const GemmPlan& p, const Batched2Args& args) {
  with_layout(a_kc, b_kc, [&](auto ak, auto bk) {
    if (!p.edge) launch_tile<ak, bk, 4, false>(ctx, grid, p, args);
    else if (p.vec == 4) launch_tile<ak, bk, 4, true>(ctx, grid, p, args);
    else launch_tile<ak, bk, 1, true>(ctx, grid, p, args);
  });
}

}  // namespace

namespace eg {
namespace gemm {

// The one internal entry: eg_sgemm_batched2 and the model layer's launches with two batch indices (host/run.cpp) both come here.
int sgemm_batched2(eg_ctx* ctx, int trans_a, int trans_b, long batch0, long batch1, long M, long N, long K, const float* A, long lda,
                   long stride_a0, long stride_a1, const float* B, long ldb, long stride_b0, long stride_b1, float* C, long ldc, long stride_c0,
                   long stride_c1, int accumulate, const float* bias) {
  EG_REQUIRE(ctx, EG_ERR_INVALID, "eg_sgemm_batched2: ctx is NULL");
  EG_REQUIRE(batch0 >= 0 && batch1 >= 0 && M >= 0 && N >= 0 && K >= 0, EG_ERR_INVALID, "eg_sgemm_batched2: negative extent");
  EG_REQUIRE(batch0 < (1L << 31) && batch1 < (1L << 31), EG_ERR_INVALID, "eg_sgemm_batched2: a batch extent of 2^31 or more");
  if (batch0 == 0 || batch1 == 0 || M == 0 || N == 0) return EG_OK;
  EG_REQUIRE(C, EG_ERR_INVALID, "eg_sgemm_batched2: C is NULL");
  EG_REQUIRE(K == 0 || (A && B), EG_ERR_INVALID, "eg_sgemm_batched2: NULL operand");
  EG_REQUIRE(lda >= (trans_a ? M : K) && ldb >= (trans_b ? K : N), EG_ERR_INVALID,
             "eg_sgemm_batched2: leading dimension smaller than the row length");
  EG_REQUIRE(stride_a0 >= 0 && stride_a1 >= 0 && stride_b0 >= 0 && stride_b1 >= 0, EG_ERR_INVALID, "eg_sgemm_batched2: negative stride");
  EG_REQUIRE(batched2_c_distinct(batch0, stride_c0, batch1, stride_c1, M, ldc, N), EG_ERR_INVALID,
             "eg_sgemm_batched2: ldc, stride_c0 and stride_c1 make elements of C share an address");
  if (M == 1 && ldc < N) ldc = N;   // a single row: ldc addresses nothing, and the plain product insists on ldc >= N
  int rc = eg::set_device(ctx);
  if (rc) return rc;

  const bool a_kc = !trans_a, b_kc = trans_b != 0;
  // an item as the planner sees it: what holds for item (0, 0) and both strides holds for every item
  const bool a16 = aligned16(A) && stride_a0 % 4 == 0 && stride_a1 % 4 == 0, b16 = aligned16(B) && stride_b0 % 4 == 0 && stride_b1 % 4 == 0,
             c16 = aligned16(C) && stride_c0 % 4 == 0 && stride_c1 % 4 == 0;
  const bool vec_a = operand_vec(lda, a_kc ? K : M, a16), vec_b = operand_vec(ldb, b_kc ? K : N, b16);
  const GemmProblem item = {M, N, K, a_kc, b_kc, lda, ldb, ldc, a16, b16, c16, bias != nullptr, aligned16(bias), false, 0,
                            vec_a && vec_b, vec_a && !vec_b, false, ctx->compute_units};
  const GemmSwitches& sw = current_switches();
  if (batched_runs_as_loop(item, sw)) {   // every item fills the chip by itself: plain products on their own routes
    for (long o = 0; o < batch0; ++o)
      for (long i = 0; i < batch1; ++i) {
        rc = sgemm_exact(ctx, trans_a, trans_b, M, N, K, A ? A + o * stride_a0 + i * stride_a1 : A, lda, B ? B + o * stride_b0 + i * stride_b1 : B,
                         ldb, C + o * stride_c0 + i * stride_c1, ldc, accumulate, bias);
        if (rc) return rc;
      }
    return EG_OK;
  }
  const long items = batch0 * batch1;   // below 2^62
  const long per_launch = std::max(1L, BATCHED_MAX_BLOCKS / (((M + TILE - 1) / TILE) * ((N + TILE - 1) / TILE)));
  for (long f0 = 0; f0 < items; f0 += per_launch) {
    const long nb = std::min(per_launch, items - f0);
    const GemmPlan p = plan_gemm_batched(item, nb, sw);
    EG_REQUIRE(p.bm == TILE && p.bn == TILE && p.grid > 0 && p.grid <= BATCHED_MAX_BLOCKS, EG_ERR_INVALID,
               "eg_sgemm_batched2: an item has too many tiles for one launch");
    Batched2Args args = {};
    args.item = {A, B, C, bias, /*partial=*/nullptr, M, N, K, lda, ldb, ldc, p.k_per_split, p.tiles_m, p.tiles_n, accumulate};
    args.item.splits = 1;
    args.item.a_rows = M;
    args.item.wide_store = p.wide_store;
    args.item.no_skew = p.no_skew;
    args.stride_a0 = stride_a0;
    args.stride_a1 = stride_a1;
    args.stride_b0 = stride_b0;
    args.stride_b1 = stride_b1;
    args.stride_c0 = stride_c0;
    args.stride_c1 = stride_c1;
    args.batch1 = (unsigned)batch1;
    args.first_outer = (unsigned)(f0 / batch1);
    args.first_inner = (unsigned)(f0 % batch1);
    args.tiles = p.tiles_m * p.tiles_n;
    launch_config(ctx, (unsigned)p.grid, a_kc, b_kc, p, args);
    EG_HIP_CHECK(hipGetLastError());
  }
  return EG_OK;
}

}  // namespace gemm
}  // namespace eg

extern "C" int eg_sgemm_batched2(eg_ctx* ctx, int trans_a, int trans_b, int64_t batch0, int64_t batch1, int64_t M, int64_t N, int64_t K,
                                 const float* A, int64_t lda, int64_t stride_a0, int64_t stride_a1, const float* B, int64_t ldb, int64_t stride_b0,
                                 int64_t stride_b1, float* C, int64_t ldc, int64_t stride_c0, int64_t stride_c1, int accumulate, const float* bias) {
  return eg::gemm::sgemm_batched2(ctx, trans_a, trans_b, batch0, batch1, M, N, K, A, lda, stride_a0, stride_a1, B, ldb, stride_b0, stride_b1, C, ldc,
                                  stride_c0, stride_c1, accumulate, bias);
}
