// Batched f32 contraction: C_b[m,n] (+)= sum_k opA_b(m,k) * opB_b(k,n) (+ bias[n]) for b in [0, batch), X_b = X + b * stride_x,
// in ONE launch of batch x tiles_m x tiles_n blocks.
//
// What the reference emits for `out[g,i,j] ++= a[g,i,k] * b[g,k,j]` and its two derived gradients is one work-item per
// output element (the generic loop nest).  Here every block runs the tile body of the plain product (gemm_block_at,
// gemm_f32_mfma.hpp) on a copy of the arguments whose three pointers are advanced to its item: the same matrix
// instructions in the same k order per output element as the unsliced exact product, on the 64 x 64 tile of
// plan_gemm_batched (gemm_plan.cpp).  No k-slices, no second pass, no workspace, no atomics, never the split-bf16 route.
#include "gemm_f32_mfma.hpp"
#include "gemm_fused.hpp"
#include "gemm_layout.hpp"
#include "gemm_plan.hpp"

#include <algorithm>
#include <type_traits>

#include "../eg_internal.hpp"

namespace {

using namespace eg::gemm;

struct BatchedArgs {
  GemmArgs item;   // item 0; tiles_m x tiles_n tiles, unsliced
  long stride_a, stride_b, stride_c;   // floats between consecutive items (0: the operand is shared)
  int tiles;       // blocks per item
};

// Block id -> (item, tile).  The batch is folded into grid x (grid y and z stop at 65 535).  xcd_remap hands every XCD a
// contiguous range of the launch's blocks, so the tiles of one item, which share its A rows and B columns, meet in one L2.
template <int BM, int BN, int BK, int WM, int WN, int MINB, bool A_KC, bool B_KC, int VEC, bool EDGE>
__global__ __launch_bounds__((Geometry<BM, BN, WM, WN>::NT), (WavesPerSimd<BM, BN, WM, WN, MINB, EDGE, VEC>::value)) void
gemm_batched_kernel(BatchedArgs b) {
  const int work = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int it = work / b.tiles;               // block-uniform: the offsets below are 64-bit scalar data
  const int tile = work - it * b.tiles;
  GemmArgs a = b.item;
  a.A += (long)it * b.stride_a;
  a.B += (long)it * b.stride_b;
  a.C += (long)it * b.stride_c;
  gemm_block_at<BM, BN, BK, WM, WN, A_KC, B_KC, VEC, EDGE, 0, 0, (VEC == 4), EpiNone>(a, tile);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

constexpr int TILE = 64;   // the one tile of plan_gemm_batched

template <bool AKC, bool BKC, int V, bool E>
void launch_tile(eg_ctx* ctx, unsigned grid, const GemmPlan& p, const BatchedArgs& args) {
  constexpr TileWaves w = tile_waves(TILE, TILE);
  hipLaunchKernelGGL((gemm_batched_kernel<TILE, TILE, BK, w.wm, w.wn, w.minb, AKC, BKC, V, E>), dim3(grid), dim3(p.block), 0, ctx->stream, args);
}

// 12 kernels: four layouts x (whole tiles | ragged with 16-byte loads | ragged with element loads)
void launch_config(eg_ctx* ctx, unsigned grid, bool a_kc, bool b_kc, const GemmPlan& p, const BatchedArgs& args) {
  with_layout(a_kc, b_kc, [&](auto ak, auto bk) {
    if (!p.edge) launch_tile<ak, bk, 4, false>(ctx, grid, p, args);
    else if (p.vec == 4) launch_tile<ak, bk, 4, true>(ctx, grid, p, args);
    else launch_tile<ak, bk, 1, true>(ctx, grid, p, args);
  });
}

// blocks of one launch (gemm_plan.hpp: the float64 batched launch keeps the same limit)
constexpr long MAX_BLOCKS = BATCHED_MAX_BLOCKS;

}  // namespace

namespace eg {
namespace gemm {

// The one internal entry: eg_sgemm_batched and the model layer's batched launches (host/run.cpp) both come here.
int sgemm_batched(eg_ctx* ctx, int trans_a, int trans_b, long batch, long M, long N, long K, const float* A, long lda, long stride_a,
                  const float* B, long ldb, long stride_b, float* C, long ldc, long stride_c, int accumulate, const float* bias) {
  EG_REQUIRE(ctx, EG_ERR_INVALID, "eg_sgemm_batched: ctx is NULL");
  EG_REQUIRE(batch >= 0 && M >= 0 && N >= 0 && K >= 0, EG_ERR_INVALID, "eg_sgemm_batched: negative extent");
  if (batch == 0 || M == 0 || N == 0) return EG_OK;
  EG_REQUIRE(C, EG_ERR_INVALID, "eg_sgemm_batched: C is NULL");
  EG_REQUIRE(K == 0 || (A && B), EG_ERR_INVALID, "eg_sgemm_batched: NULL operand");
  EG_REQUIRE(lda >= (trans_a ? M : K) && ldb >= (trans_b ? K : N) && ldc >= N, EG_ERR_INVALID,
             "eg_sgemm_batched: leading dimension smaller than the row length");
  EG_REQUIRE(stride_a >= 0 && stride_b >= 0, EG_ERR_INVALID, "eg_sgemm_batched: negative stride");
  EG_REQUIRE(batch == 1 || stride_c >= (M - 1) * ldc + N, EG_ERR_INVALID, "eg_sgemm_batched: stride_c makes the items of C overlap");
  int rc = eg::set_device(ctx);
  if (rc) return rc;

  const bool a_kc = !trans_a, b_kc = trans_b != 0;
  // an item as the planner sees it: what holds for item 0 and the strides holds for every item
  const bool a16 = aligned16(A) && stride_a % 4 == 0, b16 = aligned16(B) && stride_b % 4 == 0, c16 = aligned16(C) && stride_c % 4 == 0;
  const bool vec_a = operand_vec(lda, a_kc ? K : M, a16), vec_b = operand_vec(ldb, b_kc ? K : N, b16);
  const GemmProblem item = {M, N, K, a_kc, b_kc, lda, ldb, ldc, a16, b16, c16, bias != nullptr, aligned16(bias), false, 0,
                            vec_a && vec_b, vec_a && !vec_b, false, ctx->compute_units};
  const GemmSwitches& sw = current_switches();
  if (batched_runs_as_loop(item, sw)) {   // every item fills the chip by itself: plain products on their own routes
    for (long b = 0; b < batch; ++b) {
      rc = sgemm_exact(ctx, trans_a, trans_b, M, N, K, A ? A + b * stride_a : A, lda, B ? B + b * stride_b : B, ldb, C + b * stride_c, ldc,
                       accumulate, bias);
      if (rc) return rc;
    }
    return EG_OK;
  }
  const long per_launch = std::max(1L, MAX_BLOCKS / (((M + TILE - 1) / TILE) * ((N + TILE - 1) / TILE)));
  for (long b0 = 0; b0 < batch; b0 += per_launch) {
    const long nb = std::min(per_launch, batch - b0);
    const GemmPlan p = plan_gemm_batched(item, nb, sw);
    EG_REQUIRE(p.bm == TILE && p.bn == TILE && p.grid > 0 && p.grid <= MAX_BLOCKS, EG_ERR_INVALID, "eg_sgemm_batched: an item has too many tiles for one launch");
    BatchedArgs args = {};
    args.item = {A ? A + b0 * stride_a : A, B ? B + b0 * stride_b : B, C + b0 * stride_c, bias, /*partial=*/nullptr, M, N, K, lda, ldb, ldc,
                 p.k_per_split, p.tiles_m, p.tiles_n, accumulate};
    args.item.splits = 1;
    args.item.a_rows = M;
    args.item.wide_store = p.wide_store;
    args.item.no_skew = p.no_skew;
    args.stride_a = stride_a;
    args.stride_b = stride_b;
    args.stride_c = stride_c;
    args.tiles = p.tiles_m * p.tiles_n;
    const unsigned grid = (unsigned)p.grid;
    launch_config(ctx, grid, a_kc, b_kc, p, args);
    EG_HIP_CHECK(hipGetLastError());
  }
  return EG_OK;
}

}  // namespace gemm
}  // namespace eg

extern "C" int eg_sgemm_batched(eg_ctx* ctx, int trans_a, int trans_b, int64_t batch, int64_t M, int64_t N, int64_t K, const float* A,
                                int64_t lda, int64_t stride_a, const float* B, int64_t ldb, int64_t stride_b, float* C, int64_t ldc,
                                int64_t stride_c, int accumulate, const float* bias) {
  return eg::gemm::sgemm_batched(ctx, trans_a, trans_b, batch, M, N, K, A, lda, stride_a, B, ldb, stride_b, C, ldc, stride_c, accumulate,
                                 bias);
}
