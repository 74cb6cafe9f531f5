// Batched f32 contractions, C_x[m,n] (+)= sum_k opA_x(m,k) * opB_x(k,n) (+ bias[n]) for every item x, in ONE launch of
// items x tiles_m x tiles_n blocks:
//   eg_sgemm_batched   one batch index,    x = b in [0, batch),                       X_b = X + b * stride_x
//   eg_sgemm_batched2  two batch indices,  x = (o, i) in [0, batch0) x [0, batch1),  X_{o,i} = X + o * stride_x0 + i * stride_x1
// The second is for the multi-head products — s[b,h,i,j] ++= q[b,i,h,k] * kk[b,j,h,k], o[b,i,h,d] ++= p[b,h,i,j] * v[b,j,h,d]
// and their derived gradients —, which keep the head index inside the activation's row: the items of an operand interleave.
//
// What the reference emits for `out[g,i,j] ++= a[g,i,k] * b[g,k,j]` and its two derived gradients is one work-item per
// output element (the generic loop nest).  Here every block runs the tile body of the plain product (gemm_block_at,
// gemm_f32_mfma.hpp) on a copy of the arguments whose three pointers are advanced to its item: the same matrix
// instructions in the same k order per output element as the unsliced exact product, on the 64 x 64 tile of
// plan_gemm_batched (gemm_plan.cpp).  No k-slices, no second pass, no workspace, no atomics, never the split-bf16 route.
// One kernel and one launcher serve both entries: an operand is a View, the items are the item grid's (item_launch.hpp).
#include "gemm_f32_mfma.hpp"
#include "gemm_fused.hpp"
#include "gemm_layout.hpp"
#include "gemm_plan.hpp"
#include "item_launch.hpp"

#include <algorithm>
#include <type_traits>

#include "../eg_internal.hpp"

namespace {

using namespace eg::gemm;

// In this order of members no kernel takes more vector registers or fewer waves per SIMD than it did with its own argument
// struct per entry; with `item` first two of the twelve lose a wave (profiles/batched_items.txt).
struct BatchedArgs {
  eg::Items items;
  eg::View a, b, c;
  GemmArgs item;   // the launch's first outer index, inner index 0; tiles_m x tiles_n tiles, unsliced
};

template <int BM, int BN, int BK, int WM, int WN, int MINB, bool A_KC, bool B_KC, int VEC, bool EDGE>
__global__ __launch_bounds__((Geometry<BM, BN, WM, WN>::NT), (WavesPerSimd<BM, BN, WM, WN, MINB, EDGE, VEC>::value)) void
gemm_batched_kernel(BatchedArgs b) {
  const eg::BlockItem at = eg::block_item<true>(b.items);
  GemmArgs a = b.item;
  a.A = eg::item_base(a.A, b.a, at.outer, at.inner);
  a.B = eg::item_base(a.B, b.b, at.outer, at.inner);
  a.C = eg::item_base(a.C, b.c, at.outer, at.inner);
  gemm_block_at<BM, BN, BK, WM, WN, A_KC, B_KC, VEC, EDGE, 0, 0, (VEC == 4), EpiNone>(a, at.tile);
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

// batch0 x batch1 items behind the entry `name`, whose checks have passed.  The launches cut the flattened (o, i) range; the
// host advances the pointers to a launch's first outer index, so the kernel's outer index counts from 0 within the launch
// and batch0 has no 32-bit limit.
int launch_items(eg_ctx* ctx, const char* name, int trans_a, int trans_b, long batch0, long batch1, long M, long N, long K, const float* A,
                 const eg::View& va, const float* B, const eg::View& vb, float* C, const eg::View& vc, int accumulate, const float* bias) {
  int rc = eg::set_device(ctx);
  if (rc) return rc;
  const bool a_kc = !trans_a, b_kc = trans_b != 0;
  // an item as the planner sees it: what holds for item (0, 0) and both strides holds for every item
  auto all16 = [](const void* p, const eg::View& v) { return aligned16(p) && v.stride0 % 4 == 0 && v.stride1 % 4 == 0; };
  const bool a16 = all16(A, va), b16 = all16(B, vb), c16 = all16(C, vc);
  const bool vec_a = operand_vec(va.ld, a_kc ? K : M, a16), vec_b = operand_vec(vb.ld, b_kc ? K : N, b16);
  const GemmProblem item = {M, N, K, a_kc, b_kc, va.ld, vb.ld, vc.ld, a16, b16, c16, bias != nullptr, aligned16(bias), false, 0,
                            vec_a && vec_b, vec_a && !vec_b, false, ctx->compute_units};
  const GemmSwitches& sw = current_switches();
  auto at = [](auto* p, const eg::View& v, long o, long i) { return p ? p + o * v.stride0 + i * v.stride1 : p; };
  if (batched_runs_as_loop(item, sw)) {   // every item fills the chip by itself: plain products on their own routes
    for (long o = 0; o < batch0; ++o)
      for (long i = 0; i < batch1; ++i) {
        rc = sgemm_exact(ctx, trans_a, trans_b, M, N, K, at(A, va, o, i), va.ld, at(B, vb, o, i), vb.ld, at(C, vc, o, i), vc.ld, accumulate, bias);
        if (rc) return rc;
      }
    return EG_OK;
  }
  const GemmPlan p = plan_gemm_batched(item, 1, sw);   // p.grid: the tiles of one item
  EG_REQUIRE(p.bm == TILE && p.bn == TILE && p.grid > 0 && p.grid <= eg::BATCHED_MAX_BLOCKS, EG_ERR_INVALID,
             "%s: an item has too many tiles for one launch", name);
  const long items = batch0 * batch1;   // below 2^62 for two indices; batch1 == 1 otherwise
  const eg::Cut cut = eg::cut_items(items, p.grid);
  for (long n = 0; n < cut.launches; ++n) {
    const eg::Launch l = eg::plan_launch(items, cut, n);
    const long o = l.first / batch1;
    BatchedArgs args = {};
    args.item = {at(A, va, o, 0), at(B, vb, o, 0), at(C, vc, o, 0), bias, /*partial=*/nullptr, M, N, K, va.ld, vb.ld, vc.ld,
                 p.k_per_split, p.tiles_m, p.tiles_n, accumulate};
    args.item.splits = 1;
    args.item.a_rows = M;
    args.item.wide_store = p.wide_store;
    args.item.no_skew = p.no_skew;
    args.a = va, args.b = vb, args.c = vc;
    args.items = {(unsigned)batch1, 0u, (unsigned)(l.first % batch1), (int)cut.tiles};
    launch_config(ctx, (unsigned)l.grid, a_kc, b_kc, p, args);
    EG_HIP_CHECK(hipGetLastError());
  }
  return EG_OK;
}

}  // namespace

namespace eg {
namespace gemm {

// The internal entry of one batch index: eg_sgemm_batched comes here.
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
  // the batch index is the outer one: the host steps it from launch to launch, so `batch` has no 32-bit limit
  return launch_items(ctx, "eg_sgemm_batched", trans_a, trans_b, batch, 1, M, N, K, A, {lda, stride_a, 0}, B, {ldb, stride_b, 0}, C,
                      {ldc, stride_c, 0}, accumulate, bias);
}

// The internal entry of two batch indices: eg_sgemm_batched2 comes here.
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
  return launch_items(ctx, "eg_sgemm_batched2", trans_a, trans_b, batch0, batch1, M, N, K, A, {lda, stride_a0, stride_a1}, B,
                      {ldb, stride_b0, stride_b1}, C, {ldc, stride_c0, stride_c1}, accumulate, bias);
}

// The model layer's batched launches (host/run.cpp): batch1 == 0 is a product with one batch index, its strides each view's stride0.
int sgemm_batched_views(eg_ctx* ctx, int trans_a, int trans_b, long batch0, long batch1, long M, long N, long K, const float* A, const View& a,
                        const float* B, const View& b, float* C, const View& c, int accumulate, const float* bias) {
  if (batch1 > 0)
    return sgemm_batched2(ctx, trans_a, trans_b, batch0, batch1, M, N, K, A, a.ld, a.stride0, a.stride1, B, b.ld, b.stride0, b.stride1, C, c.ld,
                          c.stride0, c.stride1, accumulate, bias);
  return sgemm_batched(ctx, trans_a, trans_b, batch0, M, N, K, A, a.ld, a.stride0, B, b.ld, b.stride0, C, c.ld, c.stride0, accumulate, bias);
}

}  // namespace gemm
}  // namespace eg

extern "C" int eg_sgemm_batched(eg_ctx* ctx, int trans_a, int trans_b, int64_t batch, int64_t M, int64_t N, int64_t K, const float* A,
                                int64_t lda, int64_t stride_a, const float* B, int64_t ldb, int64_t stride_b, float* C, int64_t ldc,
                                int64_t stride_c, int accumulate, const float* bias) {
  return eg::gemm::sgemm_batched(ctx, trans_a, trans_b, batch, M, N, K, A, lda, stride_a, B, ldb, stride_b, C, ldc, stride_c, accumulate,
                                 bias);
}

extern "C" int eg_sgemm_batched2(eg_ctx* ctx, int trans_a, int trans_b, int64_t batch0, int64_t batch1, int64_t M, int64_t N, int64_t K,
                                 const float* A, int64_t lda, int64_t stride_a0, int64_t stride_a1, const float* B, int64_t ldb, int64_t stride_b0,
                                 int64_t stride_b1, float* C, int64_t ldc, int64_t stride_c0, int64_t stride_c1, int accumulate, const float* bias) {
  return eg::gemm::sgemm_batched2(ctx, trans_a, trans_b, batch0, batch1, M, N, K, A, lda, stride_a0, stride_a1, B, ldb, stride_b0, stride_b1, C, ldc,
                                  stride_c0, stride_c1, accumulate, bias);
}
