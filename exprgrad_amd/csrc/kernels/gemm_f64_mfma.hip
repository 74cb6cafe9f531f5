// float64 contraction on the matrix cores — the `compile[float64]` form of `c[y,x] ++= a[y,it] * b[it,x]`
// (base.nim:27-28; model.nim:253-260 instantiates every kernel of a program over Scalar64) and of the two
// gradient contractions derive makes of it (passes.nim:519-549).
//
// `v_mfma_f64_16x16x4_f64`: A fragment = one double per lane (row lane % 16, k lane / 16), B likewise
// (k lane / 16, column lane % 16), C / D four doubles per lane (column lane & 15, row (lane >> 4) + 4 r).
// One such instruction is 2 048 FLOP in 64 cycles (78.6 TFLOP/s over 1 024 SIMDs at 2.4 GHz): a wave needs
// 16 bytes of operand per lane every 64 cycles, so — unlike the float32 kernel, whose 32 x 32 x 2 tiles are
// bound by what stands between two MFMAs — a plain register-staged, double-buffered tile loop keeps the
// matrix pipe busy: 4 waves per block, a wave owns WM x WN of the BM x BN tile, 16-deep k-tiles,
// operands in LDS as [k][m | n] rows padded by 16 doubles (the four k rows a fragment read touches then
// fall into different bank halves).  All four storage orders go through one loader (strides), ragged
// tiles are zero filled, K is cut into slices with a fixed-order second pass when the tiles alone
// cannot fill the chip (deterministic: no atomics).
//
// eg_dgemm_batched — `out[g,i,j] ++= a[g,i,k] * b[g,k,j]` of a float64 program and its two derived gradients, which the
// reference runs as one work-item per output element — is the same tile body, one block per (item, tile), in one launch:
// dgemm_batched1_kernel below, planned by plan_dgemm_batched (gemm_plan.cpp).
// eg_dgemm_batched2 — the multi-head products `s[b,h,i,j] ++= q[b,i,h,k] * kk[b,j,h,k]`, `o[b,i,h,d] ++= p[b,h,i,j] * v[b,j,h,d]`
// and the four gradients derive makes of them, two batch indices with two strides per operand — is the same tile body through
// the same launcher: the items are the item grid's (item_grid.hpp, item_launch.hpp), as in gemm_batched.hip.  A float64 model
// runs these products on it where it asks for it (eg_model_batched2_f64, host/lower.cpp).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../eg_internal.hpp"
#include "gemm_fused.hpp"
#include "gemm_layout.hpp"
#include "gemm_plan.hpp"
#include "gemm_f64_tile.hpp"
#include "item_launch.hpp"

namespace {

using namespace eg::f64tile;

template <int BM, int BN, int WR, int WC, bool AKC, bool BKC, bool VEC>
__global__ __launch_bounds__(WR* WC * 64, 4) void dgemm_kernel(DgemmArgs a) {
  long tile = blockIdx.x;
  if (a.remap) {
    const long per = (long)gridDim.x >> 3;
    tile = (tile & 7) * per + (tile >> 3);
  }
  const long kbeg = (long)blockIdx.y * a.k_per_split;
  const long kend = min(a.K, kbeg + a.k_per_split);
  dgemm_tile_at<BM, BN, WR, WC, AKC, BKC, VEC>(a, tile, (long)blockIdx.y, kbeg, kend);
}

// eg_dgemm_batched2: batch0 x batch1 products of one shape in ONE launch (an extent of 1 included): the items are the
// item grid's (item_grid.hpp, item_launch.hpp) — folded into grid x, block id -> (outer, inner, tile) through
// block_item, an operand a View in doubles — and the block runs dgemm_tile_at over the whole K on a copy of the arguments
// whose three pointers are advanced to its item (block-uniform 64-bit values).  The 64 x 64 tile of eight waves, no
// k-slices: every output element is one k-ascending chain of matrix instructions, the chain eg_dgemm gives it wherever
// that takes no slices, whatever tile it picks — and whichever block of whichever launch computes it.
// The members in the order of gemm_batched.hip's BatchedArgs.
struct DgemmBatchedArgs {
  eg::Items items;
  eg::View a, b, c;   // doubles per row step and per step of the outer and the inner batch index (0: the operand is shared)
  DgemmArgs item;     // item (0, 0) of the launch's range; splits = 1
};

constexpr int BT = 64;   // the batched tile, <BT, BT, 2, 4>

template <bool AKC, bool BKC, bool VEC>
__global__ __launch_bounds__(512, 4) void dgemm_batched_kernel(DgemmBatchedArgs b) {
  const eg::BlockItem at = eg::block_item<true>(b.items);
  DgemmArgs a = b.item;
  a.A = eg::item_base(a.A, b.a, at.outer, at.inner);
  a.B = eg::item_base(a.B, b.b, at.outer, at.inner);
  a.C = eg::item_base(a.C, b.c, at.outer, at.inner);
  dgemm_tile_at<BT, BT, 2, 4, AKC, BKC, VEC>(a, at.tile, 0, 0, a.K);
}

// One batch index (eg_dgemm_batched): the arguments and the block decode this launch had before the item grid.  Measured, the
// item grid's arguments cost the one-index launch 0.5 - 0.9 us (profiles/dgemm_batched2.txt), more than repeated runs of it
// differ by, so the entry keeps this kernel until that is gone: block id -> (item, tile) with three scalar strides; remap
// (the launch's block count is a multiple of 8, dgemm_remap): every XCD gets a contiguous range of the launch's blocks.
// The same tile body over the same k range as above: an item has the same bits through either kernel.
struct DgemmBatched1Args {
  DgemmArgs item;   // item 0 of the launch; splits = 1
  long stride_a, stride_b, stride_c;   // doubles between consecutive items (0: the operand is shared)
  int tiles;        // blocks per item
  int remap;
};

template <bool AKC, bool BKC, bool VEC>
__global__ __launch_bounds__(512, 4) void dgemm_batched1_kernel(DgemmBatched1Args b) {
  int work = (int)blockIdx.x;
  if (b.remap) {
    const int per = (int)(gridDim.x >> 3);
    work = (work & 7) * per + (work >> 3);
  }
  const int it = work / b.tiles;
  const int tile = work - it * b.tiles;
  DgemmArgs a = b.item;
  a.A += (long)it * b.stride_a;
  a.B += (long)it * b.stride_b;
  a.C += (long)it * b.stride_c;
  dgemm_tile_at<BT, BT, 2, 4, AKC, BKC, VEC>(a, tile, 0, 0, a.K);
}

template <typename T>
__global__ __launch_bounds__(256) void fill_kernel_t(T* __restrict__ out, long n, T value) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = value;
}

// ---- column sum (the float64 twin of reduce.hip's two-stage tree; same geometry, same order) -------------------------
__global__ __launch_bounds__(256) void colsum_partial_f64_kernel(const double* __restrict__ in, double* __restrict__ partial, long rows, long cols,
                                                                 int colsP, long rows_per_block) {
  __shared__ double red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rpw = 64 / colsP;
  const int r_in_wave = lane / colsP;
  const long c = (long)blockIdx.y * 64 + (lane % colsP);
  const long row_begin = (long)blockIdx.x * rows_per_block;
  const long row_end = min(rows, row_begin + rows_per_block);
  double acc = 0.0;
  if (c < cols)
    for (long r = row_begin + wave * rpw + r_in_wave; r < row_end; r += 4 * rpw) acc += in[r * cols + c];
  for (int off = 32; off >= colsP; off >>= 1) acc += __shfl_xor(acc, off, 64);
  red[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && lane < colsP && c < cols) partial[(long)blockIdx.x * cols + c] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

__global__ __launch_bounds__(256) void colsum_final_f64_kernel(const double* __restrict__ partial, double* __restrict__ out, long cols, int nparts,
                                                               int accumulate) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  double s = 0.0;
  for (int p = 0; p < nparts; ++p) s += partial[(long)p * cols + c];
  out[c] = accumulate ? out[c] + s : s;
}

// element i = lo + (hi - lo) * u, u in [0, 1) from 53 bits of the same counter hash the float32 fill uses
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ULL;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebULL;
  x ^= x >> 31;
  return x;
}
__global__ __launch_bounds__(256) void fill_uniform_f64_kernel(double* __restrict__ out, long n, double lo, double hi, const uint64_t* __restrict__ state,
                                                               uint64_t stream) {
  const uint64_t seed = state[0], draw = state[1];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const uint64_t h = mix64(mix64(seed ^ (draw * 0x9e3779b97f4a7c15ULL)) ^ mix64(stream * 0xd1b54a32d192ed03ULL + (uint64_t)i));
    const double u = (double)(h >> 11) * (1.0 / 9007199254740992.0);
    out[i] = lo + (hi - lo) * u;
  }
}

using eg::gemm::DgemmPlan;

template <int BM, int BN, int WR, int WC, bool AKC, bool BKC, bool VEC>
int launch_one(eg_ctx* ctx, const DgemmPlan& p, const DgemmArgs& a) {
  using LA = TileLoader<BM, WR * WC * 64, AKC, VEC>;
  using LB = TileLoader<BN, WR * WC * 64, BKC, VEC>;
  constexpr size_t lds = (size_t)2 * (LA::LDS_DOUBLES + LB::LDS_DOUBLES) * sizeof(double);
  static bool attr_set = false;
  if (!attr_set) {
    EG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&dgemm_kernel<BM, BN, WR, WC, AKC, BKC, VEC>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set = true;
  }
  hipLaunchKernelGGL((dgemm_kernel<BM, BN, WR, WC, AKC, BKC, VEC>), dim3((unsigned)p.grid_x, (unsigned)p.grid_y), dim3(WR * WC * 64), lds, ctx->stream, a);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}

// 8 kernels per tile: four storage orders x (16-byte | 8-byte loads)
template <int BM, int BN, int WR, int WC>
int launch_dgemm(eg_ctx* ctx, const DgemmPlan& p, const DgemmArgs& a, bool akc, bool bkc) {
  int rc = EG_ERR_INVALID;
  eg::gemm::with_layout_vec(akc, bkc, p.vec, [&](auto ak, auto bk, auto v) { rc = launch_one<BM, BN, WR, WC, ak, bk, v>(ctx, p, a); });
  return rc;
}

// the kernel that takes `Args`: the item grid's (both entries' two-index form) or the one-index entry's own
template <bool AKC, bool BKC, bool VEC>
constexpr auto batched_kernel(const DgemmBatchedArgs*) { return &dgemm_batched_kernel<AKC, BKC, VEC>; }
template <bool AKC, bool BKC, bool VEC>
constexpr auto batched_kernel(const DgemmBatched1Args*) { return &dgemm_batched1_kernel<AKC, BKC, VEC>; }

template <bool AKC, bool BKC, bool VEC, class Args>
int launch_batched_one(eg_ctx* ctx, unsigned grid, const Args& b) {
  using LA = TileLoader<BT, 512, AKC, VEC>;
  using LB = TileLoader<BT, 512, BKC, VEC>;
  constexpr size_t lds = (size_t)2 * (LA::LDS_DOUBLES + LB::LDS_DOUBLES) * sizeof(double);
  constexpr auto kernel = batched_kernel<AKC, BKC, VEC>(static_cast<const Args*>(nullptr));
  static bool attr_set = false;   // (one per kernel: the function is instantiated per Args)
  if (!attr_set) {
    EG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set = true;
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(512), lds, ctx->stream, b);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}

template <class Args>
int launch_batched(eg_ctx* ctx, unsigned grid, const Args& b, bool akc, bool bkc, bool vec) {
  int rc = EG_ERR_INVALID;
  eg::gemm::with_layout_vec(akc, bkc, vec, [&](auto ak, auto bk, auto v) { rc = launch_batched_one<ak, bk, v>(ctx, grid, b); });
  return rc;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The argument checks of eg_dgemm and eg_dgemm_batched (`who`; the plain product is a batch of one).  empty: the call is
// valid and there is nothing to compute.
int check_product(const char* who, const eg_ctx* ctx, int trans_a, int trans_b, long batch, long M, long N, long K, const double* A, long lda,
                  const double* B, long ldb, const double* C, long ldc, bool& empty) {
  EG_REQUIRE(ctx, EG_ERR_INVALID, "%s: ctx is NULL", who);
  EG_REQUIRE(batch >= 0 && M >= 0 && N >= 0 && K >= 0, EG_ERR_INVALID, "%s: negative extent", who);
  empty = batch == 0 || M == 0 || N == 0;
  if (empty) return EG_OK;
  EG_REQUIRE(C, EG_ERR_INVALID, "%s: C is NULL", who);
  EG_REQUIRE(K == 0 || (A && B), EG_ERR_INVALID, "%s: NULL operand", who);
  EG_REQUIRE(lda >= (trans_a ? M : K) && ldb >= (trans_b ? K : N) && ldc >= N, EG_ERR_INVALID, "%s: leading dimension smaller than the row length",
             who);
  return EG_OK;
}

// The arguments of a plain launch (C: the destination, or the slabs of a sliced product) or of item 0 of a batched one.
DgemmArgs dgemm_args(const double* A, long lda, const double* B, long ldb, double* C, long ldc, const double* bias, long M, long N, long K,
                     int accumulate, int splits, long k_per_split, int tiles_m, int tiles_n, bool remap) {
  return {A, B, C, bias, M, N, K, lda, ldb, ldc, accumulate, splits, k_per_split, tiles_m, tiles_n, remap ? 1 : 0};
}

}  // namespace

namespace eg {

long colsum_f64_scratch_doubles(const eg_ctx* ctx, long rows, long cols) { return colsum_scratch_floats(ctx, rows, cols); }

int colsum_f64_with_scratch(eg_ctx* ctx, long rows, long cols, const double* in, double* out, int accumulate, double* scratch) {
  if (cols == 0) return EG_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  int colsP = 1;
  while (colsP < cols && colsP < 64) colsP <<= 1;
  // the geometry of reduce.hip's colsum_geometry (its scratch size is what the caller reserved)
  const long col_tiles = (cols + 63) / 64;
  long nparts = (4L * ctx->compute_units + col_tiles - 1) / col_tiles;
  const long max_parts = (rows + 63) / 64;
  if (nparts > max_parts) nparts = max_parts;
  if (nparts < 1) nparts = 1;
  const long rows_per_block = (rows + nparts - 1) / nparts;
  nparts = rows_per_block > 0 ? (rows + rows_per_block - 1) / rows_per_block : 1;
  if (nparts < 1) nparts = 1;
  hipLaunchKernelGGL(colsum_partial_f64_kernel, dim3((unsigned)nparts, (unsigned)col_tiles), dim3(256), 0, ctx->stream, in, scratch, rows, cols, colsP,
                     rows_per_block);
  hipLaunchKernelGGL(colsum_final_f64_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, ctx->stream, scratch, out, cols, (int)nparts,
                     accumulate);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}

}  // namespace eg

namespace eg {
namespace gemm {

// The one internal entry of the plain float64 product: eg_dgemm and the items of a batch that runs as a loop come here.
// plan_dgemm (gemm_plan.cpp) decides tile, k-slices and geometry; this turns its plan into launches.
int dgemm(eg_ctx* ctx, int trans_a, int trans_b, long M, long N, long K, const double* A, long lda, const double* B, long ldb, double* C,
          long ldc, int accumulate, const double* bias) {
  bool empty = false;
  int rc = check_product("eg_dgemm", ctx, trans_a, trans_b, 1, M, N, K, A, lda, B, ldb, C, ldc, empty);
  if (rc || empty) return rc;
  rc = eg::set_device(ctx);
  if (rc) return rc;
  DgemmProblem prob = {M, N, K, lda, ldb, aligned16(A), aligned16(B), ctx->compute_units};
  if (const char* e = eg::sw::text(eg::Sw::DGEMM_TILE)) {  // measurement aid: "<config>[,<splits>]"; without the count the model's slices stay
    prob.force_config = atoi(e);
    if (const char* comma = strchr(e, ',')) prob.force_splits = atol(comma + 1) > 0 ? atol(comma + 1) : 1;
  }
  const DgemmPlan p = plan_dgemm(prob);
  if (p.workspace_doubles > 0) {
    rc = eg::ensure_workspace(ctx, (size_t)p.workspace_doubles * sizeof(double));
    if (rc) return rc;
  }
  double* slabs = static_cast<double*>(ctx->workspace);
  const DgemmArgs a = dgemm_args(A, lda, B, ldb, p.reduce ? slabs : C, ldc, bias, M, N, K, accumulate, p.splits, p.k_per_split, p.tiles_m, p.tiles_n, p.remap);
  // A(m, k): [M, K] rows are k-contiguous unless transposed; B(k, n): [K, N] rows are n-contiguous unless transposed
  const bool akc = !trans_a, bkc = trans_b != 0;
  rc = p.config == 0   ? launch_dgemm<128, 128, 2, 4>(ctx, p, a, akc, bkc)
       : p.config == 1 ? launch_dgemm<128, 64, 4, 2>(ctx, p, a, akc, bkc)
                       : launch_dgemm<64, 64, 2, 4>(ctx, p, a, akc, bkc);
  if (rc) return rc;
  if (p.reduce) {
    hipLaunchKernelGGL(dgemm_reduce_kernel, dim3((unsigned)((M * N + 255) / 256)), dim3(256), 0, ctx->stream, slabs, C, bias, (long)M, (long)N,
                       (long)ldc, p.splits, accumulate);
    EG_HIP_CHECK(hipGetLastError());
  }
  return EG_OK;
}

namespace {

// batch0 x batch1 items behind the entry `name`, whose checks have passed: the one launcher of both batched entries
// (one_index: eg_dgemm_batched, batch1 == 1 and every view's stride1 unused).
// The one-launch side takes no workspace, so it may run under graph capture.  The loop side is dgemm() per item: it takes
// the workspace wherever plan_dgemm slices the item (DgemmBatchedPlan::item says whether and how much), which the model
// layer's eager run of a launch sequence sizes before the sequence is captured.
int launch_items(eg_ctx* ctx, const char* name, int trans_a, int trans_b, long batch0, long batch1, long M, long N, long K, const double* A,
                 const eg::View& va, const double* B, const eg::View& vb, double* C, const eg::View& vc, int accumulate, const double* bias, bool one_index) {
  int rc = eg::set_device(ctx);
  if (rc) return rc;
  DgemmBatchedProblem prob = {batch0, M, N, K, va.ld, vb.ld, va.stride0, vb.stride0, aligned16(A), aligned16(B), ctx->compute_units};
  prob.batch1 = batch1, prob.stride_a1 = va.stride1, prob.stride_b1 = vb.stride1;
  if (const char* e = eg::sw::text(eg::Sw::DGEMM_BATCHED_ROUTE)) prob.force = strcmp(e, "launch") == 0 ? 1 : strcmp(e, "loop") == 0 ? 2 : 0;
  const DgemmBatchedPlan plan = plan_dgemm_batched(prob);
  auto at = [](auto* p, const eg::View& v, long o, long i) { return p ? p + o * v.stride0 + i * v.stride1 : p; };
  if (plan.loop) {   // every item fills the chip by itself: plain products on their own routes
    for (long o = 0; o < batch0; ++o)
      for (long i = 0; i < batch1; ++i) {
        rc = dgemm(ctx, trans_a, trans_b, M, N, K, at(A, va, o, i), va.ld, at(B, vb, o, i), vb.ld, at(C, vc, o, i), vc.ld, accumulate, bias);
        if (rc) return rc;
      }
    return EG_OK;
  }
  EG_REQUIRE(plan.tiles > 0 && plan.tiles <= BATCHED_MAX_BLOCKS, EG_ERR_INVALID, "%s: an item has too many tiles for one launch", name);
  const bool akc = !trans_a, bkc = trans_b != 0;
  if (one_index) {   // eg_dgemm_batched: its own kernel (above), the launches of the same cut; no 32-bit limit on the batch
    for (long n = 0; n < plan.launches; ++n) {
      const DgemmBatchedLaunch l = dgemm_batched_launch(plan, batch0, n);
      EG_REQUIRE(l.items > 0 && l.grid > 0 && l.grid <= BATCHED_MAX_BLOCKS, EG_ERR_INVALID, "%s: launch out of range", name);
      const DgemmArgs item = dgemm_args(at(A, va, l.first, 0), va.ld, at(B, vb, l.first, 0), vb.ld, at(C, vc, l.first, 0), vc.ld, bias, M, N, K, accumulate,
                                        1, dgemm_k_unsliced(K), plan.tiles_m, plan.tiles_n, false);
      const DgemmBatched1Args args = {item, va.stride0, vb.stride0, vc.stride0, (int)plan.tiles, l.remap ? 1 : 0};
      rc = launch_batched(ctx, (unsigned)l.grid, args, akc, bkc, plan.vec);
      if (rc) return rc;
    }
    return EG_OK;
  }
  // two batch indices: both extents are below 2^31 (dgemm_batched2 checks), which the kernel's 32-bit item decode relies on
  const long items = batch0 * batch1;
  DgemmBatchedArgs args = {};
  args.item = dgemm_args(A, va.ld, B, vb.ld, C, vc.ld, bias, M, N, K, accumulate, 1, dgemm_k_unsliced(K), plan.tiles_m, plan.tiles_n, false);
  args.a = va, args.b = vb, args.c = vc;
  return eg::for_each_launch(name, items, eg::cut_items(items, plan.tiles), batch1, [&](const eg::Items& it, unsigned grid) {
    args.items = it;
    return launch_batched(ctx, grid, args, akc, bkc, plan.vec);
  });
}

}  // namespace

// The internal entry of one batch index: eg_dgemm_batched and the model layer's launches with one batch index come here.
int dgemm_batched(eg_ctx* ctx, int trans_a, int trans_b, long batch, long M, long N, long K, const double* A, long lda, long stride_a,
                  const double* B, long ldb, long stride_b, double* C, long ldc, long stride_c, int accumulate, const double* bias) {
  bool empty = false;
  int rc = check_product("eg_dgemm_batched", ctx, trans_a, trans_b, batch, M, N, K, A, lda, B, ldb, C, ldc, empty);
  if (rc || empty) return rc;
  EG_REQUIRE(stride_a >= 0 && stride_b >= 0, EG_ERR_INVALID, "eg_dgemm_batched: negative stride");
  EG_REQUIRE(batch == 1 || stride_c >= (M - 1) * ldc + N, EG_ERR_INVALID, "eg_dgemm_batched: stride_c makes the items of C overlap");
  return launch_items(ctx, "eg_dgemm_batched", trans_a, trans_b, batch, 1, M, N, K, A, {lda, stride_a, 0}, B, {ldb, stride_b, 0}, C,
                      {ldc, stride_c, 0}, accumulate, bias, true);
}

// The internal entry of two batch indices: eg_dgemm_batched2 comes here.  The conventions of sgemm_batched2 (gemm_batched.hip).
int dgemm_batched2(eg_ctx* ctx, int trans_a, int trans_b, long batch0, long batch1, long M, long N, long K, const double* A, long lda,
                   long stride_a0, long stride_a1, const double* B, long ldb, long stride_b0, long stride_b1, double* C, long ldc, long stride_c0,
                   long stride_c1, int accumulate, const double* bias) {
  EG_REQUIRE(ctx, EG_ERR_INVALID, "eg_dgemm_batched2: ctx is NULL");
  EG_REQUIRE(batch0 >= 0 && batch1 >= 0 && M >= 0 && N >= 0 && K >= 0, EG_ERR_INVALID, "eg_dgemm_batched2: negative extent");
  EG_REQUIRE(batch0 < (1L << 31) && batch1 < (1L << 31), EG_ERR_INVALID, "eg_dgemm_batched2: a batch extent of 2^31 or more");
  if (batch0 == 0 || batch1 == 0 || M == 0 || N == 0) return EG_OK;
  EG_REQUIRE(C, EG_ERR_INVALID, "eg_dgemm_batched2: C is NULL");
  EG_REQUIRE(K == 0 || (A && B), EG_ERR_INVALID, "eg_dgemm_batched2: NULL operand");
  EG_REQUIRE(lda >= (trans_a ? M : K) && ldb >= (trans_b ? K : N), EG_ERR_INVALID,
             "eg_dgemm_batched2: leading dimension smaller than the row length");
  EG_REQUIRE(stride_a0 >= 0 && stride_a1 >= 0 && stride_b0 >= 0 && stride_b1 >= 0, EG_ERR_INVALID, "eg_dgemm_batched2: negative stride");
  EG_REQUIRE(batched2_c_distinct(batch0, stride_c0, batch1, stride_c1, M, ldc, N), EG_ERR_INVALID,
             "eg_dgemm_batched2: ldc, stride_c0 and stride_c1 make elements of C share an address");
  if (M == 1 && ldc < N) ldc = N;   // a single row: ldc addresses nothing, and the plain product insists on ldc >= N
  return launch_items(ctx, "eg_dgemm_batched2", trans_a, trans_b, batch0, batch1, M, N, K, A, {lda, stride_a0, stride_a1}, B,
                      {ldb, stride_b0, stride_b1}, C, {ldc, stride_c0, stride_c1}, accumulate, bias, false);
}

// The model layer's batched launches (host/run.cpp): batch1 == 0 is a product with one batch index, its strides each view's stride0.
int dgemm_batched_views(eg_ctx* ctx, int trans_a, int trans_b, long batch0, long batch1, long M, long N, long K, const double* A, const View& a,
                        const double* B, const View& b, double* C, const View& c, int accumulate, const double* bias) {
  if (batch1 > 0)
    return dgemm_batched2(ctx, trans_a, trans_b, batch0, batch1, M, N, K, A, a.ld, a.stride0, a.stride1, B, b.ld, b.stride0, b.stride1, C, c.ld,
                          c.stride0, c.stride1, accumulate, bias);
  return dgemm_batched(ctx, trans_a, trans_b, batch0, M, N, K, A, a.ld, a.stride0, B, b.ld, b.stride0, C, c.ld, c.stride0, accumulate, bias);
}

}  // namespace gemm
}  // namespace eg

extern "C" int eg_dgemm(eg_ctx* ctx, int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, const double* B,
                        int64_t ldb, double* C, int64_t ldc, int accumulate, const double* bias) {
  return eg::gemm::dgemm(ctx, trans_a, trans_b, M, N, K, A, lda, B, ldb, C, ldc, accumulate, bias);
}

extern "C" int eg_dgemm_batched(eg_ctx* ctx, int trans_a, int trans_b, int64_t batch, int64_t M, int64_t N, int64_t K, const double* A,
                                int64_t lda, int64_t stride_a, const double* B, int64_t ldb, int64_t stride_b, double* C, int64_t ldc,
                                int64_t stride_c, int accumulate, const double* bias) {
  return eg::gemm::dgemm_batched(ctx, trans_a, trans_b, batch, M, N, K, A, lda, stride_a, B, ldb, stride_b, C, ldc, stride_c, accumulate,
                                 bias);
}

extern "C" int eg_dgemm_batched2(eg_ctx* ctx, int trans_a, int trans_b, int64_t batch0, int64_t batch1, int64_t M, int64_t N, int64_t K,
                                 const double* A, int64_t lda, int64_t stride_a0, int64_t stride_a1, const double* B, int64_t ldb, int64_t stride_b0,
                                 int64_t stride_b1, double* C, int64_t ldc, int64_t stride_c0, int64_t stride_c1, int accumulate, const double* bias) {
  return eg::gemm::dgemm_batched2(ctx, trans_a, trans_b, batch0, batch1, M, N, K, A, lda, stride_a0, stride_a1, B, ldb, stride_b0, stride_b1, C, ldc,
                                  stride_c0, stride_c1, accumulate, bias);
}

extern "C" int eg_fill_f64(eg_ctx* ctx, int64_t n, double value, double* out) {
  EG_REQUIRE(ctx, EG_ERR_INVALID, "eg_fill_f64: ctx is NULL");
  EG_REQUIRE(n >= 0, EG_ERR_INVALID, "eg_fill_f64: negative count");
  if (n == 0) return EG_OK;
  EG_REQUIRE(out, EG_ERR_INVALID, "eg_fill_f64: NULL tensor");
  int rc = eg::set_device(ctx);
  if (rc) return rc;
  long blocks = (n + 255) / 256;
  if (blocks > 8L * ctx->compute_units) blocks = 8L * ctx->compute_units;
  hipLaunchKernelGGL((fill_kernel_t<double>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, out, (long)n, value);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}

extern "C" int eg_fill_uniform_f64(eg_ctx* ctx, int64_t n, double lo, double hi, const uint64_t* state, uint64_t stream, double* out) {
  EG_REQUIRE(ctx && state, EG_ERR_INVALID, "eg_fill_uniform_f64: NULL argument");
  EG_REQUIRE(n >= 0, EG_ERR_INVALID, "eg_fill_uniform_f64: negative count");
  if (n == 0) return EG_OK;
  EG_REQUIRE(out, EG_ERR_INVALID, "eg_fill_uniform_f64: NULL tensor");
  int rc = eg::set_device(ctx);
  if (rc) return rc;
  long blocks = (n + 255) / 256;
  if (blocks > 8L * ctx->compute_units) blocks = 8L * ctx->compute_units;
  hipLaunchKernelGGL(fill_uniform_f64_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, out, (long)n, lo, hi, state, stream);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}

extern "C" int eg_colsum_f64(eg_ctx* ctx, int64_t rows, int64_t cols, const double* in, double* out, int accumulate) {
  EG_REQUIRE(ctx, EG_ERR_INVALID, "eg_colsum_f64: ctx is NULL");
  EG_REQUIRE(rows >= 0 && cols >= 0, EG_ERR_INVALID, "eg_colsum_f64: negative extent");
  if (cols == 0) return EG_OK;
  EG_REQUIRE(out && (rows == 0 || in), EG_ERR_INVALID, "eg_colsum_f64: NULL tensor");
  int rc = eg::ensure_workspace(ctx, (size_t)eg::colsum_f64_scratch_doubles(ctx, rows, cols) * sizeof(double));
  if (rc) return rc;
  return eg::colsum_f64_with_scratch(ctx, rows, cols, in, out, accumulate, static_cast<double*>(ctx->workspace));
}
