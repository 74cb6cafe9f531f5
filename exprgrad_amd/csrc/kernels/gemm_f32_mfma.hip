// f32 contraction  C[m,n] (+)= sum_k opA(m,k) * opB(k,n) (+ bias[n])  on CDNA4 matrix cores, and
// the direct (im2col-free) convolution built on the same kernel.
//
// Replaces what the reference emits for `c[y,x] ++= a[y,it] * b[it,x]` on its GPU target
// (tests/cache/matmul_basic.ir: one work-item per output, global-memory RMW per k; or the
// user-scheduled 16x16x16 LDS tiling of tests/cache/matmul_schedule_tiled16.ir), for the two
// gradient contractions passes.nim:519-549 derives from it, and for conv2 (dnn.nim:45-49).
// The kernel itself is in gemm_f32_mfma.hpp, the choice of route, tile, split-K and second pass in
// gemm_plan.cpp; this file turns a plan into launches.
#include "gemm_skinny.hpp"
#include "gemm_f32_pair.hpp"
#include "gemm_fused.hpp"
#include "gemm_layout.hpp"
#include "gemm_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>

#include "../eg_internal.hpp"

namespace {

using namespace eg::gemm;

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The GEMM switches as the planner wants them (a parsed tile, counts), derived again after every reload of the environment
// (eg_switches_reload): kept per thread and generation so that a product parses nothing.
const GemmSwitches& gemm_switches() {
  thread_local GemmSwitches s;
  thread_local unsigned seen = 0;
  const unsigned gen = eg::sw::generation();
  if (gen == seen) return s;
  s = GemmSwitches();
  s.no_small = eg::sw::on(eg::Sw::NO_SMALL_GEMM);
  s.no_skinny = eg::sw::on(eg::Sw::NO_SKINNY_GEMM);
  s.no_pair = eg::sw::on(eg::Sw::GEMM_NO_PAIR);
  s.no_t96 = eg::sw::on(eg::Sw::GEMM_NO_T96);
  s.no_streamk = eg::sw::on(eg::Sw::GEMM_NO_STREAMK);
  s.no_xrow = eg::sw::on(eg::Sw::GEMM_NO_XROW);
  s.no_bk32 = eg::sw::on(eg::Sw::GEMM_NO_BK32);
  s.no_wide_store = eg::sw::on(eg::Sw::GEMM_NO_WIDE_STORE);
  s.no_skew = eg::sw::on(eg::Sw::GEMM_NO_SKEW);
  s.old_tile_model = eg::sw::on(eg::Sw::GEMM_OLD_TILE_MODEL);
  s.small_bk32 = eg::sw::on(eg::Sw::GEMM_SMALL_BK32);
  s.debug_tile = eg::sw::on(eg::Sw::DEBUG_TILE);
  s.trace = eg::sw::on(eg::Sw::GEMM_TRACE);
  const char* tile = eg::sw::text(eg::Sw::GEMM_FORCE_TILE);
  const char* splits = eg::sw::text(eg::Sw::GEMM_FORCE_SPLITS);
  const char* blocks = eg::sw::text(eg::Sw::STREAMK_BLOCKS_PER_CU);
  if ((s.force_tile = tile != nullptr)) sscanf(tile, "%d,%d", &s.force_bm, &s.force_bn);
  if ((s.force_splits = splits != nullptr)) s.force_splits_n = atoi(splits);
  if ((s.streamk_blocks = blocks != nullptr)) s.streamk_blocks_per_cu = atol(blocks);
  s.streamk_min_ratio = eg::sw::real(eg::Sw::STREAMK_MIN_RATIO, 24.0);
  seen = gen;
  return s;
}

GemmProblem problem_of(const eg_ctx* ctx, const GemmArgs& a, bool a_kc, bool b_kc, int conv, bool vec_ok, bool a_vec_only,
                       bool piece = false) {
  return {a.M, a.N, a.K, a_kc, b_kc, a.lda, a.ldb, a.ldc, aligned16(a.A), aligned16(a.B), aligned16(a.C), a.bias != nullptr,
          aligned16(a.bias), a.ones_row != 0, conv, vec_ok, a_vec_only, piece, ctx->compute_units};
}

GemmArgs sgemm_args(long M, long N, long K, const float* A, long lda, const float* B, long ldb, float* C, long ldc, int accumulate,
                    const float* bias) {
  return {A, B, C, bias, /*partial=*/nullptr, M, N, K, lda, ldb, ldc, /*k_per_split=*/0, /*tiles_m=*/0, /*tiles_n=*/0, accumulate};
}

// Operand "k-contiguous" flags: A[M,K] row-major has k contiguous unless transposed; B[K,N] row-major has n contiguous
// unless transposed.
GemmProblem sgemm_problem(const eg_ctx* ctx, const GemmArgs& a, bool a_kc, bool b_kc) {
  const bool vec_a = operand_vec(a.lda, a_kc ? a.K : a.M, aligned16(a.A)), vec_b = operand_vec(a.ldb, b_kc ? a.K : a.N, aligned16(a.B));
  return problem_of(ctx, a, a_kc, b_kc, 0, vec_a && vec_b, vec_a && !vec_b);
}

template <int BM, int BN, int KB, bool AKC, bool BKC, int V, bool E, int CV>
void launch_tile(eg_ctx* ctx, const GemmPlan& p, const GemmArgs& args) {
  constexpr TileWaves w = tile_waves(BM, BN);
  // 16-byte aligned operands: interior tiles run the LDS-DMA loop (gemm_f32_mfma.hpp)
  hipLaunchKernelGGL((gemm_f32_mfma_kernel<BM, BN, KB, w.wm, w.wn, w.minb, AKC, BKC, V, E, CV, 0, (V == 4 && CV != 1)>), dim3((unsigned)p.grid),
                     dim3(p.block), 0, ctx->stream, args);
}

// The four-wave kernel on the plan's tile, and the tail tiles' second pass.
template <int BM, int BN, int KB = BK>
int launch_config(eg_ctx* ctx, bool a_kc, bool b_kc, const GemmArgs& args, const GemmPlan& p, int conv) {
  // conv 2, the filter gradient: A = gOut [pixels][F], B = im2col gathered from the image; conv 1: A gathered
  if (conv == 2 && p.vec == 4) launch_tile<BM, BN, KB, false, false, 4, true, 2>(ctx, p, args);
  else if (conv == 2) launch_tile<BM, BN, KB, false, false, 1, true, 2>(ctx, p, args);
  else if (conv && p.vec == 4) launch_tile<BM, BN, KB, true, true, 4, true, 1>(ctx, p, args);
  else if (conv) launch_tile<BM, BN, KB, true, true, 1, true, 1>(ctx, p, args);
  else
    with_layout(a_kc, b_kc, [&](auto ak, auto bk) {
      if (!p.edge) launch_tile<BM, BN, KB, ak, bk, 4, false, 0>(ctx, p, args);
      else if (p.vec == 4) launch_tile<BM, BN, KB, ak, bk, 4, true, 0>(ctx, p, args);
      else if (p.vec == 1) launch_tile<BM, BN, KB, ak, bk, 1, true, 0>(ctx, p, args);
      else if constexpr (BN == 32) launch_tile<BM, BN, KB, ak, bk, 41, true, 0>(ctx, p, args);   // (41: 128 x 32 tiles only)
    });
  EG_HIP_CHECK(hipGetLastError());
  if (p.second == Second::TailReduce) {
    hipLaunchKernelGGL((gemm_tail_reduce_kernel<BM, BN>), dim3((unsigned)(args.tail_tiles * (BM / 32))), dim3(256), 0, ctx->stream, args.partial, args.C,
                       args.bias, args.M, args.N, args.ldc, args.tiles_m, args.tiles_n, args.tail_tiles, args.tail_splits, args.accumulate);
    EG_HIP_CHECK(hipGetLastError());
  }
  return EG_OK;
}

// Convolution variants: deeper k-tiles (BK = 32) — with F = 64 filters a block has little matrix
// work per barrier, so the prefetch distance of one k-tile must cover the L2 latency.
template <int BM, int BN, int CBK, int WM, int WN, int MINB>
int launch_conv(eg_ctx* ctx, const GemmArgs& args, bool vec) {
  constexpr int NT = Geometry<BM, BN, WM, WN>::NT;
  dim3 grid((unsigned)(args.tiles_m * args.tiles_n), 1, 1);
  // channels a multiple of the k-tile: interior tiles gather with LDS-DMA (a k-tile lies inside one tap)
  if (vec && args.cC % CBK == 0)
    hipLaunchKernelGGL((gemm_f32_mfma_kernel<BM, BN, CBK, WM, WN, MINB, true, true, 4, true, 1, 0, true>), grid,
                       dim3(NT), 0, ctx->stream, args);
  else if (vec)
    hipLaunchKernelGGL((gemm_f32_mfma_kernel<BM, BN, CBK, WM, WN, MINB, true, true, 4, true, 1>), grid, dim3(NT), 0,
                       ctx->stream, args);
  else
    hipLaunchKernelGGL((gemm_f32_mfma_kernel<BM, BN, CBK, WM, WN, MINB, true, true, 1, true, 1>), grid, dim3(NT), 0,
                       ctx->stream, args);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}

int run_conv(eg_ctx* ctx, GemmArgs args, bool vec) {
  args.a_rows = args.M;
  args.partial = nullptr;
  auto tiles = [&](int bm, int bn, int bk) {
    args.tiles_m = (int)((args.M + bm - 1) / bm);
    args.tiles_n = (int)((args.N + bn - 1) / bn);
    args.k_per_split = ((args.K + bk - 1) / bk) * bk;
  };
  if (args.N > 64) return -1;  // wide filter banks: the generic tile choice
  // narrow filter banks (the second layer of the fashion_mnist network: 8 -> 16 channels, 5 x 5; its image gradient:
  // 16 -> 8): a 64-column tile multiplies 48 .. 56 columns of padding; 128 x 32 tiles
  if (args.N <= 32 && args.M >= 128L * 4 * ctx->compute_units) {
    tiles(128, 32, 16);
    return launch_conv<128, 32, 16, 32, 32, 4>(ctx, args, vec);
  }
  // measured on cfg 4 (256x256x64 -> 64, 3x3): 64x64x32 66 TF, 128x64x32 64, 256x64x32 63, 128x64x16 62
  tiles(64, 64, 32);
  return launch_conv<64, 64, 32, 32, 32, 4>(ctx, args, vec);
}


// Tiny contractions (a 32-sample batch through dense(400, 10): 320 outputs, K = 400): one matrix-core
// block would walk K alone for ~20 us.  One WAVE per output element instead: lane l sums
// k = l, l + 64, ... and a shuffle tree folds the 64 partial sums (fixed order: deterministic).
__device__ __forceinline__ void gemm_small_body(long block, const float* __restrict__ A, const float* __restrict__ B, float* C,
                                                const float* __restrict__ bias, long M, long N, long K, long a_sm, long a_sk,
                                                long b_sk, long b_sn, long ldc, int accumulate) {
  const long idx = block * 4 + (threadIdx.x >> 6);  // 4 waves per block, one output each
  if (idx >= M * N) return;
  const int lane = threadIdx.x & 63;
  const long m = idx / N, n = idx - m * N;
  const float* a = A + m * a_sm;
  const float* b = B + n * b_sn;
  float s = 0.f;
  for (long k = lane; k < K; k += 64) s = s + a[k * a_sk] * b[k * b_sk];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) {
    float* c = C + m * ldc + n;
    float v = s;
    if (accumulate) v = *c + v;
    if (bias) v = v + bias[n];
    *c = v;
  }
}

__global__ __launch_bounds__(256) void gemm_small_kernel(const float* __restrict__ A, const float* __restrict__ B, float* C,
                                                         const float* __restrict__ bias, long M, long N, long K,
                                                         long a_sm, long a_sk, long b_sk, long b_sn, long ldc,
                                                         int accumulate) {
  gemm_small_body(blockIdx.x, A, B, C, bias, M, N, K, a_sm, a_sk, b_sk, b_sn, ldc, accumulate);
}

// Two independent tiny contractions in one launch (a dense layer's weight gradient and input gradient at a small batch:
// in a captured graph each launch costs ~4.5 us whatever it does).  The first blocks0 blocks run the first, the rest the
// second; every output element is computed exactly as by gemm_small_kernel.
__global__ __launch_bounds__(256) void gemm_small_pair_kernel(eg::SmallGemm g0, eg::SmallGemm g1, long blocks0) {
  const bool second = (long)blockIdx.x >= blocks0;   // block-uniform
  const eg::SmallGemm& g = second ? g1 : g0;
  gemm_small_body(second ? (long)blockIdx.x - blocks0 : (long)blockIdx.x, g.A, g.B, g.C, g.bias, g.M, g.N, g.K, g.a_sm, g.a_sk, g.b_sk,
                  g.b_sn, g.ldc, g.accumulate);
}

// plan -> workspace -> launch
int run_gemm(eg_ctx* ctx, const GemmProblem& pr, GemmArgs args, const GemmSwitches& sw) {
  if (!args.ones_row) args.a_rows = args.M;
  const GemmPlan p = plan_gemm(pr, sw);
  const bool a_kc = pr.a_kc, b_kc = pr.b_kc;
  if (p.route == Route::Remainder) {
    for (int i = 0; i < p.nparts; ++i) {
      const auto& c = p.parts[i];
      GemmArgs part = args;
      part.A = args.A + c.row0 * (a_kc ? args.lda : 1);
      part.B = args.B + c.col0 * (b_kc ? args.ldb : 1);
      part.C = args.C + c.row0 * args.ldc + c.col0;
      if (args.bias) part.bias = args.bias + c.col0;
      part.M = part.a_rows = c.M;
      part.N = c.N;
      const int rc = run_gemm(ctx, problem_of(ctx, part, a_kc, b_kc, pr.conv, pr.vec_ok, pr.a_vec_only, /*piece=*/true), part, sw);
      if (rc) return rc;
    }
    return EG_OK;
  }
  args.tiles_m = p.tiles_m;
  args.tiles_n = p.tiles_n;
  args.splits = p.splits;
  args.k_per_split = p.k_per_split;
  args.edge_splits = p.edge_splits;
  args.k_per_split_edge = p.k_per_split_edge;
  args.tail_tiles = p.tail_tiles;
  args.tail_splits = p.tail_splits;
  args.tail_k_per_split = p.tail_k_per_split;
  args.x_rows = p.x_rows;
  args.wide_store = p.wide_store;
  args.nt_store = p.nt_store;
  args.no_skew = p.no_skew;
  args.prio = p.prio && ctx->on_side_lane;
  float* scratch = nullptr;
  if (p.workspace_floats > 0) {
    const long scratch_floats = p.second == Second::Tree ? eg::colsum_scratch_floats(ctx, p.splits, args.M * args.N) : 0;
    const int rc = eg::ensure_workspace(ctx, (size_t)(p.workspace_floats + scratch_floats) * sizeof(float));
    if (rc) return rc;
    args.partial = static_cast<float*>(ctx->workspace);
    scratch = args.partial + p.workspace_floats;
  }
  const dim3 grid((unsigned)p.grid), block(p.block);
  const hipStream_t s = ctx->stream;
  switch (p.route) {
    case Route::Small:
      hipLaunchKernelGGL(gemm_small_kernel, grid, block, 0, s, args.A, args.B, args.C, args.bias, args.M, args.N, args.K,
                         a_kc ? args.lda : 1, a_kc ? 1 : args.lda, b_kc ? 1 : args.ldb, b_kc ? args.ldb : 1, args.ldc, args.accumulate);
      break;
    case Route::Skinny:
      hipLaunchKernelGGL((eg_skinny::gemm_skinny_nn_kernel<4>), grid, block, (size_t)args.K * 64, s, args.A, args.B, args.C, args.bias,
                         args.M, (int)args.N, (int)args.K, args.lda, args.ldb, args.ldc, args.accumulate);
      break;
    case Route::ExtraRows:
      if (sw.trace) args.trace = trace_begin(ctx, grid.x, 8);
      hipLaunchKernelGGL((gemm_f32_mfma_kernel<256, 256, BK, 128, 64, 1, false, false, 4, true, 0, 0, true, true>), grid, block, 0, s, args);
      EG_HIP_CHECK(hipGetLastError());
      if (sw.trace) trace_end(ctx, args.trace, grid.x, 8, "TN 256 x 256 with extra rows, k-sliced");
      break;
    case Route::Generic: {
      int rc;
      if (p.bn == 32) rc = launch_config<128, 32>(ctx, a_kc, b_kc, args, p, pr.conv);
      else if (p.bn == 64 && p.bm == 256) rc = launch_config<256, 64>(ctx, a_kc, b_kc, args, p, pr.conv);
      else if (p.bn == 64 && p.bm == 64 && p.kb == 32) rc = launch_config<64, 64, 32>(ctx, a_kc, b_kc, args, p, pr.conv);
      else if (p.bn == 64 && p.bm == 64) rc = launch_config<64, 64>(ctx, a_kc, b_kc, args, p, pr.conv);
      else if (p.bn == 64) rc = launch_config<128, 64>(ctx, a_kc, b_kc, args, p, pr.conv);
      else if (p.bn == 128) rc = launch_config<128, 128>(ctx, a_kc, b_kc, args, p, pr.conv);
      else rc = launch_config<256, 256>(ctx, a_kc, b_kc, args, p, pr.conv);
      if (rc) return rc;
      break;
    }
    default:   // the pair kernels, stream-K and the 32-deep 256 x 256 tile: one instantiation per layout
      with_layout(a_kc, b_kc, [&](auto ak, auto bk) {
        auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, s, args); };
        if (p.route == Route::Kw8 && p.edge) go(gemm_pair_kernel<32, 32, 32, 32, ak, bk, 0, 2, 128, true, 8>);
        else if (p.route == Route::Kw8) go(gemm_pair_kernel<32, 32, 32, 32, ak, bk, 0, 2, 128, false, 8>);
        else if (p.route == Route::T96) go(gemm_pair_kernel<96, 96, 96, 32, ak, bk, 0, 2, 64, false, 4>);
        else if (p.route == Route::StreamK) go(gemm_streamk_kernel<32, ak, bk>);
        else if (p.route == Route::Bk32) go(gemm_f32_mfma_kernel<256, 256, 32, 128, 64, 1, ak, bk, 4, false, 0, 0, true>);
        else if (p.route == Route::Pair && p.edge) go(gemm_pair_kernel<64, 64, 32, 32, ak, bk, 0, 2, 64, true>);
        else if (p.route == Route::Pair) go(gemm_pair_kernel<64, 64, 32, 32, ak, bk, 0, 2, 64, false>);
      });
      break;
  }
  EG_HIP_CHECK(hipGetLastError());
  // second pass (the tail tiles' ran with their tile kernel: its template is the tile's)
  const long total = args.M * args.N;
  if (p.second == Second::Tree) {
    if (eg::slab_sum_supported(total, args.partial, args.C)) return eg::slab_sum(ctx, p.splits, total, args.partial, args.C, args.accumulate);
    return eg::colsum_with_scratch(ctx, p.splits, total, args.partial, args.C, args.accumulate, scratch);
  }
  if (p.second == Second::StreamKFixup)   // (the blocks' whole rounds of tiles come first: args.splits = rounds)
    hipLaunchKernelGGL(gemm_streamk_fixup_kernel, dim3((unsigned)(total / (64 * 64) - p.splits * p.grid)), dim3(256), 0, s, args.partial, args.C,
                       args.bias, args.ldc, args.tiles_m, args.tiles_n, p.splits * p.grid, (int)(args.K / 32), p.k_per_split, args.accumulate);
  else if (p.second == Second::SplitReduce)
    hipLaunchKernelGGL(gemm_splitk_reduce_kernel, dim3((unsigned)std::min((total + 255) / 256, 2048L)), dim3(256), 0, s, args.partial, args.C,
                       args.bias, args.M, args.N, args.ldc, p.splits, args.accumulate, p.edge_splits > 0 ? (args.tiles_m - 1) * (long)p.bm : args.M,
                       p.edge_splits);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}

}  // namespace

namespace eg {
bool gemm_small_suits(long M, long N, long K) { return small_suits(M, N, K) && !gemm_switches().no_small; }

SmallGemm small_gemm(int trans_a, int trans_b, long M, long N, long K, const float* A, long lda, const float* B, long ldb, float* C,
                     long ldc, int accumulate, const float* bias) {
  SmallGemm g = {A, B, C, bias, M, N, K, trans_a ? 1 : lda, trans_a ? lda : 1, trans_b ? 1 : ldb, trans_b ? ldb : 1, ldc, accumulate};
  return g;
}

int gemm_small_pair(eg_ctx* ctx, const SmallGemm& g0, const SmallGemm& g1) {
  int rc = set_device(ctx);
  if (rc) return rc;
  const long blocks0 = (g0.M * g0.N + 3) / 4, blocks1 = (g1.M * g1.N + 3) / 4;
  hipLaunchKernelGGL(gemm_small_pair_kernel, dim3((unsigned)(blocks0 + blocks1)), dim3(256), 0, ctx->stream, g0, g1, blocks0);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}
}  // namespace eg

namespace eg {
namespace gemm {
const GemmSwitches& current_switches() { return gemm_switches(); }

// The exact f32 product (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain per element).  Everything inside the library
// (model plans, convolutions) calls this; only the public eg_sgemm may take the split-bf16 path first.
int sgemm_exact(eg_ctx* ctx, int trans_a, int trans_b, long M, long N, long K, const float* A, long lda, const float* B, long ldb,
                float* C, long ldc, int accumulate, const float* bias, const unsigned* run_if, unsigned run_if_val) {
  EG_REQUIRE(ctx, EG_ERR_INVALID, "eg_sgemm: ctx is NULL");
  EG_REQUIRE(M >= 0 && N >= 0 && K >= 0, EG_ERR_INVALID, "eg_sgemm: negative extent");
  if (M == 0 || N == 0) return EG_OK;
  EG_REQUIRE(C, EG_ERR_INVALID, "eg_sgemm: C is NULL");
  EG_REQUIRE(K == 0 || (A && B), EG_ERR_INVALID, "eg_sgemm: NULL operand");
  EG_REQUIRE(lda >= (trans_a ? M : K) && ldb >= (trans_b ? K : N) && ldc >= N, EG_ERR_INVALID,
             "eg_sgemm: leading dimension smaller than the row length");
  int rc = eg::set_device(ctx);
  if (rc) return rc;

  GemmArgs args = sgemm_args(M, N, K, A, lda, B, ldb, C, ldc, accumulate, bias);
  args.run_if = run_if;
  args.run_if_val = run_if_val;
  return run_gemm(ctx, sgemm_problem(ctx, args, !trans_a, trans_b != 0), args, gemm_switches());
}

bool exact_single_launch(eg_ctx* ctx, int trans_a, int trans_b, long M, long N, long K, const float* A, long lda, const float* B,
                         long ldb, const float* C, long ldc, const float* bias) {
  const GemmArgs args = sgemm_args(M, N, K, A, lda, B, ldb, const_cast<float*>(C), ldc, 0, bias);
  return exact_single_launch(plan_gemm(sgemm_problem(ctx, args, !trans_a, trans_b != 0), gemm_switches()));
}
}  // namespace gemm
}  // namespace eg

extern "C" int eg_sgemm(eg_ctx* ctx, int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, const float* A,
                        int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int accumulate,
                        const float* bias) {
  // large products whose operands split exactly run on the bf16 matrix cores (gemm_split_bf16.hip); the rest, and
  // every product under EG_NO_SPLIT_GEMM=1, take the exact f32 path
  const int rc = eg::gemm::sgemm_split(ctx, trans_a, trans_b, M, N, K, A, lda, B, ldb, C, ldc, accumulate, bias);
  if (rc != EG_ERR_UNSUPPORTED) return rc;
  return eg::gemm::sgemm_exact(ctx, trans_a, trans_b, M, N, K, A, lda, B, ldb, C, ldc, accumulate, bias);
}

// C[0..M) = op(A) * op(B) and C[M] = column sums of op(B) in ONE contraction: A gets a virtual last row
// of ones (GemmArgs::ones_row).  Used by the model layer to let a bias gradient ride along with the
// weight gradient that reduces over the same batch; C must have room for M + 1 rows.  Returns
// EG_ERR_UNSUPPORTED when the operands do not qualify for the LDS-DMA loop (the caller then runs the
// two reductions separately).
namespace eg {
namespace gemm {
bool ones_row_supported(int trans_a, int trans_b, long M, long N, long K, const float* A, long lda, const float* B, long ldb) {
  const bool vec_a = operand_vec(lda, trans_a ? M : K, aligned16(A)), vec_b = operand_vec(ldb, trans_b ? K : N, aligned16(B));
  // large enough for the matrix-core path (not the one-wave-per-output kernel) and at least one k-tile
  return vec_a && vec_b && K >= 16 && !((M + 1) * N <= 16384 && K <= 2048) && !eg::sw::on(eg::Sw::NO_ONES_ROW);
}

int sgemm_ones_row(eg_ctx* ctx, int trans_a, int trans_b, long M, long N, long K, const float* A, long lda, const float* B,
                   long ldb, float* C, long ldc, int accumulate) {
  EG_REQUIRE(ctx, EG_ERR_INVALID, "sgemm_ones_row: ctx is NULL");
  // an empty batch (K = 0, possibly NULL operands), a tiny problem, unaligned operands: the caller's two-call form
  if (!A || !B || !C || M <= 0 || N <= 0 || !ones_row_supported(trans_a, trans_b, M, N, K, A, lda, B, ldb)) return EG_ERR_UNSUPPORTED;
  int rc = eg::set_device(ctx);
  if (rc) return rc;
  GemmArgs args = sgemm_args(M + 1, N, K, A, lda, B, ldb, C, ldc, accumulate, nullptr);
  args.a_rows = M;
  args.ones_row = 1;
  if (!ctx->ones) {
    static const float values[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 0.f, 0.f, 0.f};
    EG_HIP_CHECK(hipMalloc((void**)&ctx->ones, sizeof(values)));
    EG_HIP_CHECK(hipMemcpy(ctx->ones, values, sizeof(values), hipMemcpyHostToDevice));
  }
  args.ones = ctx->ones;
  return run_gemm(ctx, problem_of(ctx, args, !trans_a, trans_b != 0, /*conv=*/0, /*vec_ok=*/true, false), args, gemm_switches());
}
}  // namespace gemm
}  // namespace eg

// Direct convolution as an implicit GEMM:  M = N*Ho*Wo output pixels, N = F filters,
// K = FH*FW*C taps; A is gathered from the NHWC image inside the tile loader (no im2col
// buffer), B = the filter bank [F][FH*FW*C] is already "N x K, k-contiguous".
extern "C" int eg_conv2_nhwc(eg_ctx* ctx, int64_t N, int64_t H, int64_t W, int64_t C, int64_t F, int64_t FH,
                             int64_t FW, const float* img, const float* flt, float* out, int accumulate) {
  EG_REQUIRE(ctx, EG_ERR_INVALID, "eg_conv2_nhwc: ctx is NULL");
  EG_REQUIRE(N >= 0 && H >= 0 && W >= 0 && C >= 0 && F >= 0 && FH >= 1 && FW >= 1, EG_ERR_INVALID,
             "eg_conv2_nhwc: bad extent");
  // Output shape as the reference's linear shape solver finds it (passes.nim:1420-1436):
  // max(y) + max(dy) = H - 1.
  const long Ho = H - FH + 1, Wo = W - FW + 1;
  EG_REQUIRE(Ho >= 0 && Wo >= 0, EG_ERR_SHAPE, "eg_conv2_nhwc: filter larger than image");
  if (N == 0 || Ho == 0 || Wo == 0 || F == 0) return EG_OK;
  EG_REQUIRE(out && (C == 0 || (img && flt)), EG_ERR_INVALID, "eg_conv2_nhwc: NULL tensor");
  int rc = eg::set_device(ctx);
  if (rc) return rc;
  if (FH == 1 && FW == 1 && C > 0)  // a 1x1 filter bank is a plain contraction over the channels: out[P,F] = img[P,C] * flt[F,C]^T
    return eg::gemm::sgemm_exact(ctx, 0, 1, N * H * W, F, C, img, C, flt, C, out, F, accumulate, nullptr);
  if (C > 0) {  // a few million multiply-adds in all (a batch-32 step of a small network): one thread per output element
    bool launched = false;
    rc = eg::conv2_tiny_forward_try(ctx, N, H, W, C, F, FH, FW, img, flt, out, accumulate, &launched);
    if (rc || launched) return rc;
  }
  if (C > 0 && C <= 16 && F <= 16) {  // few channels and few filters: the filter bank as fragments of 16 x 16 x 4 matrix instructions (conv2_band.cpp)
    bool launched = false;
    rc = eg::conv2_band_forward_try(ctx, false, N, H, W, C, F, FH, FW, img, flt, out, accumulate, &launched);
    if (rc || launched) return rc;
  }
  if (C > 0 && C <= 16) {  // few channels (an image network's first layers): per-pixel kernel specialised for the filter geometry
    bool launched = false;
    rc = eg::conv2_direct_try(ctx, N, H, W, C, F, FH, FW, img, flt, out, accumulate, &launched);
    if (rc || launched) return rc;
  }
  if (C > 0) {  // 3x3-class filters on full-sized images: the LDS-halo kernel
    bool launched = false;
    rc = eg::conv2_halo_try(ctx, N, H, W, C, F, FH, FW, img, flt, out, accumulate, &launched);
    if (rc || launched) return rc;
  }
  GemmArgs args = sgemm_args(N * Ho * Wo, F, FH * FW * C, img, /*lda=*/0, flt, FH * FW * C, out, F, accumulate, nullptr);
  args.cH = H;
  args.cW = W;
  args.cC = C;
  args.cFW = FW;
  args.cHo = Ho;
  args.cWo = Wo;
  const bool vec = (C % 4 == 0) && aligned16(img) && aligned16(flt);
  rc = run_conv(ctx, args, vec);
  if (rc >= 0) return rc;
  return run_gemm(ctx, problem_of(ctx, args, true, true, /*conv=*/1, vec, false), args, gemm_switches());
}

// ---- convolution gradients ------------------------------------------------------------------------
// What derive (passes.nim:383-549) produces for conv2 (dnn.nim:45-49):
//   gFlt[f,dy,dx,c]     ++= gOut[n,y,x,f] * img[n,y+dy,x+dx,c]
//   gImg[n,y+dy,x+dx,c] ++= gOut[n,y,x,f] * flt[f,dy,dx,c]
// The reference runs both as the same 7-deep loop nest as the forward pass (the second one as a
// scatter).  Here both are contractions on the matrix cores.

namespace {

// Operands of the image gradient in ONE launch:
//  - blocks [0, pad_blocks): gOut [N,Ho,Wo,F] -> zero-bordered [N, Ho + 2(FH-1), Wo + 2(FW-1), F], one
//    thread per VEC floats of one padded pixel; 32-bit index arithmetic (the host checks the sizes);
//  - the remaining blocks: flt [F,FH,FW,C] -> [C,FH,FW,F] with both spatial axes reversed.
template <int VEC>
__global__ __launch_bounds__(256) void grad_image_operands_kernel(const float* __restrict__ g, float* __restrict__ out,
                                                                  unsigned pixels, unsigned Hp, unsigned Wp, unsigned Ho,
                                                                  unsigned Wo, unsigned F, unsigned ph, unsigned pw,
                                                                  unsigned pad_blocks, const float* __restrict__ flt,
                                                                  float* __restrict__ flipped, unsigned FH, unsigned FW,
                                                                  unsigned C) {
  if (blockIdx.x >= pad_blocks) {
    const unsigned total = F * FH * FW * C;
    const unsigned stride = (gridDim.x - pad_blocks) * blockDim.x;
    for (unsigned i = (blockIdx.x - pad_blocks) * blockDim.x + threadIdx.x; i < total; i += stride) {
      const unsigned f = i % F, p = i / F;
      const unsigned dx = p % FW, q = p / FW;
      const unsigned dy = q % FH, c = q / FH;
      flipped[i] = flt[((size_t)(f * FH + (FH - 1 - dy)) * FW + (FW - 1 - dx)) * C + c];
    }
    return;
  }
  const unsigned per_pixel = F / VEC;
  const unsigned total = pixels * per_pixel;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += pad_blocks * blockDim.x) {
    const unsigned p = i / per_pixel, f = (i - p * per_pixel) * VEC;
    const unsigned xp = p % Wp, q = p / Wp;
    const unsigned yp = q % Hp, n = q / Hp;
    const unsigned y = yp - ph, x = xp - pw;  // wraps to a huge value left of / above the image
    const bool inside = y < Ho && x < Wo;
    const size_t src = ((size_t)(n * Ho + y) * Wo + x) * F + f;
    if (VEC == 4) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (inside) v = *reinterpret_cast<const f32x4*>(g + src);
      *reinterpret_cast<f32x4*>(out + (size_t)p * F + f) = v;
    } else {
      out[(size_t)p * F + f] = inside ? g[src] : 0.f;
    }
  }
}

}  // namespace

// Filter gradient as ONE contraction over all output pixels:
//   gFlt[F, FH*FW*C] (+)= gOut^T [F, P] * im2col(img) [P, FH*FW*C],  P = N*Ho*Wo
// A = gOut is a plain [P][F] matrix (m-contiguous); B is gathered from the image inside the tile
// loader (CONV = 2), never materialised.  K = P is long and the output small: split-K.
extern "C" int eg_conv2_nhwc_grad_filter(eg_ctx* ctx, int64_t N, int64_t H, int64_t W, int64_t C, int64_t F, int64_t FH,
                                         int64_t FW, const float* img, const float* gout, float* gflt,
                                         int accumulate) {
  EG_REQUIRE(ctx, EG_ERR_INVALID, "eg_conv2_nhwc_grad_filter: ctx is NULL");
  EG_REQUIRE(N >= 0 && H >= 0 && W >= 0 && C >= 0 && F >= 0 && FH >= 1 && FW >= 1, EG_ERR_INVALID,
             "eg_conv2_nhwc_grad_filter: bad extent");
  const long Ho = H - FH + 1, Wo = W - FW + 1;
  EG_REQUIRE(Ho >= 0 && Wo >= 0, EG_ERR_SHAPE, "eg_conv2_nhwc_grad_filter: filter larger than image");
  if (F == 0 || C == 0) return EG_OK;
  EG_REQUIRE(gflt, EG_ERR_INVALID, "eg_conv2_nhwc_grad_filter: NULL tensor");
  int rc = eg::set_device(ctx);
  if (rc) return rc;
  const long P = N * Ho * Wo;
  if (P == 0) {
    if (!accumulate) return eg_fill_f32(ctx, F * FH * FW * C, 0.f, gflt);
    return EG_OK;
  }
  EG_REQUIRE(img && gout, EG_ERR_INVALID, "eg_conv2_nhwc_grad_filter: NULL tensor");
  if (FH == 1 && FW == 1)  // plain contraction: gflt[F,C] = gout[P,F]^T * img[P,C]
    return eg::gemm::sgemm_exact(ctx, 1, 0, F, C, P, gout, F, img, C, gflt, C, accumulate, nullptr);
  {  // a few million multiply-adds in all: blocks of pixels, every output element per block, slabs folded in a fixed order
    bool launched = false;
    rc = eg::conv2_tiny_grad_filter_try(ctx, N, H, W, C, F, FH, FW, img, gout, gflt, accumulate, &launched);
    if (rc || launched) return rc;
  }
  if (C <= 16 && F <= 16) {  // few channels and few filters: 16 filter rows x 4 pixels x 16 taps per matrix instruction (conv2_band.cpp)
    bool launched = false;
    rc = eg::conv2_band_grad_filter_try(ctx, false, N, H, W, C, F, FH, FW, img, gout, gflt, accumulate, &launched);
    if (rc || launched) return rc;
  }
  if (C <= 4) {
    bool launched = false;
    rc = eg::conv2_direct_grad_filter_try(ctx, N, H, W, C, F, FH, FW, img, gout, gflt, accumulate, &launched);
    if (rc || launched) return rc;
  }
  EG_REQUIRE(P < (1L << 31) && FH * FW * C < (1L << 31), EG_ERR_INVALID,
             "eg_conv2_nhwc_grad_filter: more than 2^31 output pixels or taps");
  if (FH == 3 && FW == 3 && C % 32 == 0 && F % 32 == 0) {  // the halo form: every image pixel staged once per row step, not once per tap
    bool launched = false;
    rc = eg::conv2_gradf_halo_try(ctx, N, H, W, C, F, FH, FW, img, gout, gflt, accumulate, &launched);
    if (rc || launched) return rc;
  }
  GemmArgs args = sgemm_args(F, FH * FW * C, P, gout, F, img, /*ldb=*/0, gflt, FH * FW * C, accumulate, nullptr);
  args.cH = H;
  args.cW = W;
  args.cC = C;
  args.cFW = FW;
  args.cHo = Ho;
  args.cWo = Wo;
  const bool vec = (C % 4 == 0) && (F % 4 == 0) && aligned16(img) && aligned16(gout);
  return run_gemm(ctx, problem_of(ctx, args, false, false, /*conv=*/2, vec, false), args, gemm_switches());
}

// Image gradient = "full" correlation of gOut with the flipped, channel-transposed filters:
//   gImg[n,yy,xx,c] = sum_{dy,dx,f} pad(gOut)[n, yy+dy', xx+dx', f] * fltT[c, dy', dx', f],
//   dy' = FH-1-dy, dx' = FW-1-dx, pad = (FH-1, FW-1) zeros on every side.
// That is exactly a forward convolution with F and C exchanged, so it runs on eg_conv2_nhwc
// (LDS-DMA gather and all); the padded gradient and the flipped bank live in the context's
// auxiliary scratch.
extern "C" int eg_conv2_nhwc_grad_image(eg_ctx* ctx, int64_t N, int64_t H, int64_t W, int64_t C, int64_t F, int64_t FH,
                                        int64_t FW, const float* flt, const float* gout, float* gimg, int accumulate) {
  EG_REQUIRE(ctx, EG_ERR_INVALID, "eg_conv2_nhwc_grad_image: ctx is NULL");
  EG_REQUIRE(N >= 0 && H >= 0 && W >= 0 && C >= 0 && F >= 0 && FH >= 1 && FW >= 1, EG_ERR_INVALID,
             "eg_conv2_nhwc_grad_image: bad extent");
  const long Ho = H - FH + 1, Wo = W - FW + 1;
  EG_REQUIRE(Ho >= 0 && Wo >= 0, EG_ERR_SHAPE, "eg_conv2_nhwc_grad_image: filter larger than image");
  if (N == 0 || H == 0 || W == 0 || C == 0) return EG_OK;
  EG_REQUIRE(gimg, EG_ERR_INVALID, "eg_conv2_nhwc_grad_image: NULL tensor");
  int rc = eg::set_device(ctx);
  if (rc) return rc;
  if (F == 0 || Ho == 0 || Wo == 0) {
    if (!accumulate) return eg_fill_f32(ctx, N * H * W * C, 0.f, gimg);
    return EG_OK;
  }
  EG_REQUIRE(flt && gout, EG_ERR_INVALID, "eg_conv2_nhwc_grad_image: NULL tensor");
  if (FH == 1 && FW == 1)  // plain contraction: gimg[P,C] = gout[P,F] * flt[F,C]
    return eg::gemm::sgemm_exact(ctx, 0, 0, N * H * W, C, F, gout, F, flt, C, gimg, C, accumulate, nullptr);
  {  // a few million multiply-adds in all: one thread per image element, no flipped bank, no padded gradient
    bool launched = false;
    rc = eg::conv2_tiny_grad_image_try(ctx, N, H, W, C, F, FH, FW, flt, gout, gimg, accumulate, &launched);
    if (rc || launched) return rc;
  }
  if (C <= 16 && F <= 16) {  // few channels and few filters: the forward band kernel on the gradient with a virtual zero border and the bank read flipped
    bool launched = false;
    rc = eg::conv2_band_grad_image_try(ctx, false, N, H, W, C, F, FH, FW, flt, gout, gimg, accumulate, &launched);
    if (rc || launched) return rc;
  }
  const long Hp = Ho + 2 * (FH - 1), Wp = Wo + 2 * (FW - 1);
  const size_t flt_floats = (size_t)(C * FH * FW * F);
  EG_REQUIRE(flt_floats < (1UL << 32), EG_ERR_INVALID, "eg_conv2_nhwc_grad_image: filter bank exceeds 2^32 elements");
  // The halo kernel pads by itself (pixels outside the gradient come from a block of zeros): only the flipped bank is
  // prepared — no padded copy of the gradient is written and read back (cfg 4: 2 x 17 MB, 8 -> 3 us of preparation).
  // EG_CONV_NO_VIRTUAL_PAD=1: the padded copy of rounds 1 and 2.
  const bool virtual_pad = !eg::sw::on(eg::Sw::CONV_NO_VIRTUAL_PAD);
  if (virtual_pad && FH <= 3 && FW <= 3 && F % 16 == 0 && aligned16(gout) &&
      eg::conv2_halo_suits(ctx, N, Ho, Wo, F, C, FH, FW, FH - 1, FW - 1, gout, true)) {   // (the bank goes to ctx->aux: aligned)
    rc = eg::ensure_aux(ctx, flt_floats * sizeof(float));
    if (rc) return rc;
    float* flipped_only = static_cast<float*>(ctx->aux);
    const long fb = std::min<long>(((long)flt_floats + 255) / 256, 2L * ctx->compute_units);
    hipLaunchKernelGGL(grad_image_operands_kernel<1>, dim3((unsigned)fb), dim3(256), 0, ctx->stream, gout, flipped_only, 0u,
                       (unsigned)Hp, (unsigned)Wp, (unsigned)Ho, (unsigned)Wo, (unsigned)F, (unsigned)(FH - 1), (unsigned)(FW - 1),
                       0u, flt, flipped_only, (unsigned)FH, (unsigned)FW, (unsigned)C);
    EG_HIP_CHECK(hipGetLastError());
    bool launched = false;
    rc = eg::conv2_halo_try_padded(ctx, N, Ho, Wo, F, C, FH, FW, FH - 1, FW - 1, gout, flipped_only, gimg, accumulate, &launched);
    if (rc || launched) return rc;
  }
  const size_t pad_floats = ((size_t)(N * Hp * Wp * F) + 3) & ~(size_t)3;
  rc = eg::ensure_aux(ctx, (pad_floats + flt_floats) * sizeof(float));
  if (rc) return rc;
  float* padded = static_cast<float*>(ctx->aux);
  float* flipped = padded + pad_floats;
  EG_REQUIRE(N * Hp * Wp * F < (1L << 32), EG_ERR_INVALID, "eg_conv2_nhwc_grad_image: padded gradient exceeds 2^32 elements");
  const bool vec4 = F % 4 == 0 && aligned16(gout);
  const long work = N * Hp * Wp * (vec4 ? F / 4 : F);
  const long blocks = std::min<long>((work + 255) / 256, 16L * ctx->compute_units);
  const long fblocks = std::min<long>(((long)flt_floats + 255) / 256, 2L * ctx->compute_units);
  if (vec4)
    hipLaunchKernelGGL(grad_image_operands_kernel<4>, dim3((unsigned)(blocks + fblocks)), dim3(256), 0, ctx->stream, gout,
                       padded, (unsigned)(N * Hp * Wp), (unsigned)Hp, (unsigned)Wp, (unsigned)Ho, (unsigned)Wo,
                       (unsigned)F, (unsigned)(FH - 1), (unsigned)(FW - 1), (unsigned)blocks, flt, flipped, (unsigned)FH,
                       (unsigned)FW, (unsigned)C);
  else
    hipLaunchKernelGGL(grad_image_operands_kernel<1>, dim3((unsigned)(blocks + fblocks)), dim3(256), 0, ctx->stream, gout,
                       padded, (unsigned)(N * Hp * Wp), (unsigned)Hp, (unsigned)Wp, (unsigned)Ho, (unsigned)Wo,
                       (unsigned)F, (unsigned)(FH - 1), (unsigned)(FW - 1), (unsigned)blocks, flt, flipped, (unsigned)FH,
                       (unsigned)FW, (unsigned)C);
  EG_HIP_CHECK(hipGetLastError());
  return eg_conv2_nhwc(ctx, N, Hp, Wp, F, C, FH, FW, padded, flipped, gimg, accumulate);
}

// ---- contraction with a generated epilogue (gemm_fused.hpp) ----------------------------------------

namespace {
const char* const kGemmHeaderText =
#include "gemm_src.inc"
    ;
}

namespace eg {
namespace gemm {

static_assert(sizeof(GemmArgs) <= sizeof(FusedLaunch::args), "FusedLaunch::args too small");

long long* trace_begin(eg_ctx* ctx, unsigned blocks, unsigned waves) {
  long long* buffer = nullptr;
  const size_t bytes = (size_t)blocks * waves * 4 * sizeof(long long);
  if (hipMalloc((void**)&buffer, bytes) != hipSuccess) return nullptr;
  if (hipMemsetAsync(buffer, 0, bytes, ctx->stream) != hipSuccess) {
    (void)hipFree(buffer);
    return nullptr;
  }
  return buffer;
}

void fused_set_trace(FusedLaunch& f, long long* buffer) {
  GemmArgs a;
  memcpy(&a, f.args, sizeof(a));
  a.trace = buffer;
  memcpy(f.args, &a, sizeof(a));
}

void trace_end(eg_ctx* ctx, long long* buffer, unsigned blocks, unsigned waves, const char* what) {
  if (!buffer) return;
  std::vector<long long> h((size_t)blocks * waves * 4);
  if (hipStreamSynchronize(ctx->stream) == hipSuccess &&
      hipMemcpy(h.data(), buffer, h.size() * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess) {
    double sum[4] = {0, 0, 0, 0}, mx[4] = {0, 0, 0, 0};
    long cnt = 0;
    for (size_t w = 0; w < (size_t)blocks * waves; ++w) {
      if (h[w * 4] == 0 || h[w * 4 + 3] == 0) continue;
      ++cnt;
      for (int k = 1; k < 4; ++k) {
        const double d = (double)(h[w * 4 + k] - h[w * 4]);
        sum[k] += d;
        mx[k] = d > mx[k] ? d : mx[k];
      }
    }
    if (cnt)
      fprintf(stderr, "[eg] gemm trace %s (%u blocks x %u waves; cycles since wave start, mean / max): k loop begins %.0f / %.0f, ends %.0f / %.0f, "
                      "epilogue done %.0f / %.0f\n", what, blocks, waves, sum[1] / cnt, mx[1], sum[2] / cnt, mx[2], sum[3] / cnt, mx[3]);
  }
  (void)hipFree(buffer);
}
static_assert(MAX_EPILOGUE_OPERANDS == sizeof(GemmArgs::epi) / sizeof(void*), "epilogue operand count");

int plan_fused(eg_ctx* ctx, int trans_a, int trans_b, long M, long N, long K, const float* A, long lda, const float* B,
               long ldb, float* C, long ldc, const float* bias, FusedLaunch& out) {
  EG_REQUIRE(ctx && M > 0 && N > 0 && K >= 0 && C, EG_ERR_INVALID, "plan_fused: bad problem");
  const bool a_kc = !trans_a, b_kc = trans_b != 0;
  const GemmSwitches& sw = gemm_switches();
  GemmArgs args = sgemm_args(M, N, K, A, lda, B, ldb, C, ldc, 0, bias);
  GemmProblem pr = sgemm_problem(ctx, args, a_kc, b_kc);
  pr.a_vec_only = false;   // (no 16-byte-A-only form of the generated kernel)
  const GemmPlan t = generic_tile(pr, sw, /*model_vec=*/true);
  out = FusedLaunch();
  out.bm = t.bm;
  out.bn = t.bn;
  out.bk = t.kb;
  out.splits = t.splits;
  out.wm = t.waves.wm;
  out.wn = t.waves.wn;
  out.minb = t.waves.minb;
  out.nt = (t.bm / t.waves.wm) * (t.bn / t.waves.wn) * 64;
  out.a_kc = a_kc;
  out.b_kc = b_kc;
  out.edge = t.edge;
  out.vec = t.vec;
  out.dma = out.vec == 4;
  args.a_rows = M;
  args.tiles_m = (int)((M + t.bm - 1) / t.bm);
  args.tiles_n = (int)((N + t.bn - 1) / t.bn);
  args.k_per_split = ((K + BK - 1) / BK) * BK;
  if (args.k_per_split < BK) args.k_per_split = BK;
  out.grid = (unsigned)(args.tiles_m * args.tiles_n);
  args.wide_store = wide_store_ok(pr, sw, false, true);   // set_epilogue_operands withdraws it for unaligned operands
  args.prio = ctx->on_side_lane;
  args.nt_store = 1;
  args.no_skew = sw.no_skew;
  memcpy(out.args, &args, sizeof(args));
  out.args_size = sizeof(args);
  {  // tiny K: a store stream, not matrix work (gemm_narrow_k_block)
    const bool off = eg::sw::on(eg::Sw::NO_NARROW_K);
    const long tpr = N / 4;
    if (!off && K >= 1 && K <= 16 && N % 4 == 0 && tpr >= 1 && tpr <= 256 && 256 % tpr == 0 && ldc % 4 == 0 && aligned16(C) &&
        (!bias || aligned16(bias)) && M * N >= (1L << 16)) {
      out.narrow = true;
      out.narrow_k = (int)K;
      const long rows_per_trip = 4 * (256 / tpr), blocks = (M + rows_per_trip - 1) / rows_per_trip;
      // eight blocks per CU (all resident at once): every block first loads its threads' 4 x K values of B — 40 KB per block
      // at K = 10 — so more, shorter blocks cost more than they gain here (65 536 x 512 x 10, 1 024 / 2 048 / 4 096 / 8 192
      // blocks: 28.8 / 24.3 / 28.4 / 37.2 us standalone)
      const long cap = 8L * ctx->compute_units;
      long grid = blocks < cap ? blocks : cap;
      // a block's run of rows: a multiple of what it takes per trip; the kernel reads it from k_per_split (no use for it there)
      const long per = ((M + grid - 1) / grid + rows_per_trip - 1) / rows_per_trip * rows_per_trip;
      grid = (M + per - 1) / per;
      out.narrow_grid = (unsigned)grid;
      out.matrix_k_per_split = args.k_per_split;
      args.k_per_split = per;
      memcpy(out.args, &args, sizeof(args));
    }
  }
  return EG_OK;
}

void set_epilogue_operands(FusedLaunch& f, void* const* ptrs, int count, float grad_scale, long epoch) {
  GemmArgs* a = reinterpret_cast<GemmArgs*>(f.args);
  for (int i = 0; i < MAX_EPILOGUE_OPERANDS; ++i) a->epi[i] = i < count ? ptrs[i] : nullptr;
  for (int i = 0; i < count; ++i)
    if (!aligned16(ptrs[i])) {
      a->wide_store = 0;
      fused_withdraw_narrow(f);
    }
  a->epi_gs = grad_scale;
  a->epi_ep = epoch;
}

void fused_withdraw_narrow(FusedLaunch& f) {
  if (!f.narrow) return;
  f.narrow = false;
  reinterpret_cast<GemmArgs*>(f.args)->k_per_split = f.matrix_k_per_split;
}

bool fused_wide_store(const FusedLaunch& f) {
  // (the streaming kernel covers every column of a row: predicate words are stored whole when a word is eight threads)
  if (f.narrow) return reinterpret_cast<const GemmArgs*>(f.args)->ldc % 32 == 0 && (reinterpret_cast<const GemmArgs*>(f.args)->N / 4) % 8 == 0;
  return reinterpret_cast<const GemmArgs*>(f.args)->wide_store != 0 && !f.edge;
}

std::string fused_variant(const FusedLaunch& f) {
  char buf[96];
  if (f.narrow) {
    snprintf(buf, sizeof(buf), "narrow_k%d_n%ld_%c%c", f.narrow_k, (long)reinterpret_cast<const GemmArgs*>(f.args)->N, f.a_kc ? 'k' : 'm',
             f.b_kc ? 'k' : 'n');
    return buf;
  }
  snprintf(buf, sizeof(buf), "%dx%dx%d_%dx%d_%d_%c%c_v%d%s%s", f.bm, f.bn, f.bk, f.wm, f.wn, f.minb, f.a_kc ? 'k' : 'm',
           f.b_kc ? 'k' : 'n', f.vec, f.edge ? "_edge" : "", f.dma ? "_dma" : "");
  return buf;
}

std::string fused_source(const FusedLaunch& f, const std::string& epi_struct, const std::string& epi_name,
                         const std::string& kernel_name) {
  std::string s = kGemmHeaderText;
  s += "\n" + epi_struct + "\n";
  char buf[512];
  if (f.narrow) {
    snprintf(buf, sizeof(buf),
             "extern \"C\" __global__ __launch_bounds__(256) void %s(eg::gemm::GemmArgs a) {\n"
             "  eg::gemm::gemm_narrow_k_block<%d, %d, %s, %s, %s>(a);\n}\n",
             kernel_name.c_str(), f.narrow_k, (int)(reinterpret_cast<const GemmArgs*>(f.args)->N / 4), f.a_kc ? "true" : "false",
             f.b_kc ? "true" : "false", epi_name.c_str());
    s += buf;
    return s;
  }
  const int waves = f.nt / 64;
  // a ragged tile with a generated epilogue needs a few registers more than four waves per SIMD leave
  // (48 bytes of scratch at 128 VGPRs): three there
  int per_simd = (f.minb * waves + 3) / 4;
  if (f.edge && per_simd >= 4) per_simd = 3;
  snprintf(buf, sizeof(buf),
           "extern \"C\" __global__ __launch_bounds__(%d, %d) void %s(eg::gemm::GemmArgs a) {\n"
           "  eg::gemm::gemm_block<%d, %d, %d, %d, %d, %s, %s, %d, %s, false, 0, %s, %s>(a);\n}\n",
           f.nt, per_simd, kernel_name.c_str(), f.bm, f.bn, f.bk, f.wm, f.wn, f.a_kc ? "true" : "false",
           f.b_kc ? "true" : "false", f.vec, f.edge ? "true" : "false", f.dma ? "true" : "false", epi_name.c_str());
  s += buf;
  return s;
}

}  // namespace gemm
}  // namespace eg
