// Contraction with a generated epilogue: the host plans the launch exactly as eg_sgemm would, the
// kernel is gemm_block<..., Epi> from gemm_f32_mfma.hpp compiled at run time (hiprtc) together with
// the `Epi` functor that host/epilogue.cpp generates from the fused consumer kernel.
//
// Role in the reference: none on its GPU target — every lowered kernel is its own launch
// (llvmgen.nim:455-500); on the CPU target fuseLoops (passes.nim:1929-2004) merges `dense` with
// the following activation into one loop nest.  Here the activation (and, in the backward pass,
// the activation gradient) runs on the accumulator registers of the matrix kernel, so the
// intermediate tensor is written at most once and never re-read.
#pragma once
#include <string>

#include "../eg_internal.hpp"
#include "item_grid.hpp"   // View

namespace eg {
namespace gemm {

struct FusedLaunch {
  int bm = 0, bn = 0, bk = 0, wm = 0, wn = 0, minb = 0, nt = 0;
  bool a_kc = false, b_kc = false, edge = false, dma = false;
  int vec = 1;
  int splits = 1;   // > 1: the problem needs split-K, run it unfused
  unsigned grid = 0;
  // K <= 16 and a row-major output whose rows 256 threads cover evenly: a store stream, not matrix work — the streaming
  // kernel on the vector ALUs (gemm_f32_mfma.hpp, gemm_narrow_k_block) instead of the matrix tile; narrow_grid blocks
  // of 256 threads.  Withdrawn by set_epilogue_operands for unaligned operands and by the caller for a row product.
  bool narrow = false;
  int narrow_k = 0;
  unsigned narrow_grid = 0;
  long matrix_k_per_split = 0;   // GemmArgs::k_per_split of the matrix tile (the streaming kernel reads its rows per block there)
  alignas(8) unsigned char args[336];  // the kernel's GemmArgs (opaque to host-only translation units)
  unsigned args_size = 0;
  unsigned waves = 0;   // per block (EG_GEMM_TRACE)
};
constexpr int MAX_EPILOGUE_OPERANDS = 6;

// Plan C = op(A) * op(B) (+ bias) like eg_sgemm(accumulate = 0).  `out.args` is ready to launch
// except for the epilogue operands.
int plan_fused(eg_ctx* ctx, int trans_a, int trans_b, long M, long N, long K, const float* A, long lda, const float* B,
               long ldb, float* C, long ldc, const float* bias, FusedLaunch& out);

// The exact f32 product behind eg_sgemm (gemm_f32_mfma.hip); run_if: GemmArgs::run_if (nullptr: always runs).
int sgemm_exact(eg_ctx* ctx, int trans_a, int trans_b, long M, long N, long K, const float* A, long lda, const float* B, long ldb,
                float* C, long ldc, int accumulate, const float* bias, const unsigned* run_if = nullptr, unsigned run_if_val = 0);
// Does sgemm_exact run this product as one whole-tile launch (gemm_plan.hpp, exact_single_launch)?
bool exact_single_launch(eg_ctx* ctx, int trans_a, int trans_b, long M, long N, long K, const float* A, long lda, const float* B,
                         long ldb, const float* C, long ldc, const float* bias);
// eg_sgemm's split-bf16 path (gemm_split_bf16.hip): EG_ERR_UNSUPPORTED, before any launch, when it does not apply.
int sgemm_split(eg_ctx* ctx, int trans_a, int trans_b, long M, long N, long K, const float* A, long lda, const float* B, long ldb,
                float* C, long ldc, int accumulate, const float* bias);
// The split pass in front of that product (gemm_split_pass.hip), launched on ctx->stream.  op(X) is rows x K: X[r * ld + k]
// when k_contiguous, X[k * ld + r] otherwise; rows % 32 == 0, K % 32 == 0, src 16-byte aligned.  The plane layout, which
// is all the two files share: `planes` holds bf16 [plane][k / 16][row][16], three planes per operand (piece 0, 1, 2 of
// every element), op(B)'s three planes behind op(A)'s, 6 (a.rows + b.rows) K bytes in all.  An element that does not
// split exactly sets *ctx->split_flag to `epoch`.
struct SplitPassOperand {
  const float* src;
  long ld, rows;
  bool k_contiguous;
};
int split_pass(eg_ctx* ctx, const SplitPassOperand& a, const SplitPassOperand& b, long K, void* planes, unsigned epoch);

// `batch` exact f32 products of one shape, X_b = X + b * stride_x, in one launch (gemm_batched.hip): what eg_sgemm_batched
// and the model layer's launches with one batch index run.
int sgemm_batched(eg_ctx* ctx, int trans_a, int trans_b, long batch, long M, long N, long K, const float* A, long lda, long stride_a,
                  const float* B, long ldb, long stride_b, float* C, long ldc, long stride_c, int accumulate, const float* bias);
// batch0 x batch1 exact f32 products of one shape, X_{o,i} = X + o * stride_x0 + i * stride_x1, by the same kernel and
// launcher (gemm_batched.hip): what eg_sgemm_batched2 and the model layer's launches with two batch indices run.
int sgemm_batched2(eg_ctx* ctx, int trans_a, int trans_b, long batch0, long batch1, long M, long N, long K, const float* A, long lda,
                   long stride_a0, long stride_a1, const float* B, long ldb, long stride_b0, long stride_b1, float* C, long ldc, long stride_c0,
                   long stride_c1, int accumulate, const float* bias);
// Either of the two with an operand as its View (item_grid.hpp), the model layer's one call: batch1 == 0 is sgemm_batched
// over batch0 items with every view's stride0, batch1 > 0 is sgemm_batched2.
int sgemm_batched_views(eg_ctx* ctx, int trans_a, int trans_b, long batch0, long batch1, long M, long N, long K, const float* A, const View& a,
                        const float* B, const View& b, float* C, const View& c, int accumulate, const float* bias);
// The float64 twins (gemm_f64_mfma.hip): the plain product behind eg_dgemm, and `batch` of them in one launch — what
// eg_dgemm_batched and a float64 model's batched launches run.  Strides and leading dimensions in doubles.
int dgemm(eg_ctx* ctx, int trans_a, int trans_b, long M, long N, long K, const double* A, long lda, const double* B, long ldb, double* C,
          long ldc, int accumulate, const double* bias);
int dgemm_batched(eg_ctx* ctx, int trans_a, int trans_b, long batch, long M, long N, long K, const double* A, long lda, long stride_a,
                  const double* B, long ldb, long stride_b, double* C, long ldc, long stride_c, int accumulate, const double* bias);
// batch0 x batch1 of them by the same tile body and launcher, on the item grid (what eg_dgemm_batched2 runs), and either entry with an operand as
// its View, the float64 model layer's one call: batch1 == 0 is dgemm_batched, batch1 > 0 is dgemm_batched2.
int dgemm_batched2(eg_ctx* ctx, int trans_a, int trans_b, long batch0, long batch1, long M, long N, long K, const double* A, long lda,
                   long stride_a0, long stride_a1, const double* B, long ldb, long stride_b0, long stride_b1, double* C, long ldc, long stride_c0,
                   long stride_c1, int accumulate, const double* bias);
int dgemm_batched_views(eg_ctx* ctx, int trans_a, int trans_b, long batch0, long batch1, long M, long N, long K, const double* A, const View& a,
                        const double* B, const View& b, double* C, const View& c, int accumulate, const double* bias);
// The planner's switches as the exact product reads them (gemm_plan.hpp; gemm_f32_mfma.hip keeps them per thread).
struct GemmSwitches;
const GemmSwitches& current_switches();

// Weight gradient + bias gradient in one contraction (gemm_f32_mfma.hip): C[M + 1, N] = [op(A); 1] * op(B).
bool ones_row_supported(int trans_a, int trans_b, long M, long N, long K, const float* A, long lda, const float* B, long ldb);
int sgemm_ones_row(eg_ctx* ctx, int trans_a, int trans_b, long M, long N, long K, const float* A, long lda, const float* B,
                   long ldb, float* C, long ldc, int accumulate);

// Tensors the generated epilogue reads / writes (a.epi[i]), the seed-gradient scale and the epoch.
void set_epilogue_operands(FusedLaunch& f, void* const* ptrs, int count, float grad_scale, long epoch);

// Back to the matrix tile (an operand turned out unaligned, a row product rides on the launch, the batch pipeline).
void fused_withdraw_narrow(FusedLaunch& f);

// Does every tile of the planned launch leave through the wide-store pass (after set_epilogue_operands)?
bool fused_wide_store(const FusedLaunch& f);

// Identifies the template instantiation (cache key / kernel name suffix).
std::string fused_variant(const FusedLaunch& f);

// Complete hiprtc translation unit: the kernel header, `epi_struct` (which must define
// `struct <epi_name>` with ACTIVE and apply) and an extern "C" kernel `kernel_name(GemmArgs)`.
std::string fused_source(const FusedLaunch& f, const std::string& epi_struct, const std::string& epi_name,
                         const std::string& kernel_name);

// EG_GEMM_TRACE=1: cycle stamps of every wave of a launch (entry, k loop begins, k loop ends, epilogue done) — trace_begin
// allocates and zeroes the buffer (the pointer goes into the launch's GemmArgs), trace_end waits, prints mean / max and frees.
long long* trace_begin(eg_ctx* ctx, unsigned blocks, unsigned waves);
void fused_set_trace(FusedLaunch& f, long long* buffer);
void trace_end(eg_ctx* ctx, long long* buffer, unsigned blocks, unsigned waves, const char* what);

}  // namespace gemm
}  // namespace eg
