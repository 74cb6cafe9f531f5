// Execution of a plan: one launch (whole, or one half of the batch), a range of launches (with the side lane), HIP-graph
// capture and replay, the batch pipeline, the exchange plan of the data-parallel step.
#include <algorithm>

#include <cstring>

#include "model_types.hpp"
#include "../kernels/attention.hpp"
#include <random>

namespace eg {
namespace model {

// Device-resident generator state of the model's TensorRandom tensors: {seed, fills drawn so far}.
int ensure_rng(eg_model* m, uint64_t seed, bool reseed) {
  EG_HIP_CHECK(hipSetDevice(m->ctx->device));
  const bool fresh = m->rng_state == nullptr;
  if (fresh) EG_HIP_CHECK(hipMalloc((void**)&m->rng_state, 2 * sizeof(uint64_t)));
  if (fresh || reseed) {
    const uint64_t init[2] = {seed, 0};
    EG_HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
    EG_HIP_CHECK(hipMemcpy(m->rng_state, init, sizeof(init), hipMemcpyHostToDevice));
  }
  return EG_OK;
}

namespace {

// What is being issued: launches [begin, end) of the plan (decides MODE of a row group with a tail and FOLD of a map group
// behind a sample group), and the row group whose fold the next fork of an overlap group runs on the side lane (-1: none).
struct Issue {
  int begin = 0, end = 0, defer_fold_of = -1;
};

// One half of a launch (the batch pipeline): rows [row0, row0 + rows) of the batch; second = the later half (reductions
// accumulate).  The issue functions that can cut a launch take a pointer: nullptr is the whole launch.
struct Slice {
  long row0 = 0, rows = 0;
  bool second = false;
};

// The argument list of a generated kernel: values first, their addresses when the list is complete (data()).
struct KernelArgs {
  union Cell {
    const void* p;
    long l;
    float f;
  };
  std::vector<Cell> cells;
  std::vector<void*> slots;
  KernelArgs() {
    cells.reserve(32);
    slots.reserve(32);
  }
  Cell& next() { return cells.emplace_back(); }
  void ptr(const void* p) { next().p = p; }
  void i64(long v) { next().l = v; }
  void f32(float v) { next().f = v; }
  void** data() {
    slots.clear();
    for (Cell& c : cells) slots.push_back(&c);
    return slots.data();
  }
};

// a tensor the kernel cannot do without: its pointer, or the error that it has none
int add_stored(eg_model* m, TargetState& ts, Plan& plan, int tid, KernelArgs& args) {
  float* p = tensor_ptr(m, ts, plan, tid);
  if (!p && prod(plan.shapes.at(tid)) > 0) {
    set_error("tensor %d has no device storage", tid);
    return EG_ERR_INVALID;
  }
  args.ptr(p);
  return EG_OK;
}

int run_launch(eg_model* m, TargetState& ts, Plan& plan, Launch& L, int index, const Issue& is, const Slice* sl = nullptr);

int issue_seed(eg_model* m, TargetState& ts, Plan& plan, const Launch& L) {
  if (m->f64) return eg_fill_f64(m->ctx, L.count, (double)m->grad_scale, reinterpret_cast<double*>(tensor_ptr(m, ts, plan, L.c_tensor)));
  return eg_fill_f32(m->ctx, L.count, m->grad_scale, tensor_ptr(m, ts, plan, L.c_tensor));
}

// A contraction, whole or one half of the batch.  A half by rows (slice_mode 1) has its rows of A and C; a half of a
// reduction over the batch (slice_mode 2: weight gradients, with or without the ones row) has its rows of A and B, and
// the second half adds to the first.
int issue_gemm(eg_model* m, TargetState& ts, Plan& plan, const Launch& L, const Slice* sl) {
  eg_ctx* ctx = m->ctx;
  if (m->f64) {   // (a float64 plan has no batch pipeline: never a slice)
    auto dp = [&](int t) { return reinterpret_cast<double*>(tensor_ptr(m, ts, plan, t)); };
    return eg_dgemm(ctx, L.trans_a, L.trans_b, L.M, L.N, L.K, dp(L.a_tensor), L.lda, dp(L.b_tensor), L.ldb, dp(L.c_tensor), L.ldc,
                    L.accumulate, L.bias_tensor ? dp(L.bias_tensor) : nullptr);
  }
  const float* A = tensor_ptr(m, ts, plan, L.a_tensor);
  const float* B = tensor_ptr(m, ts, plan, L.b_tensor);
  float* C = tensor_ptr(m, ts, plan, L.c_tensor);
  const float* bias = L.bias_tensor ? tensor_ptr(m, ts, plan, L.bias_tensor) : nullptr;
  long M = L.M, K = L.K;
  int accumulate = L.accumulate, ones_accumulate = 0;
  if (sl && L.slice_mode == 1) {  // rows of the batch: A(m, k) = A[m * lda + k]
    M = sl->rows;
    A += sl->row0 * L.lda;
    C += sl->row0 * L.ldc;
  } else if (sl) {  // the batch is K: A(k, m) = A[k * lda + m], B(k, n) = B[k * ldb + n]
    K = sl->rows;
    A += sl->row0 * L.lda;
    B += sl->row0 * L.ldb;
    accumulate = L.accumulate || sl->second;
    ones_accumulate = sl->second ? 1 : 0;
  }
  if (L.ones_tensor) {
    // weight gradient + bias gradient in one contraction; when the operands of this run do not
    // qualify (alignment of a caller-owned input), the two reductions run separately
    int rc = eg::gemm::sgemm_ones_row(ctx, L.trans_a, L.trans_b, M, L.N, K, A, L.lda, B, L.ldb, C, L.ldc, accumulate);
    if (rc != EG_ERR_UNSUPPORTED) return rc;
    eg::clear_error();
    rc = eg_colsum(ctx, K, L.N, B, tensor_ptr(m, ts, plan, L.ones_tensor), ones_accumulate);
    if (rc) return rc;
  }
  return eg::gemm::sgemm_exact(ctx, L.trans_a, L.trans_b, M, L.N, K, A, L.lda, B, L.ldb, C, L.ldc, accumulate, bias);
}

int issue_batched(eg_model* m, TargetState& ts, Plan& plan, const Launch& L) {
  eg_ctx* ctx = m->ctx;
  const eg::View a = {L.lda, L.stride_a, L.stride_a1}, b = {L.ldb, L.stride_b, L.stride_b1}, c = {L.ldc, L.stride_c, L.stride_c1};
  if (m->f64) {
    auto dp = [&](int t) { return reinterpret_cast<double*>(tensor_ptr(m, ts, plan, t)); };
    return eg::gemm::dgemm_batched_views(ctx, L.trans_a, L.trans_b, L.batch, L.batch1, L.M, L.N, L.K, dp(L.a_tensor), a, dp(L.b_tensor), b,
                                         dp(L.c_tensor), c, L.accumulate, nullptr);
  }
  return eg::gemm::sgemm_batched_views(ctx, L.trans_a, L.trans_b, L.batch, L.batch1, L.M, L.N, L.K, tensor_ptr(m, ts, plan, L.a_tensor), a,
                                       tensor_ptr(m, ts, plan, L.b_tensor), b, tensor_ptr(m, ts, plan, L.c_tensor), c, L.accumulate, nullptr);
}

int issue_attention(eg_model* m, TargetState& ts, Plan& plan, const Launch& L) {
  const Launch::Attn& A = L.attn;
  if (m->f64) {   // a forward group under eg_model_fuse_attention_f64: the fit route is float32-only
    auto dp = [&](const Launch::Attn::Operand& x) -> double* { return x.tensor ? reinterpret_cast<double*>(tensor_ptr(m, ts, plan, x.tensor)) : nullptr; };
    EG_REQUIRE(L.kind == StepKind::Attention, EG_ERR_INVALID, "a float64 plan has no attention backward launch");
    return eg::attention::attention_forward_f64(m->ctx, A.e, A.scale_f64, dp(A.q), A.q.view, dp(A.k), A.k.view, dp(A.v), A.v.view, dp(A.o), A.o.view,
                                                L.accumulate, dp(A.sums), A.sums.view);
  }
  auto ptr = [&](const Launch::Attn::Operand& x) -> float* { return x.tensor ? tensor_ptr(m, ts, plan, x.tensor) : nullptr; };
  if (L.kind == StepKind::Attention)   // a fit group's forward has the row sums to store for the backward launch
    return eg::attention::attention_forward(m->ctx, A.e, A.scale, ptr(A.q), A.q.view, ptr(A.k), A.k.view, ptr(A.v), A.v.view, ptr(A.o), A.o.view,
                                            L.accumulate, ptr(A.sums), A.sums.view);
  return eg::attention::attention_grad(m->ctx, A.e, A.scale, ptr(A.q), A.q.view, ptr(A.k), A.k.view, ptr(A.v), A.v.view, ptr(A.o), A.o.view,
                                       ptr(A.sums), A.sums.view, ptr(A.dout), A.dout.view, ptr(A.dq), A.dq.view, ptr(A.dk), A.dk.view,
                                       ptr(A.dv), A.dv.view, A.acc);
}

// The eg_gemm_epi* kernel of an epilogue for the variant the launch was planned as, built when first needed
// (plain: the functor without the row product).
int epilogue_kernel(eg_model* m, PlanEpilogue& pe, const eg::gemm::FusedLaunch& f, bool plain, eg_kernel** out) {
  const std::string variant = eg::gemm::fused_variant(f);
  eg_kernel*& handle = plain ? pe.built_plain[variant] : pe.built[variant];
  const std::string& struct_code = plain ? pe.plain_struct_code : pe.spec.struct_code;
  if (!handle) {
    const std::string name = "eg_gemm_epi" + std::to_string(m->kernel_serial++);
    const std::string src = eg::gemm::fused_source(f, struct_code, pe.spec.struct_name, name);
    if (const char* dump = eg::sw::text(eg::Sw::DUMP_FUSED)) {  // debugging aid: the generated translation unit
      if (FILE* fp = fopen((std::string(dump) + "/" + name + "_" + variant + ".hip").c_str(), "w")) {
        fputs(src.c_str(), fp);
        fclose(fp);
      }
    }
    int rc = eg_kernel_compile(m->ctx, name.c_str(), src.c_str(), &handle);
    if (rc) {
      std::string msg = eg_last_error();
      set_error("%s\n--- generated epilogue (%s) ---\n%s", msg.c_str(), variant.c_str(), struct_code.c_str());
      handle = nullptr;
      return rc;
    }
    m->kernels.push_back(handle);
  }
  *out = handle;
  return EG_OK;
}

// A contraction with its consumer as the epilogue, whole or one half of the batch's rows (A, C and every operand of the
// epilogue, [batch, N] tensors all).
int issue_fused(eg_model* m, TargetState& ts, Plan& plan, const Launch& L, const Issue& is, const Slice* sl) {
  eg_ctx* ctx = m->ctx;
  PlanEpilogue& pe = *plan.epilogues[L.epilogue];
  const long row0 = sl ? sl->row0 : 0;
  const float* bias = L.bias_tensor ? tensor_ptr(m, ts, plan, L.bias_tensor) : nullptr;
  const float* A = tensor_ptr(m, ts, plan, L.a_tensor) + row0 * L.lda;
  const float* B = tensor_ptr(m, ts, plan, L.b_tensor);
  float* C = tensor_ptr(m, ts, plan, L.c_tensor) + row0 * L.ldc;
  eg::gemm::FusedLaunch f;
  int rc = eg::gemm::plan_fused(ctx, L.trans_a, L.trans_b, sl ? sl->rows : L.M, L.N, L.K, A, L.lda, B, L.ldb, C, L.ldc, bias, f);
  if (rc) return rc;
  // (a row product rides on the 256 x 256 matrix tile; the batch pipeline, an experiment, keeps the matrix tile)
  if (pe.row_product || sl) eg::gemm::fused_withdraw_narrow(f);
  if (sl && f.splits > 1) {
    set_error("batch pipeline: a half of a fused contraction needs split-K");
    return EG_ERR_RUNTIME;
  }
  // The tile model may ask for k-slices at run time where it did not when the plan was made (it depends on
  // ctx->compute_units, which the data-parallel tail range lowers around its launches).  The unfused route below is
  // only valid when C holds plain values and the consumer reads plain values: a predicate tensor has M*N/32 words of
  // storage (eg_sgemm would overrun it), predicate operands hold bits, and a row product's destination would stay
  // zero.  Those launches run fused on one slice — the args of plan_fused always describe the whole K.
  const bool must_fuse = pe.pred_write || !pe.pred_reads.empty() || pe.row_product || !pe.store_c;
  if (f.splits > 1 && must_fuse) f.splits = 1;
  if (f.splits > 1) {
    rc = eg::gemm::sgemm_exact(ctx, L.trans_a, L.trans_b, L.M, L.N, L.K, A, L.lda, B, L.ldb, C, L.ldc, 0, bias);
    if (rc) return rc;
    return run_launch(m, ts, plan, pe.consumer, -1, is);
  }
  void* operands[eg::gemm::MAX_EPILOGUE_OPERANDS] = {};
  for (size_t o = 0; o < pe.spec.operands.size(); ++o) operands[o] = tensor_ptr(m, ts, plan, pe.spec.operands[o]) + row0 * L.N;
  eg::gemm::set_epilogue_operands(f, operands, (int)pe.spec.operands.size(), m->grad_scale, m->epoch);
  if (pe.pred_write && plan.pred_unzeroed.count(L.c_tensor) && !eg::gemm::fused_wide_store(f)) {
    // planned to store whole words of predicate bits, but this launch will OR single bits in: zero the words first
    rc = eg::zero_ranges(ctx, {{C, storage_floats(plan, L.c_tensor)}});
    if (rc) return rc;
  }
  // a row product rides on whole 256 x 256 tiles that leave through LDS; anything else (cannot happen for the shapes
  // the plan was made for, unless an operand turns out unaligned) runs the plain functor and the product by itself
  const bool with_product = pe.row_product && f.bm == 256 && f.bn == 256 && eg::gemm::fused_wide_store(f);
  eg_kernel* handle = nullptr;
  rc = epilogue_kernel(m, pe, f, pe.row_product && !with_product, &handle);
  if (rc) return rc;
  long long* trace = nullptr;
  if (eg::sw::on(eg::Sw::GEMM_TRACE) && !f.narrow) {
    trace = eg::gemm::trace_begin(ctx, f.grid, (unsigned)f.nt / 64);
    eg::gemm::fused_set_trace(f, trace);
  }
  void* args[] = {f.args};
  rc = f.narrow ? eg::kernel_launch_raw(handle, f.narrow_grid, 1, 1, 256, args)
                : eg::kernel_launch_raw(handle, f.grid, 1, 1, (unsigned)f.nt, args);
  if (trace) {
    eg::gemm::trace_end(ctx, trace, f.grid, (unsigned)f.nt / 64, "fused contraction");
    eg::gemm::fused_set_trace(f, nullptr);
  }
  if (rc || !pe.row_product || with_product) return rc;
  return run_launch(m, ts, plan, pe.product, -1, is);
}

int issue_conv(eg_model* m, TargetState& ts, Plan& plan, const Launch& L) {
  auto conv = L.kind == StepKind::Conv ? eg_conv2_nhwc : L.kind == StepKind::ConvGradImage ? eg_conv2_nhwc_grad_image : eg_conv2_nhwc_grad_filter;
  return conv(m->ctx, L.cN, L.cH, L.cW, L.cC, L.cF, L.cFH, L.cFW, tensor_ptr(m, ts, plan, L.a_tensor), tensor_ptr(m, ts, plan, L.b_tensor),
              tensor_ptr(m, ts, plan, L.c_tensor), L.accumulate);
}

int issue_small_group(eg_model* m, TargetState& ts, Plan& plan, const Launch& L, const Issue& is) {
  PlanSmallGroup& sg = *plan.small_groups[L.row_group];
  KernelArgs args;
  for (int tid : sg.g.ptr_args) args.ptr(tensor_ptr(m, ts, plan, tid));
  args.f32(m->grad_scale);
  args.i64(m->epoch);
  if (!sg.g.fold_offset.empty()) {  // the group can add up a sample group's slab rows itself (fuse_slab_fold)
    const float* slab = plan.sample_group ? plan.sample_group->slab : nullptr;
    // only when the sample kernel ran in THIS range: behind a backward | exchange | update split the bucket holds the
    // all-reduced totals and the slab only this rank's rows
    const bool fold = L.fold_of >= is.begin && L.fold_of < is.end && slab && slab_fold_active(plan.launches[L.fold_of], is.begin, is.end);
    args.ptr(slab);
    args.i64(fold ? 1 : 0);
  }
  return eg::kernel_launch_raw(sg.handle, (unsigned)sg.g.blocks, 1, 1, 256, args.data());
}

int issue_sample_group(eg_model* m, TargetState& ts, Plan& plan, const Launch& L, const Issue& is) {
  eg_ctx* ctx = m->ctx;
  PlanSampleGroup& sg = *plan.sample_group;
  KernelArgs args;
  args.ptr(sg.slab);
  for (int tid : sg.g.ptr_args) {
    int rc = add_stored(m, ts, plan, tid, args);
    if (rc) return rc;
  }
  args.f32(m->grad_scale);
  args.i64(m->epoch);
  int rc = eg::kernel_launch_raw(sg.handle, (unsigned)sg.g.B, 1, 1, (unsigned)sg.g.threads, args.data());
  if (rc || sg.g.slab_floats <= 0) return rc;
  if (slab_fold_active(L, is.begin, is.end)) return EG_OK;  // the optimizer's map group behind this launch adds the rows up itself
  // every sample's contribution to the parameter gradients -> the gradient bucket, in a fixed order
  float* dst = ts.bucket + sg.bucket_base;
  if (eg::slab_sum_supported(sg.g.slab_floats, sg.slab, dst)) return eg::slab_sum(ctx, sg.g.B, sg.g.slab_floats, sg.slab, dst, 0);
  // a bucket bound to caller memory that is not 16-byte aligned (a sliced view), a row that is no multiple of four
  // floats, or EG_NO_SLAB_SUM: the scalar two-pass column sum, as kernels/conv2_band.cpp falls back
  rc = eg::ensure_workspace(ctx, (size_t)eg::colsum_scratch_floats(ctx, sg.g.B, sg.g.slab_floats) * sizeof(float));
  if (rc) return rc;
  return eg::colsum_with_scratch(ctx, sg.g.B, sg.g.slab_floats, sg.slab, dst, 0, static_cast<float*>(ctx->workspace));
}

// The fold of a row group's partial rows as a launch of its own: behind the row kernel when the kernel does not fold them
// itself, on the side lane when an overlap group's fork takes it over, behind each half of a cut launch (the second half
// adds to the first).
int run_row_fold(eg_model* m, TargetState& ts, Plan& plan, PlanRowGroup& pg, int nblocks, bool second_half) {
  eg::RowFinalizeArgs fa = {};
  fa.nseg = (int)pg.red_tensors.size();
  for (int s = 0; s < fa.nseg; ++s) {
    const RowGroupTensor& gt = pg.g.tensors.at(pg.red_tensors[s]);
    fa.dst[s] = tensor_ptr(m, ts, plan, pg.red_tensors[s]);
    fa.offset[s] = (int)gt.red_offset;
    fa.accumulate[s] = (gt.accumulate || second_half) ? 1 : 0;
  }
  fa.offset[fa.nseg] = (int)pg.g.red_total;
  return eg::row_finalize(m->ctx, pg.partial, nblocks, (int)pg.g.red_total, (int)pg.g.red_stride(), fa);
}

// A row group (RowFused) or a wide one (WideRows: never single_block / in_kernel_finalize: partial rows, then the fold),
// whole or one half of the batch's rows.
int issue_row_group(eg_model* m, TargetState& ts, Plan& plan, const Launch& L, int index, const Issue& is, const Slice* sl) {
  PlanRowGroup& pg = *plan.row_groups[L.row_group];
  if (sl && pg.g.single_block) {
    set_error("batch pipeline: a single-block row group cannot be cut");
    return EG_ERR_RUNTIME;
  }
  const int nblocks = sl ? (int)((sl->rows + 255) / 256) : pg.nblocks;
  KernelArgs args;
  args.ptr(pg.partial);
  for (int tid : pg.g.ptr_args) {
    float* p = tensor_ptr(m, ts, plan, tid);
    if (sl) {  // a half: its rows of the row tensors
      const RowGroupTensor& gt = pg.g.tensors.at(tid);
      if (gt.role == RowGroupTensor::RowLocal || gt.role == RowGroupTensor::RowExternal) p += sl->row0 * gt.inner;
    }
    args.ptr(p);
  }
  args.i64(sl ? sl->rows : pg.g.B);
  args.f32(m->grad_scale);
  args.i64(m->epoch);
  if (pg.g.single_block || pg.g.in_kernel_finalize)   // totals go to their destinations from inside the kernel (rowfuse.hpp)
    for (int tid : pg.red_tensors) args.ptr(tensor_ptr(m, ts, plan, tid));
  // several blocks: the last one to arrive folds the partial rows (MODE 1) and, when the range being issued
  // holds the small group behind this launch as well, runs it (MODE 2; run_range_eager skips that launch).
  // MODE 0 leaves the fold to row_finalize: the next fork runs it (deferred), or it adds a second half to the first.
  const bool deferred = index >= 0 && is.defer_fold_of == index;
  long MODE = 0;
  if (pg.g.in_kernel_finalize) {
    MODE = (deferred || sl) ? 0 : row_tail_active(L, is.begin, is.end) ? 2 : 1;
    args.ptr(pg.counter);
    args.i64(MODE);
    for (int tid : pg.g.tail_ptr_args) args.ptr(tensor_ptr(m, ts, plan, tid));
  }
  int rc = eg::kernel_launch_raw(pg.handle, (unsigned)nblocks, 1, 1, 256, args.data());
  if (rc || deferred) return rc;
  if (pg.g.red_total > 0 && !pg.g.single_block && MODE == 0) return run_row_fold(m, ts, plan, pg, nblocks, sl && sl->second);
  return EG_OK;
}

// A generated kernel.  In a float64 program one that is a convolution or one of its gradients offers itself to the
// matrix-core kernels over double first (Launch::conv_direct64).
int issue_generic(eg_model* m, TargetState& ts, Plan& plan, Launch& L) {
  eg_ctx* ctx = m->ctx;
  if (L.blocks_x <= 0 || L.blocks_y <= 0) return EG_OK;
  if (L.conv_direct64) {
    bool launched = false;
    auto dp = [&](int t) { return reinterpret_cast<double*>(tensor_ptr(m, ts, plan, t)); };
    int rc = EG_OK;
    if (L.conv_direct64 == 1) {
      rc = eg::conv2_band_forward_try(ctx, true, L.cN, L.cH, L.cW, L.cC, L.cF, L.cFH, L.cFW, dp(L.a_tensor), dp(L.b_tensor), dp(L.c_tensor), L.accumulate, &launched);
      if (!rc && !launched)   // (images too wide for a band in LDS: column strips)
        rc = eg::conv2_direct_f64_try(ctx, L.cN, L.cH, L.cW, L.cC, L.cF, L.cFH, L.cFW, dp(L.a_tensor), dp(L.b_tensor), dp(L.c_tensor), L.accumulate, &launched);
    } else if (L.conv_direct64 == 2) {
      rc = eg::conv2_band_grad_image_try(ctx, true, L.cN, L.cH, L.cW, L.cC, L.cF, L.cFH, L.cFW, dp(L.a_tensor), dp(L.b_tensor), dp(L.c_tensor), L.accumulate, &launched);
    } else {
      rc = eg::conv2_band_grad_filter_try(ctx, true, L.cN, L.cH, L.cW, L.cC, L.cF, L.cFH, L.cFW, dp(L.a_tensor), dp(L.b_tensor), dp(L.c_tensor), L.accumulate, &launched);
    }
    if (rc || launched) return rc;
    // what band and direct decline: the implicit GEMM on the float64 matrix cores, any shape (the generated kernel under EG_CONV_NO_MFMA64)
    L.conv64_kernel = nullptr;
    rc = eg::conv2_f64_mfma(ctx, L.conv_direct64, L.cN, L.cH, L.cW, L.cC, L.cF, L.cFH, L.cFW, dp(L.a_tensor), dp(L.b_tensor), dp(L.c_tensor), L.accumulate,
                            &launched, &L.conv64_kernel);
    if (rc || launched) return rc;
  }
  const GenericSource& src = L.generic->src;
  KernelArgs args;
  float* partial = nullptr;
  float* scratch = nullptr;
  if (L.kind == StepKind::GenericB) {
    const long pfloats = ((L.partial_rows * L.partial_cols + 3) & ~3L) * m->esz;
    const long sfloats = eg::colsum_scratch_floats(ctx, L.partial_rows, L.partial_cols) * m->esz;
    int rc = eg::ensure_workspace(ctx, (size_t)(pfloats + sfloats) * sizeof(float));
    if (rc) return rc;
    partial = static_cast<float*>(ctx->workspace);
    scratch = partial + pfloats;
    args.ptr(partial);
  }
  for (int tid : src.tensor_args) {
    int rc = add_stored(m, ts, plan, tid, args);
    if (rc) return rc;
  }
  for (int slot : L.epoch_slots) L.params[slot] = m->epoch;
  long blocks_x = L.blocks_x;
  if (L.kind == StepKind::GenericA && L.vec_slot >= 0) {
    // four elements per thread need 16-byte aligned operands (arena tensors are; caller-owned ones may not be)
    bool aligned = L.vec_ok;
    for (const KernelArgs::Cell& c : args.cells) aligned = aligned && (reinterpret_cast<uintptr_t>(c.p) & 15) == 0;
    L.params[L.vec_slot] = aligned ? 1 : 0;
    blocks_x = ((aligned ? L.total_items / 4 : L.total_items) + 255) / 256;
  }
  for (long v : L.params) args.i64(v);
  int rc = eg::kernel_launch_raw(L.generic->handle, (unsigned)blocks_x, (unsigned)L.blocks_y, 1, 256, args.data());
  if (rc) return rc;
  if (L.kind == StepKind::GenericB && m->f64)
    return eg::colsum_f64_with_scratch(ctx, L.partial_rows, L.partial_cols, reinterpret_cast<const double*>(partial),
                                       reinterpret_cast<double*>(tensor_ptr(m, ts, plan, L.c_tensor)), L.accumulate,
                                       reinterpret_cast<double*>(scratch));
  if (L.kind == StepKind::GenericB)
    return eg::colsum_with_scratch(ctx, L.partial_rows, L.partial_cols, partial,
                                   tensor_ptr(m, ts, plan, L.c_tensor), L.accumulate, scratch);
  return EG_OK;
}

// One launch.  index: its place in plan.launches (-1: an epilogue's consumer or product as a launch of its own);
// sl: one half of the batch (run_launch_sliced) or nullptr.
int run_launch(eg_model* m, TargetState& ts, Plan& plan, Launch& L, int index, const Issue& is, const Slice* sl) {
  switch (L.kind) {
    case StepKind::Seed: return issue_seed(m, ts, plan, L);
    case StepKind::Gemm: return issue_gemm(m, ts, plan, L, sl);
    case StepKind::GemmBatched: return issue_batched(m, ts, plan, L);
    case StepKind::Attention:
    case StepKind::AttentionGrad: return issue_attention(m, ts, plan, L);
    case StepKind::GemmFused: return issue_fused(m, ts, plan, L, is, sl);
    case StepKind::ConvGradFilter:
    case StepKind::ConvGradImage:
    case StepKind::Conv: return issue_conv(m, ts, plan, L);
    case StepKind::SmallFused: return issue_small_group(m, ts, plan, L, is);
    case StepKind::SampleFused: return issue_sample_group(m, ts, plan, L, is);
    case StepKind::WideRows:
    case StepKind::RowFused: return issue_row_group(m, ts, plan, L, index, is, sl);
    case StepKind::GenericA:
    case StepKind::GenericB: return issue_generic(m, ts, plan, L);
  }
  return EG_OK;
}

// One half of launch `index` (the batch pipeline, plan_pipeline.cpp): the kinds that issue a slice
int run_launch_sliced(eg_model* m, TargetState& ts, Plan& plan, int index, const Issue& is, const Slice& sl) {
  Launch& L = plan.launches[(size_t)index];
  switch (L.kind) {
    case StepKind::Gemm:
    case StepKind::GemmFused:
    case StepKind::RowFused: return run_launch(m, ts, plan, L, index, is, &sl);
    default: set_error("batch pipeline: launch kind %d cannot be cut", (int)L.kind); return EG_ERR_RUNTIME;
  }
}

// ---- batch pipeline (plan_pipeline.cpp) ------------------------------------------------------------
// Stage j = the j-th long contraction of the range and the streaming launches that follow it (stage
// -1: what precedes the first one).  Main lane: contraction j of half A, of half B, contraction j + 1
// of half A, ...  Side lane: the streaming launches of stage j, half A then half B.  Events carry the
// per-half dependencies between the lanes; both lanes are in order, so nothing else needs saying.
int run_pipelined(eg_model* m, TargetState& ts, Plan& plan, const SideHook* hook) {
  eg_ctx* ctx = m->ctx;
  int rc = ensure_side_lane(ctx);
  if (rc) return rc;
  const int nb = plan.n_backward;
  const Issue is = {0, nb, -1};
  std::vector<int> heavy;  // positions of the long contractions
  for (int i = 0; i < nb; ++i)
    if (plan.launches[i].heavy) heavy.push_back(i);
  const int stages = (int)heavy.size();
  const size_t need = (size_t)(stages + 1) * 4;
  while (ctx->pipe_events.size() < need) {
    hipEvent_t e;
    EG_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ctx->pipe_events.push_back(e);
  }
  auto ev_main = [&](int stage, int h) { return ctx->pipe_events[(size_t)((stage + 1) * 4 + h)]; };      // contraction (stage, h) done
  auto ev_side = [&](int stage, int h) { return ctx->pipe_events[(size_t)((stage + 1) * 4 + 2 + h)]; };  // streaming part (stage, h) done
  const Slice halves[2] = {{0, plan.pipe.half, false}, {plan.pipe.half, plan.pipe.batch - plan.pipe.half, true}};
  // everything queued so far on the main lane (zero fills, random tensors) precedes the side lane's work
  EG_HIP_CHECK(hipEventRecord(ctx->ev_fork, ctx->stream));
  EG_HIP_CHECK(hipStreamWaitEvent(ctx->side_stream, ctx->ev_fork, 0));
  for (int stage = -1; stage < stages; ++stage) {
    const int first_light = stage < 0 ? 0 : heavy[(size_t)stage] + 1;
    const int last_light = stage + 1 < stages ? heavy[(size_t)stage + 1] : nb;  // exclusive
    if (stage >= 0) {
      for (int h = 0; h < 2; ++h) {
        if (stage > 0 || heavy[0] > 0)  // the streaming launches before it, same half
          EG_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ev_side(stage - 1, h), 0));
        rc = run_launch_sliced(m, ts, plan, heavy[(size_t)stage], is, halves[h]);
        if (rc) return rc;
        EG_HIP_CHECK(hipEventRecord(ev_main(stage, h), ctx->stream));
      }
    }
    {
      LaneSwap lane(ctx);  // ctx->stream is the side lane's from here
      for (int h = 0; h < 2; ++h) {
        if (stage >= 0) EG_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ev_main(stage, h), 0));
        for (int i = first_light; i < last_light; ++i) {
          rc = run_launch_sliced(m, ts, plan, i, is, halves[h]);
          if (rc) return rc;
        }
        if (stage == stages - 1 && h == 1 && hook && hook->big == -2) {  // data-parallel step: the early gradients go out here
          rc = hook->fn(hook->user);
          if (rc) return rc;
        }
        EG_HIP_CHECK(hipEventRecord(ev_side(stage, h), ctx->stream));
      }
    }
  }
  // join: the main lane continues after the side lane's last piece
  EG_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ev_side(stages - 1, 0), 0));
  EG_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ev_side(stages - 1, 1), 0));
  return EG_OK;
}

}  // namespace

int run_range_eager(eg_model* m, TargetState& ts, Plan& plan, int begin, int end, bool zero, const SideHook* hook) {
  if (zero) {
    // allocShapes / zeroResultTensor (model.nim:318, 383): results start from zero on every call
    {
      std::vector<std::pair<float*, long>> ranges;
      if (plan.zero_floats > 0) ranges.emplace_back(plan.arena, plan.zero_floats);
      for (int tid : plan.bucket_zero) {
        float* p = ts.bucket + ts.bucket_offset[tid];
        const long n = prod(plan.shapes.at(tid)) * m->esz;
        // neighbours in the bucket (a layer's weights and bias) are one range
        if (!ranges.empty() && ranges.back().first + ranges.back().second == p)
          ranges.back().second += n;
        else
          ranges.emplace_back(p, n);
      }
      int rc = eg::zero_ranges(m->ctx, ranges);
      if (rc) return rc;
    }
    if (eg::poison_enabled()) {
      // EG_POISON: whatever is not zeroed must be overwritten completely by its first writer
      if (plan.arena_floats > plan.zero_floats)
        EG_HIP_CHECK(hipMemsetAsync(plan.arena + plan.zero_floats, 0xFF,
                                    (size_t)(plan.arena_floats - plan.zero_floats) * sizeof(float), m->ctx->stream));
      std::set<int> zeroed(plan.bucket_zero.begin(), plan.bucket_zero.end());
      for (auto& b : ts.bucket_offset)
        if (!zeroed.count(b.first) && plan.shapes.count(b.first))
          EG_HIP_CHECK(hipMemsetAsync(ts.bucket + b.second, 0xFF, (size_t)prod(plan.shapes.at(b.first)) * m->esz * sizeof(float),
                                      m->ctx->stream));
      for (auto& rg : plan.row_groups)
        if (rg->partial)
          EG_HIP_CHECK(hipMemsetAsync(rg->partial, 0xFF, (size_t)rg->nblocks * rg->g.red_stride() * sizeof(float), m->ctx->stream));
    }
    // fresh random tensors for this call (model.nim:310-314 does it on the host); the draw counter
    // is bumped on the device so a captured sequence advances on every replay
    for (size_t r = 0; r < plan.random_tensors.size(); ++r) {
      const int tid = plan.random_tensors[r];
      const TensorDef& d = m->prog.tensors[tid];
      int rc = m->f64 ? eg_fill_uniform_f64(m->ctx, prod(plan.shapes.at(tid)), d.lo, d.hi, m->rng_state, (uint64_t)tid,
                                            reinterpret_cast<double*>(plan.arena + plan.arena_offset[tid]))
                      : eg_fill_uniform(m->ctx, prod(plan.shapes.at(tid)), (float)d.lo, (float)d.hi, m->rng_state, (uint64_t)tid,
                               plan.arena + plan.arena_offset[tid]);
      if (rc) return rc;
    }
    if (!plan.random_tensors.empty()) {
      int rc = eg_rng_advance(m->ctx, m->rng_state);
      if (rc) return rc;
    }
  }
  if (plan.pipe.active && begin == 0 && end >= plan.n_backward) {
    int rc = run_pipelined(m, ts, plan, hook);
    if (rc) return rc;
    begin = plan.n_backward;
  }
  Issue is = {begin, end, -1};
  size_t next_overlap = 0;
  for (int i = begin; i < end; ++i) {
    // a row group whose fold the fork of an overlap group inside this range runs on the side lane (plan_overlap)
    for (const Plan::Overlap& ov : plan.overlaps)
      if (ov.deferred_row == i && ov.first >= begin && ov.big < end) is.defer_fold_of = i;
    // a small group that the last block of the row group in front of it has run already (fuse_row_tails)
    if (plan.launches[i].tail_of >= begin && row_tail_active(plan.launches[plan.launches[i].tail_of], begin, end)) continue;
    while (next_overlap < plan.overlaps.size() && plan.overlaps[next_overlap].first < i) ++next_overlap;
    if (next_overlap < plan.overlaps.size() && plan.overlaps[next_overlap].first == i &&
        plan.overlaps[next_overlap].big < end) {
      // fork: the side lane takes launches [i, big) after everything issued so far, the main stream
      // goes on with the contraction; join before whatever follows
      const int big = plan.overlaps[next_overlap].big;
      eg_ctx* ctx = m->ctx;
      EG_HIP_CHECK(hipEventRecord(ctx->ev_fork, ctx->stream));
      EG_HIP_CHECK(hipStreamWaitEvent(ctx->side_stream, ctx->ev_fork, 0));
      // The contraction is issued FIRST (round 6): in a captured graph the branch whose node is created first stays on the
      // queue of what precedes it and the other branch moves to a second queue, 10 - 12 us behind (r06_step_timeline.txt: the
      // long weight gradient started 12 us after the kernel that makes its operand, and the update 10 us after the
      // gradient's last kernel).  Measured on one box, six alternating runs: 0.9708 against 0.9737 ms per step — the gaps
      // shrink by 11 us, the contraction shares its CUs from the start and takes 14 us longer.  A data-parallel step keeps
      // the side lane first: its early gradient exchange rides that lane and must not queue behind 256 resident blocks.
      // EG_OVERLAP_SIDE_FIRST=1: the order of rounds 2 - 5 everywhere.
      const bool side_first = eg::sw::on(eg::Sw::OVERLAP_SIDE_FIRST) || (hook && hook->big == big);
      if (!side_first) {
        int rc = run_launch(m, ts, plan, plan.launches[big], big, is);
        if (rc) return rc;
      }
      {
        LaneSwap lane(ctx);
        const int row = plan.overlaps[next_overlap].deferred_row;
        if (row >= 0 && is.defer_fold_of == row) {
          PlanRowGroup& pg = *plan.row_groups[plan.launches[row].row_group];
          int rc = run_row_fold(m, ts, plan, pg, pg.nblocks, false);
          is.defer_fold_of = -1;
          if (rc) return rc;
        }
        for (int s2 = i; s2 < big; ++s2) {
          int rc = run_launch(m, ts, plan, plan.launches[s2], s2, is);
          if (rc) return rc;
        }
        if (hook && hook->big == big) {  // data-parallel step: the early gradients' exchange rides the side lane
          int rc = hook->fn(hook->user);
          if (rc) return rc;
        }
        EG_HIP_CHECK(hipEventRecord(ctx->ev_join, ctx->stream));  // (the side stream, while swapped)
      }
      if (side_first) {
        int rc = run_launch(m, ts, plan, plan.launches[big], big, is);
        if (rc) return rc;
      }
      EG_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
      i = big;
      continue;
    }
    // Two independent tiny contractions next to each other (a dense layer's two gradients at a small batch): one launch
    // (EG_NO_SMALL_PAIR=1: two).  Independence is checked on the storage: neither writes what the other touches.
    // (A collapsed batched product, Launch::standalone, keeps its own launch here as everywhere else.)
    if (!eg::sw::on(eg::Sw::NO_SMALL_PAIR) && !m->f64 && i + 1 < end && i + 1 != plan.n_backward &&
        !(next_overlap < plan.overlaps.size() && plan.overlaps[next_overlap].first == i + 1)) {
      const Launch &A = plan.launches[i], &B = plan.launches[i + 1];
      if (A.kind == StepKind::Gemm && B.kind == StepKind::Gemm && !A.ones_tensor && !B.ones_tensor && !A.standalone && !B.standalone &&
          eg::gemm_small_suits(A.M, A.N, A.K) && eg::gemm_small_suits(B.M, B.N, B.K)) {
        auto ptr = [&](int t) -> float* { return t ? tensor_ptr(m, ts, plan, t) : nullptr; };
        float *ca = ptr(A.c_tensor), *cb = ptr(B.c_tensor);
        const float* touched_by_b[] = {ptr(B.a_tensor), ptr(B.b_tensor), ptr(B.bias_tensor), cb};
        const float* read_by_a[] = {ptr(A.a_tensor), ptr(A.b_tensor), ptr(A.bias_tensor)};
        bool independent = ca && cb;
        for (const float* p : touched_by_b) independent = independent && p != ca;
        for (const float* p : read_by_a) independent = independent && p != cb;
        if (independent) {
          int rc = eg::gemm_small_pair(
              m->ctx,
              eg::small_gemm(A.trans_a, A.trans_b, A.M, A.N, A.K, ptr(A.a_tensor), A.lda, ptr(A.b_tensor), A.ldb, ca, A.ldc, A.accumulate,
                             ptr(A.bias_tensor)),
              eg::small_gemm(B.trans_a, B.trans_b, B.M, B.N, B.K, ptr(B.a_tensor), B.lda, ptr(B.b_tensor), B.ldb, cb, B.ldc, B.accumulate,
                             ptr(B.bias_tensor)));
          if (rc) return rc;
          ++i;
          continue;
        }
      }
    }
    int rc = run_launch(m, ts, plan, plan.launches[i], i, is);
    if (rc) return rc;
  }
  return EG_OK;
}

bool graphs_enabled() { return !eg::sw::on(eg::Sw::NO_GRAPH); }

std::string capture_key(eg_model* m, TargetState& ts) {
  std::ostringstream key;
  for (auto& in : m->inputs)
    if (in.second.bound) key << in.first << "=" << (const void*)in.second.device << ";";
  // the scale as its bit pattern: six significant digits print 0.5f and 0.5000004f (1/3000000 and 1/3000001) alike, and a
  // key that says "same" replays the graph that holds the other scale
  uint32_t scale_bits;
  memcpy(&scale_bits, &m->grad_scale, sizeof(scale_bits));
  key << "w" << m->ctx->workspace << "x" << m->ctx->aux << "s" << m->ctx->side_workspace << "y" << m->ctx->side_aux << "b"
      << (void*)ts.bucket << "g" << std::hex << scale_bits << std::dec << "e" << m->epoch;
  return key.str();
}

// slot: 0 = whole call, 1 = backward part, 2 = update part
int run_range(eg_model* m, TargetState& ts, Plan& plan, int begin, int end, bool zero, int slot) {
  int rc = eg::set_device(m->ctx);
  if (rc) return rc;
  Plan::Captured& cap = plan.graphs[slot];
  // (a range that comes down to ONE kernel — a row group whose last block runs the small group behind it — gains nothing
  //  from a graph: replaying a one-node graph measured 19 us per XOR step against 13.7 us for the plain launch)
  int launches = 0;
  for (int i = begin; i < end; ++i) {
    const int of = plan.launches[i].tail_of;
    if (!(of >= begin && plan.launches[of].tail_launch == i)) ++launches;
  }
  if (!graphs_enabled() || launches < 2) return run_range_eager(m, ts, plan, begin, end, zero);
  // every pointer / scalar that ends up in a kernel argument: as plain words first (a replay formats no string)
  const void* now[5] = {m->ctx->workspace, m->ctx->aux, m->ctx->side_workspace, m->ctx->side_aux, ts.bucket};
  if (cap.exec && cap.stamp == m->inputs_gen && cap.grad_scale == m->grad_scale && cap.epoch == m->epoch &&
      memcmp(cap.ptrs, now, sizeof(now)) == 0) {
    EG_HIP_CHECK(hipGraphLaunch(cap.exec, m->ctx->stream));
    return EG_OK;
  }
  const std::string k = capture_key(m, ts);
  if (cap.exec && cap.key == k) {  // (the bindings were renewed with the same values)
    cap.stamp = m->inputs_gen;
    memcpy(cap.ptrs, now, sizeof(now));
    cap.grad_scale = m->grad_scale;
    cap.epoch = m->epoch;
    EG_HIP_CHECK(hipGraphLaunch(cap.exec, m->ctx->stream));
    return EG_OK;
  }
  if (cap.exec) {
    // the old sequence may still be running (launches are asynchronous): let it finish before its
    // executable graph goes away
    EG_HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
    hipGraphExecDestroy(cap.exec);
    cap.exec = nullptr;
  }
  // first execution with these arguments runs eagerly (lazy kernel builds, workspace growth);
  // the second one is captured
  if (cap.key != k || cap.runs < 1) {
    if (cap.key != k) cap.runs = 0;
    cap.key = k;
    cap.runs++;
    return run_range_eager(m, ts, plan, begin, end, zero);
  }
  hipGraph_t graph = nullptr;
  hipError_t e = hipStreamBeginCapture(m->ctx->stream, hipStreamCaptureModeThreadLocal);
  const bool debug = eg::sw::on(eg::Sw::DEBUG_GRAPH);
  if (e != hipSuccess) {  // capture unavailable on this stream: stay eager
    if (debug) fprintf(stderr, "[eg] begin capture failed: %s\n", hipGetErrorString(e));
    (void)hipGetLastError();
    return run_range_eager(m, ts, plan, begin, end, zero);
  }
  rc = run_range_eager(m, ts, plan, begin, end, zero);
  e = hipStreamEndCapture(m->ctx->stream, &graph);
  if (rc) {
    if (graph) hipGraphDestroy(graph);
    return rc;
  }
  if (e != hipSuccess || !graph) {
    if (debug) fprintf(stderr, "[eg] end capture failed: %s\n", hipGetErrorString(e));
    (void)hipGetLastError();
    return run_range_eager(m, ts, plan, begin, end, zero);
  }
  if (debug) {
    size_t n = 0;
    hipGraphGetNodes(graph, nullptr, &n);
    fprintf(stderr, "[eg] captured %zu nodes for slot %d of target %s\n", n, slot, ts.target->name.c_str());
  }
  e = hipGraphInstantiate(&cap.exec, graph, nullptr, nullptr, 0);
  hipGraphDestroy(graph);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    cap.exec = nullptr;
    return run_range_eager(m, ts, plan, begin, end, zero);
  }
  cap.stamp = m->inputs_gen;
  memcpy(cap.ptrs, now, sizeof(now));
  cap.grad_scale = m->grad_scale;
  cap.epoch = m->epoch;
  EG_HIP_CHECK(hipGraphLaunch(cap.exec, m->ctx->stream));
  return EG_OK;
}

// ---- data-parallel step with the exchange overlapped (dp_rccl.cpp) -------------------
// The gradient bucket is exchanged in two parts when the backward range ends in an overlap group whose
// long contraction produces the LAST gradient (dense nets: the first layer's weight gradient, by far
// the largest): every other gradient is complete before that contraction finishes, so its all-reduce
// is issued on the side lane and runs under the contraction; only the contraction's own gradient is
// reduced after it.  Both parts are contiguous runs of the bucket (at most a few segments).
int plan_exchange(eg_model* m, TargetState& ts, Plan& plan, ExchangePlan& ex) {
  (void)m;
  ex = ExchangePlan();
  // last launch of the backward range that writes each bucket tensor
  std::map<int, int> last_writer;
  auto note = [&](int tensor, int launch) {
    if (ts.bucket_offset.count(tensor)) last_writer[tensor] = launch;
  };
  const Target& t = *ts.target;
  for (int i = 0; i < plan.n_backward; ++i) {
    const Launch& L = plan.launches[i];
    switch (L.kind) {
      case StepKind::WideRows:
      case StepKind::RowFused:
        for (int tid : plan.row_groups[L.row_group]->red_tensors) note(tid, i);
        for (auto& kv : plan.row_groups[L.row_group]->g.tensors)
          if (kv.second.role == RowGroupTensor::RowLocal && kv.second.store) note(kv.first, i);
        break;
      case StepKind::SmallFused:
        for (int ki : plan.small_groups[L.row_group]->g.kernel_index) note(t.all[ki].write.tensor, i);
        break;
      case StepKind::SampleFused:
        for (int ki : plan.sample_group->g.kernel_index) note(t.all[ki].write.tensor, i);
        break;
      case StepKind::GemmFused:
        note(L.c_tensor, i);
        note(t.all[ts.lowered[plan.epilogues[L.epilogue]->consumer.lowered].all_index].write.tensor, i);
        break;
      case StepKind::Attention: note(L.attn.o.tensor, i); break;
      case StepKind::AttentionGrad:
        note(L.attn.dq.tensor, i);
        note(L.attn.dk.tensor, i);
        note(L.attn.dv.tensor, i);
        break;
      default:
        note(L.c_tensor, i);
        note(L.ones_tensor, i);
    }
  }
  // bucket tensors in offset order -> maximal contiguous runs of one class (padding travels with its tensor);
  // true when both classes have members
  auto split_bucket = [&](auto is_late) {
    std::vector<std::pair<long, int>> order;  // (offset, tensor)
    for (auto& b : ts.bucket_offset) order.push_back({b.second, b.first});
    std::sort(order.begin(), order.end());
    bool any[2] = {false, false};
    for (size_t i = 0; i < order.size(); ++i) {
      const long begin = order[i].first, end = i + 1 < order.size() ? order[i + 1].first : ts.bucket_floats;
      auto lw = last_writer.find(order[i].second);
      const bool late = lw != last_writer.end() && is_late(lw->second);
      any[late] = true;
      std::vector<std::pair<long, long>>& segs = late ? ex.late : ex.early;
      if (!segs.empty() && segs.back().first + segs.back().second == begin) segs.back().second += end - begin;
      else segs.push_back({begin, end - begin});
    }
    return any[0] && any[1];
  };
  if (plan.pipe.active) {
    // batch pipeline: gradients written by the streaming launches (side lane) are complete when the side
    // lane ends, before the last contraction of the main lane: they go out there (hook->big == -2)
    ex.big = split_bucket([&](int writer) { return plan.launches[(size_t)writer].heavy; }) ? -2 : -1;
  } else {
    int big = -1;
    for (auto& ov : plan.overlaps)
      if (ov.big < plan.n_backward) big = ov.big;
    ex.big = big >= 0 && split_bucket([&](int writer) { return writer >= big; }) ? big : -1;
  }
  if (ex.big == -1) {  // nothing to split: one all-reduce of the whole bucket, after the backward range
    ex.late.clear();
    ex.early.clear();
    if (ts.bucket_floats > 0) ex.late.push_back({0, ts.bucket_floats});
  }
  return EG_OK;
}

}  // namespace model
}  // namespace eg
