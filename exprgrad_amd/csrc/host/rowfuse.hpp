// Row fusion: run a chain of per-sample kernels as ONE generated kernel, one thread per sample.
//
// The layer's public header.  Units, none with a HIP header: rowfuse_row.cpp (thread per sample), rowfuse_small.cpp (small, map),
// rowfuse_sample.cpp + rowfuse_sample_conv.cpp (block per sample), rowfuse_wide.cpp (wave per sample), rowfuse_common.cpp.
//
// Role in the reference: fuseLoops (passes.nim:1929-2004, 2526-2549) merges consecutive kernels
// that share their leading loop — on the CPU target dense + bias + activation become one `y`
// loop.  The reference's GPU target does not benefit (each lowered kernel is still its own
// launch, llvmgen.nim:455-500).  Here the idea is taken further for the launch-bound small-width
// chains of the hot path (the whole forward + backward of the XOR net: 15 kernels over [B,4] /
// [B,1] tensors; the softmax / cross-entropy gradient chain of the dense net over [B,10]):
//   * a kernel is a "row kernel" if it has one loop over the batch B that indexes dimension 0 of
//     every batch-major tensor it touches ([B, inner...], inner size <= 64), all its other loops
//     are short, and everything else it touches is small (parameters, their gradients);
//   * a run of consecutive row kernels is specialised for the current shapes (all extents become
//     literals, loops fully unroll) and emitted as one kernel: thread y keeps the rows of the
//     intermediate tensors in registers, tensors needed later are stored once, tensors that are
//     dead after the run never touch memory;
//   * writes that reduce over the batch (bias / weight gradients, losses) accumulate in
//     registers, are folded across the block with wave shuffles + LDS, and one small `finalize`
//     launch adds the per-block partials into the destination tensors in fixed order
//     (deterministic, no float atomics).
#pragma once
#include <map>
#include <set>
#include <string>
#include <vector>

#include "kd.hpp"

namespace eg {
namespace kd {

struct RowKernelInfo {
  bool ok = false;
  int row_loop = -1;     // index into k.loops of the batch iterator (or of the raw iterator)
  bool raw = false;      // the batch iterator is a raw `{it}` index over B * inner elements
  long inner = 0;        // raw: inner size S (it = y * S + j)
  bool small_only = false;  // touches only small tensors and has no batch loop (the gradLoss seed)
  long work = 0;         // unrolled iterations per sample
};

// Can `k` run as part of a row group over batch size B?
RowKernelInfo analyse_row_kernel(const Program& prog, const Kernel& k, const KernelInfo& info, const Shapes& shapes,
                                 long B);

// ---- wide rows: one WAVE per sample ----------------------------------------------------------------
// Rows of 65 .. 4096 floats (a classification head with 100 or 1000 classes) do not fit one thread's registers.  The same
// chain — softmax.sums, softmax, the loss gradient, softmax's three gradient kernels, the bias gradient — runs as one
// generated kernel in which a wave owns a sample: lane l holds the columns x = l + 64 j, j = 0 .. ceil(W / 64) - 1, so
// that every load of a wave is 256 contiguous bytes, and a [B, W] intermediate is ceil(W / 64) registers per lane.
// A kernel is a wide row kernel for batch B and width W when
//   * it has one loop y over 0 .. B that indexes dimension 0, bare, of every [B, W] and [B] tensor it touches, and y is
//     not used as a value;
//   * it has at most one other loop x over 0 .. W, which indexes dimension 1, bare, of [B, W] tensors and dimension 0 of
//     [W] tensors (a bias, a bias gradient), and is not used as a value;
//   * or it is a raw `{it}` map over B * W elements of [B, W] tensors (it = y * W + x);
//   * every other tensor it touches has one element.
// The write decides the kind: [B, W] is a row-local map, [B] a reduction over the row, [W] a reduction over the batch per
// column, one element a reduction over both.  The gradLoss seed is a member like in the thread-per-sample groups.
// Two inner iterators (a contraction inside a row) do not qualify.  float32 programs only, as every fusion group.
struct WideKernelInfo {
  bool ok = false;
  int row_loop = -1;  // index into k.loops of y (or of the raw iterator)
  int col_loop = -1;  // index into k.loops of x (-1: none)
  bool raw = false;
  bool seed = false;
  enum Kind { Map, RowRed, ColRed, AllRed } kind = Map;
  std::vector<int> row_loops;  // collapsed rows (below): indices into k.loops of the row registers, in operand position order
};
constexpr long WIDE_MIN_W = 65, WIDE_MAX_W = 4096;
// floats of group state one lane may hold: ceil(W / 64) per [B, W] tensor written in the group and per [W] batch sum
// (a [B] value or the seed is one value per wave and not counted); the generated kernels must not spill
constexpr long WIDE_STATE_MAX = 128;
// the width a wide group starting with `k` would have: dimension 1 of the first [B, W] tensor it touches (0: none)
//
// Collapsed leading axes.  A dense row-major tensor [d0 .. d(r-2), W] of rank r in {3, 4} is R = d0 * .. * d(r-2) rows of W
// floats, and [d0 .. d(r-2)] is one value per row: the softmax over the last axis of multi-head scores [B, H, I, J] is the
// same chain over [B * H * I, J].  With `lead` given, wide_width_of also looks, where the kernel touches no [B, W] tensor,
// for the first operand of the highest rank among 3 and 4 and reports its leading extents in *lead (R is their product;
// rank 2: {B}, everything as without `lead`).  analyse_wide_kernel with those `lead` (two or three extents) and B = R:
//   * up to r - 1 row loops and at most one column loop x over 0 .. W, none with explicit bounds, none used as a value, no
//     computed indices;
//   * every operand is a row tensor [lead.., W] indexed by the row registers, bare and in this order, then x; a per-row
//     tensor [lead..] indexed by the same registers in the same order; a [W] tensor indexed by x; a single element; or the
//     raw `{it}` form over R * W elements of row tensors;
//   * which register is which is read from its POSITION in the row and per-row operands, never from its extent (I == J in
//     self-attention; a leading extent may equal W): a register at two positions, or at different positions in two
//     operands of one kernel, disqualifies the kernel.
// The kinds are those above with "row" for "sample".  The planner forms such a group only around a reduction over the row
// (plan_groups.cpp): softmax and normalisation chains; runs of maps over a rank-4 tensor keep their routes.
long wide_width_of(const Kernel& k, const Shapes& shapes, long B, std::vector<long>* lead = nullptr);
WideKernelInfo analyse_wide_kernel(const Program& prog, const Kernel& k, const KernelInfo& info, const Shapes& shapes, long B, long W,
                                   const std::vector<long>* lead = nullptr);

struct RowGroupTensor {
  int tensor = 0;
  enum Role { RowLocal, RowExternal, SmallExternal, SmallLocal, Reduction } role = RowExternal;
  long inner = 0;          // elements per row (row tensors) or total elements (small tensors)
  bool load_first = false;  // RowLocal: written before the group too, start from memory
  bool store = false;       // RowLocal: needed after the group
  bool accumulate = false;  // Reduction: add to the destination instead of overwriting it
  long red_offset = 0;      // Reduction: column offset inside the partial rows
};

struct RowGroup {
  std::vector<int> kernel_index;  // indices into target.all, in execution order
  std::vector<RowKernelInfo> infos;
  std::map<int, RowGroupTensor> tensors;
  long B = 0;
  long red_total = 0;  // partial row length
  // floats between two blocks' partial rows: whole 16-byte groups (the hand-off stores and loads them as such)
  long red_stride() const { return (red_total + 3) & ~3L; }
  std::string name, source;
  std::vector<int> ptr_args;  // tensor ids in pointer-argument order (after `partial`)
  // B <= 256: the one block adds its totals to their destinations itself (arguments d<id> behind `epoch`, one per
  // reduction in segment order) — no second launch; EG_NO_ROW_DIRECT=1: partial row + row_finalize as for many blocks
  bool single_block = false;
  // More than one block (round 5): the LAST block to arrive (a ticket counter) folds the partial rows itself, in the order
  // of row_finalize_kernel, instead of a second launch doing it; and it can go on with a run of small kernels that
  // directly follows the group — the optimizer updates of a small net (the whole XOR step becomes ONE launch).
  // Arguments behind `epoch`: d<id> per reduction, unsigned* counter, long MODE (0: partial rows only, the caller
  // launches row_finalize; 1: fold in the kernel; 2: fold, then the tail), u<id> per tail tensor.
  bool in_kernel_finalize = false;
  // Round 6: the grid the launch will use when it is known at generation time (fuse_row_tails: a row group with a tail runs on
  // few, long blocks).  With B a multiple of grid_blocks * 256 the strided sample loop is emitted with a literal trip count and
  // fully unrolled: the loads of all of a thread's samples are in flight together instead of one memory round trip per sample
  // (four in a row at the XOR step).  The generic loop stays in the kernel for any other grid / B.
  long grid_blocks = 0;
  // What generate_row_group emitted, for eg_model_launch_text: the literal trip count of the unrolled sample loop (0: the
  // generic strided loop, or one sample per thread).
  long unrolled_trips = 0;
  std::vector<int> tail_kernels;   // indices into target.all, in execution order
  std::vector<int> tail_ptr_args;  // tensor ids of the tail kernels, in pointer-argument order
  // Wide groups ("one wave per sample", below): W > 0, and `wide` holds the members' analysis instead of `infos`.
  long W = 0;
  std::vector<WideKernelInfo> wide;
  // A wide group over collapsed leading axes: their extents (B is their product); empty for a group over [B, W].
  std::vector<long> rows;
};

// Emit the fused kernel.  Arguments of the generated kernel:
//   (float* partial, float* / const float* t<ids>..., long B, float grad_scale, long epoch[, float* d<ids>...: single_block
//    or in_kernel_finalize][, unsigned* counter, long MODE, float* u<ids>...: in_kernel_finalize])
int generate_row_group(const std::vector<Kernel>& all, const std::vector<KernelInfo>& infos, const Shapes& shapes, RowGroup& group);

// Emit a wide group's kernel (group.W > 0, group.wide filled in; tensor roles as above with inner = W for [B, W] and [W]
// tensors and inner = 1 for [B] tensors and single elements).  256 threads, four waves, each wave walks samples with a grid
// stride.  Lanes beyond a row's end (the last j when W is no multiple of 64) run the same instructions on column `lane`
// of their own row — a load that is always in bounds, so the body has no branch and a sample's loads are issued together
// (guarded bodies cost a memory round trip per member: 176 against 65 us at 65 536 x 100) — and their values are neither
// summed nor stored.  Row reductions: every lane adds its terms in ascending j, then the eg_xor_lane butterfly leaves the total in
// all lanes (a fixed order: two runs give the same bits).  Batch reductions: per-lane accumulators over the wave's
// samples, the block's four waves folded through LDS into one partial row, row_finalize_kernel behind the launch.
// Arguments of the generated kernel: (float* partial, float* / const float* t<ids>..., long B, float grad_scale, long epoch).
int generate_wide_group(const std::vector<Kernel>& all, const Shapes& shapes, RowGroup& group);

// ---- small-kernel fusion -------------------------------------------------------------------------
// Consecutive kernels that touch only small tensors (the optimizer updates: gradientDescent's
// `param{it} ++= -grad{it} * rate` per parameter, adam's m / v / param chain, base.nim:37-53) run as
// ONE single-block kernel: each kernel's independent iterations are strided over the 256 threads,
// `__syncthreads()` separates the kernels.  Four launches of ~5 us each become one.
bool is_small_kernel(const Program& prog, const Kernel& k, const KernelInfo& info, const Shapes& shapes);

struct SmallGroup {
  std::vector<int> kernel_index;  // indices into target.all, in execution order
  std::string name, source;
  std::vector<int> ptr_args;      // tensor ids in pointer-argument order
  long blocks = 1;                // grid size (1 for a small group, sum over the segments of a map group)
  // Map groups only (round 5): gradient tensors whose sum over the batch the group takes from a sample group's slab
  // itself — thread idx adds rows 0 .. fold_rows - 1 of its element in that order, stores the total where the gradient
  // lives (other readers find it there) and goes on with its kernels: the slab_sum launch between the sample kernel and
  // the optimizer disappears.  Arguments behind `epoch`: const float* slab, long FOLD (0: the gradients are in place).
  std::map<int, long> fold_offset;  // tensor -> float offset inside a slab row
  long fold_rows = 0, fold_row_floats = 0;
};

// Arguments of the generated kernel: (float* / const float* t<ids>..., float grad_scale, long epoch).
// Every kernel accumulates into its destination (the caller zeroes first-written results).
int generate_small_group(const std::vector<Kernel>& all, const std::vector<KernelInfo>& infos, const Shapes& shapes, SmallGroup& group);

// ---- map groups ------------------------------------------------------------------------------------
// Consecutive raw elementwise kernels over whole tensors of ANY size (`p{it} ++= -g{it} * rate` for
// every parameter: gradientDescent, base.nim:37-38; adam's m / v / p chains) run as one launch: the
// kernels are grouped into segments by element count, a block belongs to one segment (block ranges
// are literals in the generated source) and a thread runs, for its element, every kernel of the
// segment in order.  Kernels of different segments cannot share a tensor (each covers its tensors
// completely), so segments are independent.  Same kernel arguments as a small group.
bool is_map_kernel(const Program& prog, const Kernel& k, const KernelInfo& info, const Shapes& shapes, long& count);
int generate_map_group(const Program& prog, const std::vector<Kernel>& all, const std::vector<KernelInfo>& infos,
                       const Shapes& shapes, SmallGroup& group);

// ---- sample groups (round 5) -----------------------------------------------------------------------------
// A whole training step at a SMALL batch is a chain of dependent launches, each at the ~4.5 us floor of a dependent
// kernel whatever it computes (Model.fit at the reference's default batch of 32, model.nim:413-454 with the network of
// examples/fashion_mnist/fashion_mnist.nim:39-57: 16 launches, 70 us).  But every kernel of the forward and backward
// pass works sample by sample — only the parameter gradients add over the batch.  A sample group runs a run of such
// kernels as ONE generated kernel with ONE BLOCK PER SAMPLE: the block walks the kernel list in order, its 256 threads
// share the independent iterations of a kernel restricted to the block's sample (reductions serial per thread,
// `__syncthreads()` between kernels; the tensors stay where they are, in L2-resident global memory), and a kernel that
// reduces over the batch writes its sample's contribution into row `sample` of a slab, which one deterministic
// slab_sum launch folds into the gradient bucket afterwards.  The reference fuses loops for its CPU target only
// (fuseLoops, passes.nim:1929-2004); its GPU target launches every kernel (llvmgen.nim:455-500).
struct SampleKernelInfo {
  bool ok = false;
  int batch_loop = -1;   // index into k.loops of the loop that walks the samples (-1: the seed, no such loop)
  bool raw = false;      // that loop is a raw iterator over B * inner elements (it = sample * inner + j)
  long inner = 0;
  bool reduced = false;  // the write is not indexed by the batch loop: a sum over the samples (parameter gradients)
  bool seed = false;     // gradLoss{i} = 1 (passes.nim:575-606): every block writes the same value
  long work = 0;         // loop iterations per sample
  // conv2's image gradient — a scatter in the derived loop nest (gimg[n, y + dy, x + dx, c] += ...) — as a gather over
  // the image gradient's own elements (tensor ids; filled in by the planner from match_conv)
  bool gather = false;
  int g_img = 0, g_out = 0, g_flt = 0;
  // Round 6: a batched conv2 member (forward, filter gradient or image gradient; planner: match_conv) on the matrix cores —
  // 16 x 16 x 4 instructions whose fragments are gathered from the block's LDS-resident tensors (generate_sample_group,
  // "matrix-core convolution members").  0 = the generic loop nest (or `gather`), 1 = forward, 2 = filter gradient,
  // 3 = image gradient; tensor ids of image, output (or its gradient) and filter bank.
  int conv_role = 0;
  int conv_img = 0, conv_out = 0, conv_flt = 0;
};

SampleKernelInfo analyse_sample_kernel(const Program& prog, const Kernel& k, const KernelInfo& info, const Shapes& shapes, long B);

// What generate_sample_group decided for one member, recorded while the member is emitted (eg_model_launch_text prints it;
// nothing reads it back into the generated text).
struct SampleMemberRoute {
  enum Kind { Seed, Raw, Items, Scatter, Split, Gather, Conv } kind = Items;
  int conv_role = 0;        // Conv: SampleKernelInfo::conv_role
  long T = 1, ragged = 0;   // Split: lanes per item; what the outermost reduction extent leaves over T (the guarded last trip)
  long R = 1;               // register blocking (1: none)
  long trips = -1;          // item loop: whole trips of the block over the items (-1: the member has no item loop)
  bool ragged_trip = false; // item loop: a last trip that not every thread takes
  bool rolled = false;      // the item loop (or a split's walk over its outer reduction iterator) has no literal trip count
  int slab = 0;             // 1: first contribution of the block to a batch sum (a store), 2: a later one (an addition)
  bool lds = false;         // the result lives in the block's LDS
};

struct SampleGroup {
  std::vector<int> kernel_index;  // indices into target.all, in execution order
  std::vector<SampleKernelInfo> infos;
  std::vector<char> overwrite;    // per member: the write is a plain store (first writer, whole tensor) instead of +=
  long B = 0;
  std::map<int, long> slab_offset;  // tensors summed over the batch -> float offset inside a slab row
  long slab_floats = 0;             // length of a slab row (a multiple of 4)
  std::string name, source;
  std::vector<int> ptr_args;        // tensor ids in pointer-argument order (behind `slab`)
  // Tensors that exist inside the group only (written and read by members, sample by sample): a block keeps its sample's
  // slice in LDS instead of global memory — an L2 round trip (~0.5 - 1 us) at the head of every one of the ~25 kernels of
  // a step is what the first version of this kernel spent most of its 85 us on.  tensor id -> floats per sample.
  std::map<int, long> lds;
  std::set<int> lds_zero;           // of those: accumulated into before being written whole (start from zero)
  int threads = 256;                // block size (a multiple of 64)
  bool narrow_index = true;         // the plan's: 32-bit index arithmetic is allowed (EG_NO_NARROW_INDEX off when the plan was made)
  // Round 6: small PARAMETER tensors the members read (filter banks, a dense layer's weights) are copied into LDS once, at the
  // kernel's start: a member that walked them with dependent loads paid an L2 round trip per iteration (the 400-term dense
  // layer of the fashion_mnist network: eight of them in a row).  tensor id -> floats.
  std::map<int, long> staged;
  // Filled in by generate_sample_group: one record per member, 32-bit index arithmetic, barriers behind members that stayed.
  std::vector<SampleMemberRoute> routes;
  bool narrow = false;
  int barriers_kept = 0;
};

// Arguments of the generated kernel: (float* slab, float* t<ids>..., float grad_scale, long epoch); grid = B blocks of `threads`.
int generate_sample_group(const std::vector<Kernel>& all, const std::vector<KernelInfo>& infos, const Shapes& shapes, SampleGroup& group);

}  // namespace kd
}  // namespace eg
