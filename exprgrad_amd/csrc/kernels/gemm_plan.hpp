// Host-side planning of the f32 contraction (gemm_f32_mfma.hip): which kernel runs a product, on which tile, with how
// many k-slices, which second pass and how much workspace.  Plain C++ (no HIP): the launch code turns a GemmPlan into
// kernel launches, and tests/test_gemm_plan_cpu.py checks plans without a GPU.
#pragma once

#include "item_grid.hpp"

namespace eg {
namespace gemm {

constexpr int BK = 16;   // k-tile depth of the four-wave kernel unless a route says otherwise

// One contraction C[M, N] (+)= op(A) * op(B) (+ bias) as the planner sees it: extents, layouts and alignment facts.
struct GemmProblem {
  long M = 0, N = 0, K = 0;
  bool a_kc = true, b_kc = false;   // operand k-contiguous (A row-major untransposed, B transposed)
  long lda = 0, ldb = 0, ldc = 0;
  bool a_aligned = true, b_aligned = true, c_aligned = true;   // 16-byte aligned base pointers
  bool has_bias = false, bias_aligned = true;
  bool ones_row = false;   // A has a virtual last row of ones (GemmArgs::ones_row)
  int conv = 0;            // 0: plain; 1: forward implicit-GEMM gather of A; 2: filter gradient (B gathered)
  bool vec_ok = false, a_vec_only = false;   // both operands / only A qualify for 16-byte loads (operand_vec)
  bool piece = false;      // a piece of a remainder split: planned without the small and skinny kernels
  int cus = 256;
};

// The switches the planner reads, filled by the caller (the planner reads no environment variable).
struct GemmSwitches {
  bool no_small = false, no_skinny = false;                     // EG_NO_SMALL_GEMM, EG_NO_SKINNY_GEMM
  bool no_pair = false, no_t96 = false, no_streamk = false;     // EG_GEMM_NO_PAIR / _NO_T96 / _NO_STREAMK
  bool no_xrow = false, no_bk32 = false, no_wide_store = false; // EG_GEMM_NO_XROW / _NO_BK32 / _NO_WIDE_STORE
  bool no_skew = false, old_tile_model = false, small_bk32 = false;   // EG_GEMM_NO_SKEW / _OLD_TILE_MODEL / _SMALL_BK32
  bool debug_tile = false, trace = false;                       // EG_DEBUG_TILE, EG_GEMM_TRACE
  bool force_tile = false, force_splits = false, streamk_blocks = false;   // EG_GEMM_FORCE_TILE / _FORCE_SPLITS,
  int force_bm = 0, force_bn = 0, force_splits_n = 0;                     // EG_STREAMK_BLOCKS_PER_CU are set, to
  long streamk_blocks_per_cu = 0;                                         // "bm,bn" / n / n
  double streamk_min_ratio = 24.0;                              // EG_STREAMK_MIN_RATIO
};

// Routes in the order they are tried (plan_gemm explains each).  Remainder: the pieces in GemmPlan::parts, each
// planned and run on its own.
enum class Route { Small, Skinny, Kw8, T96, StreamK, Remainder, ExtraRows, Bk32, Pair, Generic };
enum class Second { None, SplitReduce, TailReduce, StreamKFixup, Tree };   // Tree: slab sum, or the tree column sum

// Waves of the four-wave kernel's tiles: each wave owns a WM x WN block; MINB blocks per CU.
struct TileWaves {
  int wm, wn, minb;
};
constexpr TileWaves tile_waves(int bm, int bn) {
  return bn == 32                ? TileWaves{32, 32, 4}
         : bn == 64 && bm == 256 ? TileWaves{64, 32, 2}
         : bn == 64 && bm == 64  ? TileWaves{32, 32, 4}
         : bn == 64              ? TileWaves{64, 32, 4}
         : bn == 128             ? TileWaves{64, 64, 4}
                                 : TileWaves{128, 64, 1};
}

struct GemmPlan {
  Route route = Route::Generic;
  int bm = 0, bn = 0, kb = BK;
  TileWaves waves = {};
  int vec = 4;           // Generic: 4 (16-byte loads), 41 (A 16-byte, B scalar; 128 x 32 only), 1 (scalar)
  bool edge = false;     // the clamped form for ragged tiles (Kw8 / Pair: also for a K that ends inside a k-tile)
  // GemmArgs fields
  int tiles_m = 0, tiles_n = 0, splits = 1;
  long k_per_split = 0;
  int edge_splits = 0;
  long k_per_split_edge = 0;
  int tail_tiles = 0, tail_splits = 0;
  long tail_k_per_split = 0;
  int x_rows = 0;
  bool wide_store = false, no_skew = false;
  bool nt_store = true;  // wide stores of whole tiles are nontemporal: no launch reads its output again (4096^3: 137.1 -> 139.0 TFLOP/s)
  bool prio = true;      // raise the issue priority when launched on the side lane
  long grid = 0;   // main launch: grid x block threads
  int block = 0;
  // second pass (SplitReduce / Tree fold `splits` slabs; the last tile row's edge_splits slabs)
  Second second = Second::None;
  long workspace_floats = 0; // slabs; a Tree pass adds the column sum's scratch behind them
  int nparts = 0;            // Remainder: the pieces
  struct { long row0, col0, M, N; } parts[3] = {};
};

// 16-byte global loads of an operand need every row start and every chunk 16-byte aligned and whole (contig: the
// extent along its contiguous axis).  The LDS-DMA loaders address a tile with 32-bit byte offsets from its origin:
// 256 rows x ld x 4 bytes < 2^31.
inline bool operand_vec(long ld, long contig, bool aligned) { return ld % 4 == 0 && contig % 4 == 0 && aligned && ld < (1L << 21); }

// The one-wave-per-output kernel's range (without EG_NO_SMALL_GEMM).
bool small_suits(long M, long N, long K);

// Tile shape and split count for an M x N x K contraction on `cus` compute units.
void choose_tile(long M, long N, long K, int cus, const GemmSwitches& sw, int& bm, int& bn, int& splits, bool vec = true,
                 bool plain = true);

// The generic tile of a product: choose_tile (its time model told whether the operands are 16-byte: model_vec), the
// tile's waves and the load variant of 16-deep k-tiles.  plan_gemm starts from it; fused launches run it as it is.
GemmPlan generic_tile(const GemmProblem& p, const GemmSwitches& sw, bool model_vec);

// Whole tiles leave through LDS as 16-byte stores (GemmArgs::wide_store).
bool wide_store_ok(const GemmProblem& p, const GemmSwitches& sw, bool to_partial, bool fused = false);

GemmPlan plan_gemm(const GemmProblem& p, const GemmSwitches& sw);

// `batch` products of one shape in ONE launch (gemm_batched.hip): item.M / N / K, the layouts, the leading dimensions and the
// alignment facts describe one item (the caller folds the items' strides into the alignment facts).  The plan is always
// Route::Generic on 64 x 64 tiles, unsliced (splits = 1, no second pass, no workspace: every output element is one in-order
// sum over k), with grid = batch x tiles_m x tiles_n.  (gemm_plan.cpp has what was measured.)
GemmPlan plan_gemm_batched(const GemmProblem& item, long batch, const GemmSwitches& sw);

// Does one item fill the chip by itself?  Its own plan has at least one block per CU: such a batch runs as a loop of plain
// products on their own routes.  Decided from the item alone, so that an item has the same bits whatever batch it is part of.
bool batched_runs_as_loop(const GemmProblem& item, const GemmSwitches& sw);

// The one rule for the C of a product with two batch indices (eg_sgemm_batched2): no two of its elements
// C + o * stride_c0 + i * stride_c1 + m * ldc + n (o < batch0, i < batch1, m < M, n < N) share an address.  The axes
// (batch0, stride_c0), (batch1, stride_c1), (M, ldc), (N, 1) without those of extent 1, ordered by stride, largest first:
// every stride must be at least 1 + the sum of (extent - 1) * stride over the axes after it, i.e. one past the span of everything
// that varies faster.  Sufficient, not necessary; it holds for nested layouts in any nesting order (o[b,i,h,d]: ldc = H * D,
// stride_c1 = D) and fails for every tie, every stride below 1 and every extent below 1.
bool batched2_c_distinct(long batch0, long stride_c0, long batch1, long stride_c1, long M, long ldc, long N);

// ---- float64: the plain product (gemm_f64_mfma.hip, dgemm_kernel) -------------------------------------------------------
// One eg_dgemm call as the planner sees it.  Leading dimensions in doubles.
struct DgemmProblem {
  long M = 0, N = 0, K = 0;
  long lda = 0, ldb = 0;
  bool a_aligned = true, b_aligned = true;   // 16-byte aligned base pointers
  int cus = 256;
  int force_config = -1;   // EG_DGEMM_TILE (measurement aid), set by the caller: the config (-1: the model's) and the
  long force_splits = 0;   // slice count before normalisation (0: the model's)
};

// Tile, k-slices and launch geometry of one product: what DgemmArgs and the launch are filled from.
struct DgemmPlan {
  int config = 0;            // 0: 128 x 128, 1: 128 x 64, 2: 64 x 64 (gemm_plan.cpp has the table)
  int bm = 0, bn = 0;
  int wr = 0, wc = 0;        // the tile's wave grid: wr x wc waves of (bm / wr) x (bn / wc)
  bool vec = false;          // 16-byte loads (dgemm_vec)
  int splits = 1;            // k-slices after normalisation: none of them is empty
  long k_per_split = 0;      // a multiple of 16, at least 16
  int tiles_m = 0, tiles_n = 0;
  bool remap = false;        // dgemm_remap of the tiles
  long grid_x = 0, grid_y = 0;   // tiles x splits blocks of wr * wc * 64 threads
  long workspace_doubles = 0;    // slabs: 0 unsliced, splits * M * N sliced
  bool reduce = false;           // the slabs are folded in slice order by a second launch
};

// 16-byte loads: a piece is two doubles that are neighbours in memory, so every row start (lda, ldb even) and both bases
// must be 16-byte aligned.  Anything else: 8-byte loads.
inline bool dgemm_vec(long lda, long ldb, bool a_aligned, bool b_aligned) { return lda % 2 == 0 && ldb % 2 == 0 && a_aligned && b_aligned; }

// The kernels hand every XCD a contiguous range of a launch's `blocks` tiles (id -> (id & 7) * (blocks >> 3) + (id >> 3)): a
// permutation only for a multiple of 8, and worth it from two tiles per XCD on.
inline bool dgemm_remap(long blocks) { return blocks % 8 == 0 && blocks >= 16; }

// k range of a block of an unsliced product: the whole K in 16-deep k-tiles, at least one (K = 0 still stores C).
inline long dgemm_k_unsliced(long K) {
  const long per = ((K + BK - 1) / BK) * BK;
  return per == 0 ? BK : per;
}

DgemmPlan plan_dgemm(const DgemmProblem& p);

// ---- float64: batch x batch1 products of one shape (gemm_f64_mfma.hip, dgemm_batched_kernel) --------------------------
using eg::BATCHED_MAX_BLOCKS;   // blocks of one batched launch, float32 and float64 (item_grid.hpp)
constexpr int DGEMM_BATCHED_TILE = 64;   // the one tile the batched float64 kernel is built for

// One call as the planner sees it: eg_dgemm_batched (batch items) or eg_dgemm_batched2 (batch x batch1 items, `batch` the
// outer index).  Leading dimensions and strides in doubles; a stride of 0 shares the operand.
struct DgemmBatchedProblem {
  long batch = 0, M = 0, N = 0, K = 0;
  long lda = 0, ldb = 0, stride_a = 0, stride_b = 0;   // the strides of the outer (or only) batch index
  bool a_aligned = true, b_aligned = true;   // 16-byte aligned base pointers of item (0, 0)
  int cus = 256;
  int force = 0;   // EG_DGEMM_BATCHED_ROUTE (measurement aid), set by the caller: 1 one launch, 2 the loop
  long batch1 = 1, stride_a1 = 0, stride_b1 = 0;   // the inner batch index and its strides (one batch index: extent 1)
};

struct DgemmBatchedPlan {
  bool loop = false;   // every item is a plain float64 product on its own route; the fields behind `item` are then unused
  // loop: plan_dgemm of item 0 without EG_DGEMM_TILE.  The loop plans every item again with its own base alignment, which
  // changes `vec` alone: item.workspace_doubles — nonzero for a sliced item — is what every item of the loop takes.
  DgemmPlan item;
  bool vec = false;    // 16-byte loads (dgemm_batched_vec)
  int tiles_m = 0, tiles_n = 0;
  long tiles = 0;             // blocks per item            } cut_items(batch * batch1, tiles) of the item grid
  long items_per_launch = 0;  // BATCHED_MAX_BLOCKS / tiles  } (item_grid.hpp): the launches cut the flattened
  long launches = 0;          //                             } (outer, inner) range, outer-major
};

// Launch `index` of a plan over `batch` items in all (batch x batch1 of the problem): items [first, first + items) of the
// flattened range, grid = items x tiles blocks — plan_launch of the item grid.  The one-index entry launches from this
// (dgemm_batched1_kernel, which takes `remap`: dgemm_remap of the grid); the two-index entry goes through for_each_launch
// over the same cut, and its kernel's xcd_remap is a permutation of every grid, so it asks for no such flag.
struct DgemmBatchedLaunch {
  long first = 0, items = 0, grid = 0;
  bool remap = false;
};

// 16-byte loads: dgemm_vec of item (0, 0), and every further item 16-byte aligned as well: for A and for B, the stride of
// each batch index is even wherever that index has a second value (an index of extent 1 never applies its stride; a shared
// operand's stride of 0 is even).  Anything else: 8-byte loads.
bool dgemm_batched_vec(const DgemmBatchedProblem& p);

// Does one item fill the chip by itself?  Then the batch runs as a loop of plain float64 products, each on its own route
// (tile, k-slices).  Decided from the item alone — never from the batch —, so that an item has the same route, and the same
// bits, whatever batch it is part of.  (gemm_plan.cpp has the rule and what was measured.)
bool dgemm_batched_runs_as_loop(long M, long N, long K, int cus);

DgemmBatchedPlan plan_dgemm_batched(const DgemmBatchedProblem& p);
DgemmBatchedLaunch dgemm_batched_launch(const DgemmBatchedPlan& plan, long batch, long index);

// ---- float64: convolutions of any width (conv2_f64_mfma.hip) --------------------------------------------------------
// One convolution launch as the planner sees it.  The three roles are contractions over a gathered window operand:
//   Forward         out [P, F]       = window(img) [P, FH*FW*C] * flt [F, FH*FW*C]^T          P = N*Ho*Wo pixels
//   GradImage       gimg [N*H*W, C]  = window(gout, zero border) [N*H*W, FH*FW*F] * flipped [C, FH*FW*F]^T
//   GradFilter      gflt [F, FH*FW*C] = gout [P, F]^T * window(img) [P, FH*FW*C]               summed over the P pixels
enum class Conv64Role { Forward = 1, GradImage = 2, GradFilter = 3 };

struct Conv64Problem {
  Conv64Role role = Conv64Role::Forward;
  long N = 0, H = 0, W = 0, C = 0, F = 0, FH = 1, FW = 1;
  // 16-byte aligned base pointers: img (Forward, GradFilter), flt (Forward; GradImage reads the flipped copy in the
  // context's aligned scratch), gout (GradImage, GradFilter)
  bool img_aligned = true, flt_aligned = true, gout_aligned = true;
  int cus = 256;
};

// The kernels index pixels and taps with 32-bit integers (addresses are 64-bit): the host refuses a call whose contraction
// has 2^31 or more rows, columns or terms.
constexpr long CONV64_MAX_INDEX = 1L << 31;

struct Conv64Plan {
  bool ok = false;           // false: an extent of the contraction reaches CONV64_MAX_INDEX (nothing else is filled in)
  long M = 0, Ncols = 0, K = 0;   // the contraction: M x Ncols outputs, K terms each
  int config = 2;            // 0: 128 x 128, 2: 64 x 64 (plan_dgemm's table; both eight waves as 2 x 4)
  int bm = 0, bn = 0, wr = 0, wc = 0;
  bool vec_a = false, vec_b = false;   // 16-byte loads of the A / B operand (A: window or gout; B: bank or window)
  int tiles_m = 0, tiles_n = 0;
  bool remap = false;        // dgemm_remap of the tiles
  long grid_x = 0, grid_y = 1;
  // GradFilter: the pixels are cut into `slices` ranges of pixels_per_slice (a multiple of 16; the last may be shorter, none
  // is empty); each writes a slab of F*FH*FW*C doubles and a second launch folds the slabs in ascending order.
  int slices = 1;
  long pixels_per_slice = 0;
  long workspace_doubles = 0;
  bool reduce = false;
  long aux_doubles = 0;      // GradImage: the flipped bank [C][FH][FW][F]
};

Conv64Plan plan_conv64(const Conv64Problem& p);

// Is the plan ONE launch of the whole-tile 256 x 256 kernel (no k-slices, tail slices or second pass)?  Only such a launch
// can stand behind the split-bf16 product as its fallback: GemmArgs::run_if gates the tile kernel, not the reduce kernels.
bool exact_single_launch(const GemmPlan& p);

}  // namespace gemm
}  // namespace eg
