// Host-side planning of the fused attention forward (attention_f32.hip): whether the kernel takes a problem, on which
// tile, with which load width per operand, on how many blocks in how many launches, and with how much LDS.  Plain C++
// (no HIP, no other unit): the launcher does nothing but obey an AttentionPlan, and tests/test_attention_plan_cpu.py
// checks plans without a GPU.
#pragma once

#include "gemm_plan.hpp"   // BATCHED_MAX_BLOCKS
#include "item_grid.hpp"   // View, Cut, Launch

namespace eg {
namespace attention {

constexpr int TILE_I = 64;     // query rows of a block: four waves of 16 rows
constexpr int TILE_J = 64;     // keys of one pass of the block's loop
constexpr int MAX_HEAD = 128;  // K and D
constexpr int THREADS = 256;
constexpr long LDS_LIMIT = 160 * 1024;   // per CU on gfx950

// An operand's view and the cut of the item range into launches are the item grid's (item_grid.hpp).
using eg::View;
using eg::Cut;
using eg::cut_items;
using eg::Launch;
using eg::plan_launch;

// batch0 x batch1 items of I query rows and J keys, K the length of a query or key row, D of a value row
struct Extents {
  long batch0 = 0, batch1 = 0, I = 0, J = 0, K = 0, D = 0;
};

// The planner's operand: a view, and whether item (0, 0) starts 16-byte aligned.
struct Operand : View {
  bool aligned = true;
};

struct Problem : Extents {
  Operand q, k, v, o;
  bool sums = false;   // eg_attention_sums: the row sums are stored too, and D == 0 still has them to store
  bool has_bias = false;   // eg_attention_bias: the additive score bias, I x J per item; its ld and strides may each be 0
  Operand bias;
  int cus = 256;
};

struct Plan {
  bool supported = false;
  const char* reason = "";   // why not, naming the limit
  int tile_i = TILE_I, tile_j = TILE_J;
  int kp = 0, dp = 0;        // K and D as the kernel is instantiated: 32, 64 or 128, the rest zero-filled
  bool vec_q = false, vec_k = false, vec_v = false;   // 16-byte loads of that operand
  bool vec_b = false;        // the bias's rows start 16-byte aligned (operand_vec16; an ld of 0 is a multiple of 4)
  long tiles_i = 0;          // blocks per item: ceil(I / 64)
  long items = 0;            // batch0 * batch1
  long grid = 0, items_per_launch = 0, launches = 0;   // with tiles_i, the plan's Cut
  int block = THREADS;
  long lds_bytes = 0;
  Cut cut() const { return {tiles_i, grid, items_per_launch, launches}; }
};

// 16-byte loads of an operand: the pointer of item (0, 0) 16-byte aligned, the leading dimension and both strides multiples
// of 4 — then every row of every item starts 16-byte aligned (the rule of eg_sgemm_batched2).  A row's last chunk that holds
// fewer than four elements is read element by element in either mode.
inline bool operand_vec16(const Operand& x) { return x.aligned && x.ld % 4 == 0 && x.stride0 % 4 == 0 && x.stride1 % 4 == 0; }

// Padded head dimension: the smallest instantiation that holds n.
inline int padded_head(long n) { return n <= 32 ? 32 : n <= 64 ? 64 : 128; }

// Floats per row of the three LDS tiles: K rows [TILE_J][kp + 4] (a wave's 16 keys x 4 k land on 64 banks), V rows
// [TILE_J][dp + 16] (4 keys x 16 columns), E rows [4 waves][16][TILE_J + 4].
inline long lds_bytes_for(int kp, int dp) { return 4L * (TILE_J * (kp + 4) + TILE_J * (dp + 16) + 4 * 16 * (TILE_J + 4)); }

Plan plan_attention(const Problem& p);
// Launch `index` of a plan, index in [0, plan.launches): the cut's, for a caller that holds the plan.
inline Launch plan_launch(const Plan& plan, long index) { return plan_launch(plan.items, plan.cut(), index); }

// ---- The forward split over the keys (attention_split_f32.hip, eg_attention_stable_split): `splits` blocks per item and row
// tile, each over a contiguous range of key tiles, leave partial results (unnormalised O rows, maximum, sum) in the context's
// workspace; one more launch combines them.  Two modes of the partial kernel: above 16 query rows the block of plan_attention
// (four waves of 16 rows each); up to 16 rows the four waves hold the same 16 rows and each takes 16 keys of every 64-key tile.
constexpr int SPLIT_ROWS16 = 16;   // I up to here: the waves split the keys, not the rows

// The auto rule (splits == 0): split only when items * tiles_i is below the CU count and there are two key tiles or more; then
// splits = min(blocks_per_cu * cus / blocks, nt / SPLIT_MIN_TILES), at least 1.  Its constants, from profiles/attention_split.txt
// section 2 (one MI355X, 256 CUs; microseconds per call, median of three fresh processes, every spread at most 1.7 us and at
// most 0.8 us at the best counts; heads x I x J x K=D; `stable` is eg_attention_stable):
//   shape            stable  splits 1      2      4      8     16     32     64    128    256   auto picks
//   32x1x8192x128     833.9     387.4  200.1  106.8   64.7   72.6   86.7  114.8  173.6            8
//   32x16x8192x128    841.2     398.1  207.0  110.3   66.9   75.7   90.3  126.9  193.4            8
//   8x128x16384x64   1008.2    1008.7  519.4  268.3  141.1   80.3   75.7   94.3  128.0  199.5    32
//   128x512x512x64    110.5     111.0  125.0  136.4  165.5                                        1 (blocks >= CUs)
//   4x16x2048x128     215.5     106.5   58.0   34.1   23.3   20.1   22.5                         16
//   2x128x2048x64     131.5     131.5   71.9   40.8   27.0   22.8   27.1                         16
//  - blocks per CU: the best count makes 256 blocks at K = D = 128 (32 x 8) and 512 at K = D = 64 (16 x 32): as many as run at
//    once.  By the resource table (section 1) the kernels with kp + dp >= 192 have one wave per SIMD by registers, one block
//    per CU, and those below two or more; no count beyond two per CU measured faster, so the rule stops at two.  With one per CU
//    at 8x128x16384x64 the rule picked 16 (80.5 us against 76.2 at 32: outside the spread; section 3 keeps that run).
//  - SPLIT_MIN_TILES: on the two shapes whose blocks stay below the CUs at every count, 16 splits of two tiles beat 32 of one
//    (20.1 / 22.5 and 22.8 / 27.1) and 8 of four (23.3, 27.0).
// At every measured shape auto's count is the best measured one (the difference is within the spread), and where auto does not
// split no count measured faster than one.  Not measured: other head sizes, a bias, more than one launch.
constexpr long SPLIT_MIN_TILES = 2;
constexpr long split_blocks_per_cu(int kp, int dp) { return kp + dp >= 192 ? 1 : 2; }

struct SplitPlan {
  bool supported = false;
  const char* reason = "";
  Plan base;                 // plan_attention's: padded heads, load widths, tiles_i, items
  bool rows16 = false;       // the mode
  bool forward = false;      // nothing to split (J == 0, D == 0, or the 64-row mode with one split): eg_attention_stable, the same bits
  long nt = 0;               // key tiles of 64
  int splits = 0;            // effective: 1 .. max(nt, 1)
  long rows_pad = 0;         // rows of an item in the workspace: 16, or 64 * tiles_i
  // The workspace: O parts [items][splits][rows_pad][dp] floats, then maxima and sums [items][splits][2][rows_pad].
  long stats_offset = 0;     // in floats
  long workspace_bytes = 0;
  Cut partial;               // tiles_i * splits blocks per item
  long combine_rows = 0;     // items * rows_pad
  int combine_rows_per_block = 0;   // 256 threads, one per four columns of a row: 1024 / dp
  long combine_grid = 0;     // one launch; a block walks rows combine_rows_per_block * grid apart
  int block = THREADS;
  long lds_bytes = 0;        // of the partial kernel
};

// Floats per row of a wave's own E rows in the 16-row mode, [16][16 + 4]: attention_split_f32.hip has the bank arithmetic.
constexpr int SPLIT_ES16 = 16 + 4;
// 16-row mode: K tile [64][kp + 4], V tile [64][dp + 16], E rows [4 waves][16][20]; the merge of the four waves lives in the
// K and V tiles.
inline long split16_lds_bytes(int kp, int dp) { return 4L * (TILE_J * (kp + 4) + TILE_J * (dp + 16) + 4 * 16 * SPLIT_ES16); }

// Split s of `splits` over nt key tiles takes tiles [split_first(nt, splits, s), split_first(nt, splits, s + 1)): non-empty for
// splits <= nt, and together [0, nt).  constexpr: the kernels call it too.
constexpr long split_first(long nt, int splits, int s) { return (long)s * nt / splits; }

// splits: 0 the auto rule, n >= 1 that many, clamped to the key tiles (negative: not supported).
SplitPlan plan_attention_split(const Problem& p, int splits);

// ---- The causal kernels (attention_causal_f32.hip, attention_grad_causal_f32.hip; eg_attention_causal and its grad): key j
// is visible to query row i iff j <= i + offset, offset >= 0, so every row sees key 0.  The tiles of 64 rows and 64 keys, the
// padded heads, the load widths, the cut and the LDS are plan_attention's and plan_attention_grad's; these functions say which
// tiles a block visits.  constexpr: the kernels call them too, so a plan and its kernel cannot disagree.

// The keys that some row of an item can see: keys [0, causal_visible_keys).  Nothing at or beyond it is ever loaded.  The
// entries clamp the offset to J (any offset >= J - 1 masks nothing), so I + offset cannot overflow.
constexpr long causal_visible_keys(long I, long offset, long J) { return I <= 0 ? 0 : (J < I + offset ? J : I + offset); }

// Forward and dQ: the block of rows [i0, i0 + 64) walks key tiles [0, causal_key_tiles): the last one holds key
// min(J - 1, i0 + 63 + offset).  With J the item's causal_visible_keys a ragged last row tile stops at its last row's keys.
constexpr long causal_key_tiles(long i0, long offset, long J) {
  const long last = J - 1 < i0 + (TILE_I - 1) + offset ? J - 1 : i0 + (TILE_I - 1) + offset;
  return J <= 0 ? 0 : last / TILE_J + 1;
}

// dK/dV: the block of keys [j0, j0 + 64) starts at the row tile that holds row max(0, j0 - offset), the first that sees key j0.
// A block with j0 at or beyond the item's causal_visible_keys has no such row, and its loop is empty.
constexpr long causal_first_row_tile(long j0, long offset) { return j0 > offset ? (j0 - offset) / TILE_I : 0; }

// Whether the tile of rows [i0, i0 + 64) and keys [j0, j0 + 64), one that is visited, holds a masked pair and needs the select:
// its first row does not see its last key inside the problem.  Otherwise the tile is interior: the unmasked kernel's path.
constexpr bool causal_tile_cut(long i0, long j0, long offset, long J) {
  const long last = J - 1 < j0 + (TILE_J - 1) ? J - 1 : j0 + (TILE_J - 1);
  return last > i0 + offset;
}

// ---- The causal forward cut into chunks of key tiles (attention_causal_split_f32.hip, eg_attention_causal_split): row tile t of
// an item has n_t = causal_key_tiles(64 t, offset, visible) key tiles and is walked by P_t = ceil(n_t / chunk) blocks, piece p of
// them over tiles [split_first(n_t, P_t, p), split_first(n_t, P_t, p + 1)).  A row tile with one piece is finished by its block
// (the bits of eg_attention_causal); the pieces of a cut row tile (P_t >= 2) leave partials in the workspace and a combine launch
// merges them.  Up to 16 query rows the block is the 16-row mode's and every piece goes through the workspace.
//
// TILE_I == TILE_J, so n_t = min(nv, t + c0): nv the tiles of the visible keys, c0 the key tiles of row tile 0 without that
// bound.  n_t does not fall with t: the cut row tiles are [causal_first_cut_tile, tiles), and the pieces before row tile t have
// a closed form.  These functions are the only place where a block's index becomes (row tile, piece) and a partial's slot.
struct CausalPieces {
  long nv = 0;      // key tiles that hold a visible key
  long c0 = 0;      // (63 + offset) / 64 + 1
  long tiles = 0;   // row tiles of an item: ceil(I / 64), or 1 in the 16-row mode
  long chunk = 1;   // key tiles of a piece at the most: 1 .. max(nv, 1)
  bool rows16 = false;   // every piece leaves a partial, also a row tile's only one
};
static_assert(TILE_I == TILE_J, "n_t = min(nv, t + c0)");

// offset already clamped to [0, J]; rows16: I <= 16, one row tile that sees every visible key.
constexpr CausalPieces causal_pieces(long I, long J, long offset, long chunk, bool rows16) {
  const long nv = (causal_visible_keys(I, offset, J) + TILE_J - 1) / TILE_J;
  const long most = nv < 1 ? 1 : nv;
  return {nv, rows16 ? nv : (TILE_I - 1 + offset) / TILE_J + 1, rows16 ? 1 : (I + TILE_I - 1) / TILE_I, chunk < most ? chunk : most, rows16};
}
constexpr long causal_row_key_tiles(const CausalPieces& c, long t) { return c.nv < t + c.c0 ? c.nv : t + c.c0; }
constexpr long causal_piece_count(long n, long chunk) { return (n + chunk - 1) / chunk; }
// The sum of ceil(x / chunk) over x in [0, y).  The operands of both divisions are below 2^31 (the plan refuses nv above
// that), so they are 32-bit divisions on the device.
constexpr long causal_ceil_sum(long y, long chunk) {
  if (y <= 1) return 0;
  const unsigned m = (unsigned)(y - 1), c = (unsigned)chunk;
  const long full = m / c, rem = m % c;
  return chunk * (full * (full + 1) / 2) + rem * (full + 1);
}
// Pieces of row tiles [0, t), t in [0, tiles]: the row tiles below nv - c0 grow by one key tile each, the others have nv.
constexpr long causal_pieces_before(const CausalPieces& c, long t) {
  const long rising = c.nv - c.c0 < 0 ? 0 : (c.nv - c.c0 < t ? c.nv - c.c0 : t);
  return causal_ceil_sum(c.c0 + rising, c.chunk) - causal_ceil_sum(c.c0, c.chunk) + (t - rising) * causal_piece_count(c.nv, c.chunk);
}
// The first row tile whose pieces leave partials, those with two pieces or more: `tiles` when there is none.
constexpr long causal_first_cut_tile(const CausalPieces& c) {
  if (c.rows16) return 0;
  if (c.nv <= c.chunk) return c.tiles;
  const long t = c.chunk + 1 - c.c0 < 0 ? 0 : c.chunk + 1 - c.c0;
  return t < c.tiles ? t : c.tiles;
}
// A block's index x in [0, causal_pieces_before(c, tiles)) within its item -> (row tile, piece).  The order is the reverse of
// (row tile, piece) ascending: the row tiles with the most key tiles are issued first, as in the causal kernels.  A binary
// search over the row tiles on the closed form: ceil(log2(tiles)) steps, no table.
struct CausalPiece {
  long tile = 0;
  int piece = 0, pieces = 1;
  long t0 = 0, t1 = 0;   // its key tiles [t0, t1)
  long slot = 0;         // of a cut row tile: its partial's place among the item's partials
};
constexpr CausalPiece causal_piece_decode(const CausalPieces& c, long x) {
  const long y = causal_pieces_before(c, c.tiles) - 1 - x;
  long lo = 0, hi = c.tiles - 1;   // the last row tile with pieces_before <= y
  while (lo < hi) {
    const long mid = (lo + hi + 1) / 2;
    if (causal_pieces_before(c, mid) <= y)
      lo = mid;
    else
      hi = mid - 1;
  }
  CausalPiece r;
  const long before = causal_pieces_before(c, lo), n = causal_row_key_tiles(c, lo);
  r.tile = lo;
  r.piece = (int)(y - before);
  r.pieces = (int)causal_piece_count(n, c.chunk);
  r.t0 = split_first(n, r.pieces, r.piece), r.t1 = split_first(n, r.pieces, r.piece + 1);
  r.slot = before - causal_pieces_before(c, causal_first_cut_tile(c)) + r.piece;
  return r;
}

struct CausalSplitPlan {
  bool supported = false;
  const char* reason = "";
  Plan base;                 // plan_attention's: padded heads, load widths, tiles_i, items
  bool rows16 = false;       // the mode
  bool forward = false;      // nothing is cut (J == 0, D == 0, or the 64-row mode without a cut row tile): eg_attention_causal, the same bits
  CausalPieces pieces;       // with the effective chunk
  long pieces_per_item = 0;  // blocks of an item in the partial launch
  long first_cut = 0;        // causal_first_cut_tile
  long slots = 0;            // partials of an item: the pieces of its cut row tiles (16-row mode: of its one row tile)
  int rows = TILE_I;         // rows of a partial: 64 or 16
  // The workspace: O parts [items][slots][rows][dp] floats, then maxima and sums [items][slots][2][rows].
  long stats_offset = 0;     // in floats
  long workspace_bytes = 0;
  Cut partial;               // pieces_per_item blocks per item
  long combine_rows_per_item = 0;   // rows * the cut row tiles
  long combine_rows = 0;     // items * combine_rows_per_item
  long combine_grid = 0;     // one launch of blocks of 1024 / dp rows; a block walks rows 1024 / dp * grid apart
  int block = THREADS;
  long lds_bytes = 0;        // of the partial kernel
};

// The auto rule's constants (chunk == 0): the rule and the rows of profiles/attention_causal_split.txt they came from are beside
// plan_attention_causal_split in attention_plan.cpp.
constexpr long CAUSAL_SPLIT_MIN_TILES = 2;      // key tiles of a piece at the least
constexpr long CAUSAL_SPLIT_FULL_PIECES = 16;   // a full launch: pieces per CU's share of the key-tile visits

// chunk: 0 the auto rule, n >= 1 key tiles per piece at the most (negative: not supported).  offset as the entry clamps it.
CausalSplitPlan plan_attention_causal_split(const Problem& p, long offset, int chunk);

// ---- The float64 forward (attention_f64.hip): the same tile of 64 query rows and the same padded head dimensions on
// v_mfma_f64_16x16x4_f64.  Problem and Plan are the ones above; what differs is decided here, not in the kernel: the key tile
// (Plan::tile_j, 64 or 32 keys), the LDS rows in doubles, and 16-byte loads that hold two elements.
constexpr int TILE_J_F64[2] = {64, 32};   // the key tiles the kernel is instantiated on, largest first

// 16-byte loads of a float64 operand: the pointer of item (0, 0) 16-byte aligned, the leading dimension and both strides
// even (the rule of eg_dgemm_batched2).  A row's odd last element is read alone in either mode.
inline bool operand_vec16_f64(const Operand& x) { return x.aligned && x.ld % 2 == 0 && x.stride0 % 2 == 0 && x.stride1 % 2 == 0; }

// Doubles per row of the three LDS tiles.  A double spans two of the 64 banks and a wave's 8-byte accesses go half a wave at
// a time, so 32 lanes must land on 32 different doubles modulo 32.  K rows [tile_j][kp + 2]: a half-wave reads 16 keys x 2 k,
// at 2 c + g.  V rows [tile_j][dp + 16]: 2 keys x 16 columns, at 16 g + c.  E rows [4 waves][16][tile_j + 18]: the A-operand
// read of 16 rows x 2 keys at 18 c + g is conflict-free, the accumulator-layout write of 2 rows x 16 columns at 18 g + c
// meets itself on two doubles of 32 (a row step that is 16 modulo 32 would free the write and fold the read eight times).
constexpr int F64_PAD_K = 2, F64_PAD_V = 16, F64_PAD_E = 18;
constexpr long lds_bytes_for_f64(int kp, int dp, int tile_j) {
  return 8L * (tile_j * (kp + F64_PAD_K) + tile_j * (dp + F64_PAD_V) + 4 * 16 * (tile_j + F64_PAD_E));
}

// The key tile of a pair of padded head dimensions: the largest whose three tiles fit the LDS of a CU (0: none does).  The
// kernel is instantiated on this function's value, so a plan and its kernel cannot disagree.
constexpr int key_tile_f64(int kp, int dp) {
  for (int tj : TILE_J_F64)
    if (lds_bytes_for_f64(kp, dp, tj) <= LDS_LIMIT) return tj;
  return 0;
}

Plan plan_attention_f64(const Problem& p);

// ---- The backward pass (attention_grad_f32.hip): two kernels, one over tiles of 64 query rows (dQ), one over tiles of 64
// keys (dK and dV).  Both keep the block's own rows in registers and walk the other axis in tiles of 64.
struct GradProblem : Extents {
  Operand q, k, v, o, s, dout, dq, dk, dv;   // s: the row sums
  bool has_bias = false;                     // eg_attention_bias_grad: the forward's score bias
  Operand bias;
  bool stable = false;                       // eg_attention_stable_grad: s is the forward's Stats, two rows of I floats s.ld apart
  int cus = 256;
};

// One of the two kernels, cut along the flattened item range like the forward.
struct GradKernel : Cut {
  int tile = 64;             // rows of the block's own axis
  int step = 64;             // rows of one pass of its loop over the other axis
  long lds_bytes = 0;
};

struct GradPlan {
  bool supported = false;
  const char* reason = "";
  int kp = 0, dp = 0;
  // 16-byte accesses per operand: loads of Q, Kk, V, O, Sums and dO, stores (and, accumulating, loads) of dQ, dK and dV
  bool vec_q = false, vec_k = false, vec_v = false, vec_o = false, vec_s = false, vec_do = false, vec_dq = false, vec_dk = false, vec_dv = false;
  bool vec_b = false;   // 16-byte loads of the bias in the dK/dV kernel, where a lane holds four consecutive keys of a row
  long items = 0;
  GradKernel dq, dkv;
  int block = THREADS;
};

// Floats per LDS row of a tile that is read both as an NT operand (16 rows x 4 columns per instruction) and as an NN
// operand (4 rows x 16 columns): see attention_grad_f32.hip.
constexpr int GRAD_PAD_BOTH = 20, GRAD_PAD_NT = 4;

// dQ kernel: K tile [64][kp + 20] (NT for the scores, NN for dS * K), V tile [64][dp + 4] (NT only), the waves' dS rows
// [4][16][68], and 1 / L and delta of the block's 64 rows; `stable`: their maxima too, 256 bytes more.
inline long grad_dq_lds_bytes(int kp, int dp, bool stable = false) {
  return 4L * (64 * (kp + GRAD_PAD_BOTH) + 64 * (dp + GRAD_PAD_NT) + 4 * 16 * 68 + (stable ? 3 : 2) * 64);
}
// dK/dV kernel: Q tile [64][kp + 20] and dO tile [64][dp + 20] (both read both ways), the waves' rows, 1 / L and delta (and the
// maxima).
inline long grad_dkv_lds_bytes(int kp, int dp, bool stable = false) {
  return 4L * (64 * (kp + GRAD_PAD_BOTH) + 64 * (dp + GRAD_PAD_BOTH) + 4 * 16 * 68 + (stable ? 3 : 2) * 64);
}

GradPlan plan_attention_grad(const GradProblem& p);
// Launch `index` of one of a plan's kernels, index in [0, kernel.launches): the cut's again.
inline Launch plan_grad_launch(const GradPlan& plan, const GradKernel& kernel, long index) { return plan_launch(plan.items, kernel, index); }

// ---- The float64 backward (attention_grad_f64.hip): the same two kernels on v_mfma_f64_16x16x4_f64.  GradProblem and
// GradPlan are the ones above; decided here: each kernel's step over the other axis (GradKernel::step, 64 or 32 rows), the LDS
// rows in doubles, and the even rule of operand_vec16_f64 for all nine operands.
//
// Doubles per LDS row.  A half wave's 32 lanes must land on 32 different doubles modulo 32.  A tile read both ways has an NT
// read at s c + g and an NN read at s g + c (c < 16, g < 2 per half wave) and cannot be free of conflicts both ways: a row
// step s = 18 (mod 32) frees the NT read and folds the NN read on 2 doubles of 32 (the trade of the forward's E rows), where
// s = 2 (mod 32) would fold the NN read on 14 of 16.  Tiles read both ways (the dQ kernel's K tile, the dK/dV kernel's Q and
// dO tiles) have rows of width + 18, an NT-only tile (the dQ kernel's V tile) of width + 2, the waves' own rows of step + 18.
// Derived from the bank map, not measured.
constexpr int GRAD_F64_STEPS[2] = {64, 32};   // largest first
constexpr int GRAD_F64_PAD_BOTH = 18, GRAD_F64_PAD_NT = 2, GRAD_F64_PAD_E = 18;

// dQ kernel: K tile [step][kp + 18], V tile [step][dp + 2], the waves' dS rows [4][16][step + 18], 1 / L and delta of 64 rows.
constexpr long grad_dq_lds_bytes_f64(int kp, int dp, int step) {
  return 8L * (step * (kp + GRAD_F64_PAD_BOTH) + step * (dp + GRAD_F64_PAD_NT) + 4 * 16 * (step + GRAD_F64_PAD_E) + 2 * 64);
}
// dK/dV kernel: Q tile [step][kp + 18], dO tile [step][dp + 18], the waves' rows, 1 / L and delta of the tile's rows.
constexpr long grad_dkv_lds_bytes_f64(int kp, int dp, int step) {
  return 8L * (step * (kp + GRAD_F64_PAD_BOTH) + step * (dp + GRAD_F64_PAD_BOTH) + 4 * 16 * (step + GRAD_F64_PAD_E) + 2 * 64);
}

// 32-bit registers a lane of the dK/dV kernel holds across a tile's MFMAs: the A operands of its K and V rows and the dK
// and dV accumulators (kp + dp together), S^T and dP^T (step), and with `ahead` the next Q tile, dO tile and O parts.  The
// compiler's resource report draws the line: every instantiation at or below 320 of a lane's 512 has no scratch, and the
// four that were above it (368 to 416, at the largest step their LDS allows) spilled 62 to 130 registers; the rest goes to
// addresses and the exp's temporaries.  The line is this compiler's: nothing in the build checks for scratch, so when the
// toolchain changes, regenerate the table of profiles/attention_grad_f64.txt (its section 1 has the command) and move the
// budget if a kernel spills.
constexpr int GRAD_F64_REG_BUDGET = 320;
constexpr int grad_dkv_regs_f64(int kp, int dp, int step, bool ahead) {
  return (kp + dp) + step + (ahead ? step * (kp + dp) / 128 + step * dp / 128 : 0);
}

// The step of each kernel at a pair of padded head dimensions: the largest whose LDS fits a CU (0: none does) and, in the
// dK/dV kernel, whose registers fit with the look-ahead tile; where no step does, the dK/dV kernel takes the smallest step
// without the look-ahead (grad_dkv_ahead_f64 false: its loads wait at the top of each pass).  The kernels are instantiated on
// these functions' values, and the launcher checks them against the plan.  profiles/attention_grad_f64.txt has the table.
constexpr int grad_dq_step_f64(int kp, int dp) {
  for (int step : GRAD_F64_STEPS)
    if (grad_dq_lds_bytes_f64(kp, dp, step) <= LDS_LIMIT) return step;
  return 0;
}
constexpr int grad_dkv_step_f64(int kp, int dp) {
  for (int step : GRAD_F64_STEPS)
    if (grad_dkv_lds_bytes_f64(kp, dp, step) <= LDS_LIMIT && grad_dkv_regs_f64(kp, dp, step, true) <= GRAD_F64_REG_BUDGET) return step;
  return grad_dkv_lds_bytes_f64(kp, dp, GRAD_F64_STEPS[1]) <= LDS_LIMIT ? GRAD_F64_STEPS[1] : 0;
}
constexpr bool grad_dkv_ahead_f64(int kp, int dp) { return grad_dkv_regs_f64(kp, dp, grad_dkv_step_f64(kp, dp), true) <= GRAD_F64_REG_BUDGET; }

GradPlan plan_attention_grad_f64(const GradProblem& p);

// ---- The gradient of the score bias (attention_dbias_f32.hip): dBias (+)= sum of p * (dP - delta) over every index whose
// step in dBias is 0.  One block owns one 64 x 64 tile of one output cell, a cell being a pair (o', i1') of the batch indices
// that are not summed, and adds up in a fixed order every item that maps to the cell (and, with lddb == 0, every row tile):
// the cells are the items of the item grid.
struct DbiasProblem : Extents {
  Operand q, k, v, o, s, dout, bias, dbias;
  int cus = 256;
};

struct DbiasPlan {
  bool supported = false;
  const char* reason = "";
  int kp = 0, dp = 0;
  // 16-byte accesses: loads of Q, Kk, V, O, Sums and dO, stores (and, accumulating, loads) of dBias; the bias is read element
  // by element, straight into accumulator layout (load_bias)
  bool vec_q = false, vec_k = false, vec_v = false, vec_o = false, vec_s = false, vec_do = false, vec_db = false;
  bool row_fold = false;        // lddb == 0: the query rows are summed too, a cell is one row of J floats
  long cells0 = 0, cells1 = 0;  // the cells along batch0 and batch1: the extent where dBias steps, 1 where it sums
  long cells = 0;               // cells0 * cells1: the items of the cut
  long sum0 = 0, sum1 = 0;      // items a block adds along batch0 and batch1: 1 where dBias steps, the extent where it sums
  long tiles_i = 0, tiles_j = 0;
  Cut cut;                      // tiles per cell: tiles_i * tiles_j, or tiles_j with the row fold
  bool ahead = false;           // the next pass's tiles are loaded during this pass's MFMAs
  int block = THREADS;
  long lds_bytes = 0;
};

// Q tile and K tile [64][kp + 4], dO tile and V tile [64][dp + 4] (all four read NT only), 1 / L and delta of the 64 rows.  The
// epilogue's [64][68] staging tile and the fold's [4][64] live in the first two tiles, which are at least 2 * 64 * 36 floats.
constexpr long dbias_lds_bytes(int kp, int dp) { return 4L * (2 * 64 * (kp + GRAD_PAD_NT) + 2 * 64 * (dp + GRAD_PAD_NT) + 2 * 64); }

// 32-bit registers a lane holds across a pass's MFMAs: the A operands of its Q and dO rows ((kp + dp) / 4), the running sums, S,
// dP and the bias tile (16 each), and with `ahead` the four tiles, the O parts and the row sums of the next pass.  The
// compiler's resource report draws the lines (profiles/attention_dbias.txt has the table, with and without the look-ahead):
//   - with everything ahead the largest pair holds 292 of these and none of the 18 kernels has scratch, so the budget admits
//     every pair; when the toolchain changes, regenerate the table and lower the budget if a kernel spills;
//   - the five pairs whose LDS leaves room for one block per CU have one wave per SIMD either way: the look-ahead is free and
//     is the only thing that covers their loads.  At the other four it costs occupancy (64 x 64: 262 registers, one wave per
//     SIMD, against 222 and two), and the second block's waves cover the loads instead: these load at the top of each pass.
constexpr int DBIAS_REG_BUDGET = 320;
constexpr int dbias_regs(int kp, int dp, bool ahead) { return (kp + dp) / 4 + 64 + (ahead ? (kp + dp) / 2 + dp / 4 + 4 : 0); }
// The kernel is instantiated on this function's value, so a plan and its kernel cannot disagree.
constexpr bool dbias_ahead(int kp, int dp) { return 2 * dbias_lds_bytes(kp, dp) > LDS_LIMIT && dbias_regs(kp, dp, true) <= DBIAS_REG_BUDGET; }

DbiasPlan plan_attention_dbias(const DbiasProblem& p);
inline Launch plan_dbias_launch(const DbiasPlan& plan, long index) { return plan_launch(plan.cells, plan.cut, index); }

}  // namespace attention
}  // namespace eg
