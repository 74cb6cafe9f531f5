// plan_attention: see attention_plan.hpp.  One tile shape (64 query rows x 64 keys, four waves of 16 rows) for every
// float32 problem; what varies is the padded head dimensions, the load width per operand and the cut into launches.  The
// float64 forward (plan_attention_f64) also varies the key tile: 64 keys, or 32 where 64 do not fit the LDS.
#include "attention_plan.hpp"

#include <algorithm>

namespace eg {
namespace attention {

namespace {

// The forward's plan in either scalar type: the two differ in the key tile, the LDS rows and the 16-byte rule.
Plan plan_forward(const Problem& p, bool f64) {
  Plan r;
  if (p.batch0 < 1 || p.batch1 < 1 || p.I < 1 || p.J < 0 || p.K < 0 || p.D < (p.sums ? 0 : 1)) {
    r.reason = "an empty or negative extent";
    return r;
  }
  if (p.K > MAX_HEAD) {
    r.reason = "K above 128";
    return r;
  }
  if (p.D > MAX_HEAD) {
    r.reason = "D above 128";
    return r;
  }
  r.kp = padded_head(p.K);
  r.dp = padded_head(p.D);
  if (f64) r.tile_j = key_tile_f64(r.kp, r.dp);
  r.lds_bytes = f64 ? lds_bytes_for_f64(r.kp, r.dp, r.tile_j) : lds_bytes_for(r.kp, r.dp);
  if (r.tile_j == 0 || r.lds_bytes > LDS_LIMIT) {
    r.reason = "the tiles exceed the LDS of a CU";
    return r;
  }
  const long tiles_i = (p.I + TILE_I - 1) / TILE_I;
  if (tiles_i > eg::gemm::BATCHED_MAX_BLOCKS) {
    r.reason = "an item has more row tiles than one launch has blocks";
    return r;
  }
  r.vec_q = f64 ? operand_vec16_f64(p.q) : operand_vec16(p.q);
  r.vec_k = f64 ? operand_vec16_f64(p.k) : operand_vec16(p.k);
  r.vec_v = f64 ? operand_vec16_f64(p.v) : operand_vec16(p.v);
  r.vec_b = !f64 && p.has_bias && operand_vec16(p.bias);   // needs no LDS: lds_bytes is what it was
  r.items = p.batch0 * p.batch1;
  const Cut c = cut_items(r.items, tiles_i);
  r.tiles_i = c.tiles, r.grid = c.grid, r.items_per_launch = c.items_per_launch, r.launches = c.launches;
  r.supported = true;
  return r;
}

}  // namespace

Plan plan_attention(const Problem& p) { return plan_forward(p, false); }
Plan plan_attention_f64(const Problem& p) { return plan_forward(p, true); }

// The forward split over the keys.  The auto rule splits only a launch that leaves CUs without a block, and then into as many
// ranges as give every CU the blocks it can hold at once (split_blocks_per_cu), none shorter than SPLIT_MIN_TILES key tiles.
SplitPlan plan_attention_split(const Problem& p, int splits) {
  SplitPlan r;
  if (splits < 0) {
    r.reason = "a negative number of splits";
    return r;
  }
  r.base = plan_forward(p, false);
  if (!r.base.supported) {
    r.reason = r.base.reason;
    return r;
  }
  const Plan& b = r.base;
  r.rows16 = p.I <= SPLIT_ROWS16;
  r.nt = (p.J + TILE_J - 1) / TILE_J;
  const long most = std::max(1L, r.nt);
  if (splits == 0) {
    const long blocks = b.items * b.tiles_i, target = split_blocks_per_cu(b.kp, b.dp) * p.cus;
    r.splits = 1;
    if (blocks < p.cus && r.nt >= 2) r.splits = (int)std::max(1L, std::min(target / blocks, r.nt / SPLIT_MIN_TILES));
  } else {
    r.splits = (int)std::min((long)splits, most);
  }
  r.forward = p.J == 0 || p.D == 0 || (!r.rows16 && r.splits == 1);
  if (b.tiles_i * r.splits > eg::gemm::BATCHED_MAX_BLOCKS) {
    r.reason = "an item has more row tiles times splits than one launch has blocks";
    return r;
  }
  r.rows_pad = r.rows16 ? SPLIT_ROWS16 : TILE_I * b.tiles_i;
  r.stats_offset = b.items * r.splits * r.rows_pad * b.dp;
  r.workspace_bytes = r.forward ? 0 : 4L * (r.stats_offset + b.items * r.splits * 2 * r.rows_pad);
  r.partial = cut_items(b.items, b.tiles_i * r.splits);
  r.combine_rows = b.items * r.rows_pad;
  r.combine_rows_per_block = 4 * THREADS / b.dp;
  r.combine_grid = std::min(eg::gemm::BATCHED_MAX_BLOCKS, (r.combine_rows + r.combine_rows_per_block - 1) / r.combine_rows_per_block);
  r.lds_bytes = r.rows16 ? split16_lds_bytes(b.kp, b.dp) : b.lds_bytes;
  r.supported = true;
  return r;
}

// The causal forward in chunks of key tiles.  The auto rule (chunk == 0), with visits = the key-tile visits of the whole call
// and blocks = items x row tiles, the blocks of eg_attention_causal:
//   - blocks below split_blocks_per_cu x CUs (a launch that leaves block slots idle): chunk = visits / (split_blocks_per_cu x
//     CUs), rounded up: about as many pieces as run at once, the split's rule;
//   - a full launch whose items have more row tiles than there are items: nothing is cut.  Its blocks are issued item by item,
//     longest first, so with few items of many row tiles the whole launch is nearly longest-first already;
//   - any other full launch: chunk = visits / CUs / CAUSAL_SPLIT_FULL_PIECES, pieces of a sixteenth of a CU's share of the work,
//     which bounds what the last block of the launch can add to its time;
//   - never below CAUSAL_SPLIT_MIN_TILES; a chunk at or above the longest row tile cuts nothing: eg_attention_causal.
// The rows these came from, profiles/attention_causal_split.txt section 2 (one MI355X, 256 CUs; microseconds per call, median
// of three fresh processes, spread at most 5.5 us below 2 ms and 22.4 us above; heads x I x J x K=D, offset):
//   shape                     causal  chunk 1      2      4      8     16     32     64    128    256   auto picks
//   128x512x512x64, 0          111.1    115.9  100.2  102.0  111.0                                       2
//   128x2048x2048x64, 0        983.9   1678.6 1254.2 1092.0 1011.8  972.6  981.7                         16
//   32x128x8192x128, 8064      872.0    512.9  379.3  298.4  263.3  245.1  234.4  449.1  873.1           32
//   32x16x8192x128, 8176       861.6    205.1  133.1   94.0   77.5   68.3  112.1  208.2  400.7           16
//   32x1x8192x128, 8191        853.9    187.3  123.2   91.2   74.8   65.9  108.4  201.5  389.0           16
//   8x16384x16384x64, 0       3190.1   6567.4 4852.1 4059.3 3641.4 3427.3 3332.4 3278.1 3212.9 3178.4    256 (eg_attention_causal)
//  - the three cache shapes have their best time where the pieces are 256, one per CU at K = D = 128: the split's constant;
//  - CAUSAL_SPLIT_FULL_PIECES = 16 and CAUSAL_SPLIT_MIN_TILES = 2 are fitted to the first two rows (a CU's share is 18 and 264
//    visits: chunks 2 and 16), and the row-tiles-against-items test to the last, where no chunk measured faster than
//    eg_attention_causal.  Three rows do not make a model: full launches of other shapes are not measured.
CausalSplitPlan plan_attention_causal_split(const Problem& p, long offset, int chunk) {
  CausalSplitPlan r;
  if (chunk < 0) {
    r.reason = "a negative chunk";
    return r;
  }
  if (offset < 0) {
    r.reason = "a negative offset";
    return r;
  }
  r.base = plan_forward(p, false);
  if (!r.base.supported) {
    r.reason = r.base.reason;
    return r;
  }
  const Plan& b = r.base;
  if (p.J >= (1L << 36)) {
    r.reason = "J of 2^36 or more";
    return r;
  }
  offset = std::min(offset, p.J);
  r.rows16 = p.I <= SPLIT_ROWS16;
  r.rows = r.rows16 ? SPLIT_ROWS16 : TILE_I;
  if (chunk == 0) {
    const CausalPieces whole = causal_pieces(p.I, p.J, offset, 1, r.rows16);
    const long visits = b.items * causal_pieces_before(whole, whole.tiles);   // with chunk 1 a piece is a tile visit
    const long target = split_blocks_per_cu(b.kp, b.dp) * p.cus;
    long auto_chunk = whole.nv;   // nothing is cut
    if (b.items * whole.tiles < target)
      auto_chunk = (visits + target - 1) / target;
    else if (whole.tiles <= b.items)
      auto_chunk = visits / p.cus / CAUSAL_SPLIT_FULL_PIECES;
    r.pieces = causal_pieces(p.I, p.J, offset, std::max(CAUSAL_SPLIT_MIN_TILES, auto_chunk), r.rows16);
  } else {
    r.pieces = causal_pieces(p.I, p.J, offset, chunk, r.rows16);
  }
  const CausalPieces& c = r.pieces;
  r.first_cut = causal_first_cut_tile(c);
  r.pieces_per_item = causal_pieces_before(c, c.tiles);
  r.slots = r.pieces_per_item - causal_pieces_before(c, r.first_cut);
  r.forward = p.J == 0 || p.D == 0 || (!r.rows16 && r.first_cut == c.tiles);
  if (r.pieces_per_item > eg::gemm::BATCHED_MAX_BLOCKS) {
    r.reason = "an item has more pieces than one launch has blocks";
    return r;
  }
  r.stats_offset = b.items * r.slots * r.rows * b.dp;
  r.workspace_bytes = r.forward ? 0 : 4L * (r.stats_offset + b.items * r.slots * 2 * r.rows);
  r.partial = cut_items(b.items, r.pieces_per_item);
  r.combine_rows_per_item = r.rows * (c.tiles - r.first_cut);
  r.combine_rows = b.items * r.combine_rows_per_item;
  const long rows_per_block = 4 * THREADS / b.dp;
  r.combine_grid = std::min(eg::gemm::BATCHED_MAX_BLOCKS, (r.combine_rows + rows_per_block - 1) / rows_per_block);
  r.lds_bytes = r.rows16 ? split16_lds_bytes(b.kp, b.dp) : b.lds_bytes;
  r.supported = true;
  return r;
}

namespace {

// The backward's plan in either scalar type: the two differ in the steps, the LDS rows and the 16-byte rule.  Empty I, J, K
// and D are plans too (a kernel with no tiles has no launches; the entry decides what an empty extent writes); empty batch
// extents are not.
GradPlan plan_backward(const GradProblem& p, bool f64) {
  GradPlan r;
  if (p.batch0 < 1 || p.batch1 < 1 || p.I < 0 || p.J < 0 || p.K < 0 || p.D < 0) {
    r.reason = "an empty batch or a negative extent";
    return r;
  }
  if (p.K > MAX_HEAD) {
    r.reason = "K above 128";
    return r;
  }
  if (p.D > MAX_HEAD) {
    r.reason = "D above 128";
    return r;
  }
  r.kp = padded_head(p.K);
  r.dp = padded_head(p.D);
  if (f64) {
    r.dq.step = grad_dq_step_f64(r.kp, r.dp), r.dkv.step = grad_dkv_step_f64(r.kp, r.dp);
    r.dq.lds_bytes = grad_dq_lds_bytes_f64(r.kp, r.dp, r.dq.step);
    r.dkv.lds_bytes = grad_dkv_lds_bytes_f64(r.kp, r.dp, r.dkv.step);
  } else {
    r.dq.lds_bytes = grad_dq_lds_bytes(r.kp, r.dp, p.stable);
    r.dkv.lds_bytes = grad_dkv_lds_bytes(r.kp, r.dp, p.stable);
  }
  if (r.dq.step == 0 || r.dkv.step == 0 || r.dq.lds_bytes > LDS_LIMIT || r.dkv.lds_bytes > LDS_LIMIT) {
    r.reason = "the tiles exceed the LDS of a CU";
    return r;
  }
  const long tiles_i = (p.I + 63) / 64, tiles_j = (p.J + 63) / 64;
  if (tiles_i > eg::gemm::BATCHED_MAX_BLOCKS || tiles_j > eg::gemm::BATCHED_MAX_BLOCKS) {
    r.reason = "an item has more tiles than one launch has blocks";
    return r;
  }
  const auto vec = [f64](const Operand& x) { return f64 ? operand_vec16_f64(x) : operand_vec16(x); };
  r.vec_q = vec(p.q), r.vec_k = vec(p.k), r.vec_v = vec(p.v), r.vec_o = vec(p.o);
  r.vec_s = vec(p.s), r.vec_do = vec(p.dout);
  r.vec_dq = vec(p.dq), r.vec_dk = vec(p.dk), r.vec_dv = vec(p.dv);
  r.vec_b = !f64 && p.has_bias && operand_vec16(p.bias);
  r.items = p.batch0 * p.batch1;
  static_cast<Cut&>(r.dq) = cut_items(r.items, tiles_i);
  static_cast<Cut&>(r.dkv) = cut_items(r.items, tiles_j);
  r.supported = true;
  return r;
}

}  // namespace

GradPlan plan_attention_grad(const GradProblem& p) { return plan_backward(p, false); }
GradPlan plan_attention_grad_f64(const GradProblem& p) { return plan_backward(p, true); }

// The dBias kernel's plan.  Where dBias has a step of 0 the index is summed inside a block; the other batch indices span the
// cells.  Empty I, J, K and D and an empty summed batch are plans (the block has no passes, or the kernel no tiles); an empty
// batch extent that dBias steps over is not.
DbiasPlan plan_attention_dbias(const DbiasProblem& p) {
  DbiasPlan r;
  if (p.batch0 < 0 || p.batch1 < 0 || p.I < 0 || p.J < 0 || p.K < 0 || p.D < 0) {
    r.reason = "a negative extent";
    return r;
  }
  if (p.K > MAX_HEAD) {
    r.reason = "K above 128";
    return r;
  }
  if (p.D > MAX_HEAD) {
    r.reason = "D above 128";
    return r;
  }
  r.row_fold = p.dbias.ld == 0;
  r.cells0 = p.dbias.stride0 ? p.batch0 : 1, r.cells1 = p.dbias.stride1 ? p.batch1 : 1;
  r.sum0 = p.dbias.stride0 ? 1 : p.batch0, r.sum1 = p.dbias.stride1 ? 1 : p.batch1;
  if (r.cells0 < 1 || r.cells1 < 1) {
    r.reason = "an empty batch that dBias steps over";
    return r;
  }
  r.kp = padded_head(p.K);
  r.dp = padded_head(p.D);
  r.ahead = dbias_ahead(r.kp, r.dp);
  r.lds_bytes = dbias_lds_bytes(r.kp, r.dp);
  if (r.lds_bytes > LDS_LIMIT) {
    r.reason = "the tiles exceed the LDS of a CU";
    return r;
  }
  r.tiles_i = (p.I + 63) / 64, r.tiles_j = (p.J + 63) / 64;
  if (r.tiles_i > eg::gemm::BATCHED_MAX_BLOCKS || r.tiles_j > eg::gemm::BATCHED_MAX_BLOCKS ||
      (!r.row_fold && r.tiles_i * r.tiles_j > eg::gemm::BATCHED_MAX_BLOCKS)) {
    r.reason = "a cell has more tiles than one launch has blocks";
    return r;
  }
  r.vec_q = operand_vec16(p.q), r.vec_k = operand_vec16(p.k), r.vec_v = operand_vec16(p.v), r.vec_o = operand_vec16(p.o);
  r.vec_s = operand_vec16(p.s), r.vec_do = operand_vec16(p.dout), r.vec_db = operand_vec16(p.dbias);
  r.cells = r.cells0 * r.cells1;
  r.cut = cut_items(r.cells, r.row_fold ? r.tiles_j : r.tiles_i * r.tiles_j);
  r.supported = true;
  return r;
}

}  // namespace attention
}  // namespace eg
