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
  r.items = p.batch0 * p.batch1;
  const Cut c = cut_items(r.items, tiles_i);
  r.tiles_i = c.tiles, r.grid = c.grid, r.items_per_launch = c.items_per_launch, r.launches = c.launches;
  r.supported = true;
  return r;
}

}  // namespace

Plan plan_attention(const Problem& p) { return plan_forward(p, false); }
Plan plan_attention_f64(const Problem& p) { return plan_forward(p, true); }

// Empty I, J, K and D are plans too (a kernel with no tiles has no launches; the entry decides what an empty extent
// writes); empty batch extents are not.
GradPlan plan_attention_grad(const GradProblem& p) {
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
  r.dq.lds_bytes = grad_dq_lds_bytes(r.kp, r.dp);
  r.dkv.lds_bytes = grad_dkv_lds_bytes(r.kp, r.dp);
  if (r.dq.lds_bytes > LDS_LIMIT || r.dkv.lds_bytes > LDS_LIMIT) {
    r.reason = "the tiles exceed the LDS of a CU";
    return r;
  }
  const long tiles_i = (p.I + 63) / 64, tiles_j = (p.J + 63) / 64;
  if (tiles_i > eg::gemm::BATCHED_MAX_BLOCKS || tiles_j > eg::gemm::BATCHED_MAX_BLOCKS) {
    r.reason = "an item has more tiles than one launch has blocks";
    return r;
  }
  r.vec_q = operand_vec16(p.q), r.vec_k = operand_vec16(p.k), r.vec_v = operand_vec16(p.v), r.vec_o = operand_vec16(p.o);
  r.vec_s = operand_vec16(p.s), r.vec_do = operand_vec16(p.dout);
  r.vec_dq = operand_vec16(p.dq), r.vec_dk = operand_vec16(p.dk), r.vec_dv = operand_vec16(p.dv);
  r.items = p.batch0 * p.batch1;
  static_cast<Cut&>(r.dq) = cut_items(r.items, tiles_i);
  static_cast<Cut&>(r.dkv) = cut_items(r.items, tiles_j);
  r.supported = true;
  return r;
}

}  // namespace attention
}  // namespace eg
