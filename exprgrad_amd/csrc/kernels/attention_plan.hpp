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
  int cus = 256;
};

struct Plan {
  bool supported = false;
  const char* reason = "";   // why not, naming the limit
  int tile_i = TILE_I, tile_j = TILE_J;
  int kp = 0, dp = 0;        // K and D as the kernel is instantiated: 32, 64 or 128, the rest zero-filled
  bool vec_q = false, vec_k = false, vec_v = false;   // 16-byte loads of that operand
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
  long items = 0;
  GradKernel dq, dkv;
  int block = THREADS;
};

// Floats per LDS row of a tile that is read both as an NT operand (16 rows x 4 columns per instruction) and as an NN
// operand (4 rows x 16 columns): see attention_grad_f32.hip.
constexpr int GRAD_PAD_BOTH = 20, GRAD_PAD_NT = 4;

// dQ kernel: K tile [64][kp + 20] (NT for the scores, NN for dS * K), V tile [64][dp + 4] (NT only), the waves' dS rows
// [4][16][68], and 1 / L and delta of the block's 64 rows.
inline long grad_dq_lds_bytes(int kp, int dp) { return 4L * (64 * (kp + GRAD_PAD_BOTH) + 64 * (dp + GRAD_PAD_NT) + 4 * 16 * 68 + 2 * 64); }
// dK/dV kernel: Q tile [64][kp + 20] and dO tile [64][dp + 20] (both read both ways), the waves' rows, 1 / L and delta.
inline long grad_dkv_lds_bytes(int kp, int dp) { return 4L * (64 * (kp + GRAD_PAD_BOTH) + 64 * (dp + GRAD_PAD_BOTH) + 4 * 16 * 68 + 2 * 64); }

GradPlan plan_attention_grad(const GradProblem& p);
// Launch `index` of one of a plan's kernels, index in [0, kernel.launches): the cut's again.
inline Launch plan_grad_launch(const GradPlan& plan, const GradKernel& kernel, long index) { return plan_launch(plan.items, kernel, index); }

}  // namespace attention
}  // namespace eg
