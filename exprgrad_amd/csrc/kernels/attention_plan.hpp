// Host-side planning of the fused attention forward (attention_f32.hip): whether the kernel takes a problem, on which
// tile, with which load width per operand, on how many blocks in how many launches, and with how much LDS.  Plain C++
// (no HIP, no other unit): the launcher does nothing but obey an AttentionPlan, and tests/test_attention_plan_cpu.py
// checks plans without a GPU.
#pragma once

#include "gemm_plan.hpp"   // BATCHED_MAX_BLOCKS

namespace eg {
namespace attention {

constexpr int TILE_I = 64;     // query rows of a block: four waves of 16 rows
constexpr int TILE_J = 64;     // keys of one pass of the block's loop
constexpr int MAX_HEAD = 128;  // K and D
constexpr int THREADS = 256;
constexpr long LDS_LIMIT = 160 * 1024;   // per CU on gfx950

// One operand: floats per row step and per step of the two batch indices, and whether item (0, 0) starts 16-byte aligned.
struct Operand {
  long ld = 0, stride0 = 0, stride1 = 0;
  bool aligned = true;
};

struct Problem {
  long batch0 = 0, batch1 = 0, I = 0, J = 0, K = 0, D = 0;
  Operand q, k, v, o;
  int cus = 256;
};

// Items [first, first + items) of the flattened (o, i1) range, o-major, as grid = items * tiles_i blocks.
struct Launch {
  long first = 0, items = 0, grid = 0;
};

struct Plan {
  bool supported = false;
  const char* reason = "";   // why not, naming the limit
  int tile_i = TILE_I, tile_j = TILE_J;
  int kp = 0, dp = 0;        // K and D as the kernel is instantiated: 32, 64 or 128, the rest zero-filled
  bool vec_q = false, vec_k = false, vec_v = false;   // 16-byte loads of that operand
  long tiles_i = 0;          // blocks per item
  long items = 0;            // batch0 * batch1
  long grid = 0;             // blocks of all launches together: items * tiles_i
  long items_per_launch = 0; // at least 1; BATCHED_MAX_BLOCKS / tiles_i otherwise
  long launches = 0;
  int block = THREADS;
  long lds_bytes = 0;
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

// Launch `index` of a plan, index in [0, plan.launches).
Launch plan_launch(const Plan& plan, long index);

}  // namespace attention
}  // namespace eg
