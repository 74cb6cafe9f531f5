// The attention forward with a running row maximum, split over the keys (eg_attention_stable_split): for launches whose
// items x row tiles leave most CUs without a block — one long sequence, or a few query rows against a key/value cache.
//   partial   block (item, row tile, split s of S) walks key tiles [s nt / S, (s + 1) nt / S) with the loop of
//             attention_stable_f32.hip and leaves, per query row, m_s = max x, L_s = sum expf(x - m_s) and the unnormalised
//             O_s = sum expf(x - m_s) V in the context's workspace;
//   combine   M = max_s m_s, w_s = expf(m_s - M), L = sum_s w_s L_s, O (+)= (sum_s w_s O_s) / L, s ascending; Stats = (M, L).
// The result is eg_attention_stable's up to rounding: the same terms, added in another fixed order.  No atomics, no spin-waits;
// the workspace is written whole by the partial launch before the combine launch reads it: two runs give the same bits.
//
// Workspace (plan_attention_split): O parts [items][S][rows_pad][DP] floats, then [items][S][2][rows_pad] maxima and sums.
// rows_pad is 64 * tiles_i or 16; rows >= I are never written and never read.  Columns D .. DP - 1 are written (zeros: V is
// zero-filled there) so that the combine kernel reads whole 16-byte chunks.
//
// 1. The 64-row mode (I > 16) is attention_stable_f32_kernel's block — four waves of 16 whole rows, K tile [64][KP + 4], V tile
//    [64][DP + 16], a wave's E rows [16][68], K, V and the bias a tile ahead, two barriers per tile, the correction behind a
//    wave-uniform ballot — over the block's own tile range, with the workspace stores for an epilogue.  The item grid's tile
//    index is tile_i * S + s.
//
// 2. The 16-row mode (I <= 16): with the block above three waves would multiply zero rows.  Here all four waves hold the same
//    16 query rows as A operands (zero above I), and of each 64-key tile in LDS wave w takes keys 16 w .. 16 w + 15:
//      scores  one 16 x 16 block, KP / 4 MFMAs, B operand K tile rows 16 w + c at k = g: bank (KS c + g) mod 64 with
//              KS = 4 mod 32, as in the other kernels: conflict-free;
//      maximum row_max16 over the DPP row, then the running maximum, subtrahend and ballot-guarded correction of the stable loop;
//      E rows  the wave's own [16][20].  Accumulator-layout write: lane (c, g) writes row 4 g + r, column c, float index
//              80 g + 20 r + c; 80 = 16 (mod 64), so for one r the 64 lanes land on banks 16 g + c + 20 r: all 64 different.
//              A-operand read: lane (c, g) reads row c, column 4 jj + g, float index 20 c + g + 4 jj; 20 c (mod 64) runs over the
//              16 multiples of 4 (0 20 40 60 16 36 56 12 32 52 8 28 48 4 24 44), + g < 4: all 64 different.  Both free;
//      E . V   E[16 x 16] . V[16 keys][DP]: 4 k steps x DP / 16 column blocks, B operand V tile rows 16 w + 4 jj + g at column
//              16 nb + c: bank (VS g + c) mod 64, VS = 16 mod 64: conflict-free.
//    A wave does a quarter of a tile's matrix work and keeps its own (m, L, o[DP / 16]); every lane of every wave holds the same
//    (row, column) elements.  After the block's last tile, waves 1 .. 3 leave theirs in LDS (the K and V tiles are free by then),
//    as 16-byte chunks at [wave - 1][chunk][lane]: lane-contiguous, conflict-free; wave 0 merges them in wave order 0, 1, 2, 3
//    by the rule of the combine kernel and stores the block's partial.  A wave whose 16 keys all lie outside the problem has
//    m = -Inf, L = 0, o = 0, and weight expf(-Inf - sub) = 0.
//    Other divisions of the tile (a wave per 16 columns of D, sharing one score block through LDS) need a barrier between the
//    two products of every tile and were not measured.
//
// The subtrahend rule everywhere: a maximum still at -Inf subtracts 0, so -Inf - -Inf never appears.  The special rows are
// eg_attention_stable's: all keys -Inf gives M = -Inf, every w_s = expf(-Inf) = 0, L = 0, O = 0 / 0 = NaN; a +Inf score gives
// m_s = +Inf and L_s NaN in its split, so L and O NaN; a NaN score gives L_s and O_s NaN; a split that is wholly -Inf has
// L_s = 0, O_s = 0 and adds exactly 0 (its weight is 0 or, when every split is so, 1).
// 36 partial kernels (KP x DP x BIAS x mode), none with scratch: profiles/attention_split.txt.
#include "attention.hpp"        // the internal entries
#include "attention_tile.hpp"   // kernel operands, tiles, the MFMA loops, row_max16, the launcher

#include <cmath>

namespace {

using eg::gemm::f32x4;
using namespace eg::attention;

struct SplitArgs {
  In q, k, v;
  float* ws;           // the workspace
  long stats_offset;   // floats from ws to the maxima and sums
  long I, J;
  int K, D;
  float scale;
  int splits, rows_pad;
  Items items;         // tiles: tiles_i * splits
};

struct SplitBiasArgs : SplitArgs {
  In b;
};

// The block's place in the workspace and its key tiles.
struct SplitBlock {
  BlockItem b;
  int tile_i, split;
  long t0, t1;      // key tiles [t0, t1)
  float* o;         // row 0 of the block's rows: [rows][DP]
  float* m;         // its maxima; the sums rows_pad floats on
};

template <int DP>
__device__ __forceinline__ SplitBlock split_block(const SplitArgs& a) {
  SplitBlock s;
  s.b = block_item(a.items);
  s.tile_i = s.b.tile / a.splits;
  s.split = s.b.tile - s.tile_i * a.splits;
  const long nt = (a.J + TILE_J - 1) / TILE_J;
  s.t0 = split_first(nt, a.splits, s.split), s.t1 = split_first(nt, a.splits, s.split + 1);
  const long part = ((long)s.b.outer * a.items.batch1 + s.b.inner) * a.splits + s.split;   // (item, split)
  const long row0 = (long)s.tile_i * TILE_I;
  s.o = a.ws + (part * a.rows_pad + row0) * DP;
  s.m = a.ws + a.stats_offset + part * 2 * a.rows_pad + row0;
  return s;
}

// The lane's part of the block's partial: rows row0 + 4 g + r of the block's rows, columns 16 nb + c; `sum` already folded over
// the 16 lanes of a row.
template <int DP>
__device__ __forceinline__ void store_partial(const SplitBlock& s, int rows_pad, long rows, int row0, int c, int g, const f32x4 (&o)[DP / 16],
                                              const float (&m)[4], const float (&sum)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + 4 * g + r;
    if (row >= rows) continue;
    if (c == 0) {
      s.m[row] = m[r];
      s.m[rows_pad + row] = sum[r];
    }
#pragma unroll
    for (int nb = 0; nb < DP / 16; ++nb) s.o[(long)row * DP + nb * 16 + c] = o[nb][r];
  }
}

__device__ __forceinline__ void fold_row_sums(float (&sum)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float t = sum[r];
    t += __shfl_xor(t, 1);
    t += __shfl_xor(t, 2);
    t += __shfl_xor(t, 4);
    t += __shfl_xor(t, 8);
    sum[r] = t;
  }
}

// ---- 1. the 64-row mode ---------------------------------------------------------------------------------------------------
template <int KP, int DP, bool BIAS>
__global__ __launch_bounds__(THREADS) void attention_split64_f32_kernel(std::conditional_t<BIAS, SplitBiasArgs, SplitArgs> a) {
  constexpr int KS = KP + 4, VS = DP + 16;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const Ks = lds;                      // [64][KS]; the Q tile first
  float* const Vs = Ks + TILE_J * KS;         // [64][VS]
  float* const Es = Vs + TILE_J * VS;         // [4][16][ES]

  const SplitBlock sb = split_block<DP>(a);
  const BlockItem b = sb.b;
  const long i0 = (long)sb.tile_i * TILE_I;
  const long ldq = a.q.v.ld, ldk = a.k.v.ld, ldv = a.v.v.ld;
  const float* const Q = item_base(a.q, b.outer, b.inner) + i0 * ldq;
  const float* const Kk = item_base(a.k, b.outer, b.inner);
  const float* const V = item_base(a.v, b.outer, b.inner);

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  float* const Ew = Es + w * 16 * ES;

  float q[KP / 4];
  {
    TileRegs<KP> tq;
    load_rows<KP>(tq, Q, ldq, a.I - i0, a.K, a.q.vec != 0, tid);
    store_rows<KP, KS>(tq, Ks, tid);
    __syncthreads();
    read_a_rows<KP, KS>(Ks, w, c, g, q);
  }

  f32x4 o[DP / 16];
#pragma unroll
  for (int nb = 0; nb < DP / 16; ++nb) o[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
  float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};

  TileRegs<KP> tk;
  TileRegs<DP> tv;
  [[maybe_unused]] BiasTile bias, bias_next;
  [[maybe_unused]] const long bias_rows = a.I - i0 - w * 16 - 4 * g;
  [[maybe_unused]] long ldb = 0;
  [[maybe_unused]] const float* Bl = nullptr;
  if constexpr (BIAS) {
    ldb = a.b.v.ld;
    Bl = item_base(a.b, b.outer, b.inner) + (i0 + w * 16 + 4 * g) * ldb + c;
  }
  {   // the range is never empty: splits <= nt
    const long j0 = sb.t0 * TILE_J;
    load_rows<KP>(tk, Kk + j0 * ldk, ldk, a.J - j0, a.K, a.k.vec != 0, tid);
    load_rows<DP>(tv, V + j0 * ldv, ldv, a.J - j0, a.D, a.v.vec != 0, tid);
    if constexpr (BIAS) load_bias(bias_next, Bl + j0, ldb, bias_rows, a.J - j0 - c);
  }
  for (long t = sb.t0; t < sb.t1; ++t) {
    const long j0 = t * TILE_J;
    __syncthreads();
    store_rows<KP, KS>(tk, Ks, tid);
    store_rows<DP, VS>(tv, Vs, tid);
    __syncthreads();
    if constexpr (BIAS) bias = bias_next;
    if (t + 1 < sb.t1) {
      load_rows<KP>(tk, Kk + (j0 + TILE_J) * ldk, ldk, a.J - j0 - TILE_J, a.K, a.k.vec != 0, tid);
      load_rows<DP>(tv, V + (j0 + TILE_J) * ldv, ldv, a.J - j0 - TILE_J, a.D, a.v.vec != 0, tid);
      if constexpr (BIAS) load_bias(bias_next, Bl + j0 + TILE_J, ldb, bias_rows, a.J - j0 - TILE_J - c);
    }

    f32x4 s[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) s[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    mma_nt<KP, KS>(q, Ks, c, g, s);

#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      const bool live = j0 + nb * 16 + c < a.J;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x = s[nb][r] * a.scale;
        if constexpr (BIAS) x = x + bias.x[nb][r];
        s[nb][r] = live ? x : -INFINITY;
      }
    }

    float m_new[4], sub[4];
    bool raised = false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float tile_max = row_max16(fmaxf(fmaxf(s[0][r], s[1][r]), fmaxf(s[2][r], s[3][r])));
      m_new[r] = fmaxf(m[r], tile_max);
      sub[r] = m_new[r] == -INFINITY ? 0.f : m_new[r];
      raised |= m_new[r] > m[r];
    }
    if (__any(raised)) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float alpha = expf(m[r] - sub[r]);
        sum[r] *= alpha;
#pragma unroll
        for (int nb = 0; nb < DP / 16; ++nb) o[nb][r] *= alpha;
        m[r] = m_new[r];
      }
    }

#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = expf(s[nb][r] - sub[r]);
        sum[r] += e;
        Ew[(4 * g + r) * ES + nb * 16 + c] = e;
      }
    }
    wave_sync();

    mma_nn<DP, VS, ES>(Ew, Vs, c, g, o);
    wave_sync();
  }

  fold_row_sums(sum);
  store_partial<DP>(sb, a.rows_pad, a.I - i0, w * 16, c, g, o, m, sum);
}

// ---- 2. the 16-row mode ---------------------------------------------------------------------------------------------------
template <int KP, int DP, bool BIAS>
__global__ __launch_bounds__(THREADS) void attention_split16_f32_kernel(std::conditional_t<BIAS, SplitBiasArgs, SplitArgs> a) {
  constexpr int KS = KP + 4, VS = DP + 16, E16 = SPLIT_ES16;
  constexpr int CHUNKS = DP / 16 + 2;   // 16-byte chunks a lane leaves for the merge: o[DP / 16], m, sum
  static_assert(3 * CHUNKS * 64 * 4 <= TILE_J * KS + TILE_J * VS, "the merge fits the K and V tiles");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const Ks = lds;                      // [64][KS]; the Q tile first; the merge last
  float* const Vs = Ks + TILE_J * KS;         // [64][VS]
  float* const Es = Vs + TILE_J * VS;         // [4][16][E16]

  const SplitBlock sb = split_block<DP>(a);
  const BlockItem b = sb.b;
  const long ldq = a.q.v.ld, ldk = a.k.v.ld, ldv = a.v.v.ld;
  const float* const Q = item_base(a.q, b.outer, b.inner);
  const float* const Kk = item_base(a.k, b.outer, b.inner);
  const float* const V = item_base(a.v, b.outer, b.inner);

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  float* const Ew = Es + w * 16 * E16;

  // the 16 query rows as A operands of every k step, the same in all four waves
  float q[KP / 4];
  {
    TileRegs<KP> tq;
    load_rows<KP>(tq, Q, ldq, a.I, a.K, a.q.vec != 0, tid);   // I <= 16: rows 16 .. 63 of the tile are zeros nobody reads
    store_rows<KP, KS>(tq, Ks, tid);
    __syncthreads();
    read_a_rows<KP, KS>(Ks, 0, c, g, q);
  }

  f32x4 o[DP / 16];
#pragma unroll
  for (int nb = 0; nb < DP / 16; ++nb) o[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
  float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};

  TileRegs<KP> tk;
  TileRegs<DP> tv;
  // the lane's bias: rows 4 g + r, key 16 w + c of a tile; `next` is a tile ahead
  [[maybe_unused]] f32x4 bias = {0.f, 0.f, 0.f, 0.f}, bias_next = {0.f, 0.f, 0.f, 0.f};
  [[maybe_unused]] long ldb = 0;
  [[maybe_unused]] const float* Bl = nullptr;
  if constexpr (BIAS) {
    ldb = a.b.v.ld;
    Bl = item_base(a.b, b.outer, b.inner) + (long)(4 * g) * ldb + 16 * w + c;
  }
  const auto load_bias16 = [&](f32x4& t, long j0) {
    const bool key = j0 + 16 * w + c < a.J;
#pragma unroll
    for (int r = 0; r < 4; ++r) t[r] = (key && 4 * g + r < a.I) ? Bl[r * ldb + j0] : 0.f;
  };
  {
    const long j0 = sb.t0 * TILE_J;
    load_rows<KP>(tk, Kk + j0 * ldk, ldk, a.J - j0, a.K, a.k.vec != 0, tid);
    load_rows<DP>(tv, V + j0 * ldv, ldv, a.J - j0, a.D, a.v.vec != 0, tid);
    if constexpr (BIAS) load_bias16(bias_next, j0);
  }
  const float* const pk = Ks + (16 * w + c) * KS + g;   // the wave's keys as B operands of the scores
  const float* const pe = Ew + c * E16 + g;             // its E rows as A operands
  const float* const pv = Vs + (16 * w + g) * VS + c;   // the same keys' V rows as B operands
  for (long t = sb.t0; t < sb.t1; ++t) {
    const long j0 = t * TILE_J;
    __syncthreads();   // every wave is done with the tiles in LDS (the first time: with the Q tile)
    store_rows<KP, KS>(tk, Ks, tid);
    store_rows<DP, VS>(tv, Vs, tid);
    __syncthreads();
    if constexpr (BIAS) bias = bias_next;
    if (t + 1 < sb.t1) {   // in flight during this tile's MFMAs
      load_rows<KP>(tk, Kk + (j0 + TILE_J) * ldk, ldk, a.J - j0 - TILE_J, a.K, a.k.vec != 0, tid);
      load_rows<DP>(tv, V + (j0 + TILE_J) * ldv, ldv, a.J - j0 - TILE_J, a.D, a.v.vec != 0, tid);
      if constexpr (BIAS) load_bias16(bias_next, j0 + TILE_J);
    }

    f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KP / 4; ++kk) s = __builtin_amdgcn_mfma_f32_16x16x4f32(q[kk], pk[4 * kk], s, 0, 0, 0);

    // the scores; a key outside the problem is -Inf by a select
    const bool live = j0 + 16 * w + c < a.J;
    float m_new[4], sub[4];
    bool raised = false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float x = s[r] * a.scale;
      if constexpr (BIAS) x = x + bias[r];
      s[r] = live ? x : -INFINITY;
      m_new[r] = fmaxf(m[r], row_max16(s[r]));
      sub[r] = m_new[r] == -INFINITY ? 0.f : m_new[r];
      raised |= m_new[r] > m[r];
    }
    if (__any(raised)) {   // wave-uniform; a row that did not move would be multiplied by 1.0f
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float alpha = expf(m[r] - sub[r]);
        sum[r] *= alpha;
#pragma unroll
        for (int nb = 0; nb < DP / 16; ++nb) o[nb][r] *= alpha;
        m[r] = m_new[r];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = expf(s[r] - sub[r]);
      sum[r] += e;
      Ew[(4 * g + r) * E16 + c] = e;
    }
    wave_sync();

#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const float e = pe[4 * jj];
#pragma unroll
      for (int nb = 0; nb < DP / 16; ++nb) o[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(e, pv[4 * jj * VS + nb * 16], o[nb], 0, 0, 0);
    }
    wave_sync();   // the wave's E rows are read before its next tile overwrites them
  }

  fold_row_sums(sum);
  // The merge.  Chunk n of lane l of wave w' = 1 .. 3 at float ((w' - 1) CHUNKS + n) * 256 + 4 l.
  __syncthreads();   // every wave is done with the K and V tiles
  f32x4* const Mg = reinterpret_cast<f32x4*>(lds);
  if (w > 0) {
    f32x4* const mine = Mg + (w - 1) * CHUNKS * 64 + lane;
#pragma unroll
    for (int nb = 0; nb < DP / 16; ++nb) mine[nb * 64] = o[nb];
    mine[(DP / 16) * 64] = f32x4{m[0], m[1], m[2], m[3]};
    mine[(DP / 16 + 1) * 64] = f32x4{sum[0], sum[1], sum[2], sum[3]};
  }
  __syncthreads();
  if (w > 0) return;
  f32x4 mw[4], lw[4];   // [wave][r]
  mw[0] = f32x4{m[0], m[1], m[2], m[3]}, lw[0] = f32x4{sum[0], sum[1], sum[2], sum[3]};
#pragma unroll
  for (int v = 1; v < 4; ++v) {
    mw[v] = Mg[((v - 1) * CHUNKS + DP / 16) * 64 + lane];
    lw[v] = Mg[((v - 1) * CHUNKS + DP / 16 + 1) * 64 + lane];
  }
  f32x4 wt[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float top = fmaxf(fmaxf(mw[0][r], mw[1][r]), fmaxf(mw[2][r], mw[3][r]));
    const float sub = top == -INFINITY ? 0.f : top;
    float total = 0.f;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      wt[v][r] = expf(mw[v][r] - sub);
      total += wt[v][r] * lw[v][r];
    }
    m[r] = top, sum[r] = total;
  }
#pragma unroll
  for (int nb = 0; nb < DP / 16; ++nb) {
    f32x4 acc = o[nb] * wt[0];
#pragma unroll
    for (int v = 1; v < 4; ++v) acc += Mg[((v - 1) * CHUNKS + nb) * 64 + lane] * wt[v];
    o[nb] = acc;
  }
  store_partial<DP>(sb, a.rows_pad, a.I, 0, c, g, o, m, sum);
}

// ---- 3. the combine kernel ------------------------------------------------------------------------------------------------
struct CombineArgs {
  const float* ws;
  long stats_offset;
  Out o, st;        // st.p may be NULL
  long I, rows;     // rows: items * rows_pad
  int D, splits, rows_pad;
  unsigned batch1;
  int accumulate;
};

// A thread owns four columns of one row: DP / 4 threads read a split's row of DP floats as consecutive 16-byte chunks.  A block
// has 1024 / DP rows and walks rows gridDim.x * 1024 / DP apart.  The thread of column 0 stores the row's stats.
template <int DP>
__global__ __launch_bounds__(THREADS) void attention_split_combine_kernel(CombineArgs a) {
  constexpr int TPR = DP / 4, RPB = THREADS / TPR;
  const int col = ((int)threadIdx.x % TPR) * 4;
  for (long row_all = (long)blockIdx.x * RPB + (int)threadIdx.x / TPR; row_all < a.rows; row_all += (long)gridDim.x * RPB) {
    const long item = row_all / a.rows_pad, row = row_all - item * a.rows_pad;
    if (row >= a.I) continue;
    const float* const ms = a.ws + a.stats_offset + item * a.splits * 2 * a.rows_pad + row;   // split s: 2 rows_pad floats on
    const float* const os = a.ws + (item * a.splits * a.rows_pad + row) * DP + col;           // split s: rows_pad DP floats on
    float top = -INFINITY;
    for (int s = 0; s < a.splits; ++s) top = fmaxf(top, ms[(long)s * 2 * a.rows_pad]);
    const float sub = top == -INFINITY ? 0.f : top;
    float total = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < a.splits; ++s) {
      const float wt = expf(ms[(long)s * 2 * a.rows_pad] - sub);
      total += wt * ms[(long)s * 2 * a.rows_pad + a.rows_pad];
      acc += *reinterpret_cast<const f32x4*>(os + (long)s * a.rows_pad * DP) * wt;
    }
    const unsigned outer = (unsigned)(item / a.batch1), inner = (unsigned)(item % a.batch1);
    if (a.st.p && col == 0) {
      float* const St = item_base(a.st, outer, inner);
      St[row] = top;
      St[a.st.v.ld + row] = total;
    }
    float* const p = item_base(a.o, outer, inner) + row * a.o.v.ld + col;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      if (col + n >= a.D) break;
      const float v = acc[n] / total;
      p[n] = a.accumulate ? p[n] + v : v;
    }
  }
}

template <auto KERNEL, class Args>
int launch(eg_ctx* ctx, unsigned grid, const SplitPlan& p, const Args& args) {
  const int rc = dynamic_lds_once<KERNEL>(ctx, {p.lds_bytes});
  if (rc) return rc;
  hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(p.block), (size_t)p.lds_bytes, ctx->stream, args);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}

template <int DP>
int launch_combine(eg_ctx* ctx, const SplitPlan& p, const CombineArgs& args) {
  hipLaunchKernelGGL(attention_split_combine_kernel<DP>, dim3((unsigned)p.combine_grid), dim3(p.block), 0, ctx->stream, args);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}

}  // namespace

namespace eg {
namespace attention {

int attention_stable_split(eg_ctx* ctx, const Extents& e, float scale, const float* Q, View q, const float* Kk, View k, const float* V, View v,
                           float* O, View o, int accumulate, float* Stats, View st, const float* Bias, View bv, int splits) {
  const char* const name = "eg_attention_stable_split";
  EG_REQUIRE(splits >= 0, EG_ERR_INVALID, "%s: splits = %d is negative", name, splits);
  bool nothing = false;
  int rc = attention_stable_check(ctx, e, Q, q, Kk, k, V, v, O, o, accumulate, Stats, st, Bias, bv, name, &nothing);
  if (rc || nothing) return rc;

  Problem pr;
  static_cast<Extents&>(pr) = e;
  pr.q = {q, aligned16(Q)}, pr.k = {k, aligned16(Kk)}, pr.v = {v, aligned16(V)}, pr.o = {o, aligned16(O)};
  pr.sums = Stats != nullptr;
  pr.has_bias = Bias != nullptr;
  pr.bias = {bv, aligned16(Bias)};
  pr.cus = ctx->compute_units;
  const SplitPlan p = plan_attention_split(pr, splits);
  EG_REQUIRE(p.supported, EG_ERR_UNSUPPORTED, "%s: %s", name, p.reason);
  if (p.forward) return attention_stable(ctx, e, scale, Q, q, Kk, k, V, v, O, o, accumulate, Stats, st, Bias, bv, name);

  rc = eg::set_device(ctx);
  if (rc) return rc;
  rc = eg::ensure_workspace(ctx, (size_t)p.workspace_bytes);
  if (rc) return rc;
  float* const ws = static_cast<float*>(ctx->workspace);

  SplitBiasArgs args = {};
  args.q = {Q, q, p.base.vec_q}, args.k = {Kk, k, p.base.vec_k}, args.v = {V, v, p.base.vec_v}, args.b = {Bias, bv, p.base.vec_b};
  args.ws = ws, args.stats_offset = p.stats_offset;
  args.I = e.I, args.J = e.J, args.K = (int)e.K, args.D = (int)e.D;
  args.scale = scale;
  args.splits = p.splits, args.rows_pad = (int)p.rows_pad;
  // 36 kernels: the padded K x the padded D, with and without a bias, in either mode
  rc = for_each_launch(name, p.base.items, p.partial, e.batch1, [&](const Items& items, unsigned grid) {
    args.items = items;
    return dispatch_heads(p.base.kp, p.base.dp, [&](auto KP, auto DP) {
      constexpr int kp = KP(), dp = DP();
      if (p.rows16)
        return Bias ? launch<&attention_split16_f32_kernel<kp, dp, true>, SplitBiasArgs>(ctx, grid, p, args)
                    : launch<&attention_split16_f32_kernel<kp, dp, false>, SplitArgs>(ctx, grid, p, args);
      return Bias ? launch<&attention_split64_f32_kernel<kp, dp, true>, SplitBiasArgs>(ctx, grid, p, args)
                  : launch<&attention_split64_f32_kernel<kp, dp, false>, SplitArgs>(ctx, grid, p, args);
    });
  });
  if (rc) return rc;

  CombineArgs ca = {};
  ca.ws = ws, ca.stats_offset = p.stats_offset;
  ca.o = {O, o, 0}, ca.st = {Stats, st, 0};
  ca.I = e.I, ca.rows = p.combine_rows;
  ca.D = (int)e.D, ca.splits = p.splits, ca.rows_pad = (int)p.rows_pad;
  ca.batch1 = (unsigned)e.batch1;
  ca.accumulate = accumulate;
  switch (p.base.dp) {
    case 32: return launch_combine<32>(ctx, p, ca);
    case 64: return launch_combine<64>(ctx, p, ca);
    default: return launch_combine<128>(ctx, p, ca);
  }
}

}  // namespace attention
}  // namespace eg

extern "C" int eg_attention_stable_split(eg_ctx* ctx, int64_t batch0, int64_t batch1, int64_t I, int64_t J, int64_t K, int64_t D, float scale,
                                         const float* Q, int64_t ldq, int64_t stride_q0, int64_t stride_q1, const float* Kk, int64_t ldk,
                                         int64_t stride_k0, int64_t stride_k1, const float* V, int64_t ldv, int64_t stride_v0, int64_t stride_v1,
                                         float* O, int64_t ldo, int64_t stride_o0, int64_t stride_o1, int accumulate, float* Stats, int64_t lds,
                                         int64_t stride_s0, int64_t stride_s1, const float* Bias, int64_t ldb, int64_t stride_b0, int64_t stride_b1,
                                         int splits) {
  return eg::attention::attention_stable_split(ctx, {batch0, batch1, I, J, K, D}, scale, Q, {ldq, stride_q0, stride_q1}, Kk, {ldk, stride_k0, stride_k1},
                                               V, {ldv, stride_v0, stride_v1}, O, {ldo, stride_o0, stride_o1}, accumulate, Stats,
                                               {lds, stride_s0, stride_s1}, Bias, {ldb, stride_b0, stride_b1}, splits);
}
