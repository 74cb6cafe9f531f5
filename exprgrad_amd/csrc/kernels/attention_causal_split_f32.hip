// The causal attention forward cut into chunks of key tiles (eg_attention_causal_split): eg_attention_causal for launches whose
// blocks are few or uneven — a chunk of query rows or a decode step against a long key/value cache, one long sequence.
// eg_attention_causal gives a block to every 64-row tile, and that block walks the tile's n_t key tiles alone: 1 for the first
// row tile of a self-attention, J / 64 for the last.  Here row tile t is walked by P_t = ceil(n_t / chunk) blocks of balanced,
// never empty pieces (attention_plan.hpp: causal_piece_decode), so every block of the launch has at most `chunk` tiles:
//   partial   block (item, row tile t, piece p) walks key tiles [split_first(n_t, P_t, p), split_first(n_t, P_t, p + 1)) with the
//             loop of attention_stable_f32.hpp under CAUSAL.  P_t == 1: it finishes the row tile itself, the epilogue and the
//             bits of eg_attention_causal, and never touches the workspace.  P_t >= 2: it leaves, per query row, m_p = max x,
//             L_p = sum expf(x - m_p) and the unnormalised O_p = sum expf(x - m_p) V in the context's workspace;
//   combine   over the rows of the cut row tiles only: M = max_p m_p, w_p = expf(m_p - M), L = sum_p w_p L_p,
//             O (+)= (sum_p w_p O_p) / L, p ascending; Stats = (M, L).
// The blocks of an item are issued in descending (row tile, piece) order: the row tiles with the most pieces first.  A block
// finds its (row tile, piece) from its index alone, by a binary search over the row tiles on the closed form of the pieces
// before a row tile: no table is uploaded and no block loops over the row tiles.  Masked key tiles are in no piece: nothing at
// or beyond causal_visible_keys is loaded.  No atomics, no spin-waits; the partial launch writes every partial whole before the
// combine launch reads it: two runs give the same bits.
//
// Workspace (plan_attention_causal_split): O parts [items][slots][R][DP] floats, then [items][slots][2][R] maxima and sums; an
// item's slots are the pieces of its cut row tiles in ascending (row tile, piece) order, R = 64 rows each (16 in the 16-row
// mode).  Rows >= I are never written and never read; columns D .. DP - 1 are written (zeros) so that the combine kernel reads
// whole 16-byte chunks.
//
// 1. The 64-row mode (I > 16): the block, the LDS tiles, the prefetch of K, V and the bias a tile ahead, the two barriers per
//    tile and the ballot-guarded correction are attention_stable_f32_kernel's; the tile rules are its CAUSAL ones through the
//    same helpers: interior tiles take the unmasked path, a cut tile (causal_tile_cut) takes the lane-local select on lim[r],
//    and a wave whose 16 rows all lie above a cut tile skips that tile's products after the barriers.  In a piece that does
//    not start at key tile 0 such a wave may skip every tile: its m stays -Inf, L = 0 and O = 0, and the combine gives the
//    piece the weight expf(-Inf - M) = 0 for those rows.  The epilogue is chosen block-uniformly by P_t.
//
// 2. The 16-row mode (I <= 16) is attention_split16_f32_kernel's design (attention_split_f32.hip has the bank arithmetic of
//    the [16][20] E rows and of the merge): the four waves hold the same 16 rows, wave w takes keys 16 w .. 16 w + 15 of each
//    tile, and the waves merge through the freed K and V tiles.  The one row tile sees every visible key, so its pieces cut
//    [0, nv).  The select is per lane: key j0 + 16 w + c against row 4 g + r, j <= row + offset and j < the visible keys.  A
//    wave whose first key is at or beyond the visible keys skips its products (wave-uniform, after the barriers) and merges
//    with m = -Inf, L = 0, O = 0.  Every piece goes through the workspace, also a row tile's only one.
//
// The subtrahend rule is the split's: a maximum still at -Inf subtracts 0.  The special rows are eg_attention_causal's.
// 36 partial kernels (KP x DP x BIAS x mode) and 3 combine kernels, none with scratch: profiles/attention_causal_split.txt.
#include "attention.hpp"        // the internal entries
#include "attention_tile.hpp"   // kernel operands, tiles, the MFMA loops, row_max16, the launcher

#include <cmath>

namespace {

using eg::gemm::f32x4;
using namespace eg::attention;

struct CausalSplitArgs {
  In q, k, v;
  Out o, st;           // the direct epilogue's; st.p may be NULL
  float* ws;           // the workspace
  long stats_offset;   // floats from ws to the maxima and sums
  long I, J, offset;
  int K, D;
  float scale;
  int accumulate;
  CausalPieces pieces;
  long slots;          // partials of an item
  Items items;         // tiles: the pieces of an item
};

struct CausalSplitBiasArgs : CausalSplitArgs {
  In b;
};

// The block's item, its piece, and the piece's place in the workspace.
struct PieceBlock {
  BlockItem b;
  CausalPiece pc;
  float* o;         // row 0 of the partial: [R][DP]
  float* m;         // its maxima; the sums R floats on
};

template <int DP, int R>
__device__ __forceinline__ PieceBlock piece_block(const CausalSplitArgs& a) {
  PieceBlock s;
  s.b = block_item(a.items);
  s.pc = causal_piece_decode(a.pieces, s.b.tile);
  const long part = ((long)s.b.outer * a.items.batch1 + s.b.inner) * a.slots + s.pc.slot;   // (item, slot)
  s.o = a.ws + part * R * DP;
  s.m = a.ws + a.stats_offset + part * 2 * R;
  return s;
}

// The lane's part of the block's partial: rows row0 + 4 g + r of the partial's R, columns 16 nb + c; `sum` already folded over
// the 16 lanes of a row.  `rows`: those inside the problem.
template <int DP, int R>
__device__ __forceinline__ void store_piece(const PieceBlock& s, long rows, int row0, int c, int g, const f32x4 (&o)[DP / 16], const float (&m)[4],
                                            const float (&sum)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + 4 * g + r;
    if (row >= rows) continue;
    if (c == 0) {
      s.m[row] = m[r];
      s.m[R + row] = sum[r];
    }
#pragma unroll
    for (int nb = 0; nb < DP / 16; ++nb) s.o[(long)row * DP + nb * 16 + c] = o[nb][r];
  }
}

__device__ __forceinline__ void fold_sums(float (&sum)[4]) {
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
__global__ __launch_bounds__(THREADS) void attention_causal_split64_f32_kernel(std::conditional_t<BIAS, CausalSplitBiasArgs, CausalSplitArgs> a) {
  constexpr int KS = KP + 4, VS = DP + 16;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const Ks = lds;                      // [64][KS]; the Q tile first
  float* const Vs = Ks + TILE_J * KS;         // [64][VS]
  float* const Es = Vs + TILE_J * VS;         // [4][16][ES]

  const PieceBlock pb = piece_block<DP, TILE_I>(a);
  const BlockItem b = pb.b;
  const long i0 = pb.pc.tile * TILE_I;
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
  // the keys that are loaded; the piece's tiles [t0, t1) are never empty and all below causal_key_tiles(i0, offset, keys)
  const long keys = causal_visible_keys(a.I, a.offset, a.J);
  const long t0 = pb.pc.t0, t1 = pb.pc.t1;
  {
    const long j0 = t0 * TILE_J;
    load_rows<KP>(tk, Kk + j0 * ldk, ldk, keys - j0, a.K, a.k.vec != 0, tid);
    load_rows<DP>(tv, V + j0 * ldv, ldv, keys - j0, a.D, a.v.vec != 0, tid);
    if constexpr (BIAS) load_bias(bias_next, Bl + j0, ldb, bias_rows, keys - j0 - c);
  }
  for (long t = t0; t < t1; ++t) {
    const long j0 = t * TILE_J;
    __syncthreads();   // every wave is done with the tiles in LDS (the first time: with the Q tile)
    store_rows<KP, KS>(tk, Ks, tid);
    store_rows<DP, VS>(tv, Vs, tid);
    __syncthreads();
    if constexpr (BIAS) bias = bias_next;
    if (t + 1 < t1) {   // in flight during this tile's MFMAs
      load_rows<KP>(tk, Kk + (j0 + TILE_J) * ldk, ldk, keys - j0 - TILE_J, a.K, a.k.vec != 0, tid);
      load_rows<DP>(tv, V + (j0 + TILE_J) * ldv, ldv, keys - j0 - TILE_J, a.D, a.v.vec != 0, tid);
      if constexpr (BIAS) load_bias(bias_next, Bl + j0 + TILE_J, ldb, bias_rows, keys - j0 - TILE_J - c);
    }

    // the lane's last visible key of this tile for each of its four rows, relative to j0
    int lim[4];
    {
      const long left = a.J - 1 - j0;   // >= 0: j0 < keys <= J
      const int in_problem = left < TILE_J - 1 ? (int)left : TILE_J - 1;
      // row i0 against key j0: above -64 on a visited tile and below 63 on a cut one
      const int d0 = causal_tile_cut(i0, j0, a.offset, a.J) ? (int)(i0 + a.offset - j0) : 2 * TILE_J;
      if (d0 + __builtin_amdgcn_readfirstlane(w) * 16 + 15 < 0) continue;   // the wave's last row does not see key j0
#pragma unroll
      for (int r = 0; r < 4; ++r) lim[r] = min(in_problem, d0 + w * 16 + 4 * g + r);
    }

    f32x4 s[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) s[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    mma_nt<KP, KS>(q, Ks, c, g, s);

#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x = s[nb][r] * a.scale;
        if constexpr (BIAS) x = x + bias.x[nb][r];
        s[nb][r] = nb * 16 + c <= lim[r] ? x : -INFINITY;
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
    wave_sync();   // the wave's E rows are read before its next tile overwrites them
  }

  fold_sums(sum);
  if (pb.pc.pieces > 1) {   // block-uniform
    store_piece<DP, TILE_I>(pb, a.I - i0, w * 16, c, g, o, m, sum);
    return;
  }
  // the row tile's only piece: the epilogue of attention_stable_f32_kernel (J > 0 here)
  if (a.st.p) {
    float* const St = item_base(a.st, b.outer, b.inner);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long row = i0 + w * 16 + 4 * g + r;
      if (c == 0 && row < a.I) {
        St[row] = m[r];
        St[a.st.v.ld + row] = sum[r];
      }
    }
  }
  float* const O = item_base(a.o, b.outer, b.inner);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long row = i0 + w * 16 + 4 * g + r;
    if (row >= a.I) continue;
#pragma unroll
    for (int nb = 0; nb < DP / 16; ++nb) {
      const int col = nb * 16 + c;
      if (col >= a.D) continue;
      const float v = o[nb][r] / sum[r];
      float* const p = O + row * a.o.v.ld + col;
      *p = a.accumulate ? *p + v : v;
    }
  }
}

// ---- 2. the 16-row mode ---------------------------------------------------------------------------------------------------
template <int KP, int DP, bool BIAS>
__global__ __launch_bounds__(THREADS) void attention_causal_split16_f32_kernel(std::conditional_t<BIAS, CausalSplitBiasArgs, CausalSplitArgs> a) {
  constexpr int KS = KP + 4, VS = DP + 16, E16 = SPLIT_ES16;
  constexpr int CHUNKS = DP / 16 + 2;   // 16-byte chunks a lane leaves for the merge: o[DP / 16], m, sum
  static_assert(3 * CHUNKS * 64 * 4 <= TILE_J * KS + TILE_J * VS, "the merge fits the K and V tiles");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const Ks = lds;                      // [64][KS]; the Q tile first; the merge last
  float* const Vs = Ks + TILE_J * KS;         // [64][VS]
  float* const Es = Vs + TILE_J * VS;         // [4][16][E16]

  const PieceBlock pb = piece_block<DP, SPLIT_ROWS16>(a);
  const BlockItem b = pb.b;
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

  const long keys = causal_visible_keys(a.I, a.offset, a.J);   // I + offset or J: every key of every piece's tiles below it is seen by row I - 1
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
    const bool key = j0 + 16 * w + c < keys;
#pragma unroll
    for (int r = 0; r < 4; ++r) t[r] = (key && 4 * g + r < a.I) ? Bl[r * ldb + j0] : 0.f;
  };
  const long t0 = pb.pc.t0, t1 = pb.pc.t1;
  {
    const long j0 = t0 * TILE_J;
    load_rows<KP>(tk, Kk + j0 * ldk, ldk, keys - j0, a.K, a.k.vec != 0, tid);
    load_rows<DP>(tv, V + j0 * ldv, ldv, keys - j0, a.D, a.v.vec != 0, tid);
    if constexpr (BIAS) load_bias16(bias_next, j0);
  }
  const float* const pk = Ks + (16 * w + c) * KS + g;   // the wave's keys as B operands of the scores
  const float* const pe = Ew + c * E16 + g;             // its E rows as A operands
  const float* const pv = Vs + (16 * w + g) * VS + c;   // the same keys' V rows as B operands
  for (long t = t0; t < t1; ++t) {
    const long j0 = t * TILE_J;
    __syncthreads();   // every wave is done with the tiles in LDS (the first time: with the Q tile)
    store_rows<KP, KS>(tk, Ks, tid);
    store_rows<DP, VS>(tv, Vs, tid);
    __syncthreads();
    if constexpr (BIAS) bias = bias_next;
    if (t + 1 < t1) {   // in flight during this tile's MFMAs
      load_rows<KP>(tk, Kk + (j0 + TILE_J) * ldk, ldk, keys - j0 - TILE_J, a.K, a.k.vec != 0, tid);
      load_rows<DP>(tv, V + (j0 + TILE_J) * ldv, ldv, keys - j0 - TILE_J, a.D, a.v.vec != 0, tid);
      if constexpr (BIAS) load_bias16(bias_next, j0 + TILE_J);
    }

    // the lane's key of this tile against its four rows: row 4 g + r sees it iff key <= 4 g + r + offset and key < keys
    const long first = j0 + 16 * __builtin_amdgcn_readfirstlane(w);
    if (first >= keys) continue;   // no row sees any of the wave's 16 keys: every term would be expf(-Inf) = 0
    const long key = first + c;

    f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KP / 4; ++kk) s = __builtin_amdgcn_mfma_f32_16x16x4f32(q[kk], pk[4 * kk], s, 0, 0, 0);

    float m_new[4], sub[4];
    bool raised = false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float x = s[r] * a.scale;
      if constexpr (BIAS) x = x + bias[r];
      s[r] = (key < keys && key - 4 * g - a.offset <= r) ? x : -INFINITY;
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

  fold_sums(sum);
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
  store_piece<DP, SPLIT_ROWS16>(pb, a.I, 0, c, g, o, m, sum);
}

// ---- 3. the combine kernel ------------------------------------------------------------------------------------------------
struct CausalCombineArgs {
  const float* ws;
  long stats_offset;
  Out o, st;        // st.p may be NULL
  long I, rows;     // rows: items * rows_per_item
  long rows_per_item;   // R * the cut row tiles
  long first_cut, slots, before_cut;   // before_cut: the pieces of the row tiles before the first cut one
  CausalPieces pieces;
  int D;
  unsigned batch1;
  int accumulate;
};

// A thread owns four columns of one row of a cut row tile: DP / 4 threads read a piece's row of DP floats as consecutive 16-byte
// chunks.  A block has 1024 / DP rows and walks rows gridDim.x * 1024 / DP apart.  The row tile's pieces and its first slot
// come from the functions the partial kernel decoded its block with.  The thread of column 0 stores the row's stats.
template <int DP, int R>
__global__ __launch_bounds__(THREADS) void attention_causal_split_combine_kernel(CausalCombineArgs a) {
  constexpr int TPR = DP / 4, RPB = THREADS / TPR;
  const int col = ((int)threadIdx.x % TPR) * 4;
  for (long row_all = (long)blockIdx.x * RPB + (int)threadIdx.x / TPR; row_all < a.rows; row_all += (long)gridDim.x * RPB) {
    const long item = row_all / a.rows_per_item, rest = row_all - item * a.rows_per_item;
    const long tile = a.first_cut + rest / R;
    const int in_tile = (int)(rest % R);
    const long row = tile * R + in_tile;
    if (row >= a.I) continue;
    const int pieces = (int)causal_piece_count(causal_row_key_tiles(a.pieces, tile), a.pieces.chunk);
    const long slot = item * a.slots + causal_pieces_before(a.pieces, tile) - a.before_cut;
    const float* const ms = a.ws + a.stats_offset + slot * 2 * R + in_tile;   // piece p: 2 R floats on
    const float* const os = a.ws + (slot * R + in_tile) * DP + col;           // piece p: R DP floats on
    float top = -INFINITY;
    for (int p = 0; p < pieces; ++p) top = fmaxf(top, ms[(long)p * 2 * R]);
    const float sub = top == -INFINITY ? 0.f : top;
    float total = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < pieces; ++p) {
      const float wt = expf(ms[(long)p * 2 * R] - sub);
      total += wt * ms[(long)p * 2 * R + R];
      acc += *reinterpret_cast<const f32x4*>(os + (long)p * R * DP) * wt;
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
int launch(eg_ctx* ctx, unsigned grid, const CausalSplitPlan& p, const Args& args) {
  const int rc = dynamic_lds_once<KERNEL>(ctx, {p.lds_bytes});
  if (rc) return rc;
  hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(p.block), (size_t)p.lds_bytes, ctx->stream, args);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}

template <int DP>
int launch_combine(eg_ctx* ctx, const CausalSplitPlan& p, const CausalCombineArgs& args) {
  if (p.rows16)
    hipLaunchKernelGGL((attention_causal_split_combine_kernel<DP, SPLIT_ROWS16>), dim3((unsigned)p.combine_grid), dim3(p.block), 0, ctx->stream, args);
  else
    hipLaunchKernelGGL((attention_causal_split_combine_kernel<DP, TILE_I>), dim3((unsigned)p.combine_grid), dim3(p.block), 0, ctx->stream, args);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}

}  // namespace

namespace eg {
namespace attention {

int attention_causal_split(eg_ctx* ctx, const Extents& e, float scale, const float* Q, View q, const float* Kk, View k, const float* V, View v,
                           float* O, View o, int accumulate, float* Stats, View st, const float* Bias, View bv, long offset, int chunk) {
  const char* const name = "eg_attention_causal_split";
  EG_REQUIRE(offset >= 0, EG_ERR_INVALID, "%s: offset is negative: the first rows would see no key", name);
  EG_REQUIRE(chunk >= 0, EG_ERR_INVALID, "%s: chunk = %d is negative", name, chunk);
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
  offset = offset < e.J ? offset : e.J;   // an offset of J - 1 or more masks nothing
  const CausalSplitPlan p = plan_attention_causal_split(pr, offset, chunk);
  EG_REQUIRE(p.supported, EG_ERR_UNSUPPORTED, "%s: %s", name, p.reason);
  if (p.forward) return attention_stable(ctx, e, scale, Q, q, Kk, k, V, v, O, o, accumulate, Stats, st, Bias, bv, name, offset);

  rc = eg::set_device(ctx);
  if (rc) return rc;
  rc = eg::ensure_workspace(ctx, (size_t)p.workspace_bytes);
  if (rc) return rc;
  float* const ws = static_cast<float*>(ctx->workspace);

  CausalSplitBiasArgs args = {};
  args.q = {Q, q, p.base.vec_q}, args.k = {Kk, k, p.base.vec_k}, args.v = {V, v, p.base.vec_v}, args.b = {Bias, bv, p.base.vec_b};
  args.o = {O, o, 0}, args.st = {Stats, st, 0};
  args.ws = ws, args.stats_offset = p.stats_offset;
  args.I = e.I, args.J = e.J, args.offset = offset, args.K = (int)e.K, args.D = (int)e.D;
  args.scale = scale;
  args.accumulate = accumulate;
  args.pieces = p.pieces, args.slots = p.slots;
  // 36 kernels: the padded K x the padded D, with and without a bias, in either mode
  rc = for_each_launch(name, p.base.items, p.partial, e.batch1, [&](const Items& items, unsigned grid) {
    args.items = items;
    return dispatch_heads(p.base.kp, p.base.dp, [&](auto KP, auto DP) {
      constexpr int kp = KP(), dp = DP();
      if (p.rows16)
        return Bias ? launch<&attention_causal_split16_f32_kernel<kp, dp, true>, CausalSplitBiasArgs>(ctx, grid, p, args)
                    : launch<&attention_causal_split16_f32_kernel<kp, dp, false>, CausalSplitArgs>(ctx, grid, p, args);
      return Bias ? launch<&attention_causal_split64_f32_kernel<kp, dp, true>, CausalSplitBiasArgs>(ctx, grid, p, args)
                  : launch<&attention_causal_split64_f32_kernel<kp, dp, false>, CausalSplitArgs>(ctx, grid, p, args);
    });
  });
  if (rc) return rc;

  CausalCombineArgs ca = {};
  ca.ws = ws, ca.stats_offset = p.stats_offset;
  ca.o = {O, o, 0}, ca.st = {Stats, st, 0};
  ca.I = e.I, ca.rows = p.combine_rows, ca.rows_per_item = p.combine_rows_per_item;
  ca.first_cut = p.first_cut, ca.slots = p.slots, ca.before_cut = p.pieces_per_item - p.slots;
  ca.pieces = p.pieces;
  ca.D = (int)e.D;
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

extern "C" int eg_attention_causal_split(eg_ctx* ctx, int64_t batch0, int64_t batch1, int64_t I, int64_t J, int64_t K, int64_t D, float scale,
                                         const float* Q, int64_t ldq, int64_t stride_q0, int64_t stride_q1, const float* Kk, int64_t ldk,
                                         int64_t stride_k0, int64_t stride_k1, const float* V, int64_t ldv, int64_t stride_v0, int64_t stride_v1,
                                         float* O, int64_t ldo, int64_t stride_o0, int64_t stride_o1, int accumulate, float* Stats, int64_t lds,
                                         int64_t stride_s0, int64_t stride_s1, const float* Bias, int64_t ldb, int64_t stride_b0, int64_t stride_b1,
                                         int64_t offset, int chunk) {
  return eg::attention::attention_causal_split(ctx, {batch0, batch1, I, J, K, D}, scale, Q, {ldq, stride_q0, stride_q1}, Kk, {ldk, stride_k0, stride_k1},
                                               V, {ldv, stride_v0, stride_v1}, O, {ldo, stride_o0, stride_o1}, accumulate, Stats,
                                               {lds, stride_s0, stride_s1}, Bias, {ldb, stride_b0, stride_b1}, offset, chunk);
}
