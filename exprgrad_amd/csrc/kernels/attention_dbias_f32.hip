// The gradient of the attention score bias, exact f32 on the matrix cores.  Per item, with the quantities of
// attention_grad_f32.hip (p_ij = expf(scale * s_ij + bias_ij) / L_i, dP_ij = dO_i . v_j, delta_i = dO_i . o_i),
//   g_ij = p_ij * (dP_ij - delta_i)                      dS without the factor scale
//   dBias[o * sdb0 + i1 * sdb1 + i * lddb + j] (+)= sum of g_ij(o, i1) over every index whose step in dBias is 0.
// The bias of a model is broadcast (a table per head, a slope, a key mask), so its gradient is a sum over batch0, batch1
// and/or the query rows.  No atomics and no workspace: the sum is taken inside a block.
//
// Work split.  An output cell is a pair (o', i1') of the batch indices that dBias steps over; the cells are the items of the
// item grid.  One block owns one 64 x 64 tile of one cell (row tile ti, key tile tj; block_item's tile = ti * tiles_j + tj), a
// wave 16 of its rows in accumulator layout: lane (c, g), element (nb, r) = row 4 g + r of the wave's, key 16 nb + c.  With
// FOLD (lddb == 0, a compile-time flag) the query rows are summed too: a cell has tiles_j blocks and each walks every row
// tile.  The block's loop, one pass per (item, row tile), in this order and no other:
//   for x in [0, sum0)            o  = cell's o'  + x     (sum0 = batch0 where sdb0 == 0, else 1)
//     for y in [0, sum1)          i1 = cell's i1' + y     (sum1 = batch1 where sdb1 == 0, else 1)
//       for t in row tiles        FOLD: every row tile, ascending; otherwise the block's own
// Per pass the Q tile, K tile, dO tile and V tile go to LDS (all four read NT only: rows of width + 4 floats), the wave reads
// its Q rows and dO rows back as A operands, 1 / L and delta of the 64 rows come from the functions of the other two backward
// kernels (same bits), and
//   S = Q_rows * K_tile^T, dP = dO_rows * V_tile^T       4 + 4 accumulators, the NT loop of the forward;
//   acc += p * (dP - delta)                              16 running sums per lane, in registers across the whole loop; rows
//                                                        i >= I and keys j >= J add nothing, by a select, and are never read.
// The bias tile.  Every item a block visits has the same bias tile: the entry requires the steps of dBias to be 0 exactly
// where those of Bias are, so the indices the block sums over are the indices the bias does not depend on.  It is loaded once,
// before the loop, straight into accumulator layout (load_bias): no LDS.
// Prefetch.  With dbias_ahead(KP, DP) (attention_plan.hpp) the next pass's four tiles, O parts and row sums are loaded into
// registers during this pass's MFMAs; without it they are loaded at the top of the pass.
// Epilogue.  Without FOLD the accumulators go through LDS (stage_acc) and leave as whole rows, 16-byte stores where the plan's
// vec_db allows them; accumulating loads first.  With FOLD each of the lane's four columns is folded in this order: the lane's
// four r ascending; the four g by xor-shuffles of 16 and 32, which is (g0 + g1) + (g2 + g3); the four waves through LDS,
// ascending.  Threads 0 .. 63 then store the 64 floats.  Every sum has one order: two calls give the same bits.
#include "gemm_plan.hpp"             // batched2_c_distinct
#include "attention.hpp"             // the internal entry
#include "attention_tile.hpp"        // kernel operands, tiles, the bias tile, the MFMA loops, the launcher
#include "attention_grad_tile.hpp"   // O parts, delta, 1 / L, the accumulators' way out

#include <algorithm>
#include <cmath>

namespace {

using eg::gemm::f32x4;
using namespace eg::attention;

struct DbiasArgs {
  In q, k, v, o, s, dout, b;
  Out db;
  long I, J;
  int K, D;
  float scale;
  int accumulate;
  unsigned sum0, sum1;    // items the block adds along batch0 and batch1; sum0 == 0: no pass, the sums are zeros
  int tiles_i, tiles_j;   // row tiles and key tiles of a cell
  Items items;            // the cells of the launch
};

constexpr int TILE = 64;

template <int KP, int DP, bool FOLD>
__global__ __launch_bounds__(THREADS) void attention_dbias_kernel(DbiasArgs a) {
  constexpr bool AHEAD = dbias_ahead(KP, DP);
  constexpr int KS = KP + GRAD_PAD_NT, VS = DP + GRAD_PAD_NT;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const Qs = lds;                  // [64][KS]; with Ks the epilogue's [64][ES] or [4][64]
  float* const Ks = Qs + TILE * KS;       // [64][KS]
  float* const Ds = Ks + TILE * KS;       // [64][VS]: the dO tile
  float* const Vs = Ds + TILE * VS;       // [64][VS]
  float* const St = Vs + TILE * VS;       // [64][2]: 1 / L, delta

  const BlockItem b = block_item(a.items);
  const int tj = FOLD ? b.tile : b.tile % a.tiles_j;
  const int ti = FOLD ? 0 : b.tile / a.tiles_j;
  const long j0 = (long)tj * TILE;
  const long keys = a.J - j0;
  const int row_tiles = FOLD ? a.tiles_i : 1;
  const long passes = (long)a.sum0 * a.sum1 * row_tiles;
  const long ldq = a.q.v.ld, ldk = a.k.v.ld, ldv = a.v.v.ld, ldo = a.o.v.ld, lddo = a.dout.v.ld;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;

  // the one bias tile of every pass: rows 4 g + r of the wave's, keys c + 16 nb; with FOLD the cell's one row.  Without a
  // pass the bias has no element to read.
  BiasTile bias;
  {
    const long ldb = a.b.v.ld;
    const long row0 = (long)ti * TILE + w * 16 + 4 * g;
    const float* const Bl = item_base(a.b, b.outer, b.inner) + row0 * ldb + j0 + c;
    load_bias(bias, Bl, ldb, passes == 0 ? 0 : FOLD ? 4 : a.I - row0, keys - c);
  }

  TileRegs<KP> tq, tk;
  TileRegs<DP> td, tv;
  OPart<DP> po;
  f32x4 sums = {1.f, 1.f, 1.f, 1.f};
  // the tiles of one pass: item (o, i1), row tile t, the block's key tile
  auto load_pass = [&](unsigned o, unsigned i1, int t) {
    const long i0 = (long)t * TILE, rows = a.I - i0;
    load_rows<KP>(tq, item_base(a.q, o, i1) + i0 * ldq, ldq, rows, a.K, a.q.vec != 0, tid);
    load_rows<KP>(tk, item_base(a.k, o, i1) + j0 * ldk, ldk, keys, a.K, a.k.vec != 0, tid);
    load_rows<DP>(td, item_base(a.dout, o, i1) + i0 * lddo, lddo, rows, a.D, a.dout.vec != 0, tid);
    load_rows<DP>(tv, item_base(a.v, o, i1) + j0 * ldv, ldv, keys, a.D, a.v.vec != 0, tid);
    load_o_part<DP>(po, item_base(a.o, o, i1) + i0 * ldo, ldo, rows, a.D, a.o.vec != 0, tid);
    sums = load_sums(item_base(a.s, o, i1) + i0, rows, a.s.vec != 0, tid);
  };

  f32x4 acc[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  unsigned x = 0, y = 0;
  int t = ti;
  if (AHEAD && passes > 0) load_pass(b.outer, b.inner, t);
  for (long n = 0; n < passes; ++n) {
    const long rows = a.I - (long)t * TILE;
    if (!AHEAD) load_pass(b.outer + x, b.inner + y, t);
    __syncthreads();   // every wave is done with the tiles in LDS
    store_rows<KP, KS>(tq, Qs, tid);
    store_rows<KP, KS>(tk, Ks, tid);
    store_rows<DP, VS>(td, Ds, tid);
    store_rows<DP, VS>(tv, Vs, tid);
    store_inverse_sums(sums, St, rows, tid);
    __syncthreads();
    {
      const float d = row_delta<DP>(Ds, VS, po, tid);
      if ((tid & 3) == 0) St[2 * (tid >> 2) + 1] = d;
    }
    float q[KP / 4], dout[DP / 4];
    read_a_rows<KP, KS>(Qs, w, c, g, q);
    read_a_rows<DP, VS>(Ds, w, c, g, dout);
    // the next pass, in the documented order
    if (!FOLD || ++t == row_tiles) {
      if (FOLD) t = 0;
      if (++y == a.sum1) y = 0, ++x;
    }
    if (AHEAD && n + 1 < passes) load_pass(b.outer + x, b.inner + y, t);   // in flight during this pass's MFMAs
    __syncthreads();   // delta of every row is in St

    float inv[4], delta[4];
    bool rlive[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      inv[r] = St[2 * (w * 16 + 4 * g + r)];
      delta[r] = St[2 * (w * 16 + 4 * g + r) + 1];
      rlive[r] = w * 16 + 4 * g + r < rows;
    }
    f32x4 s[4], dp[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) s[nb] = dp[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    mma_nt<KP, KS>(q, Ks, c, g, s);
    mma_nt<DP, VS>(dout, Vs, c, g, dp);
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      const bool klive = nb * 16 + c < keys;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float e = s[nb][r] * a.scale;
        e = e + bias.x[nb][r];
        const float p = expf(e) * inv[r];
        const float gij = p * (dp[nb][r] - delta[r]);
        acc[nb][r] += (klive && rlive[r]) ? gij : 0.f;   // a select: a row or a key outside the problem adds exactly 0
      }
    }
  }

  __syncthreads();   // every wave is done with the tiles
  float* const dB = item_base(a.db, b.outer, b.inner);
  if constexpr (FOLD) {
    float* const F = lds;   // [4 waves][64 keys]
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      float v = ((acc[nb][0] + acc[nb][1]) + acc[nb][2]) + acc[nb][3];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (g == 0) F[w * TILE + nb * 16 + c] = v;
    }
    __syncthreads();
    if (tid < TILE && tid < keys) {
      const float v = ((F[tid] + F[TILE + tid]) + F[2 * TILE + tid]) + F[3 * TILE + tid];
      float* const p = dB + j0 + tid;
      *p = a.accumulate ? *p + v : v;
    }
  } else {
    const long i0 = (long)ti * TILE;
    stage_acc<TILE, ES>(acc, lds, w, c, g);
    __syncthreads();
    store_out<TILE, ES>(lds, dB + i0 * a.db.v.ld + j0, a.db.v.ld, a.I - i0, (int)std::min<long>(keys, TILE), a.db.vec != 0, a.accumulate != 0, tid);
  }
}

template <int KP, int DP>
int launch(eg_ctx* ctx, unsigned grid, const DbiasPlan& p, const DbiasArgs& args) {
  static_assert(2 * TILE * (KP + GRAD_PAD_NT) >= TILE * ES, "the epilogue's staging tile fits the Q and K tiles");
  const int rc = dynamic_lds_once<&attention_dbias_kernel<KP, DP, false>, &attention_dbias_kernel<KP, DP, true>>(
      ctx, {dbias_lds_bytes(KP, DP), dbias_lds_bytes(KP, DP)});
  if (rc) return rc;
  if (p.row_fold)
    hipLaunchKernelGGL((attention_dbias_kernel<KP, DP, true>), dim3(grid), dim3(p.block), (size_t)p.lds_bytes, ctx->stream, args);
  else
    hipLaunchKernelGGL((attention_dbias_kernel<KP, DP, false>), dim3(grid), dim3(p.block), (size_t)p.lds_bytes, ctx->stream, args);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}

}  // namespace

namespace eg {
namespace attention {

int attention_dbias(eg_ctx* ctx, const Extents& e, float scale, const float* Q, View q, const float* Kk, View k, const float* V, View v,
                    const float* O, View o, const float* Sums, View s, const float* dO, View dout, const float* Bias, View bv, float* dBias,
                    View db, int accumulate) {
  const char* const name = "eg_attention_bias_dbias";
  const long batch0 = e.batch0, batch1 = e.batch1, I = e.I, J = e.J, K = e.K, D = e.D;
  EG_REQUIRE(ctx, EG_ERR_INVALID, "%s: ctx is NULL", name);
  EG_REQUIRE(batch0 >= 0 && batch1 >= 0 && I >= 0 && J >= 0 && K >= 0 && D >= 0, EG_ERR_INVALID, "%s: negative extent", name);
  EG_REQUIRE(batch0 < (1L << 31) && batch1 < (1L << 31), EG_ERR_INVALID, "%s: a batch extent of 2^31 or more", name);
  EG_REQUIRE(q.stride0 >= 0 && q.stride1 >= 0 && k.stride0 >= 0 && k.stride1 >= 0 && v.stride0 >= 0 && v.stride1 >= 0 && o.stride0 >= 0 &&
                 o.stride1 >= 0 && s.stride0 >= 0 && s.stride1 >= 0 && dout.stride0 >= 0 && dout.stride1 >= 0,
             EG_ERR_INVALID, "%s: negative stride", name);
  EG_REQUIRE(bv.stride0 >= 0 && bv.stride1 >= 0 && db.stride0 >= 0 && db.stride1 >= 0, EG_ERR_INVALID, "%s: negative stride of Bias or dBias", name);
  EG_REQUIRE(bv.ld == 0 || bv.ld >= J, EG_ERR_INVALID, "%s: ldb is neither 0 nor at least J", name);
  EG_REQUIRE(db.ld == 0 || db.ld >= J, EG_ERR_INVALID, "%s: lddb is neither 0 nor at least J", name);
  EG_REQUIRE((db.ld == 0) == (bv.ld == 0) && (db.stride0 == 0) == (bv.stride0 == 0) && (db.stride1 == 0) == (bv.stride1 == 0), EG_ERR_INVALID,
             "%s: lddb, stride_db0 and stride_db1 must be 0 exactly where ldb, stride_b0 and stride_b1 are", name);
  EG_REQUIRE(accumulate == 0 || accumulate == 1, EG_ERR_INVALID, "%s: accumulate is neither 0 nor 1", name);
  const bool fold = db.ld == 0;
  const long cells0 = db.stride0 ? batch0 : 1, cells1 = db.stride1 ? batch1 : 1;
  if (cells0 == 0 || cells1 == 0 || J == 0 || (I == 0 && !fold)) return EG_OK;   // dBias has no elements
  EG_REQUIRE(Bias && dBias, EG_ERR_INVALID, "%s: NULL operand (Bias or dBias)", name);
  EG_REQUIRE(eg::gemm::batched2_c_distinct(cells0, db.stride0, cells1, db.stride1, fold ? 1 : I, fold ? J : db.ld, J), EG_ERR_INVALID,
             "%s: lddb, stride_db0 and stride_db1 make elements of dBias share an address", name);
  // an empty sum: zeros when not accumulating, nothing otherwise
  const bool empty = I == 0 || D == 0 || batch0 == 0 || batch1 == 0;
  if (!empty) {
    EG_REQUIRE(Sums && V && O && dO, EG_ERR_INVALID, "%s: NULL operand (V, O, Sums or dO)", name);
    EG_REQUIRE(K == 0 || (Q && Kk), EG_ERR_INVALID, "%s: NULL operand (Q or Kk)", name);
  }
  EG_REQUIRE(q.ld >= K && k.ld >= K && v.ld >= D && o.ld >= D && dout.ld >= D, EG_ERR_INVALID, "%s: leading dimension smaller than the row length",
             name);
  EG_REQUIRE(K <= MAX_HEAD, EG_ERR_UNSUPPORTED, "%s: K = %ld is above the limit of %d", name, K, MAX_HEAD);
  EG_REQUIRE(D <= MAX_HEAD, EG_ERR_UNSUPPORTED, "%s: D = %ld is above the limit of %d", name, D, MAX_HEAD);
  if (empty && accumulate) return EG_OK;
  const int rc = eg::set_device(ctx);
  if (rc) return rc;

  DbiasProblem pr;
  static_cast<Extents&>(pr) = e;
  pr.q = {q, aligned16(Q)}, pr.k = {k, aligned16(Kk)}, pr.v = {v, aligned16(V)}, pr.o = {o, aligned16(O)}, pr.s = {s, aligned16(Sums)};
  pr.dout = {dout, aligned16(dO)}, pr.bias = {bv, aligned16(Bias)}, pr.dbias = {db, aligned16(dBias)};
  pr.cus = ctx->compute_units;
  const DbiasPlan p = plan_attention_dbias(pr);
  EG_REQUIRE(p.supported, EG_ERR_UNSUPPORTED, "%s: %s", name, p.reason);

  DbiasArgs args = {};
  args.q = {Q, q, p.vec_q}, args.k = {Kk, k, p.vec_k}, args.v = {V, v, p.vec_v}, args.o = {O, o, p.vec_o}, args.s = {Sums, s, p.vec_s};
  args.dout = {dO, dout, p.vec_do}, args.b = {Bias, bv, 0}, args.db = {dBias, db, p.vec_db};
  args.I = I, args.J = J, args.K = (int)K, args.D = (int)D;
  args.scale = scale;
  args.accumulate = accumulate;
  args.sum0 = empty ? 0 : (unsigned)p.sum0, args.sum1 = (unsigned)p.sum1;
  args.tiles_i = (int)p.tiles_i, args.tiles_j = (int)p.tiles_j;
  // 9 padded K x padded D pairs, each with and without the row fold
  return for_each_launch(name, p.cells, p.cut, p.cells1, [&](const Items& items, unsigned grid) {
    args.items = items;
    return dispatch_heads(p.kp, p.dp, [&](auto KP, auto DP) { return launch<KP(), DP()>(ctx, grid, p, args); });
  });
}

}  // namespace attention
}  // namespace eg

extern "C" int eg_attention_bias_dbias(eg_ctx* ctx, int64_t batch0, int64_t batch1, int64_t I, int64_t J, int64_t K, int64_t D, float scale,
                                       const float* Q, int64_t ldq, int64_t stride_q0, int64_t stride_q1,
                                       const float* Kk, int64_t ldk, int64_t stride_k0, int64_t stride_k1,
                                       const float* V, int64_t ldv, int64_t stride_v0, int64_t stride_v1,
                                       const float* O, int64_t ldo, int64_t stride_o0, int64_t stride_o1,
                                       const float* Sums, int64_t stride_s0, int64_t stride_s1,
                                       const float* dO, int64_t lddo, int64_t stride_do0, int64_t stride_do1,
                                       const float* Bias, int64_t ldb, int64_t stride_b0, int64_t stride_b1,
                                       float* dBias, int64_t lddb, int64_t stride_db0, int64_t stride_db1, int accumulate) {
  return eg::attention::attention_dbias(ctx, {batch0, batch1, I, J, K, D}, scale, Q, {ldq, stride_q0, stride_q1}, Kk, {ldk, stride_k0, stride_k1}, V,
                                        {ldv, stride_v0, stride_v1}, O, {ldo, stride_o0, stride_o1}, Sums, {0, stride_s0, stride_s1}, dO,
                                        {lddo, stride_do0, stride_do1}, Bias, {ldb, stride_b0, stride_b1}, dBias, {lddb, stride_db0, stride_db1},
                                        accumulate);
}
