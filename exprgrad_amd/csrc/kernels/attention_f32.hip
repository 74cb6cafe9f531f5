// Fused attention forward, exact f32 on the matrix cores:
//   O_{o,i1}[i,:] (+)= (sum_j exp(scale * q_i . k_j) * V[j,:]) / (sum_j exp(scale * q_i . k_j))
// for every item (o, i1) of batch0 x batch1, X_{o,i1} = X + o * stride_x0 + i1 * stride_x1 — the scale map and the softmax of
// layers/dnn.nim:90-94 between the two multi-head products, as written, without a row maximum.  Without the maximum the
// sum over the keys is one pass with a running numerator and a running denominator: nothing is rescaled, nothing of size
// I x J is stored, and J is unbounded.
//
// One block owns one item and a tile of 64 query rows; its four waves own 16 whole rows each.  The loop over tiles of 64 keys:
//   stage  K tile [64][K] and V tile [64][D] into LDS (loaded into registers one tile ahead, during the MFMAs of the
//          tile before; rows j >= J and columns k >= K, d >= D are zero-filled, never read);
//   S      = Q_rows * K_tile^T   16 x 64 per wave: four accumulators of v_mfma_f32_16x16x4_f32, Q from registers;
//   e      = expf(S * scale)     one multiplication, then expf, as the generated kernels emit it; keys j >= J are zeroed
//          with a select; e is added into four per-lane row sums and written to the wave's own [16][64] LDS rows
//          (accumulator layout -> A-operand layout: wave-private, no block barrier);
//   O_acc += E * V_tile          16 x D per wave, D / 16 accumulators.
// After the last tile the row sums are folded across the 16 lanes that share a row (xor shuffles 1, 2, 4, 8: a fixed
// order), the accumulators divided, and the rows stored.  No atomics, no workspace, one launch per 2^22 blocks: two runs
// give the same bits.
//
// Operand conventions of the 16x16x4 instruction (gemm_f32_mfma.hpp uses the 32x32x2 form of the same maps): lane l gives
// A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; it receives D[row 4 * (l >> 4) + r][col l & 15] in element r.
// LDS row strides make every operand read and the E write conflict-free over the 64 banks: K rows of KP + 4 floats
// (16 keys x 4 k), V rows of DP + 16 (4 keys x 16 columns), E rows of 68 (rows 4g + r: 16g + 4r + c + 16 nb).
#include "gemm_plan.hpp"        // batched2_c_distinct
#include "attention.hpp"        // the internal entry
#include "attention_tile.hpp"   // kernel operands, tiles, the MFMA loops, the launcher

#include <cmath>

namespace {

using eg::gemm::f32x4;
using namespace eg::attention;

struct AttnArgs {
  In q, k, v;
  Out o;
  Out s;   // eg_attention_sums: the row sums, I floats per item (SUMS instantiations only)
  long I, J;
  int K, D;
  float scale;
  int accumulate;
  Items items;
};

// SUMS: also store each row's denominator (eg_attention_sums); a compile-time flag, so that eg_attention's kernels are the
// ones they were.
template <int KP, int DP, bool SUMS>
__global__ __launch_bounds__(THREADS) void attention_f32_kernel(AttnArgs a) {
  constexpr int KS = KP + 4, VS = DP + 16;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const Ks = lds;                      // [64][KS]; the Q tile first
  float* const Vs = Ks + TILE_J * KS;         // [64][VS]
  float* const Es = Vs + TILE_J * VS;         // [4][16][ES]

  const BlockItem b = block_item(a.items);
  const long i0 = (long)b.tile * TILE_I;
  const long ldq = a.q.v.ld, ldk = a.k.v.ld, ldv = a.v.v.ld;
  const float* const Q = item_base(a.q, b.outer, b.inner) + i0 * ldq;
  const float* const Kk = item_base(a.k, b.outer, b.inner);
  const float* const V = item_base(a.v, b.outer, b.inner);
  float* const O = item_base(a.o, b.outer, b.inner);

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  float* const Ew = Es + w * 16 * ES;

  // Q rows of the wave as A operands of every k step, for the whole loop
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

  TileRegs<KP> tk;
  TileRegs<DP> tv;
  const long nt = (a.J + TILE_J - 1) / TILE_J;
  if (nt > 0) {
    load_rows<KP>(tk, Kk, ldk, a.J, a.K, a.k.vec != 0, tid);
    load_rows<DP>(tv, V, ldv, a.J, a.D, a.v.vec != 0, tid);
  }
  for (long t = 0; t < nt; ++t) {
    const long j0 = t * TILE_J;
    __syncthreads();   // every wave is done with the tiles in LDS (the first time: with the Q tile)
    store_rows<KP, KS>(tk, Ks, tid);
    store_rows<DP, VS>(tv, Vs, tid);
    __syncthreads();
    if (t + 1 < nt) {   // in flight during this tile's MFMAs
      load_rows<KP>(tk, Kk + (j0 + TILE_J) * ldk, ldk, a.J - j0 - TILE_J, a.K, a.k.vec != 0, tid);
      load_rows<DP>(tv, V + (j0 + TILE_J) * ldv, ldv, a.J - j0 - TILE_J, a.D, a.v.vec != 0, tid);
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
        const float x = s[nb][r] * a.scale;
        float e = expf(x);
        e = live ? e : 0.f;   // a select: a key outside the problem adds exactly 0, whatever its score
        sum[r] += e;
        Ew[(4 * g + r) * ES + nb * 16 + c] = e;
      }
    }
    wave_sync();

    mma_nn<DP, VS, ES>(Ew, Vs, c, g, o);
    wave_sync();   // the wave's E rows are read before its next tile overwrites them
  }

  // Row sums: the 16 lanes of a group hold the columns = c (mod 16) of rows 4g + r.  A sum that overflowed is NaN, not
  // Inf: a row is NaN whenever its denominator is not finite (the header has the one case where the program differs).
  const bool empty = a.J == 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float t = sum[r];
    t += __shfl_xor(t, 1);
    t += __shfl_xor(t, 2);
    t += __shfl_xor(t, 4);
    t += __shfl_xor(t, 8);
    sum[r] = t == INFINITY ? NAN : t;
  }
  if constexpr (SUMS) {
    // the value row i is divided by, from the lane that holds column 0 of its group's rows; 0 when there are no keys
    float* const S = item_base(a.s, b.outer, b.inner);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long row = i0 + w * 16 + 4 * g + r;
      if (c == 0 && row < a.I) S[row] = sum[r];
    }
    if (empty && a.accumulate) return;   // an empty sum adds nothing to O
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long row = i0 + w * 16 + 4 * g + r;
    if (row >= a.I) continue;
#pragma unroll
    for (int nb = 0; nb < DP / 16; ++nb) {
      const int col = nb * 16 + c;
      if (col >= a.D) continue;
      const float v = empty ? 0.f : o[nb][r] / sum[r];
      float* const p = O + row * a.o.v.ld + col;
      *p = a.accumulate ? *p + v : v;
    }
  }
}

template <int KP, int DP, bool SUMS>
int launch(eg_ctx* ctx, unsigned grid, const Plan& p, const AttnArgs& args) {
  const int rc = dynamic_lds_once<&attention_f32_kernel<KP, DP, SUMS>>(ctx, {lds_bytes_for(KP, DP)});
  if (rc) return rc;
  hipLaunchKernelGGL((attention_f32_kernel<KP, DP, SUMS>), dim3(grid), dim3(p.block), (size_t)p.lds_bytes, ctx->stream, args);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}

}  // namespace

namespace eg {
namespace attention {

// The one launcher: eg_attention and the model layer's attention launches (host/run.cpp) come here with Sums == NULL,
// eg_attention_sums and a fit group's forward launch with the row sums' view.
int attention_forward(eg_ctx* ctx, const Extents& e, float scale, const float* Q, View q, const float* Kk, View k, const float* V, View v, float* O,
                      View o, int accumulate, float* Sums, View s) {
  const char* const name = Sums ? "eg_attention_sums" : "eg_attention";   // the entry the messages speak of
  const long batch0 = e.batch0, batch1 = e.batch1, I = e.I, J = e.J, K = e.K, D = e.D;
  EG_REQUIRE(ctx, EG_ERR_INVALID, "%s: ctx is NULL", name);
  EG_REQUIRE(batch0 >= 0 && batch1 >= 0 && I >= 0 && J >= 0 && K >= 0 && D >= 0, EG_ERR_INVALID, "%s: negative extent", name);
  EG_REQUIRE(batch0 < (1L << 31) && batch1 < (1L << 31), EG_ERR_INVALID, "%s: a batch extent of 2^31 or more", name);
  EG_REQUIRE(q.stride0 >= 0 && q.stride1 >= 0 && k.stride0 >= 0 && k.stride1 >= 0 && v.stride0 >= 0 && v.stride1 >= 0, EG_ERR_INVALID,
             "%s: negative stride", name);
  if (batch0 == 0 || batch1 == 0 || I == 0 || (D == 0 && !Sums)) return EG_OK;
  EG_REQUIRE(D == 0 || O, EG_ERR_INVALID, "%s: O is NULL", name);
  EG_REQUIRE(J == 0 || D == 0 || V, EG_ERR_INVALID, "%s: NULL operand", name);
  EG_REQUIRE(J == 0 || K == 0 || (Q && Kk), EG_ERR_INVALID, "%s: NULL operand", name);
  EG_REQUIRE(q.ld >= K && k.ld >= K && v.ld >= D, EG_ERR_INVALID, "%s: leading dimension smaller than the row length", name);
  EG_REQUIRE(D == 0 || eg::gemm::batched2_c_distinct(batch0, o.stride0, batch1, o.stride1, I, o.ld, D), EG_ERR_INVALID,
             "%s: ldo, stride_o0 and stride_o1 make elements of O share an address", name);
  // the row sums: one row of I columns per item
  EG_REQUIRE(!Sums || eg::gemm::batched2_c_distinct(batch0, s.stride0, batch1, s.stride1, 1, I, I), EG_ERR_INVALID,
             "%s: stride_s0 and stride_s1 make elements of Sums share an address", name);
  EG_REQUIRE(K <= MAX_HEAD, EG_ERR_UNSUPPORTED, "%s: K = %ld is above the limit of %d", name, K, MAX_HEAD);
  EG_REQUIRE(D <= MAX_HEAD, EG_ERR_UNSUPPORTED, "%s: D = %ld is above the limit of %d", name, D, MAX_HEAD);
  if (J == 0 && accumulate && !Sums) return EG_OK;   // an empty sum adds nothing
  const int rc = eg::set_device(ctx);
  if (rc) return rc;

  Problem pr;
  static_cast<Extents&>(pr) = e;
  pr.q = {q, aligned16(Q)}, pr.k = {k, aligned16(Kk)}, pr.v = {v, aligned16(V)}, pr.o = {o, aligned16(O)};
  pr.sums = Sums != nullptr;
  pr.cus = ctx->compute_units;
  const Plan p = plan_attention(pr);
  EG_REQUIRE(p.supported, EG_ERR_UNSUPPORTED, "%s: %s", name, p.reason);

  AttnArgs args = {};
  args.q = {Q, q, p.vec_q}, args.k = {Kk, k, p.vec_k}, args.v = {V, v, p.vec_v};
  args.o = {O, o, 0}, args.s = {Sums, s, 0};
  args.I = I, args.J = J, args.K = (int)K, args.D = (int)D;
  args.scale = scale;
  args.accumulate = accumulate;
  // 9 kernels: the padded K x the padded D; 9 more that store the row sums
  return for_each_launch(name, p.items, p.cut(), batch1, [&](const Items& items, unsigned grid) {
    args.items = items;
    return dispatch_heads(p.kp, p.dp, [&](auto KP, auto DP) {
      return Sums ? launch<KP(), DP(), true>(ctx, grid, p, args) : launch<KP(), DP(), false>(ctx, grid, p, args);
    });
  });
}

}  // namespace attention
}  // namespace eg

extern "C" int eg_attention(eg_ctx* ctx, int64_t batch0, int64_t batch1, int64_t I, int64_t J, int64_t K, int64_t D, float scale, const float* Q,
                            int64_t ldq, int64_t stride_q0, int64_t stride_q1, const float* Kk, int64_t ldk, int64_t stride_k0, int64_t stride_k1,
                            const float* V, int64_t ldv, int64_t stride_v0, int64_t stride_v1, float* O, int64_t ldo, int64_t stride_o0,
                            int64_t stride_o1, int accumulate) {
  return eg::attention::attention_forward(ctx, {batch0, batch1, I, J, K, D}, scale, Q, {ldq, stride_q0, stride_q1}, Kk, {ldk, stride_k0, stride_k1}, V,
                                          {ldv, stride_v0, stride_v1}, O, {ldo, stride_o0, stride_o1}, accumulate);
}

extern "C" int eg_attention_sums(eg_ctx* ctx, int64_t batch0, int64_t batch1, int64_t I, int64_t J, int64_t K, int64_t D, float scale, const float* Q,
                                 int64_t ldq, int64_t stride_q0, int64_t stride_q1, const float* Kk, int64_t ldk, int64_t stride_k0,
                                 int64_t stride_k1, const float* V, int64_t ldv, int64_t stride_v0, int64_t stride_v1, float* O, int64_t ldo,
                                 int64_t stride_o0, int64_t stride_o1, int accumulate, float* Sums, int64_t stride_s0, int64_t stride_s1) {
  return eg::attention::attention_forward(ctx, {batch0, batch1, I, J, K, D}, scale, Q, {ldq, stride_q0, stride_q1}, Kk, {ldk, stride_k0, stride_k1}, V,
                                          {ldv, stride_v0, stride_v1}, O, {ldo, stride_o0, stride_o1}, accumulate, Sums, {0, stride_s0, stride_s1});
}
