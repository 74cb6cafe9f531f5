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
#include "gemm_f32_mfma.hpp"   // xcd_remap, f32x4
#include "gemm_plan.hpp"       // batched2_c_distinct
#include "attention_plan.hpp"
#include "attention_tile.hpp"   // TileRegs, load_rows, store_rows, wave_sync
#include "gemm_fused.hpp"       // View, the internal entries

#include <cmath>

#include "../eg_internal.hpp"

namespace {

using eg::gemm::f32x4;
using eg::gemm::xcd_remap;
using namespace eg::attention;

struct AttnArgs {
  const float* Q;
  const float* Kk;
  const float* V;
  float* O;
  long ldq, ldk, ldv, ldo;
  long sq0, sq1, sk0, sk1, sv0, sv1, so0, so1;   // floats per step of the outer / inner batch index
  long I, J;
  int K, D;
  float scale;
  int accumulate;
  int vec_q, vec_k, vec_v;             // 16-byte loads of that operand (plan)
  unsigned batch1;                     // extent of the inner index
  unsigned first_outer, first_inner;   // the item the launch starts at: launches cut the flattened (o, i1) range
  int tiles_i;                         // blocks per item
  float* S;                            // eg_attention_sums: the row sums, I floats per item (SUMS instantiations only)
  long ss0, ss1;
};

constexpr int ES = TILE_J + 4;   // floats per E row

// SUMS: also store each row's denominator (eg_attention_sums); a compile-time flag, so that eg_attention's kernels are the
// ones they were.
template <int KP, int DP, bool SUMS>
__global__ __launch_bounds__(THREADS) void attention_f32_kernel(AttnArgs a) {
  constexpr int KS = KP + 4, VS = DP + 16;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const Ks = lds;                      // [64][KS]; the Q tile first
  float* const Vs = Ks + TILE_J * KS;         // [64][VS]
  float* const Es = Vs + TILE_J * VS;         // [4][16][ES]

  // Block id -> (outer, inner, row tile): block-uniform 32-bit arithmetic as in gemm_batched2_kernel.
  const int work = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int local = work / a.tiles_i;
  const int tile = work - local * a.tiles_i;
  unsigned inner = a.first_inner + (unsigned)local;
  const unsigned outer = a.first_outer + inner / a.batch1;
  inner %= a.batch1;
  const long i0 = (long)tile * TILE_I;
  const float* const Q = a.Q + (long)outer * a.sq0 + (long)inner * a.sq1 + i0 * a.ldq;
  const float* const Kk = a.Kk + (long)outer * a.sk0 + (long)inner * a.sk1;
  const float* const V = a.V + (long)outer * a.sv0 + (long)inner * a.sv1;
  float* const O = a.O + (long)outer * a.so0 + (long)inner * a.so1;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  float* const Ew = Es + w * 16 * ES;

  // Q rows of the wave as A operands of every k step, for the whole loop
  float q[KP / 4];
  {
    TileRegs<KP> tq;
    load_rows<KP>(tq, Q, a.ldq, a.I - i0, a.K, a.vec_q != 0, tid);
    store_rows<KP, KS>(tq, Ks, tid);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < KP / 4; ++kk) q[kk] = Ks[(w * 16 + c) * KS + 4 * kk + g];
  }

  f32x4 o[DP / 16];
#pragma unroll
  for (int nb = 0; nb < DP / 16; ++nb) o[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float sum[4] = {0.f, 0.f, 0.f, 0.f};

  TileRegs<KP> tk;
  TileRegs<DP> tv;
  const long nt = (a.J + TILE_J - 1) / TILE_J;
  if (nt > 0) {
    load_rows<KP>(tk, Kk, a.ldk, a.J, a.K, a.vec_k != 0, tid);
    load_rows<DP>(tv, V, a.ldv, a.J, a.D, a.vec_v != 0, tid);
  }
  for (long t = 0; t < nt; ++t) {
    const long j0 = t * TILE_J;
    __syncthreads();   // every wave is done with the tiles in LDS (the first time: with the Q tile)
    store_rows<KP, KS>(tk, Ks, tid);
    store_rows<DP, VS>(tv, Vs, tid);
    __syncthreads();
    if (t + 1 < nt) {   // in flight during this tile's MFMAs
      load_rows<KP>(tk, Kk + (j0 + TILE_J) * a.ldk, a.ldk, a.J - j0 - TILE_J, a.K, a.vec_k != 0, tid);
      load_rows<DP>(tv, V + (j0 + TILE_J) * a.ldv, a.ldv, a.J - j0 - TILE_J, a.D, a.vec_v != 0, tid);
    }

    f32x4 s[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) s[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KP / 4; ++kk) {
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) s[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(q[kk], Ks[(nb * 16 + c) * KS + 4 * kk + g], s[nb], 0, 0, 0);
    }

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

#pragma unroll
    for (int jj = 0; jj < TILE_J / 4; ++jj) {
      const float e = Ew[c * ES + 4 * jj + g];
#pragma unroll
      for (int nb = 0; nb < DP / 16; ++nb) o[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(e, Vs[(4 * jj + g) * VS + nb * 16 + c], o[nb], 0, 0, 0);
    }
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
    float* const S = a.S + (long)outer * a.ss0 + (long)inner * a.ss1;
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
      float* const p = O + row * a.ldo + col;
      *p = a.accumulate ? *p + v : v;
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int KP, int DP, bool SUMS>
int launch_one(eg_ctx* ctx, unsigned grid, const Plan& p, const AttnArgs& args) {
  // the attribute belongs to the device that is current (set_device has made it the context's): once per device
  constexpr int MAX_DEVICES = 64;
  static bool attr_set[MAX_DEVICES] = {};
  const bool known = ctx->device >= 0 && ctx->device < MAX_DEVICES;
  if (!known || !attr_set[ctx->device]) {
    EG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&attention_f32_kernel<KP, DP, SUMS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds_bytes_for(KP, DP)));
    if (known) attr_set[ctx->device] = true;
  }
  hipLaunchKernelGGL((attention_f32_kernel<KP, DP, SUMS>), dim3(grid), dim3(p.block), (size_t)p.lds_bytes, ctx->stream, args);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}

template <int KP, bool SUMS>
int launch_kp(eg_ctx* ctx, unsigned grid, const Plan& p, const AttnArgs& args) {
  switch (p.dp) {
    case 32: return launch_one<KP, 32, SUMS>(ctx, grid, p, args);
    case 64: return launch_one<KP, 64, SUMS>(ctx, grid, p, args);
    default: return launch_one<KP, 128, SUMS>(ctx, grid, p, args);
  }
}

// 9 kernels: the padded K x the padded D; 9 more that store the row sums
template <bool SUMS>
int launch_config(eg_ctx* ctx, unsigned grid, const Plan& p, const AttnArgs& args) {
  switch (p.kp) {
    case 32: return launch_kp<32, SUMS>(ctx, grid, p, args);
    case 64: return launch_kp<64, SUMS>(ctx, grid, p, args);
    default: return launch_kp<128, SUMS>(ctx, grid, p, args);
  }
}

}  // namespace

namespace eg {
namespace attention {

// The one launcher: eg_attention and the model layer's attention launches (host/run.cpp) come here with Sums == NULL,
// eg_attention_sums with the row sums' view.  `name` is the entry the messages speak of.
static int attention_launch(const char* name, eg_ctx* ctx, long batch0, long batch1, long I, long J, long K, long D, float scale, const float* Q,
                            long ldq, long stride_q0, long stride_q1, const float* Kk, long ldk, long stride_k0, long stride_k1, const float* V,
                            long ldv, long stride_v0, long stride_v1, float* O, long ldo, long stride_o0, long stride_o1, int accumulate, float* Sums,
                            long stride_s0, long stride_s1) {
  EG_REQUIRE(ctx, EG_ERR_INVALID, "%s: ctx is NULL", name);
  EG_REQUIRE(batch0 >= 0 && batch1 >= 0 && I >= 0 && J >= 0 && K >= 0 && D >= 0, EG_ERR_INVALID, "%s: negative extent", name);
  EG_REQUIRE(batch0 < (1L << 31) && batch1 < (1L << 31), EG_ERR_INVALID, "%s: a batch extent of 2^31 or more", name);
  EG_REQUIRE(stride_q0 >= 0 && stride_q1 >= 0 && stride_k0 >= 0 && stride_k1 >= 0 && stride_v0 >= 0 && stride_v1 >= 0, EG_ERR_INVALID,
             "%s: negative stride", name);
  if (batch0 == 0 || batch1 == 0 || I == 0 || (D == 0 && !Sums)) return EG_OK;
  EG_REQUIRE(D == 0 || O, EG_ERR_INVALID, "%s: O is NULL", name);
  EG_REQUIRE(J == 0 || D == 0 || V, EG_ERR_INVALID, "%s: NULL operand", name);
  EG_REQUIRE(J == 0 || K == 0 || (Q && Kk), EG_ERR_INVALID, "%s: NULL operand", name);
  EG_REQUIRE(ldq >= K && ldk >= K && ldv >= D, EG_ERR_INVALID, "%s: leading dimension smaller than the row length", name);
  EG_REQUIRE(D == 0 || eg::gemm::batched2_c_distinct(batch0, stride_o0, batch1, stride_o1, I, ldo, D), EG_ERR_INVALID,
             "%s: ldo, stride_o0 and stride_o1 make elements of O share an address", name);
  // the row sums: one row of I columns per item
  EG_REQUIRE(!Sums || eg::gemm::batched2_c_distinct(batch0, stride_s0, batch1, stride_s1, 1, I, I), EG_ERR_INVALID,
             "%s: stride_s0 and stride_s1 make elements of Sums share an address", name);
  EG_REQUIRE(K <= MAX_HEAD, EG_ERR_UNSUPPORTED, "%s: K = %ld is above the limit of %d", name, K, MAX_HEAD);
  EG_REQUIRE(D <= MAX_HEAD, EG_ERR_UNSUPPORTED, "%s: D = %ld is above the limit of %d", name, D, MAX_HEAD);
  if (J == 0 && accumulate && !Sums) return EG_OK;   // an empty sum adds nothing
  int rc = eg::set_device(ctx);
  if (rc) return rc;

  Problem pr;
  pr.batch0 = batch0, pr.batch1 = batch1, pr.I = I, pr.J = J, pr.K = K, pr.D = D;
  pr.q = {ldq, stride_q0, stride_q1, aligned16(Q)};
  pr.k = {ldk, stride_k0, stride_k1, aligned16(Kk)};
  pr.v = {ldv, stride_v0, stride_v1, aligned16(V)};
  pr.o = {ldo, stride_o0, stride_o1, aligned16(O)};
  pr.sums = Sums != nullptr;
  pr.cus = ctx->compute_units;
  const Plan p = plan_attention(pr);
  EG_REQUIRE(p.supported, EG_ERR_UNSUPPORTED, "%s: %s", name, p.reason);

  for (long n = 0; n < p.launches; ++n) {
    const Launch l = plan_launch(p, n);
    EG_REQUIRE(l.items > 0 && l.grid > 0 && l.grid <= eg::gemm::BATCHED_MAX_BLOCKS, EG_ERR_INVALID, "%s: launch out of range", name);
    AttnArgs args = {};
    args.Q = Q, args.Kk = Kk, args.V = V, args.O = O;
    args.ldq = ldq, args.ldk = ldk, args.ldv = ldv, args.ldo = ldo;
    args.sq0 = stride_q0, args.sq1 = stride_q1, args.sk0 = stride_k0, args.sk1 = stride_k1;
    args.sv0 = stride_v0, args.sv1 = stride_v1, args.so0 = stride_o0, args.so1 = stride_o1;
    args.I = I, args.J = J, args.K = (int)K, args.D = (int)D;
    args.scale = scale;
    args.accumulate = accumulate;
    args.vec_q = p.vec_q, args.vec_k = p.vec_k, args.vec_v = p.vec_v;
    args.batch1 = (unsigned)batch1;
    args.first_outer = (unsigned)(l.first / batch1);
    args.first_inner = (unsigned)(l.first % batch1);
    args.tiles_i = (int)p.tiles_i;
    args.S = Sums, args.ss0 = stride_s0, args.ss1 = stride_s1;
    rc = Sums ? launch_config<true>(ctx, (unsigned)l.grid, p, args) : launch_config<false>(ctx, (unsigned)l.grid, p, args);
    if (rc) return rc;
  }
  return EG_OK;
}

int attention_f32(eg_ctx* ctx, long batch0, long batch1, long I, long J, long K, long D, float scale, const float* Q, long ldq, long stride_q0,
                  long stride_q1, const float* Kk, long ldk, long stride_k0, long stride_k1, const float* V, long ldv, long stride_v0, long stride_v1,
                  float* O, long ldo, long stride_o0, long stride_o1, int accumulate) {
  return attention_launch("eg_attention", ctx, batch0, batch1, I, J, K, D, scale, Q, ldq, stride_q0, stride_q1, Kk, ldk, stride_k0, stride_k1, V,
                          ldv, stride_v0, stride_v1, O, ldo, stride_o0, stride_o1, accumulate, nullptr, 0, 0);
}

int attention_sums_f32(eg_ctx* ctx, long batch0, long batch1, long I, long J, long K, long D, float scale, const float* Q, View q, const float* Kk, View k,
                       const float* V, View v, float* O, View o, int accumulate, float* Sums, View s) {
  return attention_launch(Sums ? "eg_attention_sums" : "eg_attention", ctx, batch0, batch1, I, J, K, D, scale, Q, q.ld, q.stride0, q.stride1, Kk, k.ld,
                          k.stride0, k.stride1, V, v.ld, v.stride0, v.stride1, O, o.ld, o.stride0, o.stride1, accumulate, Sums, s.stride0, s.stride1);
}

}  // namespace attention
}  // namespace eg

extern "C" int eg_attention(eg_ctx* ctx, int64_t batch0, int64_t batch1, int64_t I, int64_t J, int64_t K, int64_t D, float scale, const float* Q,
                            int64_t ldq, int64_t stride_q0, int64_t stride_q1, const float* Kk, int64_t ldk, int64_t stride_k0, int64_t stride_k1,
                            const float* V, int64_t ldv, int64_t stride_v0, int64_t stride_v1, float* O, int64_t ldo, int64_t stride_o0,
                            int64_t stride_o1, int accumulate) {
  return eg::attention::attention_f32(ctx, batch0, batch1, I, J, K, D, scale, Q, ldq, stride_q0, stride_q1, Kk, ldk, stride_k0, stride_k1, V, ldv,
                                      stride_v0, stride_v1, O, ldo, stride_o0, stride_o1, accumulate);
}

extern "C" int eg_attention_sums(eg_ctx* ctx, int64_t batch0, int64_t batch1, int64_t I, int64_t J, int64_t K, int64_t D, float scale, const float* Q,
                                 int64_t ldq, int64_t stride_q0, int64_t stride_q1, const float* Kk, int64_t ldk, int64_t stride_k0,
                                 int64_t stride_k1, const float* V, int64_t ldv, int64_t stride_v0, int64_t stride_v1, float* O, int64_t ldo,
                                 int64_t stride_o0, int64_t stride_o1, int accumulate, float* Sums, int64_t stride_s0, int64_t stride_s1) {
  return eg::attention::attention_launch(Sums ? "eg_attention_sums" : "eg_attention", ctx, batch0, batch1, I, J, K, D, scale, Q, ldq, stride_q0,
                                         stride_q1, Kk, ldk, stride_k0, stride_k1, V, ldv, stride_v0, stride_v1, O, ldo, stride_o0, stride_o1,
                                         accumulate, Sums, stride_s0, stride_s1);
}
