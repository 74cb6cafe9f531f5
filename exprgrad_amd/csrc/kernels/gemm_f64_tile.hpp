// The float64 matrix-core tile shared by the plain products (gemm_f64_mfma.hip) and the convolutions (conv2_f64_mfma.hip):
// operand images in LDS, the loader of dense operands, the k loop of `v_mfma_f64_16x16x4_f64` and the store of a tile.
// gemm_f64_mfma.hip's header comment has the instruction's fragment maps and why the loop looks as it does.  One copy of
// the k loop: a kernel brings its loaders, nothing else.
#pragma once

#include <hip/hip_runtime.h>

namespace eg {
namespace f64tile {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int BK = 16;
constexpr int PAD = 16;

struct DgemmArgs {
  const double* A;
  const double* B;
  double* C;        // destination, or the slab block when splits > 1
  const double* bias;
  long M, N, K;
  long lda, ldb, ldc;
  int accumulate;
  int splits;       // k-slices (grid.y)
  long k_per_split; // multiple of BK
  int tiles_m, tiles_n;
  int remap;        // tiles % 8 == 0: contiguous tile ranges per XCD
};

// Tile loader.  A k-contiguous operand ((mn, k) at base[mn * ld + k]) is staged as [mn][LDK = 18] rows, an mn-contiguous one
// ((mn, k) at base[k * ld + mn]) as [k][BMN + 16] rows; either way a thread moves 16-byte pieces (two doubles that are
// neighbours in memory AND in LDS: one global_load_dwordx4, one ds_write_b128) and consecutive lanes walk consecutive
// memory.  Both row strides put the two half-waves of a fragment read (ds_read_b64) on disjoint bank sets.
// VEC = false (an odd leading dimension or a base that is not 16-byte aligned): the same pieces as two 8-byte loads.
// (round 6: row paddings of 4 / 6 / 10 doubles instead of 2 measured SLOWER — 4096^3 NT 0.836 -> 0.76 / 0.69 / 0.69 of peak, NN
//  0.78 -> 0.74 / 0.78 / 0.70 — although the counters report bank conflicts for this layout and none for [k][mn + 16]: NT, both
//  operands in this layout, is the fastest order; the conflicts counted are the 16-byte writes of two rows per pass, not the reads)
constexpr int LDK = BK + 2;

template <int BMN, int NT, bool KC, bool VEC>
struct TileLoader {
  static constexpr int PIECES = BMN * (BK / 2) / NT;
  static constexpr int LDM = BMN + PAD;
  static constexpr int LDS_DOUBLES = KC ? BMN * LDK : BK * LDM;
  double v[PIECES][2];
  // piece -> (mn, k) of its first element
  static __device__ __forceinline__ void where(int p, int& mn, int& k) {
    if (KC) {
      mn = p / (BK / 2);
      k = (p % (BK / 2)) * 2;
    } else {
      k = p / (BMN / 2);
      mn = (p % (BMN / 2)) * 2;
    }
  }
  __device__ __forceinline__ void load(const double* __restrict__ base, long ld, long mn0, long k0, long MN, long Kend, int tid) {
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      int mn, k;
      where(tid + NT * j, mn, k);
      const long gm = mn0 + mn, gk = k0 + k;
      const double* src = KC ? base + gm * ld + gk : base + gk * ld + gm;
      const bool in0 = gm < MN && gk < Kend;
      const bool in1 = KC ? (gm < MN && gk + 1 < Kend) : (gm + 1 < MN && gk < Kend);
      if (VEC && in1) {  // (in1 implies in0)
        const d2 t = *reinterpret_cast<const d2*>(src);
        v[j][0] = t[0];
        v[j][1] = t[1];
      } else {
        v[j][0] = in0 ? src[0] : 0.0;
        v[j][1] = in1 ? src[1] : 0.0;
      }
    }
  }
  __device__ __forceinline__ void store(double* lds, int tid) const {
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      int mn, k;
      where(tid + NT * j, mn, k);
      double* dst = KC ? lds + mn * LDK + k : lds + k * LDM + mn;
      *reinterpret_cast<d2*>(dst) = d2{v[j][0], v[j][1]};
    }
  }
  // fragment element (mn, k) of the staged tile
  static __device__ __forceinline__ double at(const double* lds, int mn, int k) { return KC ? lds[mn * LDK + k] : lds[k * LDM + mn]; }
};

// One wave alone issues a float64 MFMA every ~146 cycles, two waves of a SIMD together one every 64 (tools/mfma_ceiling_f64.hip:
// 34 against 77.8 TFLOP/s) — the matrix pipe needs several waves per SIMD that are multiplying at the same time.  So a tile
// is shared by WR x WC waves with small sub-tiles (128 x 128: eight waves of 64 x 32; 64 x 64: four of 32 x 32) and
// blocks are small enough in LDS for two (three) of them per CU, which meet their barriers at different times.
//
// dgemm_tile_loop is the k loop of one block: `ktiles` 16-deep k-tiles, double-buffered in LDS, the next tile's global loads
// issued before the current tile's matrix instructions and written to LDS behind them.  How a tile is fetched is the
// caller's: load_a(kt) / load_b(kt) fill la / lb with k-tile kt (TileLoader::load, or a gathering loader of
// conv2_f64_mfma.hip); the LDS images are LA's and LB's.  acc: the wave's FM x FN fragments.
template <int FM, int FN, class LA, class LB, class FA, class FB>
__device__ __forceinline__ void dgemm_tile_loop(d4 (&acc)[FM][FN], LA& la, LB& lb, int wm, int wn, long ktiles, FA&& load_a, FB&& load_b) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* As = lds;                             // [2][LA::LDS_DOUBLES]
  double* Bs = lds + 2 * LA::LDS_DOUBLES;       // [2][LB::LDS_DOUBLES]
  const int tid = threadIdx.x, lane = tid & 63;
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
  if (ktiles > 0) {
    load_a(0L);
    load_b(0L);
    la.store(As, tid);
    lb.store(Bs, tid);
  }
  __syncthreads();
  const int fr = lane & 15, fk = lane >> 4;
  for (long kt = 0; kt < ktiles; ++kt) {
    const int cur = (int)(kt & 1);
    const bool more = kt + 1 < ktiles;
    if (more) {
      load_a(kt + 1);
      load_b(kt + 1);
    }
    const double* Ac = As + cur * LA::LDS_DOUBLES;
    const double* Bc = Bs + cur * LB::LDS_DOUBLES;
    // (two k-steps per unrolled body: with all four the k-contiguous variants held every fragment of the k-tile at once and
    //  spilled 2 - 11 registers at the 128 that four waves per SIMD allow — 4096^3 NN ran 0.72 of peak where TN, which did not spill, ran 0.84)
#pragma unroll 2
    for (int s = 0; s < BK / 4; ++s) {
      double af[FM], bf[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) af[i] = LA::at(Ac, wm + 16 * i + fr, 4 * s + fk);
#pragma unroll
      for (int j = 0; j < FN; ++j) bf[j] = LB::at(Bc, wn + 16 * j + fr, 4 * s + fk);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
      la.store(As + (cur ^ 1) * LA::LDS_DOUBLES, tid);
      lb.store(Bs + (cur ^ 1) * LB::LDS_DOUBLES, tid);
    }
    __syncthreads();
  }
}

// The wave's fragments to the destination (or to slab `slice` of a sliced product).  C / D: column lane & 15, row (lane >> 4) + 4 r
template <int FM, int FN>
__device__ __forceinline__ void dgemm_tile_store(const d4 (&acc)[FM][FN], const DgemmArgs& a, long slice, long m0, long n0, int wm, int wn) {
  const int lane = threadIdx.x & 63;
  const int fr = lane & 15, fk = lane >> 4;
  const bool slab = a.splits > 1;
  double* C = slab ? a.C + slice * a.M * a.N : a.C;
  const long ldc = slab ? a.N : a.ldc;
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const long col = n0 + wn + 16 * j + fr;
      if (col >= a.N) continue;
      const double b = (!slab && a.bias) ? a.bias[col] : 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long row = m0 + wm + 16 * i + fk + 4 * r;
        if (row >= a.M) continue;
        double v = acc[i][j][r];
        if (!slab) {
          if (a.bias) v = v + b;
          if (a.accumulate) v = C[row * ldc + col] + v;
        }
        C[row * ldc + col] = v;
      }
    }
}

// dgemm_tile_at is the work of one block: tile `tile` of the output (row-major over tiles_m x tiles_n), the k range
// [kbeg, kend) of slice `slice`.  dgemm_kernel runs it on its block ids, dgemm_batched_kernel on the tile of its item.
template <int BM, int BN, int WR, int WC, bool AKC, bool BKC, bool VEC>
__device__ __forceinline__ void dgemm_tile_at(const DgemmArgs& a, long tile, long slice, long kbeg, long kend) {
  constexpr int NT = WR * WC * 64;
  constexpr int WM = BM / WR, WN = BN / WC;
  constexpr int FM = WM / 16, FN = WN / 16;
  using LA = TileLoader<BM, NT, AKC, VEC>;
  using LB = TileLoader<BN, NT, BKC, VEC>;
  const int tid = threadIdx.x, wave = tid >> 6;
  const int wm = (wave / WC) * WM, wn = (wave % WC) * WN;
  const long tm = tile / a.tiles_n, tn = tile % a.tiles_n;
  const long m0 = tm * BM, n0 = tn * BN;
  d4 acc[FM][FN];
  LA la;
  LB lb;
  const long ktiles = kend > kbeg ? (kend - kbeg + BK - 1) / BK : 0;
  dgemm_tile_loop<FM, FN>(
      acc, la, lb, wm, wn, ktiles, [&](long kt) { la.load(a.A, a.lda, m0, kbeg + kt * BK, a.M, kend, tid); },
      [&](long kt) { lb.load(a.B, a.ldb, n0, kbeg + kt * BK, a.N, kend, tid); });
  dgemm_tile_store<FM, FN>(acc, a, slice, m0, n0, wm, wn);
}

// Second pass of a sliced product: out = (accumulate ? out : 0) + (slab 0 + slab 1 + ...) + bias, slabs in order.
static __global__ __launch_bounds__(256) void dgemm_reduce_kernel(const double* __restrict__ slabs, double* __restrict__ C, const double* __restrict__ bias,
                                                           long M, long N, long ldc, int splits, int accumulate) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * N) return;
  const long row = i / N, col = i % N;
  double s = slabs[i];
  for (int z = 1; z < splits; ++z) s = s + slabs[(long)z * M * N + i];
  if (bias) s = s + bias[col];
  double* dst = C + row * ldc + col;
  *dst = accumulate ? *dst + s : s;
}


}  // namespace f64tile
}  // namespace eg
