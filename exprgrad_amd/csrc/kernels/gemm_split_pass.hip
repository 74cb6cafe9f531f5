// The split pass of eg_sgemm's split-bf16 product (gemm_split_bf16.hip has the numerics and the product kernels): op(A) and
// op(B) of any layout and leading dimension -> three bf16 planes each, in the layout stated at split_pass's declaration
// (gemm_fused.hpp).  An element that does not split exactly (Inf, NaN, f32 subnormal, a piece that underflows, a value
// that rounds to Inf) sets the context's flag word to this call's epoch.  A k-contiguous operand is read in units of 8 k
// (2 x 16 bytes per lane).  An operand whose k runs along ld is read in tiles of 16 k x 256 rows, 16 bytes (4 rows) per
// lane, and its pieces turn k-contiguous through LDS (split_tiles_kernel); with EG_SPLIT_PASS_SCALAR=1, or a leading
// dimension that is no multiple of 4, it takes the unit path with eight 4-byte loads per unit instead
// (split_planes_kernel, both operands as units).
#include <cfloat>

#include "gemm_fused.hpp"
#include "../eg_internal.hpp"
#include "../switches.hpp"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// op(X) is R x K: X[r * ld + k] when k-contiguous (kc), X[k * ld + r] otherwise.  R % 32 == 0, K % 32 == 0.
struct SplitOperand {
  const float* src;
  long ld;
  long R;
  int kc;
  __bf16* dst;  // 3 planes of R * K
};

// A unit is 8 consecutive k of one row: 32 bytes in, 16 bytes out per plane.  The 64 units of a wave cover 16 rows x 4
// units when k-contiguous (4 x 128-byte reads; 2 x 512-byte plane rows out) and 32 rows x 2 units otherwise (each of the
// 8 loads reads 2 x 128 bytes of two k-rows; 1 KiB plane rows out).
__device__ __forceinline__ void unit_coords(const SplitOperand& o, long K, long u, long& r, long& chunk) {
  const long cpr = K / 8, t = u >> 6;
  const int l = (int)(u & 63);
  if (o.kc) {
    const long per = cpr / 4;
    r = (t / per) * 16 + (l >> 2);
    chunk = (t % per) * 4 + (l & 3);
  } else {
    const long per = cpr / 2;
    r = (t / per) * 32 + (l >> 1);
    chunk = (t % per) * 2 + (l & 1);
  }
}

__device__ __forceinline__ void load_unit(const SplitOperand& o, long r, long chunk, float (&x)[8]) {
  if (o.kc) {
    const f32x4* p = reinterpret_cast<const f32x4*>(o.src + r * o.ld + chunk * 8);
    const f32x4 v0 = __builtin_nontemporal_load(p), v1 = __builtin_nontemporal_load(p + 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[j] = v0[j];
      x[4 + j] = v1[j];
    }
  } else {
    const float* p = o.src + chunk * 8 * o.ld + r;
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = __builtin_nontemporal_load(p + j * o.ld);
  }
}

// x = x0 + x1 + x2 exactly, or `bad`.  The casts are v_cvt_pk_bf16_f32 (round to nearest even; NaN stays NaN).  Both
// subtractions are exact while nothing underflows or overflows, so the split is exact iff the last remainder is x2.
__device__ __forceinline__ void split_elem(float v, __bf16& b0, __bf16& b1, __bf16& b2, bool& bad) {
  b0 = (__bf16)v;
  const float r1 = v - (float)b0;
  b1 = (__bf16)r1;
  const float f1 = (float)b1;
  const float r2 = r1 - f1;
  b2 = (__bf16)r2;
  const float f2 = (float)b2;
  bad |= !(r2 == f2);                                         // Inf, NaN, a value that rounds to Inf
  bad |= v != 0.f && __builtin_fabsf(v) < FLT_MIN;           // f32 subnormal
  bad |= (f1 != 0.f && __builtin_fabsf(f1) < FLT_MIN) || (f2 != 0.f && __builtin_fabsf(f2) < FLT_MIN);  // a piece underflows
}

__device__ __forceinline__ void split_unit(const SplitOperand& o, long K, long r, long chunk, const float (&x)[8], bool& bad) {
  bf16x8 h0, h1, h2;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    __bf16 b0, b1, b2;
    split_elem(x[j], b0, b1, b2, bad);
    h0[j] = b0;
    h1[j] = b1;
    h2[j] = b2;
  }
  const long plane = o.R * K;
  bf16x8* d = reinterpret_cast<bf16x8*>(o.dst + ((chunk >> 1) * o.R + r) * 16 + (chunk & 1) * 8);
  const long ps = plane / 8;  // plane stride in 16-byte units
  d[0] = h0;
  d[ps] = h1;
  d[2 * ps] = h2;
}

constexpr int SPLIT_NT = 256;
constexpr int SPLIT_U = 2;  // units per thread in flight

// Units [lo, hi) of the list in which [0, units_a) are op(A)'s and the rest op(B)'s, U per thread in flight.  A wave's 64
// units never straddle the two operands: units_a and lo are multiples of 64.
template <int U>
__device__ __forceinline__ void split_units(const SplitOperand& a, const SplitOperand& b, long K, long units_a, long lo, long hi,
                                            bool& bad) {
  constexpr long STEP = (long)SPLIT_NT * U;
  for (long base = lo; base < hi; base += STEP) {
    float x[U][8];
    long r[U], c[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const long u = base + i * SPLIT_NT + threadIdx.x;
      if (u >= hi) continue;
      const bool in_a = u < units_a;
      unit_coords(in_a ? a : b, K, in_a ? u : u - units_a, r[i], c[i]);
      load_unit(in_a ? a : b, r[i], c[i], x[i]);
    }
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const long u = base + i * SPLIT_NT + threadIdx.x;
      if (u >= hi) continue;
      split_unit(u < units_a ? a : b, K, r[i], c[i], x[i], bad);
    }
  }
}

// Both operands as units (EG_SPLIT_PASS_SCALAR=1, or no operand that qualifies for tiles).  A block owns one contiguous
// chunk of the list (a multiple of SPLIT_NT * SPLIT_U).
__global__ __launch_bounds__(SPLIT_NT) void split_planes_kernel(SplitOperand a, SplitOperand b, long K, long units_a, long units,
                                                              unsigned* flag, unsigned epoch) {
  constexpr long STEP = (long)SPLIT_NT * SPLIT_U;
  const long per = ((units + gridDim.x - 1) / gridDim.x + STEP - 1) / STEP * STEP;
  const long lo = (long)blockIdx.x * per, hi = lo + per < units ? lo + per : units;
  bool bad = false;
  split_units<SPLIT_U>(a, b, K, units_a, lo, hi, bad);
  if (__builtin_expect(bad, 0)) *(volatile unsigned*)flag = epoch;
}

// A tile is 16 k x 256 rows of an operand whose k runs along ld: 16 memory rows of 1 KiB, as much as SPLIT_NT * 2 units.
// Wave w fetches k-rows 4 w .. 4 w + 3 with one 16-byte-per-lane load each, so lane l holds rows 4 l .. 4 l + 3 at four
// consecutive k: per row and plane 8 bytes of the 32-byte plane row.  They meet in an LDS image of the tile's three
// plane pieces and leave it as whole 16-byte half rows, 1 KiB contiguous per plane and wave instruction.
// The image: row r at (r / 8) * REC_BYTES + (r % 8) * 32, i.e. 16 bytes of padding behind every 8 rows (two lanes).
//   ds_write_b64 (16 consecutive lanes per LDS cycle, 32 banks): a lane's rows are 128 bytes apart, so unpadded all 16
//     would meet in one bank pair; with the padding lanes 2 m, 2 m + 1 start at 16 m mod 128: 2-way, no worse.
//   ds_read_b128 (lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32; 64 banks): each group reads
//     the sixteen 16-byte pieces of ONE record (lane_unit), 256 consecutive bytes: no conflict.
constexpr int TILE_R = 256;
constexpr int REC_BYTES = 8 * 32 + 16;
constexpr int IMG_PLANE = (TILE_R / 8) * REC_BYTES;  // 8704
constexpr int IMG_BYTES = 3 * IMG_PLANE;             // 25.5 KiB
// Two images per block: three blocks fit a CU's LDS (12 waves), and three are the launch.  Two per CU: 65.0 us against
// 59.1 at 4096^3 NN; four units in flight next to the tiles: no difference (profiles/split_pass_ab.txt).
constexpr int TILE_BLOCKS_PER_CU = 3;

__device__ __forceinline__ void load_tile(const SplitOperand& o, long kt, long rb, f32x4 (&x)[4]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* p = o.src + (kt * 16 + wave * 4) * o.ld + rb * TILE_R + lane * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) x[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + i * o.ld));
}

__device__ __forceinline__ void split_tile(const f32x4 (&x)[4], unsigned char* img, bool& bad) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned char* row = img + (lane >> 1) * REC_BYTES + (lane & 1) * 128 + wave * 8;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    bf16x4 h0, h1, h2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      __bf16 b0, b1, b2;
      split_elem(x[i][c], b0, b1, b2, bad);
      h0[i] = b0;
      h1[i] = b1;
      h2[i] = b2;
    }
    *reinterpret_cast<bf16x4*>(row + c * 32) = h0;
    *reinterpret_cast<bf16x4*>(row + c * 32 + IMG_PLANE) = h1;
    *reinterpret_cast<bf16x4*>(row + c * 32 + 2 * IMG_PLANE) = h2;
  }
}

// The lane's 16-byte piece among the 64 (four records) of a wave instruction: record = its ds_read_b128 lane group.
__device__ __forceinline__ int lane_unit(int lane) {
  const int quad = (lane >> 2) & 7;  // groups take the quads {0, 3, 5, 6} (even parity) and {1, 2, 4, 7} of a wave half
  return ((lane >> 5) * 2 + (__builtin_popcount(quad) & 1)) * 16 + (quad >> 1) * 4 + (lane & 3);
}

__device__ __forceinline__ void store_tile(const SplitOperand& o, long K, long kt, long rb, const unsigned char* img) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long plane = o.R * K;
  __bf16* d = o.dst + (kt * o.R + rb * TILE_R) * 16;
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int u = (wave * 2 + i) * 64 + lane_unit(lane);  // 16-byte piece u of the plane's 8 KiB: row u / 2, half u % 2
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(img + p * IMG_PLANE + (u >> 4) * REC_BYTES + (u & 15) * 16);
      *reinterpret_cast<bf16x8*>(d + p * plane + u * 8) = v;
    }
}

// Every block takes a contiguous run of each operand: tiles when the operand's bit of `tiled` is set, else units (in
// pieces of SPLIT_NT * 2, one tile's worth), so a block's share of both kinds of work is the same as every other's.  Two
// images: the loads of tile t + 1 fly while tile t leaves, one barrier per tile (image s is written again behind the
// barrier of the tile after, which every wave passes only when its reads of s are done).
__global__ __launch_bounds__(SPLIT_NT) void split_tiles_kernel(SplitOperand a, SplitOperand b, long K, int tiled, unsigned* flag,
                                                             unsigned epoch) {
  __shared__ __attribute__((aligned(16))) unsigned char img[2][IMG_BYTES];
  bool bad = false;
  int s = 0;
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    const SplitOperand& o = which ? b : a;
    const long n = o.R * K / (TILE_R * 16);
    const long lo = n * blockIdx.x / gridDim.x, hi = n * (blockIdx.x + 1) / gridDim.x;
    if (!(tiled >> which & 1)) {
      const long units = o.R * K / 8;
      split_units<SPLIT_U>(o, o, K, units, lo * (SPLIT_NT * 2), hi * (SPLIT_NT * 2), bad);
      continue;
    }
    if (lo >= hi) continue;
    const long tr = o.R / TILE_R;
    long kt = lo / tr, rb = lo % tr;
    f32x4 x[4];
    load_tile(o, kt, rb, x);
    for (long t = lo; t < hi; ++t) {
      split_tile(x, img[s], bad);
      long nkt = kt, nrb = rb + 1;
      if (nrb == tr) {
        nrb = 0;
        ++nkt;
      }
      if (t + 1 < hi) load_tile(o, nkt, nrb, x);
      __syncthreads();
      store_tile(o, K, kt, rb, img[s]);
      s ^= 1;
      kt = nkt;
      rb = nrb;
    }
  }
  if (__builtin_expect(bad, 0)) *(volatile unsigned*)flag = epoch;
}

}  // namespace

namespace eg {
namespace gemm {

int split_pass(eg_ctx* ctx, const SplitPassOperand& a, const SplitPassOperand& b, long K, void* planes, unsigned epoch) {
  __bf16* pa = static_cast<__bf16*>(planes);
  const SplitOperand oa = {a.src, a.ld, a.rows, a.k_contiguous ? 1 : 0, pa};
  const SplitOperand ob = {b.src, b.ld, b.rows, b.k_contiguous ? 1 : 0, pa + 3 * (size_t)a.rows * K};
  // tiles for an operand whose k runs along ld, when its rows can be read 16 bytes at a time
  const bool scalar = eg::sw::on(eg::Sw::SPLIT_PASS_SCALAR);
  const int tiled = (!scalar && !oa.kc && oa.ld % 4 == 0 ? 1 : 0) | (!scalar && !ob.kc && ob.ld % 4 == 0 ? 2 : 0);
  if (tiled) {
    const long blocks = (long)TILE_BLOCKS_PER_CU * ctx->compute_units;
    hipLaunchKernelGGL(split_tiles_kernel, dim3((unsigned)blocks), dim3(SPLIT_NT), 0, ctx->stream, oa, ob, K, tiled, ctx->split_flag,
                       epoch);
  } else {
    const long units_a = oa.R * K / 8, units = (oa.R + ob.R) * K / 8;
    long blocks = (units + SPLIT_NT * SPLIT_U - 1) / (SPLIT_NT * SPLIT_U);
    if (blocks > 8L * ctx->compute_units) blocks = 8L * ctx->compute_units;
    hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)blocks), dim3(SPLIT_NT), 0, ctx->stream, oa, ob, K, units_a, units,
                       ctx->split_flag, epoch);
  }
  EG_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace gemm
}  // namespace eg
