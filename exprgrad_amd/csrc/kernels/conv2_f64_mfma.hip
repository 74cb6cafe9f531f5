// float64 convolution of any width as an implicit GEMM on `v_mfma_f64_16x16x4_f64` — the closing route of a
// `compile[float64]` model's conv2 (dnn.nim:45-49; model.nim:253-260) and of its two derived gradients
// (passes.nim:383-549), and the float64 entry points of the library: eg_conv2_nhwc_f64 and its two gradients.
//
// The tile is gemm_f64_tile.hpp's: eight waves on 64 x 64 or 128 x 128, operand images [mn][18] / [k][tile + 16] in LDS, ONE
// k loop (dgemm_tile_loop) shared with eg_dgemm.  What is new here are the loaders of the gathered operand, the window
// matrix  window(src)[p][t]: pixel p = (n, y, x) of a pixel grid, tap t = (dy, dx, c), element
//   src[n, y - ph + dy, x - pw + dx, c]   (zero outside src),
// never written to memory:
//   forward           out [P, F]          = window(img) [P, FH*FW*C] * flt [F, FH*FW*C]^T         WindowRows is operand A
//   image gradient    gimg [N*H*W, C]     = window(gout, border FH-1 / FW-1) [N*H*W, FH*FW*F] * flipped [C, FH*FW*F]^T
//                                                                                                 WindowRows<PADDED> is A
//   filter gradient   gflt [F, FH*FW*C]   = gout [P, F]^T * window(img) [P, FH*FW*C]              WindowCols is operand B
// The taps (dx, c) of one filter row are FW*C contiguous doubles of src, so a tap is (dy, r = dx*C + c): one division per
// piece.  A piece is two neighbouring taps of one pixel: one 16-byte load when the channel count is even and src is
// 16-byte aligned, two 8-byte loads otherwise.  Ragged tiles and the image gradient's border are zeros written to LDS by
// the loader: nothing outside a tensor is read.
//
// Forward and image gradient take no k-slices: every output element is one k-ascending chain of matrix instructions
// whatever tile the plan picks, so an image has the same bits whatever batch it is part of.  The filter gradient sums over
// all pixels into few tiles: the pixels are cut into slices, each writes a slab into the context's workspace, and
// dgemm_reduce_kernel folds the slabs in ascending order (no atomics; runs are bit-equal).  plan_conv64 (gemm_plan.cpp)
// decides tile, loads, slices and geometry; the code below turns its plan into launches.
//
// Pixels and taps are 32-bit indices in the kernels, every address is 64-bit: plan_conv64 refuses a contraction with 2^31
// or more rows, columns or terms (CONV64_MAX_INDEX), and the entry points return EG_ERR_INVALID for it.
#include <algorithm>
#include <type_traits>

#include "../eg_internal.hpp"
#include "gemm_f64_tile.hpp"
#include "gemm_fused.hpp"
#include "gemm_plan.hpp"

namespace {

using namespace eg::f64tile;
using eg::gemm::Conv64Plan;
using eg::gemm::Conv64Problem;
using eg::gemm::Conv64Role;

struct Window {
  const double* src;   // [n][SH][SW][SC]
  long row;            // SW * SC: doubles between two rows of src
  unsigned SC;         // channels of src
  unsigned RUN;        // FW * SC: the taps of one filter row
  unsigned K;          // FH * RUN taps
  unsigned SH, SW;
  unsigned OH, OW;     // the pixel grid: pixel p = (n * OH + y) * OW + x
  int ph, pw;          // the virtual zero border
  unsigned P;          // pixels
};

struct Pixel {
  long base;   // offset of src[n, y - ph, x - pw, 0]; may lie outside src (used only with taps that pass the border test)
  int yy, xx;  // y - ph, x - pw
  bool ok;
};

__device__ __forceinline__ Pixel pixel_of(const Window& w, unsigned p) {
  Pixel r;
  r.ok = p < w.P;
  const unsigned x = p % w.OW, q = p / w.OW;
  const unsigned y = q % w.OH, n = q / w.OH;
  r.yy = (int)y - w.ph;
  r.xx = (int)x - w.pw;
  r.base = (((long)n * w.SH + r.yy) * (long)w.SW + r.xx) * (long)w.SC;
  return r;
}

// tap -> offset from the pixel's base, and (PADDED) whether the position lies inside src
template <bool PADDED>
__device__ __forceinline__ long tap_of(const Window& w, const Pixel& px, unsigned t, bool& inside) {
  const unsigned dy = t / w.RUN, r = t - dy * w.RUN;
  inside = t < w.K;
  if (PADDED) {
    const unsigned dx = r / w.SC;
    inside = inside && (unsigned)(px.yy + (int)dy) < w.SH && (unsigned)(px.xx + (int)dx) < w.SW;
  }
  return (long)dy * w.row + r;
}

// The window as a k-contiguous operand: (mn, k) = (pixel, tap).  TileLoader's LDS image [mn][18], its pieces (a thread's
// pixels are the same for every k-tile: their offsets are found once per block) and its store / at.
template <int BMN, int NT, bool VEC, bool PADDED>
struct WindowRows : TileLoader<BMN, NT, true, VEC> {
  using T = TileLoader<BMN, NT, true, VEC>;
  Pixel px[T::PIECES];
  __device__ __forceinline__ void prepare(const Window& w, long mn0, int tid) {
#pragma unroll
    for (int j = 0; j < T::PIECES; ++j) {
      int mn, k;
      T::where(tid + NT * j, mn, k);
      px[j] = pixel_of(w, (unsigned)(mn0 + mn));
    }
  }
  __device__ __forceinline__ void load(const Window& w, long k0, int tid) {
#pragma unroll
    for (int j = 0; j < T::PIECES; ++j) {
      int mn, k;
      T::where(tid + NT * j, mn, k);
      const unsigned t = (unsigned)(k0 + k);
      if (VEC) {  // C even: taps t, t + 1 share (dy, dx), K is even
        bool in;
        const long off = tap_of<PADDED>(w, px[j], t, in);
        d2 v = {0.0, 0.0};
        if (in && px[j].ok) v = *reinterpret_cast<const d2*>(w.src + px[j].base + off);
        this->v[j][0] = v[0];
        this->v[j][1] = v[1];
      } else {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          bool in;
          const long off = tap_of<PADDED>(w, px[j], t + e, in);
          this->v[j][e] = (in && px[j].ok) ? w.src[px[j].base + off] : 0.0;
        }
      }
    }
  }
};

// The window as an mn-contiguous operand of a contraction over the pixels: (mn, k) = (tap, pixel), no border.  TileLoader's
// LDS image [k][BMN + 16].  A thread's taps are the same for every k-tile; its pixel moves on by 16 per k-tile.
template <int BMN, int NT, bool VEC>
struct WindowCols : TileLoader<BMN, NT, false, VEC> {
  using T = TileLoader<BMN, NT, false, VEC>;
  long off[T::PIECES][2];
  bool in[T::PIECES][2];
  __device__ __forceinline__ void prepare(const Window& w, long mn0, int tid) {
    Pixel none = {0, 0, 0, true};
#pragma unroll
    for (int j = 0; j < T::PIECES; ++j) {
      int mn, k;
      T::where(tid + NT * j, mn, k);
#pragma unroll
      for (int e = 0; e < 2; ++e) off[j][e] = tap_of<false>(w, none, (unsigned)(mn0 + mn + e), in[j][e]);
    }
  }
  __device__ __forceinline__ void load(const Window& w, long k0, long kend, int tid) {
#pragma unroll
    for (int j = 0; j < T::PIECES; ++j) {
      int mn, k;
      T::where(tid + NT * j, mn, k);
      const long p = k0 + k;
      const Pixel px = pixel_of(w, (unsigned)p);
      const bool ok = p < kend;   // (kend <= P)
      if (VEC) {  // C even: the taps' count is even, taps t, t + 1 share (dy, dx)
        d2 v = {0.0, 0.0};
        if (ok && in[j][0]) v = *reinterpret_cast<const d2*>(w.src + px.base + off[j][0]);
        this->v[j][0] = v[0];
        this->v[j][1] = v[1];
      } else {
#pragma unroll
        for (int e = 0; e < 2; ++e) this->v[j][e] = (ok && in[j][e]) ? w.src[px.base + off[j][e]] : 0.0;
      }
    }
  }
};

struct Conv64Args {
  DgemmArgs g;   // the contraction; the gathered operand's pointer and leading dimension are unused
  Window w;
};

__device__ __forceinline__ long tile_of_block(int remap) {
  long tile = blockIdx.x;
  if (remap) {
    const long per = (long)gridDim.x >> 3;
    tile = (tile & 7) * per + (tile >> 3);
  }
  return tile;
}

// forward, image gradient (PADDED): A = the window, B = the bank [N][K], k-contiguous
template <int BM, int BN, int WR, int WC, bool VA, bool VB, bool PADDED>
__global__ __launch_bounds__(WR* WC * 64, 4) void conv64_rows_kernel(Conv64Args c) {
  constexpr int NT = WR * WC * 64;
  constexpr int WM = BM / WR, WN = BN / WC;
  constexpr int FM = WM / 16, FN = WN / 16;
  using LA = WindowRows<BM, NT, VA, PADDED>;
  using LB = TileLoader<BN, NT, true, VB>;
  const DgemmArgs& a = c.g;
  const int tid = threadIdx.x, wave = tid >> 6;
  const int wm = (wave / WC) * WM, wn = (wave % WC) * WN;
  const long tile = tile_of_block(a.remap);
  const long m0 = (tile / a.tiles_n) * BM, n0 = (tile % a.tiles_n) * BN;
  d4 acc[FM][FN];
  LA la;
  LB lb;
  la.prepare(c.w, m0, tid);
  const long ktiles = (a.K + BK - 1) / BK;
  dgemm_tile_loop<FM, FN>(
      acc, la, lb, wm, wn, ktiles, [&](long kt) { la.load(c.w, kt * BK, tid); },
      [&](long kt) { lb.load(a.B, a.ldb, n0, kt * BK, a.N, a.K, tid); });
  dgemm_tile_store<FM, FN>(acc, a, 0, m0, n0, wm, wn);
}

// filter gradient: A = gout [P][F] (m-contiguous), B = the window, summed over the pixels [kbeg, kend) of slice blockIdx.y
template <int BM, int BN, int WR, int WC, bool VA, bool VB>
__global__ __launch_bounds__(WR* WC * 64, 4) void conv64_cols_kernel(Conv64Args c) {
  constexpr int NT = WR * WC * 64;
  constexpr int WM = BM / WR, WN = BN / WC;
  constexpr int FM = WM / 16, FN = WN / 16;
  using LA = TileLoader<BM, NT, false, VA>;
  using LB = WindowCols<BN, NT, VB>;
  const DgemmArgs& a = c.g;
  const int tid = threadIdx.x, wave = tid >> 6;
  const int wm = (wave / WC) * WM, wn = (wave % WC) * WN;
  const long tile = tile_of_block(a.remap);
  const long m0 = (tile / a.tiles_n) * BM, n0 = (tile % a.tiles_n) * BN;
  const long kbeg = (long)blockIdx.y * a.k_per_split;
  const long kend = min(a.K, kbeg + a.k_per_split);
  d4 acc[FM][FN];
  LA la;
  LB lb;
  lb.prepare(c.w, n0, tid);
  const long ktiles = kend > kbeg ? (kend - kbeg + BK - 1) / BK : 0;
  dgemm_tile_loop<FM, FN>(
      acc, la, lb, wm, wn, ktiles, [&](long kt) { la.load(a.A, a.lda, m0, kbeg + kt * BK, a.M, kend, tid); },
      [&](long kt) { lb.load(c.w, kbeg + kt * BK, kend, tid); });
  dgemm_tile_store<FM, FN>(acc, a, (long)blockIdx.y, m0, n0, wm, wn);
}

// flt [F][FH][FW][C] -> [C][FH][FW][F] with both spatial axes reversed: the bank of the image gradient
__global__ __launch_bounds__(256) void conv64_flip_kernel(const double* __restrict__ flt, double* __restrict__ flipped, long F, long FH, long FW, long C) {
  const long total = F * FH * FW * C;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long f = i % F, p = i / F;
    const long dx = p % FW, q = p / FW;
    const long dy = q % FH, ch = q / FH;
    flipped[i] = flt[((f * FH + (FH - 1 - dy)) * FW + (FW - 1 - dx)) * C + ch];
  }
}

template <class Fn>
void with_bool(bool b, Fn&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

template <class Kernel>
int launch_tile(eg_ctx* ctx, Kernel kernel, bool& attr_set, size_t lds, const Conv64Plan& p, const Conv64Args& c) {
  if (!attr_set) {
    EG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set = true;
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)p.grid_x, (unsigned)p.grid_y), dim3((unsigned)(p.wr * p.wc * 64)), lds, ctx->stream, c);
  EG_HIP_CHECK(hipGetLastError());
  return EG_OK;
}

template <int BM, int BN, bool VA, bool VB, bool PADDED>
int launch_rows_one(eg_ctx* ctx, const Conv64Plan& p, const Conv64Args& c) {
  constexpr size_t lds = (size_t)2 * (WindowRows<BM, 512, VA, PADDED>::LDS_DOUBLES + TileLoader<BN, 512, true, VB>::LDS_DOUBLES) * sizeof(double);
  static bool attr_set = false;
  return launch_tile(ctx, &conv64_rows_kernel<BM, BN, 2, 4, VA, VB, PADDED>, attr_set, lds, p, c);
}

template <int BM, int BN, bool VA, bool VB>
int launch_cols_one(eg_ctx* ctx, const Conv64Plan& p, const Conv64Args& c) {
  constexpr size_t lds = (size_t)2 * (TileLoader<BM, 512, false, VA>::LDS_DOUBLES + WindowCols<BN, 512, VB>::LDS_DOUBLES) * sizeof(double);
  static bool attr_set = false;
  return launch_tile(ctx, &conv64_cols_kernel<BM, BN, 2, 4, VA, VB>, attr_set, lds, p, c);
}

template <int BM, int BN>
int launch_rows(eg_ctx* ctx, const Conv64Plan& p, const Conv64Args& c, bool padded) {
  int rc = EG_ERR_INVALID;
  with_bool(p.vec_a, [&](auto va) {
    with_bool(p.vec_b, [&](auto vb) { with_bool(padded, [&](auto pd) { rc = launch_rows_one<BM, BN, va, vb, pd>(ctx, p, c); }); });
  });
  return rc;
}

template <int BM, int BN>
int launch_cols(eg_ctx* ctx, const Conv64Plan& p, const Conv64Args& c) {
  int rc = EG_ERR_INVALID;
  with_bool(p.vec_a, [&](auto va) { with_bool(p.vec_b, [&](auto vb) { rc = launch_cols_one<BM, BN, va, vb>(ctx, p, c); }); });
  return rc;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// window of a dense [n][SH][SW][SC] tensor under an FH x FW filter, on an OH x OW pixel grid
Window window_of(const double* src, long SH, long SW, long SC, long FH, long FW, long OH, long OW, long ph, long pw, long P) {
  Window w;
  w.src = src;
  w.row = SW * SC;
  w.SC = (unsigned)SC;
  w.RUN = (unsigned)(FW * SC);
  w.K = (unsigned)(FH * FW * SC);
  w.SH = (unsigned)SH;
  w.SW = (unsigned)SW;
  w.OH = (unsigned)OH;
  w.OW = (unsigned)OW;
  w.ph = (int)ph;
  w.pw = (int)pw;
  w.P = (unsigned)P;
  return w;
}

const char* const kKernelNames[4] = {"", "eg_conv64_mfma_fwd", "eg_conv64_mfma_gimg", "eg_conv64_mfma_gflt"};

}  // namespace

namespace eg {

bool conv2_f64_mfma_enabled() { return !eg::sw::on(eg::Sw::CONV_NO_MFMA64); }

// The one internal entry of the three roles: the C entry points below and the model layer (host/run.cpp) both come here
// with checked, non-empty extents.  a / b as the library's entry points take them: image + filters (forward), filters +
// output gradient (image gradient), image + output gradient (filter gradient).  *launched stays false under
// EG_CONV_NO_MFMA64.  The filter gradient's slabs take the context's workspace and the image gradient's flipped bank its
// auxiliary block: the model layer's eager run of a launch sequence sizes both before the sequence is captured, and a
// replay asks for the same sizes, so neither block moves under capture.
int conv2_f64_mfma(eg_ctx* ctx, int role, long N, long H, long W, long C, long F, long FH, long FW, const double* a, const double* b, double* out,
                   int accumulate, bool* launched, const char** kernel) {
  *launched = false;
  const long Ho = H - FH + 1, Wo = W - FW + 1;
  if (role < 1 || role > 3 || N <= 0 || Ho <= 0 || Wo <= 0 || C <= 0 || F <= 0 || !conv2_f64_mfma_enabled()) return EG_OK;
  const Conv64Role r = static_cast<Conv64Role>(role);
  const double* img = r == Conv64Role::GradImage ? nullptr : a;
  const double* flt = r == Conv64Role::Forward ? b : r == Conv64Role::GradImage ? a : nullptr;
  const double* gout = r == Conv64Role::Forward ? nullptr : b;
  Conv64Problem prob;
  prob.role = r;
  prob.N = N, prob.H = H, prob.W = W, prob.C = C, prob.F = F, prob.FH = FH, prob.FW = FW;
  prob.img_aligned = aligned16(img), prob.flt_aligned = aligned16(flt), prob.gout_aligned = aligned16(gout);
  prob.cus = ctx->compute_units;
  const Conv64Plan p = eg::gemm::plan_conv64(prob);
  EG_REQUIRE(p.ok, EG_ERR_INVALID, "%s: the contraction has 2^31 or more rows, columns or terms", kKernelNames[role]);
  int rc = eg::set_device(ctx);
  if (rc) return rc;
  const long P = N * Ho * Wo;
  Conv64Args c = {};
  DgemmArgs& g = c.g;
  g.M = p.M, g.N = p.Ncols, g.K = p.K;
  g.C = out, g.ldc = p.Ncols;
  g.accumulate = accumulate;
  g.splits = 1, g.k_per_split = p.pixels_per_slice;
  g.tiles_m = p.tiles_m, g.tiles_n = p.tiles_n, g.remap = p.remap ? 1 : 0;
  if (r == Conv64Role::Forward) {
    c.w = window_of(img, H, W, C, FH, FW, Ho, Wo, 0, 0, P);
    g.B = flt, g.ldb = p.K;
    rc = p.config == 0 ? launch_rows<128, 128>(ctx, p, c, false) : launch_rows<64, 64>(ctx, p, c, false);
  } else if (r == Conv64Role::GradImage) {
    rc = eg::ensure_aux(ctx, (size_t)p.aux_doubles * sizeof(double));
    if (rc) return rc;
    double* flipped = static_cast<double*>(ctx->aux);
    const long fb = std::min<long>((p.aux_doubles + 255) / 256, 2L * ctx->compute_units);
    hipLaunchKernelGGL(conv64_flip_kernel, dim3((unsigned)fb), dim3(256), 0, ctx->stream, flt, flipped, F, FH, FW, C);
    EG_HIP_CHECK(hipGetLastError());
    c.w = window_of(gout, Ho, Wo, F, FH, FW, H, W, FH - 1, FW - 1, N * H * W);
    g.B = flipped, g.ldb = p.K;
    rc = p.config == 0 ? launch_rows<128, 128>(ctx, p, c, true) : launch_rows<64, 64>(ctx, p, c, true);
  } else {
    if (p.workspace_doubles > 0) {
      rc = eg::ensure_workspace(ctx, (size_t)p.workspace_doubles * sizeof(double));
      if (rc) return rc;
    }
    double* slabs = static_cast<double*>(ctx->workspace);
    c.w = window_of(img, H, W, C, FH, FW, Ho, Wo, 0, 0, P);
    g.A = gout, g.lda = F;
    g.splits = p.slices;
    if (p.reduce) g.C = slabs;
    rc = p.config == 0 ? launch_cols<128, 128>(ctx, p, c) : launch_cols<64, 64>(ctx, p, c);
    if (!rc && p.reduce) {
      hipLaunchKernelGGL(dgemm_reduce_kernel, dim3((unsigned)((p.M * p.Ncols + 255) / 256)), dim3(256), 0, ctx->stream, slabs, out,
                         static_cast<const double*>(nullptr), p.M, p.Ncols, p.Ncols, p.slices, accumulate);
      EG_HIP_CHECK(hipGetLastError());
    }
  }
  if (rc) return rc;
  *launched = true;
  if (kernel) *kernel = kKernelNames[role];
  return EG_OK;
}

}  // namespace eg

namespace {

// The closing route of an entry point: the kernel above, or — under EG_CONV_NO_MFMA64 — the refusal (the library has no other
// float64 convolution for these shapes; a model runs its generated kernel).
int closing_route(const char* who, eg_ctx* ctx, int role, long N, long H, long W, long C, long F, long FH, long FW, const double* a, const double* b,
                  double* out, int accumulate) {
  bool launched = false;
  int rc = eg::conv2_f64_mfma(ctx, role, N, H, W, C, F, FH, FW, a, b, out, accumulate, &launched, nullptr);
  if (rc || launched) return rc;
  EG_REQUIRE(false, EG_ERR_INVALID, "%s: EG_CONV_NO_MFMA64 is set and no other float64 convolution kernel takes this shape", who);
  return EG_ERR_INVALID;
}

}  // namespace

extern "C" int eg_conv2_nhwc_f64(eg_ctx* ctx, int64_t N, int64_t H, int64_t W, int64_t C, int64_t F, int64_t FH, int64_t FW, const double* img,
                                 const double* flt, double* out, int accumulate) {
  EG_REQUIRE(ctx, EG_ERR_INVALID, "eg_conv2_nhwc_f64: ctx is NULL");
  EG_REQUIRE(N >= 0 && H >= 0 && W >= 0 && C >= 0 && F >= 0 && FH >= 1 && FW >= 1, EG_ERR_INVALID, "eg_conv2_nhwc_f64: bad extent");
  const long Ho = H - FH + 1, Wo = W - FW + 1;
  EG_REQUIRE(Ho >= 0 && Wo >= 0, EG_ERR_SHAPE, "eg_conv2_nhwc_f64: filter larger than image");
  if (N == 0 || Ho == 0 || Wo == 0 || F == 0) return EG_OK;
  EG_REQUIRE(out && (C == 0 || (img && flt)), EG_ERR_INVALID, "eg_conv2_nhwc_f64: NULL tensor");
  int rc = eg::set_device(ctx);
  if (rc) return rc;
  if (C == 0) return accumulate ? EG_OK : eg_fill_f64(ctx, N * Ho * Wo * F, 0.0, out);   // an empty sum
  if (FH == 1 && FW == 1)  // out[P,F] = img[P,C] * flt[F,C]^T
    return eg::gemm::dgemm(ctx, 0, 1, N * H * W, F, C, img, C, flt, C, out, F, accumulate, nullptr);
  bool launched = false;
  if (C <= 16 && F <= 16) {
    rc = eg::conv2_band_forward_try(ctx, true, N, H, W, C, F, FH, FW, img, flt, out, accumulate, &launched);
    if (rc || launched) return rc;
  }
  rc = eg::conv2_direct_f64_try(ctx, N, H, W, C, F, FH, FW, img, flt, out, accumulate, &launched);
  if (rc || launched) return rc;
  return closing_route("eg_conv2_nhwc_f64", ctx, 1, N, H, W, C, F, FH, FW, img, flt, out, accumulate);
}

extern "C" int eg_conv2_nhwc_grad_filter_f64(eg_ctx* ctx, int64_t N, int64_t H, int64_t W, int64_t C, int64_t F, int64_t FH, int64_t FW,
                                             const double* img, const double* gout, double* gflt, int accumulate) {
  EG_REQUIRE(ctx, EG_ERR_INVALID, "eg_conv2_nhwc_grad_filter_f64: ctx is NULL");
  EG_REQUIRE(N >= 0 && H >= 0 && W >= 0 && C >= 0 && F >= 0 && FH >= 1 && FW >= 1, EG_ERR_INVALID, "eg_conv2_nhwc_grad_filter_f64: bad extent");
  const long Ho = H - FH + 1, Wo = W - FW + 1;
  EG_REQUIRE(Ho >= 0 && Wo >= 0, EG_ERR_SHAPE, "eg_conv2_nhwc_grad_filter_f64: filter larger than image");
  if (F == 0 || C == 0) return EG_OK;
  EG_REQUIRE(gflt, EG_ERR_INVALID, "eg_conv2_nhwc_grad_filter_f64: NULL tensor");
  int rc = eg::set_device(ctx);
  if (rc) return rc;
  const long P = N * Ho * Wo;
  if (P == 0) return accumulate ? EG_OK : eg_fill_f64(ctx, F * FH * FW * C, 0.0, gflt);
  EG_REQUIRE(img && gout, EG_ERR_INVALID, "eg_conv2_nhwc_grad_filter_f64: NULL tensor");
  if (FH == 1 && FW == 1)  // gflt[F,C] = gout[P,F]^T * img[P,C]
    return eg::gemm::dgemm(ctx, 1, 0, F, C, P, gout, F, img, C, gflt, C, accumulate, nullptr);
  if (C <= 16 && F <= 16) {
    bool launched = false;
    rc = eg::conv2_band_grad_filter_try(ctx, true, N, H, W, C, F, FH, FW, img, gout, gflt, accumulate, &launched);
    if (rc || launched) return rc;
  }
  return closing_route("eg_conv2_nhwc_grad_filter_f64", ctx, 3, N, H, W, C, F, FH, FW, img, gout, gflt, accumulate);
}

extern "C" int eg_conv2_nhwc_grad_image_f64(eg_ctx* ctx, int64_t N, int64_t H, int64_t W, int64_t C, int64_t F, int64_t FH, int64_t FW,
                                            const double* flt, const double* gout, double* gimg, int accumulate) {
  EG_REQUIRE(ctx, EG_ERR_INVALID, "eg_conv2_nhwc_grad_image_f64: ctx is NULL");
  EG_REQUIRE(N >= 0 && H >= 0 && W >= 0 && C >= 0 && F >= 0 && FH >= 1 && FW >= 1, EG_ERR_INVALID, "eg_conv2_nhwc_grad_image_f64: bad extent");
  const long Ho = H - FH + 1, Wo = W - FW + 1;
  EG_REQUIRE(Ho >= 0 && Wo >= 0, EG_ERR_SHAPE, "eg_conv2_nhwc_grad_image_f64: filter larger than image");
  if (N == 0 || H == 0 || W == 0 || C == 0) return EG_OK;
  EG_REQUIRE(gimg, EG_ERR_INVALID, "eg_conv2_nhwc_grad_image_f64: NULL tensor");
  int rc = eg::set_device(ctx);
  if (rc) return rc;
  if (F == 0 || Ho == 0 || Wo == 0) return accumulate ? EG_OK : eg_fill_f64(ctx, N * H * W * C, 0.0, gimg);
  EG_REQUIRE(flt && gout, EG_ERR_INVALID, "eg_conv2_nhwc_grad_image_f64: NULL tensor");
  if (FH == 1 && FW == 1)  // gimg[P,C] = gout[P,F] * flt[F,C]
    return eg::gemm::dgemm(ctx, 0, 0, N * H * W, C, F, gout, F, flt, C, gimg, C, accumulate, nullptr);
  if (C <= 16 && F <= 16) {
    bool launched = false;
    rc = eg::conv2_band_grad_image_try(ctx, true, N, H, W, C, F, FH, FW, flt, gout, gimg, accumulate, &launched);
    if (rc || launched) return rc;
  }
  return closing_route("eg_conv2_nhwc_grad_image_f64", ctx, 2, N, H, W, C, F, FH, FW, flt, gout, gimg, accumulate);
}
