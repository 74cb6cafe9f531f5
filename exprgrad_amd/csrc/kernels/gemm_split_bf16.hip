// Large f32 products of the public eg_sgemm on the bf16 matrix cores, by an exact three-way split of the operands.
//
// Every f32 operand element is cut into three bf16 pieces x = x0 + x1 + x2, each the round-to-nearest bf16 of the
// remainder before it (x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1)).  For a normal x whose pieces stay
// normal the three hold its 24 significand bits exactly.  The product then keeps the six terms down to 2^-16 of |ab|:
//   a.b = a0b0 + (a0b1 + a1b0) + (a0b2 + a1b1 + a2b0)      (dropped: a1b2, a2b1, a2b2 <= ~2^-23 |ab|, signs random)
// Each bf16 x bf16 product is exact in f32.  One v_mfma_f32_16x16x32_bf16 (16 cycles) takes two terms of a 16 x 16 x 16
// block, so the six terms are three instructions, 48 cycles; the block costs 4 x 32 cycles on v_mfma_f32_16x16x4_f32, so
// the split takes 2.67x fewer matrix cycles.  (The 16x16x32 shape holds a higher clock under load than 32x32x16 at the
// same cycles per FLOP.)
//
// Two launches, then the exact kernel behind them as a device-side fallback:
//   1. the split pass (gemm_split_pass.hip): op(A) and op(B) of any layout and leading dimension -> three bf16 planes
//      each, in the layout stated at split_pass's declaration (gemm_fused.hpp): k-contiguous in 16-deep k-tiles, so the
//      8 KiB a 256-row tile needs per plane and k-tile are one contiguous piece.  An element that does not split
//      exactly sets the context's flag word to this call's epoch.
//   2. the product: 256 x 256 tiles, eight waves of 128 x 64 (8 x 4 blocks of 16 x 16), LDS-DMA stages of one 16-deep
//      k-tile (3 planes x 512 rows x 32 bytes = 48 KiB), three stages, C written through LDS as 16-byte row pieces.
//      Returns at entry when the flag is set.  Two kernels share everything but the k loop (split_product):
//        split_pingpong_kernel (default): two barriers per k-tile, a load phase and an MFMA phase, with the two waves of
//          a SIMD permanently one barrier apart, so that one multiplies (at raised priority) while the other issues and
//          reads.  The schedule is kernels/split_schedule.hpp, replayed on the CPU by tests/test_split_schedule_cpu.py.
//        split_gemm_kernel (EG_GEMM_NO_SKEW=1): one barrier per k-tile, every wave in phase; the independent loop the
//          default is compared against bit for bit (same MFMAs, same accumulators, same k order).
//   3. the exact f32 kernel (sgemm_exact with GemmArgs::run_if): returns at entry unless the flag is set.
// Only shapes whose exact product is one whole-tile launch qualify (exact_single_launch), so the fallback is one launch.
#include <algorithm>

#include "gemm_fused.hpp"
#include "split_schedule.hpp"
#include "../eg_internal.hpp"
#include "../switches.hpp"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BM = 256, BN = 256, WM = 128, WN = 64, NT = 512;
constexpr int STAGES = 3;
constexpr int PLANE_BYTES = BM * 16 * 2;                  // one plane of one operand for one 16-deep k-tile: 8 KiB
constexpr int STAGE_BYTES = 6 * PLANE_BYTES;               // A planes 0..2, then B planes 0..2: 48 KiB
constexpr int LOADS = STAGE_BYTES / (NT * 16);             // 16-byte LDS-DMA pieces per thread and stage: 6

// pa, pb: the planes the split pass wrote (layout: split_pass's declaration, gemm_fused.hpp)
struct SplitGemmArgs {
  const __bf16* pa;  // op(A) planes, M * K each
  const __bf16* pb;  // op(B) planes, N * K each
  float* C;
  const float* bias;
  long M, N, K, ldc;
  int tiles_m, tiles_n;
  int accumulate;
  const unsigned* flag;
  unsigned epoch;
};

// Tile order of the exact kernel (gemm_f32_mfma.hpp xcd_remap / tile_origin): every XCD gets a contiguous range of
// block ids, and those walk groups of 8 tile rows column-major, so co-resident tiles share panels inside one L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  constexpr int NXCD = 8;
  const int q = nwg / NXCD, r = nwg % NXCD;
  const int xcd = bid % NXCD, local = bid / NXCD;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
}
__device__ __forceinline__ void tile_origin(int wgid, int tiles_m, int tiles_n, long& m_blk, long& n_blk) {
  constexpr int GROUP = 8;
  const int per_group = GROUP * tiles_n;
  const int first_m = (wgid / per_group) * GROUP;
  const int gsize = min(tiles_m - first_m, GROUP);
  const int in_group = wgid % per_group;
  m_blk = (long)(first_m + in_group % gsize) * BM;
  n_blk = (long)(in_group / gsize) * BN;
}

__device__ __forceinline__ const void* uniform_ptr(const void* p) {
  const unsigned long v = reinterpret_cast<unsigned long>(p);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return reinterpret_cast<const void*>(((unsigned long)hi << 32) | lo);
}

// Waves w and w ^ PARTNER share a SIMD: w and w + 4 (measured both ways: DESIGN.md, the split-bf16 product's row).
constexpr int PARTNER = 4;

// The sub-tile leaves through LDS as 16-byte row pieces (the 16x16 C/D map, column lane & 15 and row 4 (lane >> 4) + r,
// would store 64-byte pieces).  Each wave parks half of its 128 x 64 sub-tile at a time in a 16 KiB region of its own
// ([row][64] floats; 2-way on the b32 writes, which costs nothing, none on the b128 reads) and writes it back as
// 4 rows x 256 bytes per instruction.  The barrier: every wave is done reading the last k-tile's stage.
__device__ __forceinline__ void store_c(const SplitGemmArgs& a, unsigned char (&lds)[STAGES * STAGE_BYTES], const f32x4 (&acc)[8][4], long m_blk,
                                        long n_blk, int wave, int lane) {
  const int wr = wave >> 2, wc = wave & 3;
  __syncthreads();
  float* park = reinterpret_cast<float*>(lds) + wave * 64 * WN;
  const int prow = lane >> 4, pc4 = (lane & 15) * 4;
  const long col = n_blk + wc * WN + pc4;
  f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
  if (a.bias) b4 = *reinterpret_cast<const f32x4*>(a.bias + col);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) park[(i * 16 + 4 * prow + r) * WN + j * 16 + (lane & 15)] = acc[4 * h + i][j][r];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (one wave: its LDS accesses complete in order)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int row = 4 * q + prow;
      f32x4 v = *reinterpret_cast<const f32x4*>(park + row * WN + pc4);
      f32x4* c = reinterpret_cast<f32x4*>(a.C + (m_blk + wr * WM + h * 64 + row) * a.ldc + col);
      if (a.accumulate) v = *c + v;
      if (a.bias) v = v + b4;
      *c = v;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
}

// Both product kernels: everything but the k loop is the same text.  PINGPONG picks the loop (below).
template <bool PINGPONG>
__device__ __forceinline__ void split_product(const SplitGemmArgs& a, unsigned char (&lds)[STAGES * STAGE_BYTES]) {
  if (*(volatile const unsigned*)a.flag == a.epoch) return;  // an operand did not split: the exact kernel behind runs

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;  // 2 x 4 waves of 128 x 64
  long m_blk, n_blk;
  tile_origin(xcd_remap(blockIdx.x, gridDim.x), a.tiles_m, a.tiles_n, m_blk, n_blk);

  // buffer descriptors of the block's row panels: operand origin + first row; k-tile, plane and wave go in the scalar offset
  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(uniform_ptr(a.pa + m_blk * 16)), (short)0, -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(uniform_ptr(a.pb + n_blk * 16)), (short)0, -1, 0x00020000);
  const unsigned a_plane = (unsigned)(a.M * a.K * 2), b_plane = (unsigned)(a.N * a.K * 2);
  const unsigned a_ktile = (unsigned)(a.M * 32), b_ktile = (unsigned)(a.N * 32);
  const unsigned voff = (unsigned)lane * 16;

  // wave w's 1 KiB of each 8 KiB piece: LDS destination = w's base + lane * 16 (lane-linear, like the global source), so
  // any wave can load any wave's share
  auto pieces = [&](int kt, int s, int w) {
    unsigned char* st = lds + s * STAGE_BYTES + w * 1024;
    const unsigned at = (unsigned)kt * a_ktile + (unsigned)w * 1024, bt = (unsigned)kt * b_ktile + (unsigned)w * 1024;
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      __attribute__((address_space(3))) void* dst = (__attribute__((address_space(3))) void*)(st + i * PLANE_BYTES);
      if (i < 3)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, dst, 16, voff, (unsigned)i * a_plane + at, 0, 0);
      else
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, dst, 16, voff, (unsigned)(i - 3) * b_plane + bt, 0, 0);
    }
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;

  // v_mfma_f32_16x16x32_bf16: lane l holds row (l & 15) of its 16-row block at k = 8 (l >> 4) .. + 7.  The k of a 16-deep
  // k-tile sit in lane groups 0-1, and groups 2-3 take the same k of another plane: one MFMA sums two terms.  So the
  // lane's plane is picked by sel = l >> 5 and its half of the 32-byte row by (l >> 4) & 1; per 16 x 16 block
  //   [a0 | a1] x [b2 | b1] = a0b2 + a1b1,   [a0 | a1] x [b1 | b0] = a0b1 + a1b0,   [a0 | a2] x [b0 | b0] = a0b0 + a2b0.
  // The 16 lanes of each ds_read_b128 bank group hit 16 distinct 16-byte bank quads (no conflicts, no swizzle).
  const int sel = lane >> 5;
  const int a_row = (wr * WM + (lane & 15)) * 32 + ((lane >> 4) & 1) * 16;
  const int b_row = 3 * PLANE_BYTES + (wc * WN + (lane & 15)) * 32 + ((lane >> 4) & 1) * 16;
  const int a01_off = a_row + sel * PLANE_BYTES, a02_off = a_row + 2 * sel * PLANE_BYTES;
  const int b21_off = b_row + (2 - sel) * PLANE_BYTES, b10_off = b_row + (1 - sel) * PLANE_BYTES, b00_off = b_row;

  // the fragments a period starts from: all of B and the first of A (the other seven A fragments are read between the MFMAs)
  bf16x8 fb21[4], fb10[4], fb00[4], fa01, fa02;
  auto read_head = [&](const unsigned char* st) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      fb21[j] = *reinterpret_cast<const bf16x8*>(st + b21_off + j * 512);
      fb10[j] = *reinterpret_cast<const bf16x8*>(st + b10_off + j * 512);
      fb00[j] = *reinterpret_cast<const bf16x8*>(st + b00_off + j * 512);
    }
    fa01 = *reinterpret_cast<const bf16x8*>(st + a01_off);
    fa02 = *reinterpret_cast<const bf16x8*>(st + a02_off);
  };
#pragma unroll
  for (int j = 0; j < 4; ++j) fb21[j] = fb10[j] = fb00[j] = bf16x8{};
  fa01 = fa02 = bf16x8{};

  // The 96 MFMAs of one k-tile, from the fragments read_head left: per block the 2^-16 pair first, then the 2^-8 pair,
  // then a0b0 with a2b0.
  // The A fragments of block row i + 1 are read in front of block row i's twelve MFMAs and waited for behind them.  The
  // fences keep them there: left alone the scheduler sinks each read to its first use, and a wave that has the matrix
  // pipe to itself (its partner is in its front or at the barrier) then stands for an LDS latency per block row
  // (stamped: 1840 cycles per 96 MFMAs of 16).
  auto multiply = [&](const unsigned char* st) {
    bf16x8 c01 = fa01, c02 = fa02;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      bf16x8 n01 = c01, n02 = c02;
      __builtin_amdgcn_sched_barrier(0);
      if (i + 1 < 8) {
        n01 = *reinterpret_cast<const bf16x8*>(st + a01_off + (i + 1) * 512);
        n02 = *reinterpret_cast<const bf16x8*>(st + a02_off + (i + 1) * 512);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(c01, fb21[j], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(c01, fb10[j], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(c02, fb00[j], acc[i][j], 0, 0, 0);
      c01 = n01;
      c02 = n02;
    }
  };

  if constexpr (PINGPONG) {
    // Two barriers per k-tile, the two waves of a SIMD permanently one barrier apart (kernels/split_schedule.hpp has the
    // schedule and its hazard argument; every count and stage number below is taken from there).  Waves 4 - 7 (role Y)
    // issue every LDS-DMA piece, their own and their partners', and are the only ones that wait for any.
    namespace ss = eg::split_sched;
    static_assert(ss::STAGES == STAGES && ss::PIECES == 2 * LOADS && ss::WAVES * 64 == NT, "split_schedule.hpp is this kernel's");
    auto issue_both = [&](int kt, int s) {
      pieces(kt, s, wave);
      pieces(kt, s, wave ^ PARTNER);
    };
    const int role = ss::role_of(wave);
    const int KT = (int)(a.K / 16);
    if (role == ss::Y) {
      for (int t = 0; t < ss::prologue_tiles(ss::Y, KT); ++t) issue_both(t, ss::stage_of(t));
      // k-tile 0 has landed; the k-tiles behind it may fly
      const int fly = ss::prologue_vmcnt(KT);
      if (fly == 2 * ss::PIECES) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
      else if (fly == ss::PIECES) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    static_assert(ss::barriers_before_loop(ss::X) == 1 && ss::barriers_before_loop(ss::Y) == 2, "barrier S, then Y's stagger");
    __builtin_amdgcn_s_barrier();
    if (role == ss::Y) __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    int s = 0, s2 = 2;  // stage_of(kt), stage_of(kt + 2)
    for (int kt = 0; kt < KT; ++kt) {
      // what the role does in this load phase, made opaque in every iteration: ONE loop body with scalar branches
      // around the issue and the wait (as loop invariants the compiler would write a loop per role)
      int go = __builtin_amdgcn_readfirstlane(ss::load_issues(role, kt, KT) ? 1 : 0);
      int fly = __builtin_amdgcn_readfirstlane(ss::load_waits(role) ? ss::load_vmcnt(kt, KT) : -1);  // the vmcnt to wait for, -1: none
      asm volatile("" : "+s"(go), "+s"(fly));
      if (go) issue_both(ss::load_issue_tile(kt), s2);
      const unsigned char* st = lds + s * STAGE_BYTES;
      read_head(st);
      static_assert(ss::load_vmcnt(0, 3) == 12 && ss::load_vmcnt(0, 2) == 0, "the counts written out below");
      if (fly == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
      else if (fly == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      // MFMA phase.  The fence keeps all 96 in front of the closing barrier (left alone the scheduler sinks the last
      // eleven behind it, into the partner's turn); the wait says this phase's fragment reads are done before the stage
      // may be refilled one barrier later.  The raised priority is the hardware's part: the SIMD issues the multiplying
      // wave's instructions ahead of its partner's load phase.  Without it the loop is no faster than one barrier per
      // k-tile with staggered roles, with it 2.2 - 2.6 % (profiles/split_pingpong_ab.txt).
      __builtin_amdgcn_s_setprio(1);
      multiply(st);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      s = s == STAGES - 1 ? 0 : s + 1;
      s2 = s2 == STAGES - 1 ? 0 : s2 + 1;
    }
    static_assert(ss::barriers_after_loop(ss::X) == 1 && ss::barriers_after_loop(ss::Y) == 0, "X catches up");
    if (role == ss::X) __builtin_amdgcn_s_barrier();
    store_c(a, lds, acc, m_blk, n_blk, wave, lane);
    return;
  }

  // split_gemm_kernel's loop from here on: one barrier per k-tile, every wave in phase.  The wait in front of barrier kt
  // retires this wave's six pieces of k-tile kt (the six of kt + 1 may still fly); the barrier makes every wave's visible,
  // so a read of k-tile kt is one barrier behind the wait that retired its pieces.  The stage refilled behind barrier kt
  // is k-tile kt - 1's, which every wave finished reading before it arrived at this barrier.
  const int KT = (int)(a.K / 16);
  pieces(0, 0, wave);
  if (KT > 1) pieces(1, 1, wave);
  int s = 0;
  for (int kt = 0; kt < KT; ++kt) {
    if (kt + 1 < KT) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (kt + 2 < KT) pieces(kt + 2, s == 0 ? 2 : s - 1, wave);
    const unsigned char* st = lds + s * STAGE_BYTES;
    read_head(st);
    multiply(st);
    s = s == STAGES - 1 ? 0 : s + 1;
  }
  store_c(a, lds, acc, m_blk, n_blk, wave, lane);
}

// One barrier per k-tile, every wave in phase (EG_GEMM_NO_SKEW=1): the loop the default is compared against.
__global__ __launch_bounds__(NT) void split_gemm_kernel(SplitGemmArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[STAGES * STAGE_BYTES];
  split_product<false>(a, lds);
}
// Two barriers per k-tile, SIMD partners one barrier apart (kernels/split_schedule.hpp): the library's default.
__global__ __launch_bounds__(NT) void split_pingpong_kernel(SplitGemmArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[STAGES * STAGE_BYTES];
  split_product<true>(a, lds);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Largest plane set (6 (M + N) K bytes) the context's workspace grows to for it: 4096^3 needs 192 MiB.
constexpr size_t kPlaneCap = 1ull << 30;

}  // namespace

namespace eg {
namespace gemm {

int sgemm_split(eg_ctx* ctx, int trans_a, int trans_b, long M, long N, long K, const float* A, long lda, const float* B, long ldb,
                float* C, long ldc, int accumulate, const float* bias) {
  // anything the exact entry would refuse or that does not qualify goes there untouched
  if (!ctx || !A || !B || !C || M <= 0 || N <= 0 || K <= 0) return EG_ERR_UNSUPPORTED;
  if (lda < (trans_a ? M : K) || ldb < (trans_b ? K : N) || ldc < N) return EG_ERR_UNSUPPORTED;
  if (eg::sw::on(eg::Sw::NO_SPLIT_GEMM)) return EG_ERR_UNSUPPORTED;
  // Shape gate: whole 256 x 256 tiles that fill the chip at least once and K >= 2048 (smaller products keep the exact path:
  // none of them is bound by matrix cycles the way a full round is), and an exact product that is one launch (the fallback).
  if (M % BM != 0 || N % BN != 0 || K % 32 != 0 || K < 2048) return EG_ERR_UNSUPPORTED;
  if ((M / BM) * (N / BN) < ctx->compute_units) return EG_ERR_UNSUPPORTED;
  const size_t plane_bytes = 6 * (size_t)(M + N) * (size_t)K;
  // (the product kernel's buffer offsets are 32-bit: three planes of one operand below 2^31 bytes)
  if (plane_bytes > kPlaneCap || 6 * (size_t)std::max(M, N) * (size_t)K >= (1ull << 31)) return EG_ERR_UNSUPPORTED;
  if (!aligned16(A) || !aligned16(B) || (!trans_a && lda % 4 != 0) || (trans_b && ldb % 4 != 0)) return EG_ERR_UNSUPPORTED;
  if (!aligned16(C) || ldc % 4 != 0 || (bias && !aligned16(bias))) return EG_ERR_UNSUPPORTED;  // 16-byte C row pieces
  if (!exact_single_launch(ctx, trans_a, trans_b, M, N, K, A, lda, B, ldb, C, ldc, bias)) return EG_ERR_UNSUPPORTED;

  int rc = eg::set_device(ctx);
  if (rc) return rc;
  if (!ctx->split_flag) {
    EG_HIP_CHECK(hipMalloc((void**)&ctx->split_flag, sizeof(unsigned)));
    EG_HIP_CHECK(hipMemset(ctx->split_flag, 0, sizeof(unsigned)));
  }
  rc = eg::ensure_workspace(ctx, plane_bytes);
  if (rc) return rc;
  if (++ctx->split_epoch == 0) ctx->split_epoch = 1;  // 0 is the flag's initial value
  const unsigned epoch = ctx->split_epoch;

  __bf16* pa = static_cast<__bf16*>(ctx->workspace);
  __bf16* pb = pa + 3 * (size_t)M * K;
  rc = split_pass(ctx, {A, lda, M, !trans_a}, {B, ldb, N, trans_b != 0}, K, pa, epoch);
  if (rc) return rc;

  SplitGemmArgs g = {};
  g.pa = pa;
  g.pb = pb;
  g.C = C;
  g.bias = bias;
  g.M = M;
  g.N = N;
  g.K = K;
  g.ldc = ldc;
  g.tiles_m = (int)(M / BM);
  g.tiles_n = (int)(N / BN);
  g.accumulate = accumulate;
  g.flag = ctx->split_flag;
  g.epoch = epoch;
  // EG_GEMM_NO_SKEW=1: the in-phase loop, the independent kernel the default one is compared against bit for bit
  if (eg::sw::on(eg::Sw::GEMM_NO_SKEW))
    hipLaunchKernelGGL(split_gemm_kernel, dim3((unsigned)(g.tiles_m * g.tiles_n)), dim3(NT), 0, ctx->stream, g);
  else
    hipLaunchKernelGGL(split_pingpong_kernel, dim3((unsigned)(g.tiles_m * g.tiles_n)), dim3(NT), 0, ctx->stream, g);
  EG_HIP_CHECK(hipGetLastError());

  // the exact product, run only when the split pass set the flag
  return sgemm_exact(ctx, trans_a, trans_b, M, N, K, A, lda, B, ldb, C, ldc, accumulate, bias, ctx->split_flag, epoch);
}

}  // namespace gemm
}  // namespace eg
