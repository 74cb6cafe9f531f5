// The contractions' planner (gemm_plan.hpp): cost models, tile choice and the route of a product, f32 first, float64 behind it.
#include "gemm_plan.hpp"

#include <algorithm>
#include <cstdio>

namespace eg {
namespace gemm {

namespace {

struct TileCfg {
  int bm, bn, blocks_per_cu;
};

// Time of a ragged last-row tile relative to a full one per k-tile (it skips its empty 32x32
// sub-blocks and loads only its valid rows, but stages the whole B tile).  Calibrated on
// 784 x 512 x 65536 (TN): 128-row tiles 0.55, 256-row tiles 0.36 (a ragged 256-row tile's k-tile takes 1.2 us
// against 3.8 us; 0.40 / 0.36 / 0.33: dense step 1.111 / 1.101 / 1.103 ms).
double ragged_tile_share(int bm, long m_rest) {
  const double live = (double)((m_rest + 31) / 32 * 32) / bm;
  const double floor = bm >= 256 ? 0.36 : 0.55;
  return live > floor ? live : floor;
}

// Relative cost of running the problem with a given tile: (block rounds on the chip) x (work of
// the co-resident blocks of one CU), slightly favouring the larger tile whose measured
// efficiency is higher (tools/gemm_tune.hip: 135 vs 128 TFLOP/s at 4096^3).
double tile_cost(const TileCfg& t, long M, long N, long k_tiles, int cus, int& splits_out) {
  const long tm = (M + t.bm - 1) / t.bm, tn = (N + t.bn - 1) / t.bn;
  const long tiles = tm * tn;
  const long slots = (long)cus * t.blocks_per_cu;
  // split K when the output alone cannot fill the chip and K is long (weight gradients:
  // K = batch); every slice keeps at least 8 k-tiles
  int splits = 1;
  // bias-sized outputs (N <= 32) with at least one tile per CU stream their big operand once whatever the
  // split: slabs and a second pass only add traffic (65536 x 10 x 512: 35 us as one pass of A)
  const bool skinny = N <= 32 && tiles >= cus;
  if (tiles < slots && k_tiles >= 32 && !skinny) {
    long want = slots / tiles;  // floor: one more slice would spill a few blocks into a second round
    long max_by_k = k_tiles / 8;
    splits = (int)(want < max_by_k ? want : max_by_k);
    if (splits < 1) splits = 1;
    if (splits > 1024) splits = 1024;
  }
  long per = (k_tiles + splits - 1) / splits;
  if (per < 1) per = 1;
  splits = (int)((k_tiles + per - 1) / per);
  if (splits < 1) splits = 1;
  splits_out = splits;
  const long blocks = tiles * splits;
  const long rounds = (blocks + slots - 1) / slots;
  // short K: the launch is bound by writing the output, which wants many waves in flight rather
  // than the 8-wave 256x256 block (one per CU)
  const double big = k_tiles >= 8 ? 1.05 : 0.8;
  const double eff = t.bm * t.bn >= 256 * 256 ? big : (t.bm * t.bn >= 128 * 128 ? 1.0 : 0.9);
  // edge tiles skip their empty 32x32 sub-blocks; co-resident blocks of a CU share the matrix
  // pipe, so with several blocks per CU the saved work shortens the round
  double fill = 1.0;
  if (t.blocks_per_cu > 1) {
    const double m32 = (double)((M + 31) / 32 * 32), n32 = (double)((N + 31) / 32 * 32);
    // only the matrix work shrinks (operand staging does not): credit half of it
    fill = 0.5 + 0.5 * (m32 * n32) / ((double)tm * t.bm * (double)tn * t.bn);
  }
  // a partial last round: its blocks have their CU (almost) to themselves and finish sooner than a
  // full round of co-resident blocks — but never faster than about 1.3 / blocks_per_cu of it
  const long tail = blocks % slots;
  double eff_rounds = (double)(blocks / slots);
  if (tail) {
    const double alone = 1.3 / t.blocks_per_cu < 1.0 ? 1.3 / t.blocks_per_cu : 1.0;
    const double share = (double)tail / (double)slots;
    eff_rounds += share > alone ? share : alone;
  }
  double cost = eff_rounds * t.blocks_per_cu * t.bm * t.bn * (double)per * fill / eff;
  // split-K with a ragged last tile row: plan_gemm cuts those tiles into fewer slices, the k-slices
  // of the full tiles shrink accordingly
  const long m_rest = M % t.bm;
  if (splits > 1 && rounds == 1 && m_rest != 0 && m_rest * 2 <= t.bm && tm >= 2) {
    const double share = ((double)(tm - 1) * tn + tn * ragged_tile_share(t.bm, m_rest)) / (double)tiles;
    cost = cost / fill * share;
  }
  if (splits > 1) cost += (double)M * N * splits * 0.02;  // second pass traffic
  return cost;
}

// ---- outputs wider than one narrow tile in both directions (M, N > 64): a time estimate per (tile, split).
//
// Calibrated on tools/sweep_mid.py (square problems 256 .. 4096, every tile x split, round 2).  A block
// needs `mfma` us of matrix-core time per 16-deep k-tile; alone on its CU it cannot go faster than `alone`
// us per k-tile (one wave per SIMD: the LDS-DMA round trip of the next k-tile is not hidden by the little
// matrix work of a small tile).  The busiest CU runs ceil(blocks / CUs) blocks, co-resident up to `blocks_per_cu`:
//     T = k-tiles per block x max(mfma x blocks on the busiest CU, alone x rounds) + fixed x rounds + second pass
// 1024^3: 64 x 64 tiles, one per CU, no split: 23.9 us (the old choice, 256 x 256 x 16 splits: 38.5 us);
// 3072^3: 64 x 64: 484 us (144 tiles of 256 x 256 leave 112 CUs idle: 584 us); 4096^3 keeps 256 x 256.
struct WideTile {
  int bm, bn, wm, wn, blocks_per_cu;
  double mfma, alone, alone_k32, fixed;
};
const WideTile kWideTiles[] = {
    {256, 256, 128, 64, 1, 3.80, 1.30, 1.30, 8.0},
    {128, 128, 64, 64, 4, 1.05, 0.70, 0.70, 8.0},
    {64, 64, 32, 32, 4, 0.25, 0.44, 0.27, 4.5},   // (0.275 / 0.30 until round 4; re-measured with sustained clocks: 2048^3 131.6 us, 3072^3 432; one block per CU = the wave-pair kernel: 1024 x 1024 x 4096 73.4)
};

// Matrix time of a tile with `rows` x `cols` valid outputs relative to a whole tile.  A ragged tile skips
// its empty 32 x 32 blocks, but the block is as slow as its busiest SIMD: wave w runs on SIMD w % 4, so
// 128 valid columns of a 256 x 256 tile (wave columns 2 and 3 idle) leave two SIMDs with the work of a whole
// tile (8192 x 128 x 8192 on 256 x 256 tiles: 278 us, as long as N = 256), while 128 valid ROWS halve it.
double ragged_tile_factor(const WideTile& t, long rows, long cols) {
  const int waves_m = t.bm / t.wm, waves_n = t.bn / t.wn, mi = t.wm / 32, ni = t.wn / 32;
  long load[4] = {0, 0, 0, 0};
  for (int wr = 0; wr < waves_m; ++wr)
    for (int wc = 0; wc < waves_n; ++wc) {
      long lm = (rows - (long)wr * t.wm + 31) / 32, ln = (cols - (long)wc * t.wn + 31) / 32;
      lm = lm < 0 ? 0 : (lm > mi ? mi : lm);
      ln = ln < 0 ? 0 : (ln > ni ? ni : ln);
      load[(wr * waves_n + wc) % 4] += lm * ln;
    }
  long worst = 0;
  for (long l : load) worst = l > worst ? l : worst;
  const long whole = (long)((waves_m * waves_n + 3) / 4) * mi * ni;
  return (double)worst / (double)whole;
}

double wide_tile_time(const WideTile& t, long M, long N, long k_tiles, int cus, bool vec, int& splits_out, bool k64 = false) {
  const long tm = (M + t.bm - 1) / t.bm, tn = (N + t.bn - 1) / t.bn;
  const long tiles = tm * tn;
  const long slots = (long)cus * t.blocks_per_cu;
  // whole tiles, the ragged last row / column / corner (clamped loop: ~10 % slower per k-tile)
  const long m_rest = M % t.bm, n_rest = N % t.bn;
  const long full_m = M / t.bm, full_n = N / t.bn;
  const double f_m = m_rest ? 1.1 * ragged_tile_factor(t, m_rest, t.bn) : 0, f_n = n_rest ? 1.1 * ragged_tile_factor(t, t.bm, n_rest) : 0;
  const double f_mn = m_rest && n_rest ? 1.1 * ragged_tile_factor(t, m_rest, n_rest) : 0;
  const double mean = ((double)full_m * full_n + f_m * full_n + f_n * full_m + f_mn) / (double)tiles;
  double worst = full_m && full_n ? 1.0 : 0;
  if (full_n && f_m > worst) worst = f_m;
  if (full_m && f_n > worst) worst = f_n;
  if (f_mn > worst) worst = f_mn;
  const long max_by_k = k_tiles / 8 > 1 ? k_tiles / 8 : 1;  // every slice keeps at least 8 k-tiles
  double best = 0;
  splits_out = 1;
  long last = 0;
  // candidate slice counts: a geometric ladder plus the counts that fill the CUs / the block slots exactly
  long cand[40];
  int ncand = 0;
  for (long want = 1; want <= 1024 && ncand < 32; want = want < 4 ? want + 1 : want + want / 2) cand[ncand++] = want;
  for (long fillers : {(long)cus / tiles, slots / tiles, 2 * (long)cus / tiles, (long)cus / tiles + 1})
    if (fillers > 1) cand[ncand++] = fillers;
  std::sort(cand, cand + ncand);
  for (int ci = 0; ci < ncand; ++ci) {
    const long want = cand[ci];
    if (want > max_by_k) break;
    const long per = (k_tiles + want - 1) / want;
    const long s = (k_tiles + per - 1) / per;
    if (s == last) continue;
    last = s;
    const long blocks = tiles * s;
    if (s > 1 && blocks > 2 * slots) break;  // more slices than the chip can hold at once only add slabs
    const long on_cu = (blocks + cus - 1) / cus, rounds = (blocks + slots - 1) / slots;
    // (one unsliced block per CU of 64 x 64 tiles: the wave-pair kernel, 0.27 for whole tiles, 0.285 ragged; otherwise the
    // four-wave kernel with 32-deep k-tiles, 0.30)
    const bool pair = s == 1 && on_cu == 1;
    const bool pair_whole = pair && k64 && m_rest == 0 && n_rest == 0;
    const double alone = (vec && t.bm == 64 && on_cu <= 2) ? (pair_whole ? t.alone_k32 : pair ? 0.285 : 0.30) : t.alone;
    // the busiest CU: its blocks are a sample of the tiles, never faster than one of the slowest kind.  More blocks than
    // slots of a tile that shares its CU four ways: the CUs pick up blocks as slots free up, so the busiest one carries
    // the average plus about half a block, not the next whole number (2304^3 on 64 x 64 tiles, 5.06 blocks per CU:
    // 202 us measured; "6 blocks" predicted 225 and lost to a sliced 256 x 256 launch that takes 230)
    double load = (double)on_cu;
    if (blocks > slots && t.blocks_per_cu >= 4) {
      const double avg = (double)blocks / (double)cus;
      load = blocks % cus == 0 ? avg : avg + 0.5;
    }
    double matrix = t.mfma * (load * mean > worst ? load * mean : worst);
    if (s > 1 && rounds == 1 && m_rest != 0 && m_rest * 2 <= t.bm && tm >= 2)  // plan_gemm: ragged rows get fewer slices
      matrix = t.mfma * (double)on_cu * ((double)(tm - 1) * tn + tn * ragged_tile_share(t.bm, m_rest)) / (double)tiles;
    const double step = matrix > alone * rounds ? matrix : alone * rounds;
    double time = (double)per * step + t.fixed * rounds;
    if (s > 1) {
      const double mb = (double)M * N * 4e-6;           // one slab, MB
      time += 4.5 + mb * (double)s / 4.0 + mb * (double)(s + 1) / 4.5;  // second launch (3.0 until round 4: 384^3 and 512^3 sliced 11.0 / 13.1 us, unsliced 9.7 / 11.9) + slabs out at ~4 TB/s, second pass at ~4.5
    }
    if (best == 0 || time < best) {
      best = time;
      splits_out = (int)s;
    }
  }
  return best;
}

// blocks of a tile that share one CU
long blocks_per_cu(int bm, int bn) { return bm * bn >= 256 * 256 ? 1 : (bm == 256 ? 2 : 4); }

}  // namespace

bool small_suits(long M, long N, long K) {
  // (2.6 M multiply-adds: above that the matrix tiles are faster since round 4 — 128 x 128 x 256 10.1 us here, 5.2 on eight-wave
  // 32 x 32 tiles; 96 x 96 x 400 10.8 / 6.8; 80 x 160 x 300 10.7 / 5.7; equal at 100 x 128 x 200 and below)
  return M * N <= 16384 && K <= 2048 && M * N * K <= (5L << 19) && K > 0 && M > 0 && N > 0;
}

void choose_tile(long M, long N, long K, int cus, const GemmSwitches& sw, int& bm, int& bn, int& splits, bool vec, bool plain) {
  const long k_tiles = (K + BK - 1) / BK;
  // (convolutions keep their measured choices; with fewer than 8 k-tiles a launch is bound by writing its output, which
  // the time model does not describe: 65536 x 512 x 10 with a generated epilogue, 67 us on the tile the older rule picks, 79 us)
  if (plain && M > 64 && N > 64 && k_tiles >= 8 && !sw.old_tile_model && !sw.force_tile) {
    double best = 0;
    for (const WideTile& t : kWideTiles) {
      int sp;
      const double time = wide_tile_time(t, M, N, k_tiles, cus, vec, sp, K % 64 == 0);
      if (sw.debug_tile) fprintf(stderr, "[eg] tile model %ld x %ld x %ld: %d x %d, %d slices: %.1f us\n", M, N, K, t.bm, t.bn, sp, time);
      if (best == 0 || time < best * 0.97) {  // larger tiles listed first: a smaller one has to win by 3 %
        best = time;
        bm = t.bm;
        bn = t.bn;
        splits = sp;
      }
    }
  } else {
    // Candidates: 256x256 (16 waves, 1 block/CU) for large outputs, 128x128 (4 waves, 4 blocks/CU),
    // and narrow tiles for bias-sized N (the N = 1/4/10 layers of the XOR and dense nets, F = 64
    // filter banks) so the padding wasted in the matrix core stays small.
    static const TileCfg cfgs[] = {{256, 256, 1}, {128, 128, 4}, {128, 64, 4}, {128, 32, 4}, {256, 64, 2}, {64, 64, 4}};
    const int forced_bm = sw.force_tile ? sw.force_bm : 0, forced_bn = sw.force_tile ? sw.force_bn : 0;  // tuning aid
    int best = 1, best_splits = 1;
    double best_cost = 0;
    for (int c = 0; c < 6; ++c) {
      if (forced_bm && (cfgs[c].bm != forced_bm || cfgs[c].bn != forced_bn)) continue;
      if (!forced_bm) {
        // 64-wide tiles: narrow outputs, or a single tile row (M <= BM: the filter gradient of a
        // convolution, M = F)
        if (cfgs[c].bn == 64 && N > 64 && M > cfgs[c].bm) continue;
        if (cfgs[c].bn == 32 && N > 32) continue;
        if (cfgs[c].bn >= 128 && N <= 64) continue;
      }
      int sp;
      const double cost = tile_cost(cfgs[c], M, N, k_tiles, cus, sp);
      if (best_cost == 0 || cost < best_cost) {
        best = c;
        best_cost = cost;
        best_splits = sp;
      }
    }
    bm = cfgs[best].bm;
    bn = cfgs[best].bn;
    splits = best_splits;
  }
  if (sw.force_splits) {  // tuning aid
    const int want = sw.force_splits_n;
    if (want >= 1 && want <= k_tiles) {
      const long per = (k_tiles + want - 1) / want;
      splits = (int)((k_tiles + per - 1) / per);
    }
  }
}

// The load variant of a tile kb deep: the clamped form for ragged tiles; whole tiles and 16-byte operands load with
// LDS-DMA, and 128 x 32 tiles have a form for a 16-byte A next to a scalar B.
void set_variant(GemmPlan& t, const GemmProblem& p) {
  t.edge = p.conv || !(p.vec_ok && p.M % t.bm == 0 && p.N % t.bn == 0 && p.K % t.kb == 0 && p.K > 0);
  t.vec = !t.edge || p.vec_ok ? 4 : (t.bn == 32 && p.a_vec_only ? 41 : 1);
}

GemmPlan generic_tile(const GemmProblem& p, const GemmSwitches& sw, bool model_vec) {
  GemmPlan t;
  choose_tile(p.M, p.N, p.K, p.cus, sw, t.bm, t.bn, t.splits, model_vec, p.conv == 0);
  t.waves = tile_waves(t.bm, t.bn);
  set_variant(t, p);
  return t;
}

// Whole tiles leave through LDS as 16-byte stores (GemmArgs::wide_store) when every address the
// epilogue touches is 16-byte aligned: the output (or the split-K slabs, which come from the
// workspace), the bias, and whole rows of four.
bool wide_store_ok(const GemmProblem& p, const GemmSwitches& sw, bool to_partial, bool fused) {
  if (sw.no_wide_store || p.N % 4 != 0) return false;
  // measured: +2.5 % at 4096^3, -10 % on a 65536 x 512 x 10 product (two barriers per block row against
  // almost no k loop): plain contractions with fewer than 8 k-tiles keep the direct stores
  if (!fused && p.K < 8 * BK) return false;
  if (to_partial) return (p.M * p.N) % 4 == 0;   // slabs are [split][M][N] in the 256-byte aligned workspace
  return p.ldc % 4 == 0 && p.c_aligned && (!p.has_bias || p.bias_aligned);
}

GemmPlan plan_gemm(const GemmProblem& p, const GemmSwitches& sw) {
  const long M = p.M, N = p.N, K = p.K, cus = p.cus;
  GemmPlan r;
  const bool whole_call = !p.piece && !p.ones_row && !p.conv;
  if (whole_call && small_suits(M, N, K) && !sw.no_small) {
    r.route = Route::Small;
    r.grid = (M * N + 3) / 4;
    r.block = 256;
    return r;
  }
  // tall and skinny: stream A once with B resident in LDS
  if (whole_call && p.a_kc && !p.b_kc && N <= 16 && K >= 64 && K <= 1024 && K % 16 == 0 && M >= 4096 && p.lda % 4 == 0 && p.a_aligned &&
      !sw.no_skinny) {
    r.route = Route::Skinny;
    const long groups = (M + 15) / 16;
    r.grid = std::min((groups + 3) / 4, 8L * cus);  // (LDS: K x 64 bytes per block; eight blocks of four waves per CU)
    r.block = 256;
    return r;
  }
  r = generic_tile(p, sw, p.vec_ok);
  const int BM = r.bm, BN = r.bn;
  int splits = r.splits;
  r.splits = 1;
  r.k_per_split = K;
  r.no_skew = sw.no_skew;
  // the pair kernels and stream-K: 16-byte operands, a plain product, 16-byte aligned whole rows of C and the bias
  const bool pair_ok = !p.conv && p.vec_ok && !p.a_vec_only && !p.ones_row;
  const bool c_rows16 = p.ldc % 4 == 0 && p.c_aligned && (!p.has_bias || p.bias_aligned);
  const bool tuned = sw.force_tile || sw.force_splits;
  // Small outputs — between half a chip and three chips of 32 x 32 tiles (512 x 512: 256 of them, 64 of 64 x 64): one
  // 32 x 32 tile per block, eight waves that split every 128-deep k-tile (gemm_f32_pair.hpp, KW = 8), unsliced whatever K
  // is, up to K = 4096: 512^3 13.1 -> 8.0 us NN, 13.4 -> 6.1 TN; 384^3 10.7 -> 6.4; 500 x 500 x 1000 17.3 -> 9.3; 512 x 512 x 2048
  // 20.1 -> 13.3; equal at K = 4096 (25.3 / 26.4); a long K is bound by the tile's loads (512 x 512 x 65536: 337 us against 282
  // for sliced 64 x 64 tiles).  EG_GEMM_NO_PAIR=1 (or a forced tile / slice count) keeps the choice below.
  // (whole tiles: 64 KB of LDS, two blocks share a CU — up to three blocks per CU pay: 640^3 14.4 -> 9.4 us, 768^3 16.7 -> 14.9,
  // 768 x 768 x 2048 35.9 -> 31.6; 896^3 and 1024^3 do not.  Ragged: 96 KB, one block per CU: up to two per CU, 576^3 13.5 -> 12.8)
  // (fewer tiles than half a chip: still better than slices with their second launch while K is short — 256 x 256 x 512
  // 12.0 -> 6.7 us, 256 x 256 x 1024 14.9 -> 8.1, 320 x 320 x 1024 14.7 -> 7.8, 256^3 7.9 -> 6.4; at K = 2048 the slices win, 10.6
  // against 12.6.)
  // (four stages — three 128-deep k-tiles in flight, 128 KB of LDS — measured equal: 512^3 5.7 / 5.7 us back to back, 512 x 512 x 2048 13.3 / 12.9)
  const long t32 = ((M + 31) / 32) * ((N + 31) / 32);
  const bool kw8_ragged = M % 32 != 0 || N % 32 != 0 || K % 128 != 0;
  if (!sw.no_pair && !tuned && pair_ok && t32 <= (kw8_ragged ? 2L : 3L) * cus && (2 * t32 >= cus || (K <= 1024 && t32 >= 4)) &&
      K >= 256 && K <= 4096 && N % 4 == 0 && c_rows16) {
    r.route = Route::Kw8;
    r.edge = kw8_ragged;
    r.tiles_m = (int)((M + 31) / 32);
    r.tiles_n = (int)((N + 31) / 32);
    r.grid = t32;
    r.block = 512;
    return r;
  }
  // 96 x 96 tiles (round 5): an output that is ONE round of them — 1536^2 = 256 tiles on 256 CUs — is 2.25 rounds of 64 x 64
  // tiles (576 blocks: three on some CUs, two on others: 0.59 of peak) and a quarter of a round of 256 x 256.  Same kernel as
  // the wave pairs (gemm_f32_pair.hpp), three 96 x 32 sub-tiles per block, each shared by FOUR waves that split every
  // 64-deep k-tile (12 waves = three per SIMD, 24 matrix instructions per wave and k-tile).  EG_GEMM_NO_PAIR=1 keeps 64 x 64.
  const long t96 = (M / 96) * (N / 96);
  if (!sw.no_pair && !sw.no_t96 && !tuned && pair_ok && M % 96 == 0 && N % 96 == 0 && K % 64 == 0 && K >= 512 && t96 <= cus &&
      4 * t96 > 3L * cus && c_rows16) {
    r.route = Route::T96;
    r.tiles_m = (int)(M / 96);
    r.tiles_n = (int)(N / 96);
    r.grid = t96;
    r.block = 768;
    return r;
  }
  // Stream-K on 64 x 64 tiles (round 6; gemm_streamk_kernel): the planner's choice is unsliced 64 x 64 tiles, there are more
  // tiles than CUs, and they do not divide evenly over the four block slots of a CU — the launch is as long as its busiest
  // CU (1280^3: 400 tiles, 1.56 per CU; 1792^3: 784 tiles, 3.06 per CU).  Persistent blocks (four per CU) share the
  // (tile, k-tile) space evenly instead; the tiles they cut are folded in k order by one more launch.  EG_GEMM_NO_STREAMK=1 off.
  if (BM == 64 && BN == 64 && splits == 1 && pair_ok && M % 64 == 0 && N % 64 == 0 && K % 32 == 0 && K >= 256 && c_rows16 &&
      !sw.no_streamk && !tuned) {
    const long tiles = (M / 64) * (N / 64), slots = 4 * cus;
    const long nk = K / 32;
    const long busiest = (tiles + cus - 1) / cus;
    const double even = (double)tiles / (double)cus;
    // Every tile's units are shared (rounds = 0) by four blocks per CU (two when there are fewer than two tiles per CU).  The
    // hybrid form — `rounds` whole tiles per block first, only the remaining tiles shared — is kept behind the tuning aid
    // EG_STREAMK_BLOCKS_PER_CU: it wins at 2560^3 (278 -> 265 us) and loses at 1792^3 (three blocks per CU: 118 against 105).
    long g = tiles > 2 * cus ? 4 : 2, rounds = 0;
    // More tiles than block slots: whole rounds of tiles first (one per block and round, stored directly), only the tiles of
    // the partial last round shared — worth it while that round is at most 0.6 full and K is long (2432^3 238 -> 233 us, 2560^3
    // 280 -> 269, 2560 x 2560 x 4096 446 -> 425, 3584^3 733 -> 720; 2688^3 / 2816^3, last round 0.72 / 0.89 full: 3 % slower;
    // K = 1024: slower).
    bool hybrid = false;
    if (tiles >= slots && nk >= 64) {
      const long last = tiles % slots;
      if (last > 0 && 10 * last <= 6 * slots) {
        g = 4;
        rounds = tiles / slots;
        hybrid = true;
      }
    }
    if (sw.streamk_blocks) {   // tuning aid
      g = sw.streamk_blocks_per_cu;
      rounds = tiles / (g * cus);
      hybrid = false;
    }
    const long grid = g * cus;
    const long rest = tiles - rounds * grid;          // tiles the blocks share unit by unit
    // a block's share of the units: even, but at least four k-tiles (a piece pays a prologue and a slab)
    long per = (rest * nk + grid - 1) / grid;
    if (per < 4) per = 4;
    // What it buys: (1 - even / busiest) of the one-block-per-tile launch, whose length is about busiest x nk x 0.51 us
    // (2048^3: four blocks per CU, 64 k-tiles, 131 us); with more tiles than block slots the dispatcher refills slots as they
    // free up and the busiest CU carries about even + 0.5.  What it costs: nearly every tile is cut, so the output travels
    // through the slabs and a second launch — 14 us at 1792^3.  Measured (tools/streamk_ab.py): 1792^3 115 -> 105 us, 1280 x
    // 1280 x 4096 139 -> 122, 1152^3 42.6 -> 39.3; equal at 1280^3; 3 - 5 % slower at 1664^3 / 1920^3 / 2304^3 — hence the bar.
    const double busiest_eff = tiles >= slots ? even + 0.5 : (double)busiest;
    const double saved_us = (1.0 - even / busiest_eff) * busiest_eff * (double)nk * 0.51;
    if (tiles > cus && tiles < 6 * slots && rest > 0 && (hybrid || saved_us >= sw.streamk_min_ratio)) {
      r.route = Route::StreamK;
      r.tiles_m = (int)(M / 64);
      r.tiles_n = (int)(N / 64);
      r.splits = (int)rounds;
      r.k_per_split = per;
      r.nt_store = r.no_skew = r.prio = false;
      r.grid = grid;
      r.block = 256;
      r.workspace_floats = grid * 2 * 64 * 64;
      r.second = Second::StreamKFixup;
      return r;
    }
  }
  // (the same design on one round of 128 x 128 tiles — four 64 x 64 sub-tiles x four waves — measured equal to what the model
  //  picks: 2048^3 129.1 against 130.7 us, 1792^3 113.1 / 113.9, 2048 x 2048 x 512 40.8 / 39.2: the gain above is the whole round, not the wave count)
  // A few rows / columns beyond whole 256 x 256 tiles of a large output (4100 = 16 x 256 + 4): the ragged
  // tile row and column stage whole operand tiles for 1/64 of the matrix work and push the launch into another
  // round of blocks (4100 x 4096 x 4096: +76 us, 4096 x 4100 x 4096: +154 us over 969 us).  As contractions
  // of their own they are one pass over the other operand (4 x 4100 x 4100: 30 us), so the output is cut into
  // whole tiles + remainder rows + remainder columns when the ragged tiles would cost a round.  Split-K launches keep
  // their ragged tiles: those get fewer, longer k-slices next to the whole tiles at about the same cost.
  if (!p.conv && p.vec_ok && !p.a_vec_only && splits == 1 && !p.ones_row) {
    const long m_rem = M % 256, n_rem = N % 256;
    const long m0 = M - (m_rem <= 32 ? m_rem : 0), n0 = N - (n_rem <= 32 ? n_rem : 0);
    const long tiles_all = ((M + 255) / 256) * ((N + 255) / 256), tiles_main = ((m0 + 255) / 256) * ((n0 + 255) / 256);
    const bool saves_round = (tiles_all + cus - 1) / cus > (tiles_main + cus - 1) / cus;
    int bm_main = 0, bn_main = 0, splits_main = 0;
    if ((m0 < M || n0 < N) && m0 >= 256 && n0 >= 256 && n0 % 4 == 0 && m0 % 4 == 0 && saves_round)
      choose_tile(m0, n0, K, p.cus, sw, bm_main, bn_main, splits_main, p.vec_ok);  // the whole-tile part on its own: 256 x 256 tiles, no split-K?
    if (bm_main == 256 && bn_main == 256 && splits_main == 1) {
      r.route = Route::Remainder;
      r.parts[r.nparts++] = {0, 0, m0, n0};
      if (m0 < M) r.parts[r.nparts++] = {m0, 0, M - m0, N};    // remainder rows, every column
      if (n0 < N) r.parts[r.nparts++] = {0, n0, m0, N - n0};   // remainder columns of the whole-tile rows
      return r;
    }
  }
  // Extra rows (GemmArgs::x_rows): a TN product with a long K (a weight gradient: K = the batch) whose M is a few rows
  // beyond whole 256-row tiles and whose tiles cannot fill the chip by themselves.  The last tile row's blocks carry the
  // extra rows as a ninth accumulator block (+ 1/8 matrix work) and get proportionally more, shorter k-slices, so every
  // block finishes together; no ragged tile row exists.  EG_GEMM_NO_XROW=1: the ragged tile row of round 2.
  if (!sw.no_xrow && !p.conv && p.vec_ok && !p.a_vec_only && !p.a_kc && !p.b_kc && M > 256 && M % 256 > 0 && M % 256 <= 32 &&
      N % 256 == 0 && K % BK == 0 && p.ldc % 4 == 0 && !sw.force_tile) {
    const long tm = M / 256, tn = N / 256, k_tiles = K / BK;
    const long full = (tm - 1) * tn;
    long best_s1 = 0, best_s2 = 0;
    double best_t = 0;
    // k-tile of a strip-carrying block relative to a plain one
    constexpr double xw = 1.2;  // measured on 784 x 512 x 65536: 1.0 449 us, 1.125 441, 1.2 428, 1.3 446, 1.4 452 (the strip adds 2 DMA pieces and 16 LDS reads per k-tile to its 4 MFMAs)
    for (long s1 = 2; full * s1 + tn * 2 <= cus && s1 <= k_tiles / 8; ++s1) {
      long s2 = (cus - full * s1) / tn;
      if (s2 > k_tiles / 8) s2 = k_tiles / 8;
      if (s2 < 2) continue;
      const long per1 = (k_tiles + s1 - 1) / s1, per2 = (k_tiles + s2 - 1) / s2;
      const double t = std::max((double)per1, xw * (double)per2);  // k-tiles of the slowest block, in whole-tile units
      if (best_s1 == 0 || t < best_t) {
        best_t = t;
        best_s1 = s1;
        best_s2 = s2;
      }
    }
    if (full == 0) {  // a single tile row: every block carries the strip
      long s2 = cus / tn;
      if (s2 > k_tiles / 8) s2 = k_tiles / 8;
      if (s2 >= 2) best_s1 = best_s2 = s2;
    }
    if (best_s1 >= 2 && best_s2 >= 2) {
      const long per1 = (k_tiles + best_s1 - 1) / best_s1, per2 = (k_tiles + best_s2 - 1) / best_s2;
      const long s1 = (k_tiles + per1 - 1) / per1, s2 = (k_tiles + per2 - 1) / per2;
      r.route = Route::ExtraRows;
      r.bm = r.bn = 256;
      r.tiles_m = (int)tm;
      r.tiles_n = (int)tn;
      r.x_rows = (int)(M % 256);
      r.splits = (int)s1;
      r.k_per_split = per1 * BK;
      r.edge_splits = (int)s2;
      r.k_per_split_edge = per2 * BK;
      r.wide_store = wide_store_ok(p, sw, true);
      r.grid = full * s1 + tn * s2;
      r.block = 512;
      r.workspace_floats = ((std::max(s1, s2) * M * N + 3) & ~3L);
      // rows of the last tile row and the extra rows were cut into s2 slices, the others into s1
      r.second = Second::SplitReduce;
      return r;
    }
  }
  // (32-deep k-tiles for the 256x256 tile were measured in round 2: +1 % at 4096^3, -7 % at K = 784, 0 elsewhere)
  // the convolution's filter gradient (M = F = 64 rows, 64 x 64 tiles, K = every output pixel): a block has
  // little matrix work per barrier, so its k-tiles are 32 deep like the forward gather's
  int KB = (p.conv == 2 && BM == 64 && BN == 64 && p.vec_ok) ? 32 : BK;
  // 64 x 64 tiles with at most two blocks per CU are bound by the LDS-DMA round trip of the next k-tile, not
  // by matrix work: 32-deep k-tiles halve the round trips (1024^3: 28.1 -> 23.9 us; four blocks per CU hide
  // it by themselves: 2048^3 142.5 vs 146.5 us).
  // Round 4, sustained clocks: 32 also wins with up to four blocks per CU (1536^3 81.4 -> 77.0 us, 1792^3 120.8 -> 114.4,
  // 2048^3 137.9 -> 131.6); beyond that the two are equal within 1 % (2304^3 202 / 206, 3072^3 432 / 439): 16 stays there.
  if (!p.conv && BM == 64 && BN == 64 && p.vec_ok && K >= 256 && ((M + 63) / 64 * ((N + 63) / 64) * splits <= 4L * cus || sw.small_bk32))
    KB = 32;
  const long k_tiles = (K + KB - 1) / KB;
  r.kb = KB;
  r.tiles_m = (int)((M + BM - 1) / BM);
  r.tiles_n = (int)((N + BN - 1) / BN);
  long tiles_per_split = (k_tiles + splits - 1) / splits;
  if (tiles_per_split < 1) tiles_per_split = 1;
  r.k_per_split = tiles_per_split * KB;
  splits = (int)((k_tiles + tiles_per_split - 1) / tiles_per_split);  // no empty slice (the count was planned in 16-deep k-tiles)
  if (splits < 1) splits = 1;
  r.splits = splits;
  // Tiny outputs split many ways (the XOR net's [2,4] and [4,1] weight gradients): a
  // per-element serial walk over hundreds of slabs is latency bound, so the slabs are folded
  // with the tree column-sum instead of the serial second pass.
  const long total = M * N;
  const bool tree_reduce = splits > 1 && (total <= 4096 || (splits >= 64 && total <= 65536)) && p.ldc == N && !p.has_bias;
  // Ragged last tile row (M = 784 with 128-row tiles: 16 rows): its blocks run a fraction of the
  // matrix work but, cut like the others, would occupy their CU slots just as long.  Give them
  // fewer, longer slices so every block carries about the same work; the freed slots go to the
  // full tiles.  Needs the LDS-DMA loop (cheap ragged tiles) and the serial second pass.
  const long m_rest = M % BM;
  if (splits > 1 && !tree_reduce && !p.conv && p.vec_ok && m_rest != 0 && m_rest * 2 <= BM && r.tiles_m >= 2) {
    const double frac = ragged_tile_share(BM, m_rest);
    const long full_tiles = (long)(r.tiles_m - 1) * r.tiles_n;
    const long slots = cus * blocks_per_cu(BM, BN);
    long s_full = (long)((double)slots / ((double)full_tiles + r.tiles_n * frac));
    const long max_by_k = k_tiles / 8;
    if (s_full > max_by_k) s_full = max_by_k;
    long s_edge = (long)(s_full * frac + 0.5);
    if (s_full >= 2 && s_edge >= 1 && s_edge < s_full) {
      long per_full = (k_tiles + s_full - 1) / s_full;
      s_full = (k_tiles + per_full - 1) / per_full;
      long per_edge = (k_tiles + s_edge - 1) / s_edge;
      s_edge = (k_tiles + per_edge - 1) / per_edge;
      r.k_per_split = per_full * KB;
      r.splits = (int)s_full;
      r.edge_splits = (int)s_edge;
      r.k_per_split_edge = per_edge * KB;
    }
  }
  // Tail tiles: more tiles than block slots and a short last round -> cut the last round's tiles along K.
  if (splits == 1 && !p.conv) {
    const long tiles = (long)r.tiles_m * r.tiles_n;
    const long slots = cus * blocks_per_cu(BM, BN);
    const long tail = tiles % slots;
    if (tiles > slots && tail > 0 && tail * 2 <= slots && k_tiles >= 16) {
      long ts = slots / tail;
      if (ts > k_tiles / 8) ts = k_tiles / 8;
      if (ts > 16) ts = 16;
      if (ts >= 2) {
        const long per = (k_tiles + ts - 1) / ts;
        ts = (k_tiles + per - 1) / per;
        r.tail_tiles = (int)tail;
        r.tail_splits = (int)ts;
        r.tail_k_per_split = per * KB;
      }
    }
  }
  r.wide_store = wide_store_ok(p, sw, splits > 1);
  set_variant(r, p);
  const bool one_pass = splits <= 1 && r.tail_tiles == 0 && r.edge_splits == 0;
  // Whole 256 x 256 tiles of a long, unsliced product: 32-deep k-tiles (half the barriers and half the load issues per
  // MFMA; 128 KB of LDS, still one block per CU).  With the skewed waves of round 4 on top: 4096^3 949 -> 941 us in the
  // harness (+0.8 %); short products keep 16 (K = 784: round 2 measured -7 % with 32).  EG_GEMM_NO_BK32=1: 16 everywhere.
  if (!sw.no_bk32 && BM == 256 && BN == 256 && !r.edge && !p.conv && one_pass && K % 32 == 0 && K >= 2048 && r.k_per_split == K) {
    r.route = Route::Bk32;
    r.kb = 32;
    r.grid = (long)r.tiles_m * r.tiles_n;
    r.block = 512;
    return r;
  }
  // Wave pairs (gemm_f32_pair.hpp): whole 64 x 64 tiles of an unsliced product with at most one block per CU — one wave
  // per SIMD on the four-wave kernel, where a k-tile costs 1.36x its matrix time (barrier + fragment reads, measured with
  // the loads removed).  Two waves per sub-tile split every 64-deep k-tile, the odd one a k-group late: 1024^3 22.1 ->
  // 20.9 us (NN / NT), 23.1 -> 19.8 (TN), 512^3 12.3 -> 11.6.  With two or more blocks per CU the four-wave kernel is
  // as fast or faster (1536^3, 3072^3), so those keep it.  Not bit-identical to it (two f32 chains per element instead
  // of one); EG_GEMM_NO_PAIR=1 keeps the four-wave kernel.
  // Ragged tiles and a K that ends inside a k-tile take the EDGE form of the same kernel (clamped row / column offsets,
  // masked stores, the k-tile K ends in loaded in the prologue and multiplied behind the loop): 1000^3 28.1 -> 23.1 us (NN),
  // 27.5 -> 22.0 (TN), 1000 x 1024 x 4096 90.8 -> 74.6.
  // (four waves per sub-tile, 16 per block, 128-deep k-tiles: 1024^3 21.9 us either way, 1024 x 1024 x 4096 76.1 against 77.2 — not taken)
  if (!sw.no_pair && BM == 64 && BN == 64 && p.vec_ok && !p.conv && one_pass && r.wide_store && !p.ones_row &&
      (long)r.tiles_m * r.tiles_n <= cus) {
    r.route = Route::Pair;
    r.edge = r.edge || K % 64 != 0;
    r.grid = (long)r.tiles_m * r.tiles_n;
    r.block = 512;
    return r;
  }
  r.block = (BM / r.waves.wm) * (BN / r.waves.wn) * 64;
  if (r.tail_tiles > 0) {
    r.grid = (long)r.tiles_m * r.tiles_n - r.tail_tiles + (long)r.tail_tiles * r.tail_splits;
    r.workspace_floats = (long)r.tail_tiles * r.tail_splits * BM * BN;
    r.second = Second::TailReduce;
    return r;
  }
  const long rows_m = r.edge_splits > 0 ? r.tiles_m - 1 : r.tiles_m;
  r.grid = rows_m * r.tiles_n * r.splits + (long)r.tiles_n * r.edge_splits;
  if (splits > 1) {
    r.workspace_floats = ((long)r.splits * total + 3) & ~3L;
    r.second = tree_reduce ? Second::Tree : Second::SplitReduce;
  }
  return r;
}

GemmPlan plan_gemm_batched(const GemmProblem& item, long batch, const GemmSwitches& sw) {
  const long M = item.M, N = item.N, K = item.K;
  GemmPlan r;
  r.route = Route::Generic;
  // 64 x 64 tiles for every item: the most blocks, and four of them per CU.  The only tile that is built.
  // (Tried and dropped: 128 x 128 tiles whenever the launch still had two blocks for every CU, slower at every shape that
  // reached them — the figures are in profiles/batched_gemm.txt; items large enough to want a larger tile fill the chip by
  // themselves and run as plain products, batched_runs_as_loop.  Not measured, so not built: 128 x 32 tiles for a
  // bias-sized N.  sw.force_tile is not read: the launch has this one tile.)
  r.bm = r.bn = 64;
  r.kb = BK;
  r.waves = tile_waves(r.bm, r.bn);
  set_variant(r, item);
  r.tiles_m = (int)((M + r.bm - 1) / r.bm);
  r.tiles_n = (int)((N + r.bn - 1) / r.bn);
  r.splits = 1;
  r.k_per_split = std::max<long>(((K + BK - 1) / BK) * BK, BK);
  r.wide_store = wide_store_ok(item, sw, false);
  r.no_skew = sw.no_skew;
  r.grid = batch * r.tiles_m * r.tiles_n;
  r.block = (r.bm / r.waves.wm) * (r.bn / r.waves.wn) * 64;
  return r;
}

bool batched_runs_as_loop(const GemmProblem& item, const GemmSwitches& sw) {
  const GemmPlan p = plan_gemm(item, sw);
  if (p.route == Route::Remainder) return true;   // (whole 256 x 256 tiles and then some)
  return p.grid >= item.cus && p.route != Route::Small;
}

bool batched2_c_distinct(long batch0, long stride_c0, long batch1, long stride_c1, long M, long ldc, long N) {
  struct Axis {
    long extent, stride;
  };
  Axis axes[4] = {{batch0, stride_c0}, {batch1, stride_c1}, {M, ldc}, {N, 1}};
  int n = 0;
  for (const Axis& a : axes) {
    if (a.extent < 1) return false;
    if (a.extent > 1) axes[n++] = a;
  }
  std::sort(axes, axes + n, [](const Axis& x, const Axis& y) { return x.stride > y.stride; });
  // from the fastest axis up: `span` is the largest offset the axes behind this one reach (128-bit: extents and strides are
  // the caller's 64-bit numbers)
  __int128 span = 0;
  for (int q = n - 1; q >= 0; --q) {
    if ((__int128)axes[q].stride < span + 1) return false;
    span += (__int128)(axes[q].extent - 1) * axes[q].stride;
  }
  return true;
}

// ---- float64 -----------------------------------------------------------------------------------------------------------
namespace {

// Tile shape by a small time model.  What a SIMD's matrix pipe delivers depends on how many waves multiply on it at the
// same time (tools/mfma_ceiling_f64.hip: one wave 0.44 of peak, two 0.99 in a bare loop), so a launch is priced as
// rounds of resident blocks, each round at the rate of the waves it puts on a SIMD:
//   config        waves      blocks / CU (LDS)   relative loop efficiency
//   128 x 128     8 (2 x 4)  2 (74 KB)           1.00
//   128 x  64     8 (4 x 2)  2 (55 KB)           0.97
//    64 x  64     8 (2 x 4)  4 (37 KB)           0.92
struct DgemmCfg {
  int bm, bn, wr, wc, cap;
  double eff;
};
const DgemmCfg kDgemmCfgs[3] = {{128, 128, 2, 4, 2, 1.0}, {128, 64, 4, 2, 2, 0.97}, {64, 64, 2, 4, 4, 0.92}};

double dgemm_rate(long waves_per_simd) { return waves_per_simd <= 1 ? 0.44 : waves_per_simd == 2 ? 0.80 : waves_per_simd == 3 ? 0.88 : 0.92; }

double dgemm_cost(const DgemmCfg& c, long M, long N, long K, long cus, long splits) {
  const long tiles = ((M + c.bm - 1) / c.bm) * ((N + c.bn - 1) / c.bn) * splits;
  const double t_tile = (double)c.bm * c.bn * ((double)K / splits) / c.eff;  // matrix work of one block at the pipe's full rate
  const long slots = cus * c.cap;
  const long full = tiles / slots, rem = tiles % slots;
  double t = (double)full * c.cap * t_tile / dgemm_rate(2L * c.cap);  // 8-wave blocks: two waves per SIMD each
  if (rem > 0) {
    const long per_cu = (rem + cus - 1) / cus;
    t += (double)per_cu * t_tile / dgemm_rate(2L * per_cu);
  }
  // slabs out and back (16 bytes per element and slice at ~3 TB/s, in units of a CU's 64 multiply-adds per clock) and a second launch (~5 us)
  if (splits > 1) t += (double)M * N * splits * 1.0 + 8.0e5;
  return t;
}

}  // namespace

DgemmPlan plan_dgemm(const DgemmProblem& p) {
  const long M = p.M, N = p.N, K = p.K, cus = p.cus;
  // the cheapest (config, slices): 1, 2, 4, ... 64 slices of at least 256 each; on a tie the larger tile and the fewer slices
  int best = 0;
  long best_splits = 1;
  double best_t = 1e300;
  for (int c = 0; c < 3; ++c)
    for (long splits = 1; splits <= 64 && (splits == 1 || K / splits >= 256); splits *= 2) {
      const double t = dgemm_cost(kDgemmCfgs[c], M, N, K, cus, splits);
      if (t < best_t) {
        best_t = t;
        best = c;
        best_splits = splits;
      }
    }
  if (p.force_config >= 0) best = p.force_config % 3;
  if (p.force_splits > 0) best_splits = p.force_splits;
  DgemmPlan r;
  r.config = best;
  const DgemmCfg& cfg = kDgemmCfgs[best];
  r.bm = cfg.bm;
  r.bn = cfg.bn;
  r.wr = cfg.wr;
  r.wc = cfg.wc;
  r.vec = dgemm_vec(p.lda, p.ldb, p.a_aligned, p.b_aligned);
  r.k_per_split = dgemm_k_unsliced(K);
  // slices of whole k-tiles, none of them empty; one slice is the unsliced product (no slabs, no second launch)
  if (best_splits > 1) {
    long per = (K + best_splits - 1) / best_splits;
    per = ((per + BK - 1) / BK) * BK;
    const long splits = (K + per - 1) / per;
    if (splits > 1) {
      r.splits = (int)splits;
      r.k_per_split = per;
      r.workspace_doubles = splits * M * N;
      r.reduce = true;
    }
  }
  r.tiles_m = (int)((M + r.bm - 1) / r.bm);
  r.tiles_n = (int)((N + r.bn - 1) / r.bn);
  r.grid_x = (long)r.tiles_m * r.tiles_n;
  r.grid_y = r.splits;
  r.remap = dgemm_remap(r.grid_x);
  return r;
}

bool dgemm_batched_vec(const DgemmBatchedProblem& p) {
  const bool outer_even = p.batch <= 1 || (p.stride_a % 2 == 0 && p.stride_b % 2 == 0);
  const bool inner_even = p.batch1 <= 1 || (p.stride_a1 % 2 == 0 && p.stride_b1 % 2 == 0);
  return dgemm_vec(p.lda, p.ldb, p.a_aligned, p.b_aligned) && outer_even && inner_even;
}

// The rule: an item whose 64 x 64 tiles number at least DGEMM_LOOP_TILES_PER_CU per CU runs as a plain product — it
// has a block for every CU by itself, the condition of the float32 rule (batched_runs_as_loop), and eg_dgemm may give it a
// larger tile.  K does not enter, although plan_dgemm slices many items on the loop side: a tile per CU is one block of
// the four a CU holds, and with a long K two slices per tile put more waves on every SIMD (64 CUs: 64 x 4096 x 4096 takes
// 64 x 64 tiles in two slices).  Such a loop uses the workspace, DgemmBatchedPlan::item.workspace_doubles of it, and its
// items do not have the bits of the unsliced chain.
// THE THRESHOLD HAS NOT BEEN MEASURED: tools/bench_batched_f64.py times both sides of it (its "forced" columns, at one tile
// row less than, exactly and one more than a tile per CU), but no run of it on an MI355X exists yet, so there are no
// figures to write beside the rule and profiles/ has no batched_dgemm.txt.  1 is the float32 rule's number, not a result.
constexpr long DGEMM_LOOP_TILES_PER_CU = 1;

bool dgemm_batched_runs_as_loop(long M, long N, long K, int cus) {
  (void)K;
  const long T = DGEMM_BATCHED_TILE;
  const long tiles = ((M + T - 1) / T) * ((N + T - 1) / T);
  return tiles >= DGEMM_LOOP_TILES_PER_CU * std::max(cus, 1) || tiles > BATCHED_MAX_BLOCKS;
}

DgemmBatchedPlan plan_dgemm_batched(const DgemmBatchedProblem& p) {
  DgemmBatchedPlan r;
  const long T = DGEMM_BATCHED_TILE;
  r.loop = dgemm_batched_runs_as_loop(p.M, p.N, p.K, p.cus);
  if (p.force == 2) r.loop = true;
  if (p.force == 1) r.loop = ((p.M + T - 1) / T) * ((p.N + T - 1) / T) > BATCHED_MAX_BLOCKS;
  if (r.loop) {
    r.item = plan_dgemm({p.M, p.N, p.K, p.lda, p.ldb, p.a_aligned, p.b_aligned, p.cus});
    return r;
  }
  if (p.batch <= 0 || p.batch1 <= 0 || p.M <= 0 || p.N <= 0) return r;
  r.vec = dgemm_batched_vec(p);
  r.tiles_m = (int)((p.M + T - 1) / T);
  r.tiles_n = (int)((p.N + T - 1) / T);
  const Cut c = cut_items(p.batch * p.batch1, (long)r.tiles_m * r.tiles_n);
  r.tiles = c.tiles, r.items_per_launch = c.items_per_launch, r.launches = c.launches;
  return r;
}

DgemmBatchedLaunch dgemm_batched_launch(const DgemmBatchedPlan& plan, long batch, long index) {
  const Launch l = plan_launch(batch, {plan.tiles, batch * plan.tiles, plan.items_per_launch, plan.launches}, index);
  return {l.first, l.items, l.grid, dgemm_remap(l.grid)};
}

// ---- float64 convolutions ------------------------------------------------------------------------------------------------
// Tile: the cheaper of 128 x 128 and 64 x 64 by plan_dgemm's time model (the same loop, the same blocks per CU).
// GradFilter: the output has few tiles (64 -> 64 channels, 3 x 3: 1 x 9 of 64 x 64), so the P pixels are cut until the
// launch has CONV64_SLICE_BLOCKS_PER_CU blocks per CU (two eight-wave blocks: four waves per SIMD, dgemm_rate's plateau),
// but no slice below CONV64_MIN_SLICE_PIXELS pixels: a slab costs 16 bytes per output element to write and read back, the
// matrix work of about 8 pixels, so a slice of 256 keeps the slabs a few per cent of the launch.
// NEITHER NUMBER HAS BEEN MEASURED AGAINST ALTERNATIVES: tools/conv64_general_bench.py reports the kernel as planned.
constexpr long CONV64_SLICE_BLOCKS_PER_CU = 2;
constexpr long CONV64_MIN_SLICE_PIXELS = 256;

Conv64Plan plan_conv64(const Conv64Problem& p) {
  Conv64Plan r;
  const long Ho = p.H - p.FH + 1, Wo = p.W - p.FW + 1;
  const long P = p.N * Ho * Wo;
  long terms = 0;
  switch (p.role) {
    case Conv64Role::Forward:
      r.M = P, r.Ncols = p.F, r.K = p.FH * p.FW * p.C, terms = r.K;
      r.vec_a = p.C % 2 == 0 && p.img_aligned;     // two taps of one pixel: neighbours in memory when they share (dy, dx) or the row run
      r.vec_b = r.K % 2 == 0 && p.flt_aligned;     // bank rows [F][K]
      break;
    case Conv64Role::GradImage:
      r.M = p.N * p.H * p.W, r.Ncols = p.C, r.K = p.FH * p.FW * p.F, terms = r.K;
      r.vec_a = p.F % 2 == 0 && p.gout_aligned;    // a pair never straddles two positions, whose border tests may differ
      r.vec_b = r.K % 2 == 0;                      // the flipped bank lies in the context's scratch, which is aligned
      r.aux_doubles = p.C * r.K;
      break;
    case Conv64Role::GradFilter:
      r.M = p.F, r.Ncols = p.FH * p.FW * p.C, r.K = P, terms = r.Ncols;
      r.vec_a = p.F % 2 == 0 && p.gout_aligned;    // gout [P][F], two filters of one pixel
      r.vec_b = p.C % 2 == 0 && p.img_aligned;
      break;
  }
  if (r.M >= CONV64_MAX_INDEX || r.Ncols >= CONV64_MAX_INDEX || r.K >= CONV64_MAX_INDEX || terms >= CONV64_MAX_INDEX) return r;
  r.ok = true;
  const long cus = std::max(p.cus, 1);
  r.config = dgemm_cost(kDgemmCfgs[0], r.M, r.Ncols, r.K, cus, 1) < dgemm_cost(kDgemmCfgs[2], r.M, r.Ncols, r.K, cus, 1) ? 0 : 2;
  const DgemmCfg& cfg = kDgemmCfgs[r.config];
  r.bm = cfg.bm, r.bn = cfg.bn, r.wr = cfg.wr, r.wc = cfg.wc;
  r.tiles_m = (int)((r.M + r.bm - 1) / r.bm);
  r.tiles_n = (int)((r.Ncols + r.bn - 1) / r.bn);
  r.grid_x = (long)r.tiles_m * r.tiles_n;
  r.remap = dgemm_remap(r.grid_x);
  r.pixels_per_slice = dgemm_k_unsliced(r.K);
  if (p.role == Conv64Role::GradFilter && r.grid_x > 0) {
    long want = (CONV64_SLICE_BLOCKS_PER_CU * cus + r.grid_x - 1) / r.grid_x;
    want = std::min(want, std::min(r.K / CONV64_MIN_SLICE_PIXELS, 65535L));
    if (want > 1) {
      long per = (r.K + want - 1) / want;
      per = ((per + BK - 1) / BK) * BK;
      const long slices = (r.K + per - 1) / per;
      if (slices > 1) {
        r.slices = (int)slices;
        r.pixels_per_slice = per;
        r.workspace_doubles = slices * r.M * r.Ncols;
        r.reduce = true;
      }
    }
  }
  r.grid_y = r.slices;
  return r;
}

bool exact_single_launch(const GemmPlan& p) {
  return p.route == Route::Bk32 || (p.route == Route::Generic && p.bm == 256 && p.bn == 256 && !p.edge && p.splits <= 1 &&
                                    p.tail_tiles == 0 && p.second == Second::None);
}

}  // namespace gemm
}  // namespace eg
