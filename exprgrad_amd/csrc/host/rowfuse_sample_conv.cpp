// Sample groups (rowfuse.hpp): matrix-core convolution members (round 6; SampleKernelInfo::conv_role).  The scalar members spend their time in LDS reads (two per multiply-add:
// conv1 forward 7.5 us, its filter gradient 12.3, conv2's three 3.5 + 5.4 + 4.9 of the 31 us kernel at batch 32).  Here a
// member is a handful of v_mfma_f32_16x16x4_f32 per wave: the SMALL operand (filter bank / its transpose) sits in
// registers as B fragments for the whole member, the other fragment is ONE gathered element per lane and instruction
// (window element, output gradient), the eight waves share row blocks (forward, image gradient) or the pixel range
// (filter gradient: the waves' accumulator blocks meet in LDS in wave order — a fixed order).  Padding lanes multiply by
// an exact 0.0f from the small operand (or read an element that is part of the true sum), never uninitialised memory.
// Shapes of the loops below (round 6, after the cycle stamps of EG_SAMPLE_TRACE):
//  * a wave's row blocks are a lambda called with a LITERAL trip count (the whole trips; the ragged one under a
//    wave-uniform guard) so that the gathers of block i + 1 are in flight under the MFMAs of block i — the rolled
//    `for (pb = wave; ...)` exposed the LDS latency and the whole dependent MFMA chain of every block; k-steps
//    alternate between two accumulators (one chain of KS dependent MFMAs becomes two of KS / 2);
//  * gathers of FOUR k-values per lane and instruction: with the channels (forward) / the filters (image gradient) a
//    multiple of 4 and the gathered tensor in LDS, the k index is permuted so that lane group l4 holds
//    k = 16 g + 4 l4 + j in the j-th MFMA of group g — four consecutive channels of ONE tap, one ds_read_b128, one
//    address, one bounds test.  Any bijection of k is the same sum; the B fragments use the same one;
//  * a forward member's row block of 16 output pixels is 16 consecutive pixels of the row-major image or — when the
//    output tiles exactly into bw x (16 / bw) patches — such a patch, and a wave then takes whole ROWS of patches:
//    patch row and column are literals at every call, every gather and store a per-lane base plus a literal
//    offset, no pixel of a block lies past the end (the store tests the filter only).
#include "rowfuse_internal.hpp"

namespace eg::kd {

namespace {

std::string S(long v) { return std::to_string(v); }

struct ConvMember : MemberEmitter {
  long W, C, Ho, Wo, F, FH, FW, K, P, Q, NW;

  explicit ConvMember(const MemberEmitter& e) : MemberEmitter(e) {
    const std::vector<long>&is = shapes.at(si.conv_img), &os = shapes.at(si.conv_out), &fs = shapes.at(si.conv_flt);
    W = is[2], C = is[3], Ho = os[1], Wo = os[2], F = os[3], FH = fs[1], FW = fs[2];
    K = FH * FW * C, P = Ho * Wo, Q = is[1] * is[2];
    NW = g.threads / 64;
  }

  std::string at(int tensor, const std::string& idx) const {   // element idx of this sample's slice (the filter bank: of the bank)
    const std::string name = "t" + std::to_string(tensor);
    if (tensor == si.conv_flt) return name + "[" + idx + "]";
    const long inner = prodv(shapes.at(tensor)) / std::max(1L, shapes.at(tensor)[0]);
    return local(tensor) ? name + "[" + idx + "]" : name + "[n * " + S(inner) + "L + " + idx + "]";
  }

  // A row block's store without a branch when the destination lives in LDS: lanes outside the tensor write their value
  // to a slot of `dummy_` of their own instead (a guarded store is a basic-block boundary the compiler moves no gather
  // across).
  std::string guarded_store(int tensor, const std::string& cond, const std::string& idx, const std::string& value) {
    const std::string o = at(tensor, idx);
    if (!local(tensor))
      return "          if (" + cond + ") " + o + " = " + (g.overwrite[gi] ? std::string("0.0f") : o) + " + " + value + ";\n";
    m.needs_dummy = true;   // (not `scratch`: a member behind an elided barrier may be using that)
    std::string d = "          float* const dst_ = (" + cond + ") ? &" + o + " : &dummy_[threadIdx.x];\n";
    d += "          *dst_ = " + (g.overwrite[gi] ? std::string("0.0f") : std::string("*dst_")) + " + " + value + ";\n";
    return d;
  }

  std::string trips(const std::string& fn, long units) const {   // calls fn(unit) for unit = wave, wave + NW, ...
    std::string d;
    const long whole = units / NW, ragged = units % NW;
    if (whole > 0) d += "    _Pragma(\"unroll\") for (int it_ = 0; it_ < " + S(whole) + "; ++it_) " + fn + "(wave + it_ * " + S(NW) + ");\n";
    if (ragged > 0) d += "    if (wave < " + S(ragged) + ") " + fn + "(wave + " + S(whole * NW) + ");\n";
    return d;
  }

  void forward();
  void image_gradient();
  void filter_gradient();
};

// out[p, f] (+)= sum_t img[pix(p) + tap(t)] * flt[f, t].  One frame; B fragments and k loop by the gather (4 values or one).
void ConvMember::forward() {
  std::string fw_head, fw_store, fw_pre, fw_calls;
  long fw_blocks = 1;   // row blocks per call of the member's lambda
  long bw = 0;
  for (long cand : {16L, 8L, 4L, 2L})
    if (!bw && Wo % cand == 0 && Ho % (16 / cand) == 0) bw = cand;
  const std::string value = "(acc[bi][0][nb][j] + acc[bi][1][nb][j])";
  if (bw) {
    // patch row = wave + NW * ri
    const long bh = 16 / bw, nbc = Wo / bw, nbr = Ho / bh, whole = nbr / NW, ragged = nbr % NW;
    fw_pre = "    const int wu = __builtin_amdgcn_readfirstlane(wave);\n";
    fw_blocks = nbc <= 4 ? nbc : 1;
    if (whole > 0)
      fw_calls += "    _Pragma(\"unroll\") for (int ri = 0; ri < " + S(whole) + "; ++ri) _Pragma(\"unroll\") for (int bc = 0; bc < " + S(nbc) +
                  "; bc += " + S(fw_blocks) + ") block(ri * " + S(nbc) + " + bc);\n";
    if (ragged > 0)
      fw_calls += "    if (wu < " + S(ragged) + ") { _Pragma(\"unroll\") for (int bc = 0; bc < " + S(nbc) + "; bc += " + S(fw_blocks) + ") block(" +
                  S(whole * nbc) + " + bc); }\n";
    fw_head = "      const int br = wu + " + S(NW) + " * (pb / " + S(nbc) + "), bc = pb % " + S(nbc) + ";\n";
    fw_head += "      const int poff = ((br * " + S(bh) + " + l15 / " + S(bw) + ") * " + S(W) + " + bc * " + S(bw) + " + l15 % " + S(bw) + ") * " + S(C) + ";\n";
    fw_store = "          const int m_ = 4 * l4 + j, f = 16 * nb + l15;\n";
    fw_store += guarded_store(si.conv_out, "f < " + S(F),
                              "((br * " + S(bh) + " + m_ / " + S(bw) + ") * " + S(Wo) + " + bc * " + S(bw) + " + m_ % " + S(bw) + ") * " + S(F) + " + f", value);
  } else {
    fw_head = "      int p = 16 * pb + l15;\n      if (p > " + S(P - 1) + ") p = " + S(P - 1) + ";\n";
    fw_head += "      const int poff = ((p / " + S(Wo) + ") * " + S(W) + " + p % " + S(Wo) + ") * " + S(C) + ";\n";
    fw_store = "          const int pr = 16 * pb + 4 * l4 + j, f = 16 * nb + l15;\n";
    fw_store += guarded_store(si.conv_out, "pr < " + S(P) + " && f < " + S(F), "pr * " + S(F) + " + f", value);
    fw_calls = trips("block", (P + 15) / 16);
  }
  const long NB = (F + 15) / 16;
  std::string k_loop;
  if (C % 4 == 0 && local(si.conv_img)) {   // four k-values per gather
    const long G = (K + 15) / 16;
    c += "    float bf[" + S(NB) + "][" + S(4 * G) + "];\n    int toff[" + S(G) + "];\n";
    c += "    _Pragma(\"unroll\") for (int g4 = 0; g4 < " + S(G) + "; ++g4) {\n";
    c += "      const int t0 = 16 * g4 + 4 * l4, tc = t0 < " + S(K) + " ? t0 : 0;\n";
    c += "      toff[g4] = ((tc / " + S(FW * C) + ") * " + S(W) + " + (tc / " + S(C) + ") % " + S(FW) + ") * " + S(C) + " + tc % " + S(C) + ";\n";
    c += "      _Pragma(\"unroll\") for (int nb = 0; nb < " + S(NB) + "; ++nb) {\n        const int f = 16 * nb + l15;\n";
    // (columns f >= F of B are never stored: they read filter F - 1 instead of a masked zero; only k past the end is masked)
    c += "        const int fc = f < " + S(F) + " ? f : " + S(F - 1) + ";\n";
    if (K % 16 == 0) {
      c += "        _Pragma(\"unroll\") for (int j = 0; j < 4; ++j) bf[nb][4 * g4 + j] = " + at(si.conv_flt, "fc * " + S(K) + " + t0 + j") + ";\n      }\n    }\n";
    } else {
      c += "        const bool in_ = t0 < " + S(K) + ";\n";
      c += "        _Pragma(\"unroll\") for (int j = 0; j < 4; ++j) {\n          const float bv = " + at(si.conv_flt, "fc * " + S(K) + " + (in_ ? t0 : 0) + j") +
           ";\n          bf[nb][4 * g4 + j] = in_ ? bv : 0.0f;\n        }\n      }\n    }\n";
    }
    k_loop += "      _Pragma(\"unroll\") for (int g4 = 0; g4 < " + S(G) + "; ++g4) {\n";
    k_loop += "        const mf4 a4 = *reinterpret_cast<const mf4*>(&" + at(si.conv_img, "poff + toff[g4]") + ");\n";
    k_loop += "        _Pragma(\"unroll\") for (int j = 0; j < 4; ++j)\n          _Pragma(\"unroll\") for (int nb = 0; nb < " + S(NB) +
         "; ++nb) acc[bi][j & 1][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[j], bf[nb][4 * g4 + j], acc[bi][j & 1][nb], 0, 0, 0);\n      }\n";
  } else {
    const long KS = (K + 3) / 4;
    c += "    float bf[" + S(NB) + "][" + S(KS) + "];\n    int toff[" + S(KS) + "];\n";
    c += "    _Pragma(\"unroll\") for (int ks = 0; ks < " + S(KS) + "; ++ks) {\n";
    c += "      const int t = 4 * ks + l4, tc = t < " + S(K) + " ? t : 0;\n";
    c += "      toff[ks] = ((tc / " + S(FW * C) + ") * " + S(W) + " + (tc / " + S(C) + ") % " + S(FW) + ") * " + S(C) + " + tc % " + S(C) + ";\n";
    c += "      _Pragma(\"unroll\") for (int nb = 0; nb < " + S(NB) + "; ++nb) {\n        const int f = 16 * nb + l15;\n";
    c += "        const bool in_ = t < " + S(K) + ";\n        const float bv = " + at(si.conv_flt, "(f < " + S(F) + " ? f : " + S(F - 1) + ") * " + S(K) + " + tc") + ";\n";
    c += "        bf[nb][ks] = in_ ? bv : 0.0f;   // (columns f >= F are never stored: they repeat filter F - 1)\n      }\n    }\n";
    k_loop += "      _Pragma(\"unroll\") for (int ks = 0; ks < " + S(KS) + "; ++ks) {\n";
    k_loop += "        const float a = " + at(si.conv_img, "poff + toff[ks]") + ";\n";
    k_loop += "        _Pragma(\"unroll\") for (int nb = 0; nb < " + S(NB) + "; ++nb) acc[bi][ks & 1][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bf[nb][ks], acc[bi][ks & 1][nb], 0, 0, 0);\n      }\n";
  }
  // A call covers fw_blocks row blocks (a whole row of patches, or one block): first the gathers and MFMAs of ALL of
  // them — one straight-line run the scheduler can interleave: block by block, every block's LDS latency and dependent
  // MFMA chain stood in line (conv1 forward: 4 300 cycles for 42 MFMAs per wave whatever was trimmed around them) —
  // then all their stores.
  c += fw_pre + "    auto block = [&](const int pb0) {\n";
  c += "      mf4 acc[" + S(fw_blocks) + "][2][" + S(NB) + "];\n";
  c += "      _Pragma(\"unroll\") for (int bi = 0; bi < " + S(fw_blocks) + "; ++bi) {\n      const int pb = pb0 + bi;\n" + fw_head;
  c += "      _Pragma(\"unroll\") for (int nb = 0; nb < " + S(NB) + "; ++nb) acc[bi][0][nb] = acc[bi][1][nb] = mf4{0.0f, 0.0f, 0.0f, 0.0f};\n";
  c += k_loop;
  c += "      }\n      _Pragma(\"unroll\") for (int bi = 0; bi < " + S(fw_blocks) + "; ++bi) {\n      const int pb = pb0 + bi;\n" + fw_head + "      (void)poff;\n";
  c += "      _Pragma(\"unroll\") for (int nb = 0; nb < " + S(NB) + "; ++nb)\n        _Pragma(\"unroll\") for (int j = 0; j < 4; ++j) {\n";
  c += fw_store + "        }\n      }\n    };\n";
  c += fw_calls;
}

// gimg[q, ch] (+)= sum_{s, f} gout[pixel(q) - tap(s), f] * flt[f, s, ch].  One frame for both gathers, as in forward().
void ConvMember::image_gradient() {
  const long KD = FH * FW * F, NB = (C + 15) / 16, QB = (Q + 15) / 16;
  std::string k_loop;
  if (F % 4 == 0 && local(si.conv_out)) {   // four k-values per gather
    const long G = (KD + 15) / 16;
    // (F a multiple of 16: the tap of group g4 is a literal)
    const std::string tap_s = F % 16 == 0 ? "g4 / " + S(F / 16) : "k0 / " + S(F);
    const std::string tap_f = F % 16 == 0 ? "16 * (g4 % " + S(F / 16) + ") + 4 * l4" : "k0 % " + S(F);
    c += "    float bf[" + S(NB) + "][" + S(4 * G) + "];\n";
    c += "    _Pragma(\"unroll\") for (int g4 = 0; g4 < " + S(G) + "; ++g4) {\n      const int k0 = 16 * g4 + 4 * l4, s = " + tap_s + ", f0 = " + tap_f + ";\n";
    c += "      _Pragma(\"unroll\") for (int nb = 0; nb < " + S(NB) + "; ++nb) {\n        const int ch = 16 * nb + l15;\n";
    c += "        const int cc = ch < " + S(C) + " ? ch : " + S(C - 1) + ";   // (columns ch >= C are never stored)\n";
    if (KD % 16 == 0) {
      c += "        _Pragma(\"unroll\") for (int j = 0; j < 4; ++j) bf[nb][4 * g4 + j] = " + at(si.conv_flt, "(f0 + j) * " + S(K) + " + s * " + S(C) + " + cc") + ";\n      }\n    }\n";
    } else {
      c += "        const bool in_ = k0 < " + S(KD) + ";\n";
      c += "        _Pragma(\"unroll\") for (int j = 0; j < 4; ++j) {\n          const float bv = " +
           at(si.conv_flt, "(in_ ? (f0 + j) * " + S(K) + " + s * " + S(C) + " + cc : 0)") + ";\n          bf[nb][4 * g4 + j] = in_ ? bv : 0.0f;\n        }\n      }\n    }\n";
    }
    k_loop += "      _Pragma(\"unroll\") for (int g4 = 0; g4 < " + S(G) + "; ++g4) {\n";
    k_loop += "        const int k0 = 16 * g4 + 4 * l4, s = " + tap_s + ", f0 = " + tap_f + ", y = qy - s / " + S(FW) + ", x = qx - s % " + S(FW) + ";\n";
    k_loop += "        const bool ok = k0 < " + S(KD) + " && y >= 0 && y < " + S(Ho) + " && x >= 0 && x < " + S(Wo) + ";\n";
    // (outside the output: the lane reads four zeros kept in LDS — one select of the address instead of four of the values)
    m.reads_zeros4 = true;
    k_loop += "        const float* const ap = ok ? &" + at(si.conv_out, "(y * " + S(Wo) + " + x) * " + S(F) + " + f0") + " : zeros4_;\n";
    k_loop += "        const mf4 a4 = *reinterpret_cast<const mf4*>(ap);\n";
    k_loop += "        _Pragma(\"unroll\") for (int j = 0; j < 4; ++j) {\n          const float a = a4[j];\n";
    k_loop += "          _Pragma(\"unroll\") for (int nb = 0; nb < " + S(NB) +
         "; ++nb) acc[j & 1][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bf[nb][4 * g4 + j], acc[j & 1][nb], 0, 0, 0);\n        }\n      }\n";
  } else {
    const long KS = (KD + 3) / 4;
    // With F a multiple of 4 the four lanes groups of a k-step share their tap: tap and window offset of k-step ks are
    // literals (the bounds test is per tap, not per k-step, and the gather's address is the pixel's base + a literal).
    const bool f4 = F % 4 == 0;
    const std::string tap_s = f4 ? "ks / " + S(F / 4) : "kk / " + S(F), tap_f = f4 ? "4 * (ks % " + S(F / 4) + ") + l4" : "kk % " + S(F);
    c += "    float bf[" + S(NB) + "][" + S(KS) + "];\n";
    c += "    _Pragma(\"unroll\") for (int ks = 0; ks < " + S(KS) + "; ++ks) {\n      const int kk = 4 * ks + l4, s = " + tap_s + ", f = " + tap_f + ";\n";
    c += "      _Pragma(\"unroll\") for (int nb = 0; nb < " + S(NB) + "; ++nb) {\n        const int ch = 16 * nb + l15;\n";
    c += "        const bool in_ = kk < " + S(KD) + ";\n        const float bv = " + at(si.conv_flt, "(in_ ? f * " + S(K) + " + s * " + S(C) + " + (ch < " + S(C) + " ? ch : " + S(C - 1) + ") : 0)") + ";\n";
    c += "        bf[nb][ks] = in_ ? bv : 0.0f;   // (columns ch >= C are never stored)\n      }\n    }\n";
    k_loop += "      _Pragma(\"unroll\") for (int ks = 0; ks < " + S(KS) + "; ++ks) {\n";
    k_loop += "        const int kk = 4 * ks + l4, s = " + tap_s + ", f = " + tap_f + ", y = qy - s / " + S(FW) + ", x = qx - s % " + S(FW) + ";\n";
    k_loop += "        const bool ok = kk < " + S(KD) + " && y >= 0 && y < " + S(Ho) + " && x >= 0 && x < " + S(Wo) + ";\n";
    k_loop += "        const int go = ok ? (y * " + S(Wo) + " + x) * " + S(F) + " + f : 0;\n";
    k_loop += "        const float av = " + at(si.conv_out, "go") + ";\n        const float a = ok ? av : 0.0f;\n";
    k_loop += "        _Pragma(\"unroll\") for (int nb = 0; nb < " + S(NB) + "; ++nb) acc[ks & 1][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bf[nb][ks], acc[ks & 1][nb], 0, 0, 0);\n      }\n";
  }
  c += "    auto block = [&](const int qb) {\n";
  c += "      int q = 16 * qb + l15;\n      if (q > " + S(Q - 1) + ") q = " + S(Q - 1) + ";\n      const int qy = q / " + S(W) + ", qx = q % " + S(W) + ";\n";
  c += "      mf4 acc[2][" + S(NB) + "];\n      _Pragma(\"unroll\") for (int nb = 0; nb < " + S(NB) + "; ++nb) acc[0][nb] = acc[1][nb] = mf4{0.0f, 0.0f, 0.0f, 0.0f};\n";
  c += k_loop;
  c += "      _Pragma(\"unroll\") for (int nb = 0; nb < " + S(NB) + "; ++nb)\n        _Pragma(\"unroll\") for (int j = 0; j < 4; ++j) {\n";
  c += "          const int qr = 16 * qb + 4 * l4 + j, ch = 16 * nb + l15;\n";
  c += guarded_store(si.conv_img, "qr < " + S(Q) + " && ch < " + S(C), "qr * " + S(C) + " + ch", "(acc[0][nb][j] + acc[1][nb][j])") + "        }\n    };\n";
  c += trips("block", QB);
}

// gflt[f, t] (+)= sum_p gout[p, f] * img[pix(p) + tap(t)]
void ConvMember::filter_gradient() {
  const long MB = (F + 15) / 16, NB = (K + 15) / 16, PS = (P + 3) / 4;
  const bool first = cx.slab_seen.count(k.write.tensor) == 0;   // the first contribution of this block to that slab range
  const long off = g.slab_offset.at(k.write.tensor);
  c += "    int toff[" + S(NB) + "];\n";
  c += "    _Pragma(\"unroll\") for (int nb = 0; nb < " + S(NB) + "; ++nb) {\n      int t = 16 * nb + l15;\n      if (t > " + S(K - 1) + ") t = " + S(K - 1) + ";\n";
  c += "      toff[nb] = ((t / " + S(FW * C) + ") * " + S(W) + " + (t / " + S(C) + ") % " + S(FW) + ") * " + S(C) + " + t % " + S(C) + ";\n    }\n";
  c += "    mf4 acc[" + S(MB) + "][" + S(NB) + "];\n";
  c += "    _Pragma(\"unroll\") for (int mb = 0; mb < " + S(MB) + "; ++mb) _Pragma(\"unroll\") for (int nb = 0; nb < " + S(NB) + "; ++nb) acc[mb][nb] = mf4{0.0f, 0.0f, 0.0f, 0.0f};\n";
  // Output rows a multiple of 4 pixels wide: a wave takes WHOLE ROWS (row = wave + NW * ri) and walks them in literal
  // steps of 4 pixels, so every gather is a per-lane base (computed once) plus a literal offset — the linear walk
  // `p = 4 ps + l4` paid a division by Wo, two multiplies and three additions per step and lane (the members are bound
  // by instruction issue: EG_SAMPLE_TRACE, 5 000 cycles for 18 steps of 2 MFMAs).
  // (rows not a multiple of 4 wide but even, an even number of them: the four pixels of a step are a 2 x 2 tile)
  const long th = Wo % 4 == 0 ? 1 : 2, tw = 4 / th, trows = Ho / th;
  const bool by_rows = Wo % tw == 0 && Ho % th == 0 && (trows / NW + 1) * (Wo / tw) <= 40;
  if (by_rows) {
    // (rows go to the waves from the LAST one down: the row-block members in front of this one — no barrier in between
    // when they are independent — give their ragged extra block to the first waves)
    c += "    const int wu = " + S(NW - 1) + " - __builtin_amdgcn_readfirstlane(wave), lr = l4 / " + S(tw) + ", lc = l4 % " + S(tw) + ";\n";
    c += "    const int pbase = ((wu * " + S(th) + " + lr) * " + S(W) + " + lc) * " + S(C) + ";\n";
    c += "    int abase[" + S(MB) + "];\n    _Pragma(\"unroll\") for (int mb = 0; mb < " + S(MB) + "; ++mb) {\n      const int f = 16 * mb + l15;\n";
    c += "      abase[mb] = ((wu * " + S(th) + " + lr) * " + S(Wo) + " + lc) * " + S(F) + " + (f < " + S(F) + " ? f : 0);\n    }\n";
    c += "    auto rowstep = [&](const int ri) {\n      _Pragma(\"unroll\") for (int cg = 0; cg < " + S(Wo / tw) + "; ++cg) {\n";
    c += "        float a[" + S(MB) + "];\n        _Pragma(\"unroll\") for (int mb = 0; mb < " + S(MB) + "; ++mb) a[mb] = " +
         at(si.conv_out, "abase[mb] + (" + S(NW * th * Wo) + " * ri + " + S(tw) + " * cg) * " + S(F)) + ";\n";
    c += "        _Pragma(\"unroll\") for (int nb = 0; nb < " + S(NB) + "; ++nb) {\n          const float b = " +
         at(si.conv_img, "pbase + toff[nb] + (" + S(NW * th * W) + " * ri + " + S(tw) + " * cg) * " + S(C)) + ";\n";
    c += "          _Pragma(\"unroll\") for (int mb = 0; mb < " + S(MB) + "; ++mb) acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mb], b, acc[mb][nb], 0, 0, 0);\n        }\n      }\n    };\n";
    const long whole = trows / NW, ragged = trows % NW;
    if (whole > 0) c += "    _Pragma(\"unroll\") for (int ri = 0; ri < " + S(whole) + "; ++ri) rowstep(ri);\n";
    if (ragged > 0) c += "    if (wu < " + S(ragged) + ") rowstep(" + S(whole) + ");\n";
  }
  c += "    auto step = [&](const int ps) {\n";
  c += "      const int p = 4 * ps + l4, pc = p < " + S(P) + " ? p : " + S(P - 1) + ";\n";
  c += "      const int poff = ((pc / " + S(Wo) + ") * " + S(W) + " + pc % " + S(Wo) + ") * " + S(C) + ";\n";
  // (rows f >= F of the result are never stored: they repeat filter 0; pixels past the end are masked, if there are any)
  c += "      float a[" + S(MB) + "];\n      _Pragma(\"unroll\") for (int mb = 0; mb < " + S(MB) + "; ++mb) {\n        const int f = 16 * mb + l15, fc = f < " + S(F) + " ? f : 0;\n";
  c += "        const float av = " + at(si.conv_out, "pc * " + S(F) + " + fc") + ";\n        a[mb] = " + (P % 4 == 0 ? std::string("av") : "p < " + S(P) + " ? av : 0.0f") + ";\n      }\n";
  c += "      _Pragma(\"unroll\") for (int nb = 0; nb < " + S(NB) + "; ++nb) {\n        const float b = " + at(si.conv_img, "poff + toff[nb]") + ";\n";
  c += "        _Pragma(\"unroll\") for (int mb = 0; mb < " + S(MB) + "; ++mb) acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mb], b, acc[mb][nb], 0, 0, 0);\n      }\n    };\n";
  // (more than 24 whole trips: the unrolled body would not fit the instruction cache's reach; a rolled loop of 4)
  if (by_rows) {
    c += "    (void)step;\n";
  } else if (PS / NW <= 24) {
    c += trips("step", PS);
  } else {
    c += "    _Pragma(\"unroll 4\") for (int ps = wave; ps < " + S(PS) + "; ps += " + S(NW) + ") step(ps);\n";
  }
  // the waves' accumulator blocks meet in LDS — as many of the MB x NB at a time as 16 KB of scratch hold (the planner's
  // LDS budget leaves that much: plan_groups.cpp) — and are added in wave order
  const long BL = MB * NB, per_round = std::max(1L, 4096 / (NW * 256));
  for (long b0 = 0; b0 < BL; b0 += per_round) {
    const long nb_round = std::min(per_round, BL - b0);
    if (b0 > 0) c += "    __syncthreads();\n";
    for (long b = b0; b < b0 + nb_round; ++b)
      c += "    _Pragma(\"unroll\") for (int j = 0; j < 4; ++j) scratch[(" + S(b - b0) + " * " + S(NW) + " + wave) * 256 + (4 * l4 + j) * 16 + l15] = acc[" +
           S(b / NB) + "][" + S(b % NB) + "][j];\n";
    c += "    __syncthreads();\n";
    c += "    _Pragma(\"unroll\") for (int e0 = 0; e0 < " + S(nb_round * 256) + "; e0 += " + NT + ") {\n      const int e = e0 + threadIdx.x, bl = " + S(b0) +
         " + (e >> 8), el = e & 255;\n";
    c += "      if (e < " + S(nb_round * 256) + ") {\n        float s = 0.0f;\n        _Pragma(\"unroll\") for (int w = 0; w < " + S(NW) +
         "; ++w) s = s + scratch[((e >> 8) * " + S(NW) + " + w) * 256 + el];\n";
    c += "        const int f = 16 * (bl / " + S(NB) + ") + (el >> 4), t = 16 * (bl % " + S(NB) + ") + (el & 15);\n";
    const std::string o = "row[" + S(off) + " + f * " + S(K) + " + t]";
    c += "        if (f < " + S(F) + " && t < " + S(K) + ") " + o + " = " + (first ? std::string("0.0f") : o) + " + s;\n      }\n    }\n";
  }
  m.uses_scratch = true;
  m.scratch_floats = NW * 256 * std::min(per_round, BL);
  cx.slab_seen.insert(k.write.tensor);
}

}  // namespace

void emit_conv_member(MemberEmitter e) {
  ConvMember cm(e);
  cm.c += "    typedef float mf4 __attribute__((ext_vector_type(4)));\n";
  cm.c += "    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;\n";
  if (cm.si.conv_role == 1) cm.forward();
  else if (cm.si.conv_role == 3) cm.image_gradient();
  else cm.filter_gradient();
}

}  // namespace eg::kd
