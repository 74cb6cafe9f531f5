// Sample groups: one BLOCK per sample (rowfuse.hpp).  Members are emitted with the facts assembly needs (SampleMember).
#include <regex>

#include "rowfuse_internal.hpp"

namespace eg::kd {

SampleKernelInfo analyse_sample_kernel(const Program& prog, const Kernel& k, const KernelInfo& info, const Shapes& shapes, long B) {
  (void)prog;
  SampleKernelInfo r;
  if (!info.ok || B <= 0 || k.gen != Gen::None) return r;
  const std::vector<const Op*> ops = ops_of(k);
  for (const Op* op : ops)
    if (!shapes.count(op->tensor)) return r;
  long all_work = 1;
  for (size_t l = 0; l < k.loops.size(); ++l) all_work *= std::max(0L, info.bounds[l].second - info.bounds[l].first);
  if (k.is_seed) {
    if (all_work > 4096 || !k.index_instrs.empty()) return r;
    r.ok = true;
    r.seed = true;
    r.work = all_work;
    return r;
  }
  auto used_as_value = [&](int y) {
    for (auto& ins : k.instrs)
      for (int a : ins.args)
        if (a == y) return true;
    for (auto& ins : k.index_instrs)
      for (int a : ins.args)
        if (a == y) return true;
    return false;
  };
  for (size_t l = 0; l < k.loops.size(); ++l) {
    const int y = k.loops[l].reg;
    const long lo = info.bounds[l].first, hi = info.bounds[l].second;
    if (lo != 0 || used_as_value(y)) continue;
    bool any_raw = false, any = false, ok = true;
    for (const Op* op : ops)
      if (op_has(*op, y) && op->raw) any_raw = true;
    bool raw = false;
    long inner = 0;
    if (hi == B && !any_raw) {
      for (const Op* op : ops) {
        if (!op_has(*op, y)) continue;
        any = true;
        const std::vector<long>& shp = shapes.at(op->tensor);
        if (op->raw || shp.empty() || shp[0] != B || op->dims.empty() || op->dims[0].only_register() != y) ok = false;
        for (size_t d = 1; ok && d < op->dims.size(); ++d)
          if (lin_has(op->dims[d], y)) ok = false;
      }
    } else if (any_raw && hi >= B && hi % B == 0) {
      raw = true;
      inner = hi / B;
      for (const Op* op : ops) {
        if (!op_has(*op, y)) continue;
        any = true;
        const std::vector<long>& shp = shapes.at(op->tensor);
        if (!op->raw || op->dims.size() != 1 || op->dims[0].only_register() != y || shp.empty() || shp[0] != B || prodv(shp) != hi)
          ok = false;
      }
      if (!op_has(k.write, y)) ok = false;
    } else {
      continue;
    }
    if (!ok || !any) continue;
    r.ok = true;
    r.batch_loop = (int)l;
    r.raw = raw;
    r.inner = inner;
    r.reduced = !op_has(k.write, y);
    r.work = raw ? inner : all_work / B;
    return r;
  }
  return r;
}

namespace {

// The kernel's signature (into sig) and the text in front of the first member: staged copies, LDS declarations and zeroing.
std::string emit_prologue(SampleGroup& g, const std::string& NT, const std::set<int>& touched, const std::set<int>& written, std::string& sig) {
  g.ptr_args.clear();
  for (int t : touched)
    if (!g.lds.count(t)) g.ptr_args.push_back(t);
  sig = "extern \"C\" __global__ void __launch_bounds__(" + NT + ") " + g.name + "(float* __restrict__ slab";
  // (a staged parameter's argument is g<id>; t<id> names its copy in LDS, so the members' text does not change)
  for (int t : g.ptr_args) sig += std::string(written.count(t) ? ", float* t" : (g.staged.count(t) ? ", const float* __restrict__ g" : ", const float* t")) + std::to_string(t);
  sig += ", float GS, long EP)";
  std::string c = "  const long n = blockIdx.x;  // this block's sample\n";
  // Staged parameters: ALL loads first (literal trip counts, one register each), then the stores.  As one copy loop per
  // parameter the compiler emitted load - wait - store round trips one after the other (rolled loops for the longer ones):
  // ten dependent trips to L2 in front of the first member, 5 - 6 us of a 23 us kernel (ISA of the batch-32 fit step).
  if (!g.staged.empty()) {
    std::string loads, stores;
    long nv = 0;
    for (auto& kv : g.staged) {
      const std::string id = std::to_string(kv.first);
      c += "  __shared__ __attribute__((aligned(16))) float t" + id + "[" + std::to_string(kv.second) + "];\n";
      for (long base = 0; base < kv.second; base += g.threads, ++nv) {
        const std::string v = "sv" + std::to_string(nv), i = "threadIdx.x + " + std::to_string(base);
        const bool whole = base + g.threads <= kv.second;
        const std::string guard = whole ? "" : "if (threadIdx.x < " + std::to_string(kv.second - base) + ") ";
        loads += "    float " + v + " = 0.0f; " + guard + v + " = g" + id + "[" + i + "];\n";
        stores += "    " + guard + "t" + id + "[" + i + "] = " + v + ";\n";
      }
    }
    c += "  {\n" + loads + stores + "  }\n";
  }
  for (auto& kv : g.lds) c += "  __shared__ __attribute__((aligned(16))) float t" + std::to_string(kv.first) + "[" + std::to_string(kv.second) + "];\n";
  for (int t : g.lds_zero)
    c += "  for (int i = threadIdx.x; i < " + std::to_string(g.lds.at(t)) + "; i += " + NT + ") t" + std::to_string(t) + "[i] = 0.0f;\n";
  return c;
}

// A member as the kernel's own loop nest over the block's sample: independent iterations go to the threads, reductions are
// serial per thread (choose_blocking) or split over T lanes (choose_split); conv2's image gradient as a gather (emit_gather).
struct LoopNest : MemberEmitter {
  const std::vector<Ty> ty = infer_types(k);
  std::vector<int> indep, red;
  bool scatter = false;
  long total = 1, rtotal = 1;   // independent / reduction iterations per sample
  std::string w;                // where the value goes
  bool plain = false;           // ... as a plain store instead of +=
  int blk = -1;                 // register blocking: position in indep of the blocked iterator, R values per thread
  long R = 1, items = 0;
  std::string RS, breg, zero_acc;
  long T = 1;                   // threads that share an item's reduction

  explicit LoopNest(const MemberEmitter& e) : MemberEmitter(e) {}

  int setup() {
    split_loops(k, indep, red, scatter);
    auto drop = [&](std::vector<int>& v, int l) { v.erase(std::remove(v.begin(), v.end(), l), v.end()); };
    if (!si.seed) {   // (the seed: every block writes the same values, no batch loop)
      drop(indep, si.batch_loop);
      drop(red, si.batch_loop);
    }
    if (si.raw) total = si.inner;
    else
      for (int l : indep) total *= std::max(0L, info.bounds[l].second - info.bounds[l].first);
    if (si.raw && !indep.empty()) {
      set_error("internal: raw sample kernel with further independent loops");
      return EG_ERR_INVALID;
    }
    plain = g.overwrite[gi] != 0;
    if (si.reduced) {
      const long off = g.slab_offset.at(k.write.tensor);
      const std::string e = literal_element(k.write, shapes, "row");
      w = e.substr(0, 4) + std::to_string(off) + "L + " + e.substr(4);   // row[<off> + index]
      plain = cx.slab_seen.count(k.write.tensor) == 0;  // the first contribution of this block to that tensor
    } else {
      w = literal_element(k.write, shapes, "t" + std::to_string(k.write.tensor), local(k.write.tensor));
    }
    for (int l : red) rtotal *= std::max(0L, info.bounds[l].second - info.bounds[l].first);
    m.route.slab = si.reduced ? (plain ? 1 : 2) : 0;
    m.route.lds = !si.reduced && local(k.write.tensor) > 0;
    return EG_OK;
  }

  // Register blocking.  A convolution member spends its time in LDS reads — two per multiply-add, 921 KB per sample for
  // 115 K multiply-adds against 128 B per clock and CU — not in arithmetic.  A thread therefore owns R consecutive
  // values of the fastest independent iterator (R <= 8 dividing its extent) and walks the reduction once for all of
  // them: the unrolled copies share every load that does not depend on that iterator (the compiler merges them).
  void choose_blocking() {
    if (!scatter && !si.raw && !si.seed && !red.empty() && rtotal >= 4) {
      // NOT the fastest iterator: consecutive lanes walk that one, so that a wave's LDS reads fall into consecutive banks
      // (blocking it measured 47 us against 32 for the whole kernel: eight-way bank conflicts); the next one up —
      // `x` of out[n, y, x, f], `dx` of gflt[f, dy, dx, c] — is where the window operand and the other operand repeat.
      long seen = 0;
      for (size_t i = indep.size(); i-- > 0 && blk < 0;) {
        const long ext = info.bounds[indep[i]].second - info.bounds[indep[i]].first;
        if (ext < 2) continue;
        if (seen++ < 1) continue;
        // R by what a thread ends up doing, not "as large as divides": the threads run ceil(items / threads) rounds of R
        // multiply-adds with R loads of every read that moves with the iterator and one of every read that does not
        // (4 608 outputs on 512 threads: R = 8 is 2 rounds of 17 with 7 of 8 waves idle in the second, R = 3 is 3 of 7);
        // with few items the outermost reduction iterator is split over T threads instead (below).
        const int breg_c = k.loops[indep[i]].reg;
        long nd = 0, ns = 0;
        for (auto& rd : k.reads) (op_has(rd, breg_c) ? nd : ns) += 1;
        const long outer = red.empty() ? 1 : std::max(1L, info.bounds[red[0]].second - info.bounds[red[0]].first);
        double best_cost = 1e30;
        for (long r = 1; r <= std::min<long>(ext, 8); ++r) {
          if (ext % r != 0) continue;
          const long it = total / r;
          double rounds = (double)((it + g.threads - 1) / g.threads);
          if (it * 2 <= g.threads && rtotal >= 16 && outer >= 2) {  // the split-reduction path
            const long t = std::max(1L, std::min<long>(g.threads / it, std::min<long>(outer, 64)));
            rounds = (double)((outer + t - 1) / t) / (double)outer;
          }
          const double cost = rounds * (double)(r * (1 + nd) + ns);
          if (cost < best_cost - 1e-9) {
            best_cost = cost;
            R = r;
          }
        }
        if (R > 1) blk = (int)i;
        break;
      }
    }
    items = total / R;
    m.route.R = R;
    RS = std::to_string(R);
    breg = blk >= 0 ? "r" + std::to_string(k.loops[indep[blk]].reg) : "";
    zero_acc = "      float acc[" + RS + "];\n      _Pragma(\"unroll\") for (int u = 0; u < " + RS + "; ++u) acc[u] = 0.0f;\n";
  }

  std::string decode_indep(const std::string& from, const std::string& ind) const {
    std::string d;
    for (auto& s : k.setup) d += ind + "const long r" + std::to_string(s.res) + " = " + std::to_string(info.vals.at(s.res)) + "L;\n";
    if (si.raw) {
      d += ind + "const long r" + std::to_string(k.loops[si.batch_loop].reg) + " = n * " + std::to_string(si.inner) + "L + " + from + ";\n";
      return d;
    }
    if (!si.seed) d += ind + "const long r" + std::to_string(k.loops[si.batch_loop].reg) + " = n;\n";
    d += ind + "long rem = " + from + ";\n";
    for (size_t i = indep.size(); i-- > 0;) {
      const int l = indep[i];
      const long ext = info.bounds[l].second - info.bounds[l].first;
      const std::string lo = std::to_string(info.bounds[l].first) + "L";
      if ((int)i == blk) {
        d += ind + "const long " + breg + "_0 = " + lo + " + (rem % " + std::to_string(ext / R) + "L) * " + RS + "L; rem /= " +
             std::to_string(ext / R) + "L;\n";
      } else {
        d += ind + "const long r" + std::to_string(k.loops[l].reg) + " = " + lo + " + rem % " + std::to_string(ext) + "L; rem /= " +
             std::to_string(ext) + "L;\n";
      }
    }
    d += ind + "(void)rem;\n";
    return d;
  }

  std::string term(const std::string& ind) const {  // loads + expression of one point of the loop nest
    std::string d;
    for (auto& ins : k.index_instrs) d += ind + "const long r" + std::to_string(ins.res) + " = " + instr_expression(ins, "0L", "r") + ";\n";
    for (auto& rd : k.reads)
      d += ind + "const float r" + std::to_string(rd.reg) + " = " + literal_element(rd, shapes, "t" + std::to_string(rd.tensor), local(rd.tensor)) + ";\n";
    for (auto& ins : k.instrs) d += instr_line(k, ins, ty, shapes, "        ");
    return d;
  }

  // one point of the reduction for the thread's R values: acc[u] += term(u)
  std::string accumulate(const std::string& ind) const {
    std::string d;
    if (blk < 0) {
      d += term(ind);
      d += ind + "acc[0] = acc[0] + r" + std::to_string(k.result) + ";\n";
      return d;
    }
    d += ind + "_Pragma(\"unroll\")\n" + ind + "for (int u = 0; u < " + RS + "; ++u) {\n";
    d += ind + "  const long " + breg + " = " + breg + "_0 + u;\n";
    d += term(ind + "  ");
    d += ind + "  acc[u] = acc[u] + r" + std::to_string(k.result) + ";\n" + ind + "}\n";
    return d;
  }

  // store acc[u] for the thread's R values
  std::string store(const std::string& ind) const {
    std::string d;
    if (blk < 0) return ind + w + " = " + (plain ? std::string("0.0f") : w) + " + acc[0];\n";
    d += ind + "_Pragma(\"unroll\")\n" + ind + "for (int u = 0; u < " + RS + "; ++u) {\n";
    d += ind + "  const long " + breg + " = " + breg + "_0 + u;\n";
    d += ind + "  " + w + " = " + (plain ? std::string("0.0f") : w) + " + acc[u];\n" + ind + "}\n";
    return d;
  }

  std::string inner_loops(size_t from, const std::string& ind) const {  // reduction loops red[from ...], innermost unrolled
    std::string d;
    for (size_t i = from; i < red.size(); ++i) {
      const int l = red[i];
      const long ext = info.bounds[l].second - info.bounds[l].first;
      const std::string r = "r" + std::to_string(k.loops[l].reg);
      // loads of several iterations in flight
      if (i + 1 == red.size()) d += ind + (ext * R <= 64 ? "_Pragma(\"unroll\")\n" : "_Pragma(\"unroll 4\")\n");
      d += ind + "for (long " + r + " = " + std::to_string(info.bounds[l].first) + "L; " + r + " < " + std::to_string(info.bounds[l].second) +
           "L; ++" + r + ") {\n";
    }
    return d;
  }

  // Few outputs, long reductions (a dense layer's 10 outputs of 400 terms each, a first-layer filter gradient's 200
  // outputs of 576): one thread per output would leave most of the block idle for hundreds of serial iterations.
  // T threads share an item: thread `part` takes the values part, part + T, ... of the OUTERMOST reduction iterator
  // (the inner ones stay plain nested loops); the T partial sums meet in a fixed order (run-to-run identical).
  void choose_split() {
    const long outer_ext = red.empty() ? 0 : std::max(0L, info.bounds[red[0]].second - info.bounds[red[0]].first);
    if (!scatter && !si.raw && items > 0 && items * 2 <= g.threads && rtotal >= 16 && outer_ext >= 2) {
      T = std::min<long>(g.threads / items, std::min<long>(outer_ext, 64));
      if (T < 2) T = 1;
      // a power of two: the T threads of an item are consecutive lanes of ONE wave and their partial sums meet in a
      // butterfly of shuffles (log2 T steps, every lane ends with the same sum) instead of LDS, a block barrier and one
      // thread adding T values one after the other (the dense member of the fashion_mnist step: 51 dependent additions)
      if (T >= 2) {
        long p2 = 2;
        while (p2 * 2 <= T) p2 *= 2;
        T = p2;
      }
    }
  }

  // gimg[n, Y, X, c] = sum over (dy, dx, f) of gout[n, Y - dy, X - dx, f] * flt[f, dy, dx, c] where the output pixel exists
  void emit_gather() {
    const std::vector<long>&gi_s = shapes.at(si.g_img), &go_s = shapes.at(si.g_out), &fl_s = shapes.at(si.g_flt);
    const long H = gi_s[1], W = gi_s[2], C = gi_s[3], Ho = go_s[1], Wo = go_s[2], F = go_s[3], FH = fl_s[1], FW = fl_s[2];
    auto L = [](long v) { return std::to_string(v) + "L"; };
    m.route.kind = SampleMemberRoute::Gather;
    m.route.lds = local(si.g_img) > 0;
    const std::string img = "t" + std::to_string(si.g_img), out = "t" + std::to_string(si.g_out), flt = "t" + std::to_string(si.g_flt);
    c += "    for (long idx = threadIdx.x; idx < " + L(H * W * C) + "; idx += " + NT + ") {\n";
    c += "      const long ch = idx % " + L(C) + ", X = (idx / " + L(C) + ") % " + L(W) + ", Y = idx / " + L(C * W) + ";\n";
    c += "      float acc = 0.0f;\n";
    c += "      for (long dy = 0; dy < " + L(FH) + "; ++dy) {\n        const long y = Y - dy;\n        if (y < 0 || y >= " + L(Ho) + ") continue;\n";
    c += "        for (long dx = 0; dx < " + L(FW) + "; ++dx) {\n          const long x = X - dx;\n          if (x < 0 || x >= " + L(Wo) + ") continue;\n";
    c += "          const float* go = " + out + " + ((" + (local(si.g_out) ? std::string("0L") : std::string("n")) + " * " + L(Ho) + " + y) * " + L(Wo) + " + x) * " + L(F) + ";\n";
    c += "          const float* fl = " + flt + " + (dy * " + L(FW) + " + dx) * " + L(C) + " + ch;\n";
    c += "          for (long f = 0; f < " + L(F) + "; ++f) acc = acc + go[f] * fl[f * " + L(FH * FW * C) + "];\n        }\n      }\n";
    const std::string w = img + "[" + (local(si.g_img) ? std::string("0L") : std::string("n")) + " * " + L(H * W * C) + " + idx]";
    c += "      " + w + " = " + (g.overwrite[gi] ? std::string("0.0f") : w) + " + acc;\n    }\n";
  }

  void emit_split() {   // T > 1
    const std::string TS = std::to_string(T);
    c += "    {\n      const long out = threadIdx.x / " + TS + "L, part = threadIdx.x % " + TS + "L;\n" + zero_acc;
    c += "      if (out < " + std::to_string(items) + "L) {\n";
    c += decode_indep("out", "        ");
    {
      const int l = red[0];
      const std::string r = "r" + std::to_string(k.loops[l].reg);
      // literal trip count for the whole trips (their loads go out together), the ragged last one guarded
      const long ext0 = info.bounds[l].second - info.bounds[l].first, whole = ext0 / T, ragged = ext0 % T;
      m.route.kind = SampleMemberRoute::Split;
      m.route.T = T;
      m.route.ragged = ragged;
      m.route.rolled = whole > 16;
      std::string body = inner_loops(1, "          ") + accumulate("          ");
      for (size_t i = 1; i < red.size(); ++i) body += "          }\n";
      if (whole <= 16) {
        if (whole > 0)
          c += "        _Pragma(\"unroll\") for (int it_ = 0; it_ < " + std::to_string(whole) + "; ++it_) {\n          const long " + r + " = " +
               std::to_string(info.bounds[l].first) + "L + part + it_ * " + TS + "L;\n" + body + "        }\n";
        if (ragged > 0)
          c += "        if (part < " + std::to_string(ragged) + "L) {\n          const long " + r + " = " +
               std::to_string(info.bounds[l].first + whole * T) + "L + part;\n" + body + "        }\n";
      } else {
        c += "        for (long " + r + " = " + std::to_string(info.bounds[l].first) + "L + part; " + r + " < " +
             std::to_string(info.bounds[l].second) + "L; " + r + " += " + TS + "L) {\n" + body + "        }\n";
      }
    }
    c += "      }\n";
    c += "      _Pragma(\"unroll\") for (int m_ = " + std::to_string(T / 2) + "; m_ >= 1; m_ >>= 1)\n        _Pragma(\"unroll\") for (int u = 0; u < " + RS +
         "; ++u) acc[u] = acc[u] + __shfl_xor(acc[u], m_, " + TS + ");\n";
    c += "      if (out < " + std::to_string(items) + "L && part == 0) {\n";
    c += decode_indep("out", "        ");
    c += store("        ");
    c += "      }\n    }\n";
  }

  void emit_items() {
    std::string body = decode_indep("idx", "      "), body_store;
    if (scatter) {
      // the element depends on the reduction iterators: add term by term (the destination starts from zero)
      body += inner_loops(0, "      ");
      body += term("        ");
      body += "        " + w + " = " + w + " + r" + std::to_string(k.result) + ";\n";
      for (size_t i = 0; i < red.size(); ++i) body += "      }\n";
    } else {
      body += zero_acc;
      body += inner_loops(0, "      ");
      body += accumulate("        ");
      for (size_t i = 0; i < red.size(); ++i) body += "      }\n";
      body_store = store("      ");
    }
    // The whole trips of the item loop with a literal trip count (a thread's start depends on threadIdx.x, so the
    // compiler cannot count the trips of `for (idx = threadIdx.x; idx < items; idx += threads)` and leaves it rolled: every
    // trip a read - compute - write round trip to LDS; unrolled, the reads of all trips go out together), the ragged last
    // trip computes element 0 again in the threads past the end and guards only its STORE (a guarded trip is a branch the
    // compiler does not move loads across: the 784-float copy of a sample's image was two dependent trips to memory).  A
    // scatter adds onto elements other trips may touch: it keeps the rolled loop.
    const long whole_trips = items / g.threads, ragged_items = items % g.threads;
    m.route.kind = si.seed ? SampleMemberRoute::Seed : scatter ? SampleMemberRoute::Scatter : si.raw ? SampleMemberRoute::Raw : SampleMemberRoute::Items;
    m.route.trips = whole_trips;
    m.route.ragged_trip = ragged_items > 0;
    m.route.rolled = !(!scatter && whole_trips <= 12 && rtotal * whole_trips <= 256);
    if (!scatter && whole_trips <= 12 && rtotal * whole_trips <= 256) {
      if (ragged_items > 0)
        c += "    {\n      const bool ok_ = threadIdx.x < " + std::to_string(ragged_items) + ";\n      const long idx = ok_ ? threadIdx.x + " +
             std::to_string(whole_trips * g.threads) + "L : 0L;\n" + body + "      if (ok_) {\n" + body_store + "      }\n    }\n";
      if (whole_trips > 0)
        c += "    _Pragma(\"unroll\") for (int it_ = 0; it_ < " + std::to_string(whole_trips) + "; ++it_) {\n      const long idx = threadIdx.x + it_ * " +
             NT + "L;\n" + body + body_store + "    }\n";
    } else {
      c += "    for (long idx = threadIdx.x; idx < " + std::to_string(items) + "L; idx += " + NT + ") {\n" + body + body_store + "    }\n";
    }
  }
};

// Barriers between INDEPENDENT members go.  Member b needs no barrier in front of it when, for every member a since the
// last barrier that stays, a's result is neither read nor written by b, b's result is not read by a, and at most one of
// them uses `scratch`.  Then the waves that are done with a (a row-block member with 9 blocks for 8 waves leaves seven
// waves waiting for the ninth block) start on b; the barrier behind b orders both against what follows.
// prologue_barrier goes when the first member touches none of what the prologue writes (its loads travel with the staged ones).
void elide_barriers(const SampleCtx& cx, bool& prologue_barrier, std::vector<SampleMember>& members) {
  const SampleGroup& g = cx.g;
  struct Use {
    std::set<int> reads, writes;
    bool scratch = false;
  };
  std::vector<Use> use(members.size());
  for (size_t gi = 0; gi < members.size(); ++gi) {
    const Kernel& k = cx.all[g.kernel_index[gi]];
    for (auto& rd : k.reads) use[gi].reads.insert(rd.tensor);
    use[gi].writes.insert(k.write.tensor);
    if (!g.overwrite[gi]) use[gi].reads.insert(k.write.tensor);
    use[gi].scratch = members[gi].uses_scratch;
    if (members[gi].reads_zeros4) use[gi].reads.insert(-4);   // (the prologue writes them)
  }
  Use prologue;
  for (auto& kv : g.staged) prologue.writes.insert(kv.first);
  for (int t : g.lds_zero) prologue.writes.insert(t);
  prologue.writes.insert(-4);
  auto conflict = [](const Use& a, const Use& b) {   // b behind a without a barrier
    for (int w : a.writes)
      if (b.reads.count(w) || b.writes.count(w)) return true;
    for (int w : b.writes)
      if (a.reads.count(w)) return true;
    return a.scratch && b.scratch;
  };
  std::vector<const Use*> since;   // the members (and the prologue) since the last barrier that stays
  if (!members.empty()) {
    if (prologue_barrier && !conflict(prologue, use[0])) {
      prologue_barrier = false;
      since.push_back(&prologue);
    }
    since.push_back(&use[0]);
  }
  for (size_t b = 1; b < members.size(); ++b) {
    bool independent = true;
    for (const Use* a : since)
      if (conflict(*a, use[b])) independent = false;
    if (independent) members[b - 1].barrier_after = false;
    else since.clear();
    since.push_back(&use[b]);
  }
}

// 32-bit index arithmetic where it is exact: every tensor (and the slab) has fewer than 2^31 elements and no member
// computes with Index VALUES (`toScalar(i * 100000)`: only addressing is known to fit — the rule of Slot::Narrow,
// codegen.hpp).  64-bit divisions and multiply-adds per element were most of a convolution member's time.
bool index_fits_32_bits(const SampleCtx& cx, const std::set<int>& touched) {
  bool narrow = cx.g.narrow_index && cx.g.B * std::max(1L, cx.g.slab_floats) < (1L << 31);
  for (int t : touched) narrow = narrow && prodv(cx.shapes.at(t)) < (1L << 31);
  for (int ki : cx.g.kernel_index) {
    const Kernel& k = cx.all[ki];
    const std::vector<Ty> ty = infer_types(k);
    for (auto& ins : k.instrs) {
      const bool index_typed = ins.res > 0 && ins.res < (int)ty.size() && ty[ins.res] == Ty::Index;
      const bool derived = ins.kind != IK::Shape && ins.kind != IK::Len && ins.kind != IK::ShapeLen && ins.kind != IK::Epoch;
      if (index_typed && derived) narrow = false;
    }
  }
  return narrow;
}

// The kernel's body from its parts.  narrow: 32-bit index arithmetic (index_fits_32_bits).
// EG_SAMPLE_TRACE=1 (detector): block 0 stamps the cycle counter behind every member's barrier and prints the stamps
// (cycles since the first) at the end — where a sample kernel's time goes, without the dead-code elimination that makes
// EG_SAMPLE_STOP's differences hard to read (a member whose result never leaves LDS disappears with its producers).
// (EG_SAMPLE_TRACE=100 + k: member k runs twice — idempotent when it overwrites its result — so that the stamps show
// what its second, instruction-cache-warm execution costs)
std::string assemble(const SampleCtx& cx, const std::string& head, bool head_barrier, const std::string& row,
                     const std::vector<SampleMember>& members, bool narrow) {
  const bool trace = eg::sw::is_set(eg::Sw::SAMPLE_TRACE);
  const long repeat = eg::sw::integer(eg::Sw::SAMPLE_TRACE, 0) - 100;   // (unset: negative, no member repeats)
  const std::string barrier = "  __syncthreads();\n";
  const std::string stamp = trace ? "  if (threadIdx.x == 0 && blockIdx.x == 0 && trn_ < 48) tr_[trn_++] = __builtin_readcyclecounter();\n" : "";
  const std::regex long_type("\\blong\\b"), long_literal("\\b([0-9]+)L\\b");
  auto text = [&](const std::string& s) { return narrow ? std::regex_replace(std::regex_replace(s, long_type, "int"), long_literal, "$1") : s; };
  std::string c = trace ? "  long long tr_[48]; int trn_ = 0;\n" + stamp : "";
  c += text(head);
  if (head_barrier) c += barrier + stamp;
  c += text(row);
  for (size_t i = 0; i < members.size(); ++i) {
    if (repeat >= 0 && (long)i == repeat && i + 1 < members.size()) {
      c += "  _Pragma(\"nounroll\") for (int rep_ = 0; rep_ < 2; ++rep_) {\n" + text(members[i].text) + barrier + stamp + "  }\n";
    } else {
      c += text(members[i].text);
      if (members[i].barrier_after) c += barrier + stamp;
    }
  }
  if (trace)
    c += "  if (threadIdx.x == 0 && blockIdx.x == 0) {\n    printf(\"[eg] " + cx.g.name + " cycles behind each member barrier:\");\n"
         "    for (int k_ = 1; k_ < trn_; ++k_) printf(\" %d:%lld\", k_, tr_[k_] - tr_[0]);\n    printf(\"\\n\");\n  }\n";
  return c;
}

}  // namespace

int generate_sample_group(const std::vector<Kernel>& all, const std::vector<KernelInfo>& infos, const Shapes& shapes, SampleGroup& g) {
  std::set<int> touched, written;
  for (size_t i = 0; i < g.kernel_index.size(); ++i) {
    const Kernel& k = all[g.kernel_index[i]];
    for (auto& rd : k.reads) touched.insert(rd.tensor);
    if (!g.infos[i].reduced) {
      touched.insert(k.write.tensor);
      written.insert(k.write.tensor);
    }
  }
  SampleCtx cx{all, infos, shapes, g, std::to_string(g.threads), {}};
  std::string sig;
  std::string head = emit_prologue(g, cx.NT, touched, written, sig);
  // EG_SAMPLE_STOP=<k> (tuning aid): the kernel ends behind member k — wrong numbers, the time of the first k + 1 members
  const long stop = eg::sw::integer(eg::Sw::SAMPLE_STOP, -1);
  std::vector<SampleMember> members;
  long scratch_floats = 0;
  bool need_dummy = false, need_zeros4 = false;
  for (size_t gi = 0; gi < g.kernel_index.size(); ++gi) {
    if (stop >= 0 && (long)gi > stop) break;
    SampleMember m;
    m.text = "  {  // kernel " + std::to_string(gi) + ": " + to_text(all[g.kernel_index[gi]]).substr(0, 100) + "\n";
    const MemberEmitter e{cx, gi, m};
    if (e.si.conv_role != 0) {
      m.route.kind = SampleMemberRoute::Conv;
      m.route.conv_role = e.si.conv_role;
      m.route.slab = e.si.reduced ? (cx.slab_seen.count(e.k.write.tensor) ? 2 : 1) : 0;
      m.route.lds = !e.si.reduced && e.local(e.k.write.tensor) > 0;
      emit_conv_member(e);
    } else if (LoopNest nest(e); e.si.gather) {
      nest.emit_gather();
    } else {
      if (int rc = nest.setup()) return rc;
      nest.choose_blocking();
      nest.choose_split();
      if (nest.T > 1) nest.emit_split();
      else nest.emit_items();
      if (e.si.reduced) cx.slab_seen.insert(e.k.write.tensor);
    }
    m.text += "  }\n";
    scratch_floats = std::max(scratch_floats, m.scratch_floats);
    need_dummy = need_dummy || m.needs_dummy;
    need_zeros4 = need_zeros4 || m.reads_zeros4;
    members.push_back(std::move(m));
  }
  // ONE barrier behind the prologue (staged copies, zeroed tensors, the four zeros of the image-gradient gathers); it goes
  // too when the first member touches none of that
  bool prologue_barrier = !g.staged.empty() || !g.lds_zero.empty();
  const bool zeros4_barrier = need_zeros4 && !prologue_barrier;   // (no prologue barrier to ride on)
  if (need_zeros4) head += "  __shared__ __attribute__((aligned(16))) float zeros4_[4];\n  if (threadIdx.x < 4) zeros4_[threadIdx.x] = 0.0f;\n";
  if (need_dummy) head = "  __shared__ float dummy_[" + cx.NT + "];\n" + head;   // (not `scratch`: a member behind an elided barrier may be using that)
  if (scratch_floats > 0) head = "  __shared__ float scratch[" + std::to_string(scratch_floats) + "];\n" + head;
  if (!eg::sw::on(eg::Sw::SAMPLE_KEEP_BARRIERS)) elide_barriers(cx, prologue_barrier, members);
  const std::string row = g.slab_floats > 0 ? "  float* const row = slab + n * " + std::to_string(g.slab_floats) + "L;\n" : "";
  g.narrow = index_fits_32_bits(cx, touched);
  g.routes.clear();
  g.barriers_kept = 0;
  for (auto& mem : members) {
    g.routes.push_back(mem.route);
    if (mem.barrier_after) ++g.barriers_kept;
  }
  g.source = sig + " {\n" + assemble(cx, head, prologue_barrier || zeros4_barrier, row, members, g.narrow) + "}\n";
  return EG_OK;
}

}  // namespace eg::kd
