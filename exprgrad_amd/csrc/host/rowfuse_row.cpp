// Row groups: one THREAD per sample (rowfuse.hpp).
#include "rowfuse_internal.hpp"

namespace eg::kd {

RowKernelInfo analyse_row_kernel(const Program& prog, const Kernel& k, const KernelInfo& info, const Shapes& shapes,
                                 long B) {
  RowKernelInfo r;
  if (!info.ok || B <= 0 || !k.index_instrs.empty()) return r;
  const std::vector<const Op*> ops = ops_of(k);
  for (const Op* op : ops)
    if (!shapes.count(op->tensor)) return r;
  auto small = [&](const Op* op) { return prodv(shapes.at(op->tensor)) <= SMALL_MAX; };
  auto state = [&](const Op* op) {
    const TK kind = prog.tensors[op->tensor].kind;
    return kind == TK::Param || kind == TK::Cache;
  };

  long other_work = 1;
  for (size_t l = 0; l < k.loops.size(); ++l) other_work *= std::max(0L, info.bounds[l].second - info.bounds[l].first);

  // the gradLoss seed and similar: no batch loop at all, everything small
  if (k.is_seed) {
    bool all_small = true;
    for (const Op* op : ops) all_small = all_small && small(op);
    if (all_small && other_work <= 64) {
      r.ok = true;
      r.small_only = true;
      r.work = other_work;
    }
    return r;
  }
  if (!k.setup.empty()) return r;

  for (size_t l = 0; l < k.loops.size(); ++l) {
    const int y = k.loops[l].reg;
    const long lo = info.bounds[l].first, hi = info.bounds[l].second;
    if (lo != 0) continue;
    bool ok = true, any = false;
    bool raw = false;
    long inner = 0;
    // a raw iterator ({it}) shows in raw ops only; [B,1] tensors make its extent equal B as well
    bool any_raw = false;
    for (const Op* op : ops)
      if (op_has(*op, y) && op->raw) any_raw = true;
    if (hi == B && !any_raw) {
      for (const Op* op : ops) {
        if (!op_has(*op, y)) {
          if (!small(op)) ok = false;
          continue;
        }
        any = true;
        const std::vector<long>& shp = shapes.at(op->tensor);
        if (op->raw || state(op) || shp.empty() || shp[0] != B || op->dims[0].only_register() != y ||
            prodv(shp, 1) > MAX_INNER)
          ok = false;
        for (size_t d = 1; ok && d < op->dims.size(); ++d)
          if (lin_has(op->dims[d], y)) ok = false;
      }
    } else if (any_raw && hi >= B && hi % B == 0 && hi / B <= MAX_INNER) {
      // raw iterator over B * S elements: it = y * S + j
      raw = true;
      inner = hi / B;
      for (const Op* op : ops) {
        if (!op_has(*op, y)) {
          if (!small(op)) ok = false;
          continue;
        }
        any = true;
        const std::vector<long>& shp = shapes.at(op->tensor);
        if (!op->raw || state(op) || op->dims.size() != 1 || op->dims[0].only_register() != y || shp.empty() ||
            shp[0] != B || prodv(shp) != hi)
          ok = false;
      }
    } else {
      continue;
    }
    if (!ok || !any) continue;
    // the iterator must not be used as a value by the expression (it only indexes)
    for (auto& ins : k.instrs)
      for (int a : ins.args)
        if (a == y) ok = false;
    if (!ok) continue;
    const long span = hi - lo;
    long work = span > 0 ? other_work / span : 0;
    if (raw) work *= inner;
    if (work > MAX_WORK) continue;
    r.ok = true;
    r.row_loop = (int)l;
    r.raw = raw;
    r.inner = inner;
    r.work = work;
    return r;
  }
  return r;
}

namespace {

struct GroupEmitter {
  const Shapes& shapes;
  RowGroup& g;
  std::string code;

  std::string tname(int t) const { return "t" + std::to_string(t); }

  // text of the element a tensor op refers to
  std::string element(const Op& op, const RowKernelInfo& ri, const Kernel& k, const std::string& raw_j) {
    const RowGroupTensor& gt = g.tensors.at(op.tensor);
    const std::vector<long>& shp = shapes.at(op.tensor);
    const int yreg = ri.row_loop >= 0 ? k.loops[ri.row_loop].reg : 0;
    const bool row_op = ri.row_loop >= 0 && op_has(op, yreg);
    std::string idx;
    if (row_op) {
      if (ri.raw) {
        idx = raw_j;
      } else {
        long stride = 1;
        std::vector<std::string> terms;
        for (size_t d = shp.size(); d-- > 1;) {
          terms.push_back(std::to_string(stride) + "L * " + lin_text(op.dims[d], {}));
          stride *= shp[d];
        }
        idx = "0L";
        for (auto& t : terms) idx += " + " + t;
      }
      if (gt.role == RowGroupTensor::RowLocal) return "L" + std::to_string(op.tensor) + "[" + idx + "]";
      return tname(op.tensor) + "[y * " + std::to_string(gt.inner) + "L + " + idx + "]";
    }
    // small tensor
    switch (gt.role) {
      case RowGroupTensor::SmallLocal: return literal_element(op, shapes, "S" + std::to_string(op.tensor));
      case RowGroupTensor::Reduction: return literal_element(op, shapes, "R" + std::to_string(op.tensor));
      default: return literal_element(op, shapes, tname(op.tensor));
    }
  }

  void emit_kernel(const Kernel& k, const KernelInfo& info, const RowKernelInfo& ri, int serial) {
    const std::vector<Ty> ty = infer_types(k);
    std::string raw_j;
    code += "  if (active) {  // kernel " + std::to_string(serial) + ": " + to_text(k).substr(0, 90) + "\n";
    for (auto& s : k.setup) {  // host-evaluated values become literals (shapes are fixed for this build)
      code += "    const long r" + std::to_string(s.res) + " = " + std::to_string(info.vals.at(s.res)) + "L;\n";
    }
    int depth = 0;
    for (size_t l = 0; l < k.loops.size(); ++l) {
      const std::string r = "r" + std::to_string(k.loops[l].reg);
      if ((int)l == ri.row_loop) {
        if (ri.raw) {
          raw_j = "j" + std::to_string(serial);
          code += "    _Pragma(\"unroll\") for (long " + raw_j + " = 0; " + raw_j + " < " + std::to_string(ri.inner) + "L; ++" +
                  raw_j + ") {\n";
          ++depth;
        }
        continue;  // the batch iterator is the thread's row
      }
      code += "    _Pragma(\"unroll\") for (long " + r + " = " + std::to_string(info.bounds[l].first) + "L; " + r + " < " +
              std::to_string(info.bounds[l].second) + "L; ++" + r + ") {\n";
      ++depth;
    }
    for (auto& rd : k.reads)
      code += "      const float r" + std::to_string(rd.reg) + " = " + element(rd, ri, k, raw_j) + ";\n";
    for (auto& ins : k.instrs) code += instr_line(k, ins, ty, shapes, "      ");
    const std::string w = element(k.write, ri, k, raw_j);
    code += "      " + w + " = " + w + " + r" + std::to_string(k.result) + ";\n";
    for (int d = 0; d < depth; ++d) code += "    }\n";
    code += "  }\n";
  }
};

}  // namespace

int generate_row_group(const std::vector<Kernel>& all, const std::vector<KernelInfo>& infos,
                       const Shapes& shapes, RowGroup& g) {
  GroupEmitter em{shapes, g, {}};
  set_pointer_args(g);
  // Large batches with little per-thread state: cap the kernel at 96 registers (5 waves per SIMD) so its
  // waves fit next to a long contraction's on the same SIMD (a 256x256 tile leaves 128 of 512 registers
  // per lane): on the side lane of the batch pipeline a 7 us row group took 53 us waiting for whole CUs.
  long state = 0;
  for (auto& kv : g.tensors)
    if (kv.second.role != RowGroupTensor::RowExternal && kv.second.role != RowGroupTensor::SmallExternal) state += kv.second.inner;
  const bool slim = g.B >= 4096 && state <= 64;
  std::string sig = std::string("extern \"C\" __global__ void __launch_bounds__(256") + (slim ? ", 5" : "") + ") " + g.name +
                    "(float* __restrict__ partial";
  // a tensor the tail kernels touch is also reachable through u<t> (and written there): its t<t> must not promise
  // that nobody else modifies it
  std::set<int> tail_touched;
  if (g.in_kernel_finalize && g.red_total > 0)
    for (int ki : g.tail_kernels) {
      tail_touched.insert(all[ki].write.tensor);
      for (auto& rd : all[ki].reads) tail_touched.insert(rd.tensor);
    }
  for (int t : g.ptr_args) {
    const RowGroupTensor& gt = g.tensors.at(t);
    sig += gt.role == RowGroupTensor::RowLocal ? ", float* t" : tail_touched.count(t) ? ", const float* t" : ", const float* __restrict__ t";
    sig += std::to_string(t);
  }
  sig += ", long B, float GS, long EP";
  // One block (a batch of at most 256 rows): the totals go straight to their destinations.  In a captured graph a
  // dependent launch costs ~4.5 us whatever it does, and row_finalize of one partial row does nothing but copy
  // (p + 0 + 0 + 0 in its tree: the same value).
  g.single_block = g.B <= 256 && g.red_total > 0 && !eg::sw::on(eg::Sw::NO_ROW_DIRECT);
  if (g.single_block) g.in_kernel_finalize = false;
  if (g.red_total <= 0) g.in_kernel_finalize = false;
  if (!g.in_kernel_finalize) g.tail_kernels.clear();
  if (g.single_block || g.in_kernel_finalize)
    for (auto& kv : g.tensors)
      if (kv.second.role == RowGroupTensor::Reduction) sig += ", float* d" + std::to_string(kv.first);
  g.tail_ptr_args.clear();
  if (g.in_kernel_finalize) {
    sig += ", unsigned* counter, long MODE";
    g.tail_ptr_args.assign(tail_touched.begin(), tail_touched.end());
    // NOT __restrict__: the same tensors are reachable through d<t> (the totals just written) and t<t> (parameters the
    // tail overwrites) in this kernel; the barriers between those accesses order them, the qualifier would deny them
    for (int t : g.tail_ptr_args) sig += ", float* u" + std::to_string(t);
  }
  sig += ")";

  std::string& c = em.code;
  // in_kernel_finalize: the samples are walked with a grid stride, so that a launch may use FEWER blocks than B / 256 (a
  // row group with a tail: 64 blocks — fewer arrivals at the ticket counter, fewer partial rows for the last block);
  // with ceil(B / 256) blocks the loop runs once and every value is what the one-sample-per-thread form computes.
  const bool strided = g.in_kernel_finalize;
  g.unrolled_trips = 0;
  if (!strided) c += "  const long y = (long)blockIdx.x * 256 + threadIdx.x;\n  const bool active = y < B;\n";
  std::string init;  // per-sample state: (re)initialised for every sample
  for (auto& kv : g.tensors) {
    const RowGroupTensor& t = kv.second;
    const std::string id = std::to_string(kv.first);
    if (t.role == RowGroupTensor::RowLocal) {
      c += "  float L" + id + "[" + std::to_string(t.inner) + "];\n";
      init += "  _Pragma(\"unroll\") for (int j = 0; j < " + std::to_string(t.inner) + "; ++j) L" + id + "[j] = ";
      init += t.load_first ? "active ? t" + id + "[y * " + std::to_string(t.inner) + "L + j] : 0.0f;\n" : "0.0f;\n";
    } else if (t.role == RowGroupTensor::SmallLocal || t.role == RowGroupTensor::Reduction) {
      const char* p = t.role == RowGroupTensor::SmallLocal ? "S" : "R";
      c += std::string("  float ") + p + id + "[" + std::to_string(t.inner) + "];\n";
      std::string z = "  _Pragma(\"unroll\") for (int j = 0; j < " + std::to_string(t.inner) + "; ++j) " + p + id + "[j] = 0.0f;\n";
      if (t.role == RowGroupTensor::Reduction) c += z;  // batch totals: once
      else init += z;
    }
  }
  if (strided) c += "  auto one_sample = [&](const long y) {\n  const bool active = true;\n";
  c += init;
  for (size_t i = 0; i < g.kernel_index.size(); ++i)
    em.emit_kernel(all[g.kernel_index[i]], infos[g.kernel_index[i]], g.infos[i], (int)i);
  // rows that are needed after the group
  for (auto& kv : g.tensors) {
    const RowGroupTensor& t = kv.second;
    if (t.role != RowGroupTensor::RowLocal || !t.store) continue;
    const std::string id = std::to_string(kv.first);
    c += "  if (active) { _Pragma(\"unroll\") for (int j = 0; j < " + std::to_string(t.inner) + "; ++j) t" + id + "[y * " +
         std::to_string(t.inner) + "L + j] = L" + id + "[j]; }\n";
  }
  if (strided) {
    c += "  };\n";
    const long per_trip = g.grid_blocks * 256;
    const long trips = per_trip > 0 && g.B % per_trip == 0 ? g.B / per_trip : 0;
    g.unrolled_trips = trips >= 2 && trips <= 8 ? trips : 0;
    if (trips >= 2 && trips <= 8) {
      // the launch this kernel was generated for: every thread has exactly `trips` samples, no bounds test between them
      c += "  if (gridDim.x == " + std::to_string(g.grid_blocks) + " && B == " + std::to_string(g.B) + "L) {\n";
      c += "    _Pragma(\"unroll\") for (int trip = 0; trip < " + std::to_string(trips) + "; ++trip) one_sample((long)blockIdx.x * 256 + threadIdx.x + (long)trip * " +
           std::to_string(per_trip) + "L);\n  } else {\n";
      c += "    for (long y = (long)blockIdx.x * 256 + threadIdx.x; y < B; y += (long)gridDim.x * 256) one_sample(y);\n  }\n";
    } else {
      c += "  for (long y = (long)blockIdx.x * 256 + threadIdx.x; y < B; y += (long)gridDim.x * 256) one_sample(y);\n";
    }
  }
  // batch reductions: wave shuffles, then the four wave totals through LDS, one partial row per block
  if (g.red_total > 0) {
    const std::string E = std::to_string(g.red_total);
    c += "  __shared__ float red[4 * " + E + "];\n";
    c += "  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;\n";
    for (auto& kv : g.tensors) {
      const RowGroupTensor& t = kv.second;
      if (t.role != RowGroupTensor::Reduction) continue;
      const std::string id = std::to_string(kv.first);
      // The butterfly runs over ALL the values of a step together (round 6, EG_ROW_TRACE: one value after the other — the
      // guarded store behind each kept the compiler from interleaving them — every one of the 6 x 17 shuffles of the XOR
      // step's totals waited out the LDS crossbar's latency by itself: 7 700 cycles, and again in the last block's fold;
      // together 6.5 of the kernel's 11.8 us).  Same additions per value, same order.
      for (int off = 32; off >= 1; off >>= 1)
        c += "  _Pragma(\"unroll\") for (int j = 0; j < " + std::to_string(t.inner) + "; ++j) R" + id + "[j] += eg_xor_lane<" + std::to_string(off) +
             ">(R" + id + "[j]);\n";
      c += "  if (lane == 0) {\n    _Pragma(\"unroll\") for (int j = 0; j < " + std::to_string(t.inner) + "; ++j) red[wave * " + E + " + " +
           std::to_string(t.red_offset) + " + j] = R" + id + "[j];\n  }\n";
    }
    c += "  __syncthreads();\n";
    if (g.single_block) {
      for (auto& kv : g.tensors) {
        const RowGroupTensor& t = kv.second;
        if (t.role != RowGroupTensor::Reduction) continue;
        const std::string id = std::to_string(kv.first), off = std::to_string(t.red_offset);
        c += "  for (int j = threadIdx.x; j < " + std::to_string(t.inner) + "; j += 256) {\n";
        c += "    const int e = " + off + " + j;\n";
        c += "    const float s = (red[e] + red[" + E + " + e]) + (red[2 * " + E + " + e] + red[3 * " + E + " + e]);\n";
        c += std::string("    d") + id + "[j] = " + (t.accumulate ? "d" + id + "[j] + s" : std::string("s")) + ";\n  }\n";
      }
    } else {
      // A block's partial row: whole 16-byte groups at a stride of ES floats.  With the in-kernel fold the groups go out as
      // ONE `global_store_dwordx4 sc0 sc1` each and come back as `global_load_dwordx4 sc0 sc1` (round 6, EG_ROW_TRACE: as
      // 4-byte accesses — every one a transaction of its own on the fabric — the last block of the XOR step waited 3.6 us for
      // its 17 stores to drain and 3.8 us for 64 x 17 loads: 7.4 of the kernel's 11.8 us).
      const std::string ES = std::to_string(g.red_stride()), G4 = std::to_string(g.red_stride() / 4);
      if (g.in_kernel_finalize) {
        c += "  typedef float f4_ __attribute__((ext_vector_type(4)));\n";
        c += "  if (threadIdx.x < " + G4 + ") {\n    f4_ tv;\n";
        c += "    _Pragma(\"unroll\") for (int k = 0; k < 4; ++k) {\n      const int e = 4 * threadIdx.x + k;\n";
        c += "      tv[k] = e < " + E + " ? (red[e] + red[" + E + " + e]) + (red[2 * " + E + " + e] + red[3 * " + E + " + e]) : 0.0f;\n    }\n";
        c += "    float* const dst = partial + (long)blockIdx.x * " + ES + " + 4 * threadIdx.x;\n";
        c += "    asm volatile(\"global_store_dwordx4 %0, %1, off sc0 sc1\" : : \"v\"(dst), \"v\"(tv) : \"memory\");\n  }\n";
      } else {
        c += "  for (int e = threadIdx.x; e < " + E + "; e += 256) {\n";
        c += "    const float total = (red[e] + red[" + E + " + e]) + (red[2 * " + E + " + e] + red[3 * " + E + " + e]);\n";
        c += "    partial[(long)blockIdx.x * " + ES + " + e] = total;\n  }\n";
      }
      if (g.in_kernel_finalize) {
        // The last block to arrive folds the partial rows.  No agent-scope fences (each costs ~1.7 us on MI355X, and
        // every block would pay one): the partial rows go out as write-through stores (system scope: sc0 sc1) and are
        // read back with loads of the same scope, which bypass the non-coherent caches on both sides
        // (MI355X_MICROARCH.md, "Workgroup dispatch ... inter-workgroup visibility": sc0 sc1 stores and loads on both
        // sides are a valid hand-off; the stores are drained — vmcnt(0) — before the block takes its ticket).
        // Sums in the order of row_finalize_kernel (reduce.hip): thread t of 256 adds rows t, t + 256, ...; xor-shuffle
        // tree per wave; ((w0 + w1) + w2) + w3 — the same value to the bit for the same number of blocks.
        // This hand-off is OUTSIDE the HIP / LLVM memory model (relaxed atomics + an explicit vmcnt drain instead of a
        // release / acquire pair on the ticket): it holds on gfx9-family ISAs, where stores count in vmcnt and sc0 sc1
        // accesses go to memory.  The library is built for gfx950 only; the generated text refuses anything else.
        c += "#if !defined(__gfx950__)\n#error \"row-tail hand-off relies on gfx950 cache-bypass stores and vmcnt store counting\"\n#endif\n";
        c += "  if (MODE != 0) {\n";
        c += "    __shared__ int s_last;\n";
        c += "    asm volatile(\"s_waitcnt vmcnt(0)\" ::: \"memory\");\n";
        c += "    __syncthreads();\n";
        c += "    if (threadIdx.x == 0) {\n";
        c += "      const unsigned ticket = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);\n";
        c += "      s_last = ticket == gridDim.x - 1 ? 1 : 0;\n";
        c += "      if (s_last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch\n";
        c += "    }\n";
        c += "    __syncthreads();\n";
        c += "    if (s_last) {\n";
        c += "      const int NB = (int)gridDim.x;\n";
        c += "      float acc[" + E + "];\n";
        c += "      _Pragma(\"unroll\") for (int e = 0; e < " + E + "; ++e) acc[e] = 0.0f;\n";
        c += "      for (int b = threadIdx.x; b < NB; b += 256) {\n";
        c += "        const float* const src = partial + (long)b * " + ES + ";\n        f4_ q_[" + G4 + "];\n";
        {
          std::string tie;
          for (long q = 0; q < g.red_stride() / 4; ++q) {
            c += "        asm volatile(\"global_load_dwordx4 %0, %1, off sc0 sc1\" : \"=v\"(q_[" + std::to_string(q) + "]) : \"v\"(src + " +
                 std::to_string(4 * q) + ") : \"memory\");\n";
            tie += std::string(q ? ", " : "") + "\"+v\"(q_[" + std::to_string(q) + "])";
          }
          // (the compiler does not count loads issued from inline assembly: the wait is explicit and tied to the registers)
          c += "        asm volatile(\"s_waitcnt vmcnt(0)\" : " + tie + " : : \"memory\");\n";
        }
        c += "        _Pragma(\"unroll\") for (int e = 0; e < " + E + "; ++e) acc[e] += q_[e >> 2][e & 3];\n      }\n";
        for (int off = 32; off >= 1; off >>= 1)
          c += "      _Pragma(\"unroll\") for (int e = 0; e < " + E + "; ++e) acc[e] += eg_xor_lane<" + std::to_string(off) + ">(acc[e]);\n";
        c += "      if (lane == 0) {\n        _Pragma(\"unroll\") for (int e = 0; e < " + E + "; ++e) red[wave * " + E + " + e] = acc[e];\n      }\n";
        c += "      __syncthreads();\n";
        for (auto& kv : g.tensors) {
          const RowGroupTensor& t = kv.second;
          if (t.role != RowGroupTensor::Reduction) continue;
          const std::string id = std::to_string(kv.first), off = std::to_string(t.red_offset);
          c += "      for (int j = threadIdx.x; j < " + std::to_string(t.inner) + "; j += 256) {\n";
          c += "        const int e = " + off + " + j;\n";
          c += "        const float s = ((red[e] + red[" + E + " + e]) + red[2 * " + E + " + e]) + red[3 * " + E + " + e];\n";
          c += std::string("        d") + id + "[j] = " + (t.accumulate ? "d" + id + "[j] + s" : std::string("s")) + ";\n      }\n";
        }
        if (!g.tail_kernels.empty()) {
          c += "      if (MODE == 2) {  // the kernels that follow the group, on the totals just written\n";
          c += "      __syncthreads();\n";
          // Kernels none of which touches what another one writes (one gradientDescent kernel per parameter,
          // base.nim:37-38) need no barrier between them: a thread's loads of all of them can be in flight together —
          // one memory round trip for the tail instead of one per kernel.
          bool independent = true;
          for (size_t i = 0; i < g.tail_kernels.size() && independent; ++i)
            for (size_t j = 0; j < g.tail_kernels.size() && independent; ++j) {
              if (i == j) continue;
              const Kernel &a = all[g.tail_kernels[i]], &b = all[g.tail_kernels[j]];
              if (a.write.tensor == b.write.tensor) independent = false;
              for (auto& rd : b.reads)
                if (rd.tensor == a.write.tensor) independent = false;
            }
          for (size_t i = 0; i < g.tail_kernels.size(); ++i)
            c += small_kernel_body(all[g.tail_kernels[i]], infos[g.tail_kernels[i]], shapes, "u", (int)i, !independent);
          c += "      }\n";
        }
        c += "    }\n  }\n";
        // EG_ROW_TRACE=1 (detector): the last block to arrive prints where ITS time went — cycles since its own start at:
        // samples done, partial row stored and drained, ticket taken, partial rows of all blocks read, totals and tail done
        if (eg::sw::on(eg::Sw::ROW_TRACE)) {
          auto insert_before = [&](const std::string& anchor, const std::string& text, size_t from) {
            const size_t at = c.find(anchor, from);
            if (at == std::string::npos) return std::string::npos;
            c.insert(at, text);
            return at + text.size() + anchor.size();
          };
          auto stamp = [](int k) { return "  tr_[" + std::to_string(k) + "] = __builtin_readcyclecounter();\n"; };
          c = "  long long tr_[8];\n" + stamp(0) + c;
          size_t pos = insert_before("  __shared__ float red[", stamp(1), 0);
          if (pos != std::string::npos) pos = insert_before("  if (threadIdx.x < ", stamp(6), pos);                  // wave totals in LDS
          if (pos != std::string::npos) pos = insert_before("    asm volatile(\"s_waitcnt vmcnt(0)\" ::: \"memory\");\n", stamp(7), pos);   // store issued
          if (pos != std::string::npos) pos = insert_before("    if (threadIdx.x == 0) {\n      const unsigned ticket", stamp(2), pos);
          if (pos != std::string::npos) pos = insert_before("    if (s_last) {\n", stamp(3), pos);
          if (pos != std::string::npos) pos = insert_before("      __syncthreads();\n", stamp(4), pos);
          const size_t end = c.rfind("    }\n  }\n");
          if (pos != std::string::npos && end != std::string::npos)
            c.insert(end, stamp(5) + "      if (threadIdx.x == 0) printf(\"[eg] " + g.name +
                              " last block (%d of %d): samples %lld, wave totals %lld, store issued %lld, drained %lld, ticket %lld, partials in %lld, done %lld cycles\\n\", "
                              "(int)blockIdx.x, (int)gridDim.x, tr_[1] - tr_[0], tr_[6] - tr_[0], tr_[7] - tr_[0], tr_[2] - tr_[0], tr_[3] - tr_[0], tr_[4] - tr_[0], tr_[5] - tr_[0]);\n");
        }
      }
    }
  }
  g.source = xor_lane_prelude() + sig + " {\n" + c + "}\n";
  return EG_OK;
}

}  // namespace eg::kd
