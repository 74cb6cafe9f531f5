#include "rowfuse_internal.hpp"

namespace eg::kd {

long prodv(const std::vector<long>& s, size_t from) {
  long p = 1;
  for (size_t i = from; i < s.size(); ++i) p *= s[i];
  return p;
}

std::vector<const Op*> ops_of(const Kernel& k) {
  std::vector<const Op*> ops;
  for (auto& rd : k.reads) ops.push_back(&rd);
  ops.push_back(&k.write);
  return ops;
}

bool lin_has(const Lin& l, int reg) { return l.factor_of(reg) != 0; }

// every loop of the kernel runs once
bool single_extent(const KernelInfo& info) {
  for (auto& b : info.bounds)
    if (b.second - b.first != 1) return false;
  return true;
}

bool op_has(const Op& op, int reg) {
  for (auto& d : op.dims)
    if (lin_has(d, reg)) return true;
  return false;
}

std::string lin_text(const Lin& l, const std::map<int, std::string>& subst) {
  std::string s = std::to_string(l.constant) + "L";
  for (auto& f : l.factors) {
    auto it = subst.find(f.first);
    const std::string var = it != subst.end() ? it->second : "r" + std::to_string(f.first);
    s += " + " + std::to_string(f.second) + "L * " + var;
  }
  return "(" + s + ")";
}

std::string literal_element(const Op& op, const Shapes& shapes, const std::string& name, long local_inner) {
  const std::vector<long>& shp = shapes.at(op.tensor);
  const std::map<int, std::string> no_subst;
  std::string idx;
  if (op.raw) {
    idx = lin_text(op.dims[0], no_subst);
  } else {
    long stride = 1;
    idx = "0L";
    for (size_t d = shp.size(); d-- > 0;) {
      idx += " + " + std::to_string(stride) + "L * " + lin_text(op.dims[d], no_subst);
      stride *= shp[d];
    }
  }
  // a block's own slice of a [B, ...] tensor (kept in LDS): the same element, counted from the start of sample n
  if (local_inner > 0) idx = "(" + idx + ") - n * " + std::to_string(local_inner) + "L";
  return name + "[" + idx + "]";
}

std::string instr_line(const Kernel& k, const Instr& ins, const std::vector<Ty>& ty, const Shapes& shapes, const std::string& indent) {
  const Ty t = ty[ins.res];
  const char* ctype = t == Ty::Scalar ? "float" : (t == Ty::Index ? "long" : "bool");
  std::string special;
  if (ins.kind == IK::Epoch) {
    special = "EP";
  } else if (ins.kind == IK::Shape || ins.kind == IK::Len || ins.kind == IK::ShapeLen) {
    const std::vector<long>& shp = shapes.at(ins.tensor);
    long v = 0;
    if (ins.kind == IK::Len) v = prodv(shp);
    else if (ins.kind == IK::ShapeLen) v = (long)shp.size();
    else {
      int d = ins.dim < 0 ? ins.dim + (int)shp.size() : ins.dim;
      v = (d >= 0 && d < (int)shp.size()) ? shp[d] : 0;
    }
    special = std::to_string(v) + "L";
  }
  std::string e = instr_expression(ins, special, "r");
  if (k.is_seed && ins.kind == IK::Scalar) e = "GS";
  return indent + "const " + ctype + " r" + std::to_string(ins.res) + " = " + e + ";\n";
}

void set_pointer_args(RowGroup& g) {
  g.ptr_args.clear();
  for (auto& kv : g.tensors) {
    const RowGroupTensor& t = kv.second;
    const bool mem = t.role == RowGroupTensor::RowExternal || t.role == RowGroupTensor::SmallExternal ||
                     (t.role == RowGroupTensor::RowLocal && (t.load_first || t.store));
    if (mem) g.ptr_args.push_back(kv.first);
  }
}

// eg_xor_lane<OFF>(v): the value of lane (l ^ OFF) — what __shfl_xor(v, OFF, 64) returns through the LDS crossbar, here as
// DPP moves for OFF < 16 (quad permutations for 1 and 2; for 4 and 8 two row shifts whose bank masks pick, per group of four
// lanes, the one that comes from the right side): four of a butterfly's six steps become vector instructions without a
// trip to LDS.  Same partner lanes, so the same sums to the bit (tests/test_gpu_row_tail.py holds the in-kernel fold
// against row_finalize_kernel, which shuffles).
static const char* const kXorLane =
    "#ifndef EG_XOR_LANE\n#define EG_XOR_LANE\n"
    "template <int OFF> __device__ __forceinline__ float eg_xor_lane(float v) {\n"
    "  const int b = __builtin_bit_cast(int, v);\n"
    "  if constexpr (OFF == 1) return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(b, b, 0xB1, 0xF, 0xF, false));\n"
    "  else if constexpr (OFF == 2) return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(b, b, 0x4E, 0xF, 0xF, false));\n"
    "  else if constexpr (OFF == 4) {\n"
    "    int t = __builtin_amdgcn_update_dpp(b, b, 0x104, 0xF, 0x5, false);   // row_shl:4 into lanes 0-3, 8-11 of a row\n"
    "    t = __builtin_amdgcn_update_dpp(t, b, 0x114, 0xF, 0xA, false);       // row_shr:4 into lanes 4-7, 12-15\n"
    "    return __builtin_bit_cast(float, t);\n"
    "  } else if constexpr (OFF == 8) {\n"
    "    int t = __builtin_amdgcn_update_dpp(b, b, 0x108, 0xF, 0x3, false);   // row_shl:8 into lanes 0-7\n"
    "    t = __builtin_amdgcn_update_dpp(t, b, 0x118, 0xF, 0xC, false);       // row_shr:8 into lanes 8-15\n"
    "    return __builtin_bit_cast(float, t);\n"
    "  } else return __shfl_xor(v, OFF, 64);\n"
    "}\n#endif\n";
std::string xor_lane_prelude() {
  return eg::sw::on(eg::Sw::NO_DPP_BUTTERFLY) ? std::string("#ifndef EG_XOR_LANE\n#define EG_XOR_LANE\ntemplate <int OFF> __device__ __forceinline__ float "
                                                          "eg_xor_lane(float v) { return __shfl_xor(v, OFF, 64); }\n#endif\n")
                                            : std::string(kXorLane);
}

}  // namespace eg::kd
