// Shared by the row-fusion units (rowfuse_*.cpp) and by nothing else; rowfuse.hpp is the layer's public header.  No HIP header.
#pragma once
#include <algorithm>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../error.hpp"
#include "../switches.hpp"
#include "codegen.hpp"
#include "exprgrad_hip.h"
#include "rowfuse.hpp"

namespace eg::kd {

constexpr long MAX_INNER = 64;     // floats of one tensor row kept in registers
constexpr long SMALL_MAX = 4096;   // a "small" tensor (parameters, their gradients, scalars)
constexpr long MAX_WORK = 2048;    // unrolled iterations of one kernel per sample

long prodv(const std::vector<long>& s, size_t from = 0);
// the reads of a kernel, then its write
std::vector<const Op*> ops_of(const Kernel& k);
bool lin_has(const Lin& l, int reg);
bool op_has(const Op& op, int reg);
// every loop of the kernel runs once
bool single_extent(const KernelInfo& info);
std::string lin_text(const Lin& l, const std::map<int, std::string>& subst);
// literal element offset of a tensor op (extents are literals in a per-plan kernel)
std::string literal_element(const Op& op, const Shapes& shapes, const std::string& name, long local_inner = 0);
// `<indent>const <type> r<res> = <expression>;`: one instruction of a member, shapes and lengths as literals
std::string instr_line(const Kernel& k, const Instr& ins, const std::vector<Ty>& ty, const Shapes& shapes, const std::string& indent);
// g.ptr_args of a row or wide group: every tensor that touches memory
void set_pointer_args(RowGroup& g);
// the prelude of a generated kernel that uses eg_xor_lane (EG_NO_DPP_BUTTERFLY: every step through __shfl_xor)
std::string xor_lane_prelude();
// One small kernel as a loop of a single 256-thread block over its independent iterations, reductions serial per
// thread, `__syncthreads()` behind it: the body of a small group, and of the tail a row group's last block runs
// (pointer names <prefix><tensor id>).
std::string small_kernel_body(const Kernel& k, const KernelInfo& info, const Shapes& shapes, const std::string& prefix, int serial,
                              bool barrier = true);

// ---- sample groups.  One member of the kernel, and what the assembly of the kernel has to know about it:
struct SampleMember {
  std::string text;            // `  {  // kernel <i>: ...` through its closing brace; the barrier behind it is not part of it
  bool uses_scratch = false;   // the waves' accumulator blocks meet in `scratch` ...
  long scratch_floats = 0;     // ... of that many floats
  bool reads_zeros4 = false;   // gathers read the four zeros the prologue keeps in LDS
  bool needs_dummy = false;    // row blocks store the lanes outside their tensor to a slot per thread of `dummy_`
  bool barrier_after = true;   // cleared by the barrier elision when the next member is independent of this one
  SampleMemberRoute route;     // the decisions taken while `text` was written (SampleGroup::routes)
};

struct SampleCtx {
  const std::vector<Kernel>& all;
  const std::vector<KernelInfo>& infos;
  const Shapes& shapes;
  SampleGroup& g;
  const std::string NT;       // the block size as text
  std::set<int> slab_seen;    // tensors summed over the batch that a member has contributed to already
};

// Member gi while it is emitted: the context, and the member's own kernel, analysis and text.
struct MemberEmitter {
  SampleCtx& cx;
  const size_t gi;
  SampleMember& m;
  const Shapes& shapes = cx.shapes;
  const SampleGroup& g = cx.g;
  const std::string& NT = cx.NT;
  const Kernel& k = cx.all[g.kernel_index[gi]];
  const KernelInfo& info = cx.infos[g.kernel_index[gi]];
  const SampleKernelInfo& si = g.infos[gi];
  std::string& c = m.text;

  // floats of the block's own slice of `tensor` in LDS (0: the tensor lives in global memory)
  long local(int tensor) const {
    auto it = g.lds.find(tensor);
    return it == g.lds.end() ? 0 : it->second;
  }
};

// The body of a member on the matrix cores (si.conv_role != 0), appended to its text.
void emit_conv_member(MemberEmitter e);

}  // namespace eg::kd
