// Pattern matching of lowered kernels against the hand-written library (match.cpp).  No HIP header: kernel descriptions only.
#pragma once
#include "kd.hpp"

namespace eg {
namespace model {

using namespace eg::kd;

struct GemmMatch {
  int a_read = 0, b_read = 0;  // indices into k.reads
  bool trans_a = false, trans_b = false;
  int li = 0, lj = 0, lk = 0;  // loop indices of m, n, k
};

struct ConvMatch {
  // which operand plays which part: -1 = the written tensor, 0 / 1 = k.reads[i]
  int out_op = -1, img_op = 0, flt_op = 1;
  bool batched = true;
  enum Role { Forward, GradImage, GradFilter } role = Forward;
};

bool bare2(const Op& op, int& r0, int& r1);
int loop_index(const Kernel& k, int reg);
bool match_gemm(const Kernel& k, GemmMatch& m);
bool match_bias(const Kernel& k, int tensor);
bool match_conv(const Kernel& k, ConvMatch& m);

}  // namespace model
}  // namespace eg
