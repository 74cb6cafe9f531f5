// Host-side dispatch from the runtime storage order of a product's operands to kernels instantiated per order
// (gemm_f32_mfma.hip, gemm_batched.hip, gemm_f64_mfma.hip).
// Operand "k-contiguous" flags: A[M,K] row-major has k contiguous unless transposed; B[K,N] row-major has n contiguous
// unless transposed.
#pragma once
#include <type_traits>

namespace eg {
namespace gemm {

// Calls f(std::bool_constant<A_KC>, std::bool_constant<B_KC>) for the runtime operand layout.
template <class F>
void with_layout(bool a_kc, bool b_kc, F&& f) {
  if (a_kc && !b_kc) f(std::true_type(), std::false_type());         // NN
  else if (a_kc && b_kc) f(std::true_type(), std::true_type());      // NT
  else if (!a_kc && !b_kc) f(std::false_type(), std::false_type());  // TN
  else f(std::false_type(), std::true_type());                       // TT
}

// The same with a third flag: f(A_KC, B_KC, std::bool_constant<VEC>), the float64 kernels' 16-byte / 8-byte loads.
// (Kernels are emitted in the order f is instantiated here — load form first, then NT, NN, TT, TN, the order the float64
// kernels have always had — so the code object keeps its layout.)
template <class F>
void with_layout_vec(bool a_kc, bool b_kc, bool vec, F&& f) {
  const auto layout = [&](auto v) {
    if (a_kc && b_kc) f(std::true_type(), std::true_type(), v);         // NT
    else if (a_kc && !b_kc) f(std::true_type(), std::false_type(), v);  // NN
    else if (!a_kc && b_kc) f(std::false_type(), std::true_type(), v);  // TT
    else f(std::false_type(), std::false_type(), v);                    // TN
  };
  if (vec) layout(std::true_type());
  else layout(std::false_type());
}

}  // namespace gemm
}  // namespace eg
