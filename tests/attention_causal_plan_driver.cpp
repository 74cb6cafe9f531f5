// Prints the causal tile bounds of csrc/kernels/attention_plan.hpp (constexpr, header only) for tests/test_attention_causal_plan_cpu.py.
//   attention_causal_plan_driver I J offset
// One line "visible=N", then per row tile "row T key_tiles=N cut=<the key tiles, of those visited, that need the select>", then
// per key tile "key T first_row_tile=N" (-1: the dK/dV block's loop is empty).
#include <cstdio>
#include <cstdlib>

#include "kernels/attention_plan.hpp"

using namespace eg::attention;

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "expected 3 arguments\n");
    return 2;
  }
  const long I = std::atol(argv[1]), J = std::atol(argv[2]);
  const long offset = std::atol(argv[3]) < J ? std::atol(argv[3]) : J;   // the entries' clamp
  const long visible = causal_visible_keys(I, offset, J);
  std::printf("visible=%ld\n", visible);
  for (long t = 0; t < (I + TILE_I - 1) / TILE_I; ++t) {
    const long nt = causal_key_tiles(t * TILE_I, offset, visible);
    std::printf("row %ld key_tiles=%ld cut=", t, nt);
    for (long u = 0; u < nt; ++u)
      if (causal_tile_cut(t * TILE_I, u * TILE_J, offset, J)) std::printf("%ld,", u);
    std::printf("\n");
  }
  for (long u = 0; u < (J + TILE_J - 1) / TILE_J; ++u)   // -1: no row sees the block's keys
    std::printf("key %ld first_row_tile=%ld\n", u, u * TILE_J < visible ? causal_first_row_tile(u * TILE_J, offset) : -1);
  return 0;
}
