// Prints plan_attention_causal_split (csrc/kernels/attention_plan.cpp, the only unit linked) and the decode of every block of an
// item for tests/test_attention_causal_split_plan_cpu.py.
//   attention_causal_split_plan_driver I J offset chunk [K D items cus]
// One line "key=value ..." for the plan, then one line "piece tile p pieces t0 t1 slot" per block index, in issue order.
#include <cstdio>
#include <cstdlib>

#include "kernels/attention_plan.hpp"

using namespace eg::attention;

int main(int argc, char** argv) {
  if (argc != 5 && argc != 9) {
    std::fprintf(stderr, "expected 4 or 8 arguments\n");
    return 2;
  }
  long a[8] = {0, 0, 0, 0, 20, 12, 2, 256};
  for (int i = 0; i + 1 < argc; ++i) a[i] = std::atol(argv[i + 1]);
  Problem p;
  p.batch0 = 1, p.batch1 = a[6], p.I = a[0], p.J = a[1], p.K = a[4], p.D = a[5], p.cus = (int)a[7];
  p.q.ld = p.k.ld = p.K, p.v.ld = p.o.ld = p.D;
  const CausalSplitPlan r = plan_attention_causal_split(p, a[2], (int)a[3]);
  std::printf("supported=%d rows16=%d forward=%d chunk=%ld nv=%ld tiles=%ld pieces=%ld first_cut=%ld slots=%ld rows=%d stats_offset=%ld workspace=%ld "
              "grid=%ld combine_rows=%ld combine_grid=%ld dp=%d items=%ld reason=%s\n",
              (int)r.supported, (int)r.rows16, (int)r.forward, r.pieces.chunk, r.pieces.nv, r.pieces.tiles, r.pieces_per_item, r.first_cut, r.slots, r.rows,
              r.stats_offset, r.workspace_bytes, r.partial.grid, r.combine_rows, r.combine_grid, r.base.dp, r.base.items, r.reason);
  if (r.supported && r.pieces_per_item <= 4096)
    for (long x = 0; x < r.pieces_per_item; ++x) {
      const CausalPiece c = causal_piece_decode(r.pieces, x);
      std::printf("piece %ld %d %d %ld %ld %ld\n", c.tile, c.piece, c.pieces, c.t0, c.t1, c.slot);
    }
  return 0;
}
