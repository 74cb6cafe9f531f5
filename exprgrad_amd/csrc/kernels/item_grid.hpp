// The item grid: many items of one shape, `tiles` blocks per item, cut into launches of at most BATCHED_MAX_BLOCKS blocks.
// The one description that the batched products, float32 and float64, over one batch index and over two (gemm_batched.hip;
// gemm_f64_mfma.hip, planned in gemm_plan.cpp) and the attention kernels (attention_plan.hpp) share.  Plain C++ (no HIP, no unit of its own): item_launch.hpp has the kernels' side and
// the launch loop.
#pragma once

#include <algorithm>

namespace eg {

// Blocks of one launch, float32 and float64: grid x block threads stays below 2^32 and the block id an int.
constexpr long BATCHED_MAX_BLOCKS = 1L << 22;

// One item's view of an operand, the one description from the model's plan to the kernels' arguments: elements per row step
// and per step of the outer and the inner batch index.  The attention row sums have no rows to step over: their ld is unused (0).
struct View {
  long ld = 0, stride0 = 0, stride1 = 0;
};
inline bool operator==(const View& a, const View& b) { return a.ld == b.ld && a.stride0 == b.stride0 && a.stride1 == b.stride1; }

// How the flattened (o, i1) range of items, o-major, is cut into launches of one kernel with `tiles` blocks per item.
struct Cut {
  long tiles = 0;             // blocks per item
  long grid = 0;              // blocks of all launches together: items * tiles
  long items_per_launch = 0;  // at least 1; BATCHED_MAX_BLOCKS / tiles otherwise
  long launches = 0;          // none for a kernel without tiles
};

inline Cut cut_items(long items, long tiles) {
  Cut c;
  c.tiles = tiles;
  c.grid = items * tiles;
  c.items_per_launch = std::max(1L, BATCHED_MAX_BLOCKS / std::max(1L, tiles));
  c.launches = tiles > 0 ? (items + c.items_per_launch - 1) / c.items_per_launch : 0;
  return c;
}

// Items [first, first + items) of that range as grid = items * tiles blocks.
struct Launch {
  long first = 0, items = 0, grid = 0;
};

// Launch `index` of a cut of `items` items, index in [0, cut.launches).
inline Launch plan_launch(long items, const Cut& cut, long index) {
  Launch l;
  l.first = index * cut.items_per_launch;
  l.items = std::min(cut.items_per_launch, items - l.first);
  l.grid = l.items * cut.tiles;
  return l;
}

}  // namespace eg
