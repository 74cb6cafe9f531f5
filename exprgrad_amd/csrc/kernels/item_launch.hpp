// The item grid (item_grid.hpp) as the kernels and their launchers see it: the items of one launch as a kernel argument, a
// block's item of them, an operand's base for that item, and the one loop over the launches of a cut.
#pragma once

#include "../eg_internal.hpp"
#include "gemm_f32_mfma.hpp"   // xcd_remap
#include "item_grid.hpp"

namespace eg {

// The items of one launch: launches cut the flattened (o, i1) range, and every item has `tiles` blocks.
struct Items {
  unsigned batch1;                     // extent of the inner index
  unsigned first_outer, first_inner;   // the item the launch starts at
  int tiles;                           // blocks per item
};

// Block id -> (outer, inner, tile).  The items are folded into grid x (grid y and z stop at 65 535), and xcd_remap hands every
// XCD a contiguous range of the launch's blocks, so the tiles of one item meet in one L2.  All of it is block-uniform 32-bit
// arithmetic (first_inner < batch1 < 2^31 and at most 2^22 items per launch: the sum stays below 2^32); only an operand's
// offset (item_base) is 64-bit.
struct BlockItem {
  unsigned outer, inner;
  int tile;
};

// ONE_INDEX: the kernel also serves launches with one batch index (batch1 == 1), whose blocks skip the second divide behind a
// block-uniform branch.
template <bool ONE_INDEX = false>
__device__ __forceinline__ BlockItem block_item(const Items& it) {
  const int work = eg::gemm::xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int local = work / it.tiles;
  BlockItem b;
  b.tile = work - local * it.tiles;
  const unsigned inner = it.first_inner + (unsigned)local;
  if (ONE_INDEX && it.batch1 == 1) {
    b.outer = it.first_outer + inner;
    b.inner = 0;
    return b;
  }
  b.outer = it.first_outer + inner / it.batch1;
  b.inner = inner % it.batch1;
  return b;
}

template <class T>
__device__ __forceinline__ T* item_base(T* p, const View& v, unsigned outer, unsigned inner) {
  return p + (long)outer * v.stride0 + (long)inner * v.stride1;
}

// One launch after the other of a cut: launch(items of the launch, grid).  `name` is the entry the message speaks of.
template <class F>
int for_each_launch(const char* name, long items, const Cut& cut, long batch1, F&& launch) {
  for (long n = 0; n < cut.launches; ++n) {
    const Launch l = plan_launch(items, cut, n);
    EG_REQUIRE(l.items > 0 && l.grid > 0 && l.grid <= BATCHED_MAX_BLOCKS, EG_ERR_INVALID, "%s: launch out of range", name);
    const Items it = {(unsigned)batch1, (unsigned)(l.first / batch1), (unsigned)(l.first % batch1), (int)cut.tiles};
    const int rc = launch(it, (unsigned)l.grid);
    if (rc) return rc;
  }
  return EG_OK;
}

}  // namespace eg
