// The library's environment switches: ONE closed list (EG_SWITCHES below), read through here and nowhere else.
//
// Every name the library honours is a row of the list with an id, a class, a kind and a one-line purpose; enum class Sw
// and the table that eg_switch_table prints are generated from it, so a name outside the list does not compile.
// DESIGN.md section 4 is generated from the table and tests/test_cabi.py holds the sources to it (a getenv() outside
// switches.cpp and rtc.cpp's HOME / XDG_CACHE_HOME, a row nobody reads, or a static that caches a switch, is a red test).
//
// Reads are live.  The environment is read into an immutable snapshot at first use and again by eg_switches_reload()
// (what a test that flips a switch between two runs calls; tests/conftest.py wraps monkeypatch.setenv / delenv with it);
// an accessor is one atomic load and one array index, without a lock, and nobody keeps a copy: what is read while a plan
// is made (lowering, planning, the kernel generators) holds for that plan, what is read at launch is read on every call.
// Three rows are fixed at first use because they configure something that is opened once: EG_HIPRTC_LIB, EG_KERNEL_CACHE
// and EG_NO_KERNEL_CACHE (rtc.cpp) - the only statics initialised from here.
//
// ONE truth rule: a row of kind `flag` is on when it is set, not empty, and does not begin with '0' (NAME=0 and NAME=
// are off).  Rows of class "tuning" (measurement aids: forced tiles, forced slice counts, thresholds) are honoured only
// under EG_TUNING=1, so a stray variable in a production environment cannot change a launch.
//
// A superseded snapshot is retired, never freed (reload is a test facility, a snapshot a few KB): a pointer that text()
// returned stays valid, with the value it had, for the life of the process.
#pragma once
#include <atomic>
#include <cassert>
#include <cstdlib>

// X(id, environment name, class, kind, purpose).  class: execution | data-parallel | compiler | detector | tuning -
// execution: turn ONE optimisation off (bisecting a wrong result, measuring what it buys; tools/stress_suite.sh runs the
// GPU suite under rotations of them).  detector: dumps, traces, poison.  tuning: honoured under EG_TUNING=1 only.
#define EG_SWITCHES(X)                                                                                                                              \
  X(TUNING, "EG_TUNING", "execution", flag, "honour the rows of class `tuning` (measurement aids); unset: they are ignored")                       \
  X(NO_GRAPH, "EG_NO_GRAPH", "execution", flag, "launch one by one instead of replaying captured HIP graphs")                                      \
  X(NO_DPP_BUTTERFLY, "EG_NO_DPP_BUTTERFLY", "execution", flag, "row groups exchange lanes through the LDS crossbar in every step of a wave reduction (no DPP moves)") \
  X(NO_DEFERRED_FOLD, "EG_NO_DEFERRED_FOLD", "execution", flag, "a row group in front of a side-lane group folds its partial rows itself, not on the side lane") \
  X(NO_OVERLAP, "EG_NO_OVERLAP", "execution", flag, "no side lane: bandwidth-bound launches run in front of the long contraction, not next to it") \
  X(NO_ROWFUSE, "EG_NO_ROWFUSE", "execution", flag, "no row / sample / map / small fusion groups: one launch per kernel")                          \
  X(NO_EPILOGUE, "EG_NO_EPILOGUE", "execution", flag, "elementwise consumers of a contraction stay their own launches")                            \
  X(NO_INLINE, "EG_NO_INLINE", "execution", flag, "no producer / consumer inlining of elementwise kernels into generated kernels")                 \
  X(NO_ALIAS, "EG_NO_ALIAS", "execution", flag, "whole-tensor raw copies (reshape) are copied instead of sharing storage")                         \
  X(NO_ONES_ROW, "EG_NO_ONES_ROW", "execution", flag, "bias gradient as its own column sum instead of the weight gradient's virtual row of ones")  \
  X(NO_SMALL_GEMM, "EG_NO_SMALL_GEMM", "execution", flag, "tiny contractions on the matrix tiles instead of one wave per output element")          \
  X(NO_NARROW_INDEX, "EG_NO_NARROW_INDEX", "execution", flag, "64-bit index arithmetic everywhere in generated kernels")                           \
  X(NO_PREDICATE, "EG_NO_PREDICATE", "execution", flag, "pre-activations stored as values, not as predicate bits")                                 \
  X(NO_ROW_PRODUCT, "EG_NO_ROW_PRODUCT", "execution", flag, "the 10-wide forward product as its own launch, not in the previous layer's epilogue") \
  X(NO_ROW_DIRECT, "EG_NO_ROW_DIRECT", "execution", flag, "a one-block row group writes a partial row for row_finalize instead of its totals")     \
  X(NO_BATCHED_GEMM, "EG_NO_BATCHED_GEMM", "execution", flag, "products with a leading batch index as generated kernels instead of eg_bgemm launches / collapsed products") \
  X(NO_SMALL_PAIR, "EG_NO_SMALL_PAIR", "execution", flag, "two independent tiny contractions as two launches")                                     \
  X(NO_SKINNY_GEMM, "EG_NO_SKINNY_GEMM", "execution", flag, "N <= 16 products on the matrix tiles instead of the streaming skinny kernel")         \
  X(NO_NARROW_K, "EG_NO_NARROW_K", "execution", flag, "K <= 16 products with a generated epilogue on the matrix tile instead of the streaming kernel") \
  X(NO_SAMPLE_FUSE, "EG_NO_SAMPLE_FUSE", "execution", flag, "no sample groups (one block per sample): the launch chain of a small-batch step")     \
  X(OVERLAP_SIDE_FIRST, "EG_OVERLAP_SIDE_FIRST", "execution", flag, "the side lane's launches are issued in front of the long contraction they run beside (the order of rounds 2 - 5)") \
  X(SAMPLE_KEEP_BARRIERS, "EG_SAMPLE_KEEP_BARRIERS", "execution", flag, "sample kernels keep the barrier between independent members")             \
  X(SAMPLE_NO_STAGE, "EG_SAMPLE_NO_STAGE", "execution", flag, "a sample group's members read parameters from global memory, not from a copy in LDS") \
  X(SAMPLE_NO_MFMA, "EG_SAMPLE_NO_MFMA", "execution", flag, "convolution members of a sample group as scalar loop nests, not on the matrix cores") \
  X(NO_SLAB_FOLD, "EG_NO_SLAB_FOLD", "execution", flag, "the optimizer's map group does not add up the sample kernel's slab rows itself")          \
  X(NO_SLAB_SUM, "EG_NO_SLAB_SUM", "execution", flag, "k-slices folded by the two-launch column sum instead of slab_sum")                          \
  X(NO_ROW_TAIL, "EG_NO_ROW_TAIL", "execution", flag, "a row group's last block neither folds the partial rows nor runs the update")               \
  X(PIPELINE, "EG_PIPELINE", "execution", flag, "the batch pipeline (two half batches, streaming launches under the other half's contraction): OFF unless 1") \
  X(NO_SPLIT_GEMM, "EG_NO_SPLIT_GEMM", "execution", flag, "eg_sgemm runs every product on the exact f32 matrix path, never as three-way split bf16") \
  X(SPLIT_PASS_SCALAR, "EG_SPLIT_PASS_SCALAR", "execution", flag, "the split pass reads an operand whose k runs along ld as 4-byte loads per lane (units), not as 16-byte tiles through LDS") \
  X(GEMM_NO_SKEW, "EG_GEMM_NO_SKEW", "execution", flag, "every wave of a contraction block runs the k loop in phase (the round-3 loop)")           \
  X(GEMM_NO_BK32, "EG_GEMM_NO_BK32", "execution", flag, "16-deep k-tiles for long whole-tile products")                                            \
  X(GEMM_NO_PAIR, "EG_GEMM_NO_PAIR", "execution", flag, "no wave-pair / eight-wave small-tile kernels")                                            \
  X(GEMM_NO_T96, "EG_GEMM_NO_T96", "execution", flag, "no 96 x 96 whole-round tiles")                                                              \
  X(GEMM_NO_STREAMK, "EG_GEMM_NO_STREAMK", "execution", flag, "64 x 64 tiles one block per tile, not persistent stream-K blocks")                  \
  X(GEMM_NO_XROW, "EG_GEMM_NO_XROW", "execution", flag, "1 .. 32 rows beyond whole tiles as a ragged tile row, not a ninth accumulator block")     \
  X(GEMM_NO_WIDE_STORE, "EG_GEMM_NO_WIDE_STORE", "execution", flag, "tiles leave as 128-byte pieces instead of through LDS as whole rows")         \
  X(CONV_NO_TINY, "EG_CONV_NO_TINY", "execution", flag, "small convolutions on the contraction route")                                             \
  X(CONV_NO_GRADF_HALO, "EG_CONV_NO_GRADF_HALO", "execution", flag, "filter gradient as one gathered contraction")                                 \
  X(CONV_NO_WIDE_STORE, "EG_CONV_NO_WIDE_STORE", "execution", flag, "halo convolution stores 128-byte pieces")                                     \
  X(CONV_NO_VIRTUAL_PAD, "EG_CONV_NO_VIRTUAL_PAD", "execution", flag, "image gradient reads a padded copy of the output gradient")                 \
  X(CONV_NO_HALO, "EG_CONV_NO_HALO", "execution", flag, "3 x 3-class convolutions on the implicit-GEMM route")                                     \
  X(CONV_NO_DIRECT, "EG_CONV_NO_DIRECT", "execution", flag, "few-channel convolutions on the implicit-GEMM route")                                 \
  X(CONV_NO_BAND, "EG_CONV_NO_BAND", "execution", flag, "small-channel convolutions on the routes the band kernels replaced")                      \
  X(CONV_NO_MFMA64, "EG_CONV_NO_MFMA64", "execution", flag, "float64 convolutions that the band and direct kernels decline: generated kernels in a model, refused by the eg_conv2_nhwc*_f64 entry points") \
  X(NO_STAGED_COPY, "EG_NO_STAGED_COPY", "execution", flag, "downloads into pageable memory as one runtime copy")                                  \
  X(FIT_NO_DIRECT, "EG_FIT_NO_DIRECT", "execution", flag, "fit copies every batch into the inputs' staging buffers")                               \
  X(DP_REAGREE_STEPS, "EG_DP_REAGREE_STEPS", "data-parallel", integer, "steps between two negotiations of the exchange schedule (default 256; 0: only the first)") \
  X(DP_INIT_TIMEOUT_S, "EG_DP_INIT_TIMEOUT_S", "data-parallel", real, "watchdog on ncclCommInitRank, seconds (default 180)")                       \
  X(DP_RESERVE_CUS, "EG_DP_RESERVE_CUS", "data-parallel", integer, "compute units the tail range leaves to RCCL's kernel (default 8)")             \
  X(DP_TEST_AS_MULTI, "EG_DP_TEST_AS_MULTI", "data-parallel", flag, "a one-rank group takes the N > 1 code paths (one-GPU boxes)")                 \
  X(DP_NO_SPLIT, "EG_DP_NO_SPLIT", "data-parallel", flag, "groups start with the early / late split of the bucket forbidden (eg_dp_set_split)")    \
  X(HIPRTC_LIB, "EG_HIPRTC_LIB", "compiler", text, "path of the libhiprtc the library opens (fixed at first use)")                                 \
  X(KERNEL_CACHE, "EG_KERNEL_CACHE", "compiler", text, "directory of the on-disk code-object cache (fixed at first use)")                          \
  X(NO_KERNEL_CACHE, "EG_NO_KERNEL_CACHE", "compiler", flag, "no on-disk code-object cache (fixed at first use)")                                  \
  X(POISON, "EG_POISON", "detector", flag, "NaN patterns in every scratch block and every slot that is overwritten, before each run")              \
  X(NO_PLAN_CHECK, "EG_NO_PLAN_CHECK", "detector", flag, "skip the plan invariants (host/plan_check.cpp)")                                         \
  X(DEBUG_GRAPH, "EG_DEBUG_GRAPH", "detector", flag, "print graph captures, replays and refusals")                                                 \
  X(DEBUG_OVERLAP, "EG_DEBUG_OVERLAP", "detector", flag, "print the side-lane groups of a plan")                                                   \
  X(DEBUG_TILE, "EG_DEBUG_TILE", "detector", flag, "print the tile model's estimate per candidate")                                                \
  X(DEBUG_SAMPLE, "EG_DEBUG_SAMPLE", "detector", flag, "print why a sample group did or did not form")                                             \
  X(DUMP_FUSED, "EG_DUMP_FUSED", "detector", text, "directory: generated translation units of fused contractions")                                 \
  X(DUMP_CODE, "EG_DUMP_CODE", "detector", text, "directory: hiprtc code objects and the text they were built from")                               \
  X(DUMP_BAND, "EG_DUMP_BAND", "detector", text, "directory: generated band-convolution sources")                                                  \
  X(GRADF_TRACE, "EG_GRADF_TRACE", "detector", flag, "per-wave cycle stamps of the halo filter-gradient kernel")                                   \
  X(HALO_TRACE, "EG_HALO_TRACE", "detector", flag, "per-wave cycle stamps of the halo convolution kernel")                                         \
  X(GEMM_TRACE, "EG_GEMM_TRACE", "detector", flag, "per-wave cycle stamps of the fused and the extra-row contraction kernels (k loop begins / ends, epilogue done)") \
  X(ROW_TRACE, "EG_ROW_TRACE", "detector", flag, "the last block of a row group with a tail prints cycle stamps of its hand-off")                  \
  X(SAMPLE_TRACE, "EG_SAMPLE_TRACE", "detector", integer, "block 0 of a sample kernel prints cycle stamps behind every member's barrier")          \
  X(GEMM_FORCE_TILE, "EG_GEMM_FORCE_TILE", "tuning", text, "bm,bn: force the contraction tile")                                                    \
  X(GEMM_FORCE_SPLITS, "EG_GEMM_FORCE_SPLITS", "tuning", integer, "n: force the k-slice count")                                                    \
  X(GEMM_OLD_TILE_MODEL, "EG_GEMM_OLD_TILE_MODEL", "tuning", flag, "round-1 cost model for wide outputs")                                          \
  X(STREAMK_BLOCKS_PER_CU, "EG_STREAMK_BLOCKS_PER_CU", "tuning", integer, "persistent blocks per CU of a stream-K launch")                         \
  X(STREAMK_MIN_RATIO, "EG_STREAMK_MIN_RATIO", "tuning", real, "microseconds the balance model must promise before a 64 x 64 launch goes stream-K (default 24)") \
  X(GEMM_SMALL_BK32, "EG_GEMM_SMALL_BK32", "tuning", flag, "32-deep k-tiles for every 64 x 64 launch")                                             \
  X(DGEMM_TILE, "EG_DGEMM_TILE", "tuning", text, "config[,splits]: force the float64 tile")                                                        \
  X(DGEMM_BATCHED_ROUTE, "EG_DGEMM_BATCHED_ROUTE", "tuning", text, "launch | loop: force eg_dgemm_batched onto the one-launch kernel or the loop of plain products") \
  X(CONV_BAND_PIXELS, "EG_CONV_BAND_PIXELS", "tuning", integer, "pixels per band of the band convolutions")                                        \
  X(CONV_DIRECT_BLOCKS, "EG_CONV_DIRECT_BLOCKS", "tuning", integer, "block cap of the direct filter gradient")                                     \
  X(ROW_TAIL_BLOCKS, "EG_ROW_TAIL_BLOCKS", "tuning", integer, "blocks of a row group that carries a tail (default: 12 KB of rows per block, at least 64)") \
  X(SAMPLE_STOP, "EG_SAMPLE_STOP", "tuning", integer, "k: a sample kernel ends behind member k (wrong numbers: the time of its first k + 1 members)") \
  X(SAMPLE_FUSE_MAX_BATCH, "EG_SAMPLE_FUSE_MAX_BATCH", "tuning", integer, "largest batch that forms a sample group (default 1280)")                \
  X(EPILOGUE_MIN_ELEMS, "EG_EPILOGUE_MIN_ELEMS", "tuning", integer, "smallest output that gets a generated epilogue (default 2^20; tests: 0)")     \
  X(PIPELINE_MIN_FLOPS, "EG_PIPELINE_MIN_FLOPS", "tuning", real, "smallest contraction the batch pipeline cuts")                                   \
  X(FIT_GROUP, "EG_FIT_GROUP", "tuning", integer, "batches per captured graph launch in fit (1: every batch its own launch)")                      \
  X(FIT_PIECE_BYTES, "EG_FIT_PIECE_BYTES", "tuning", integer, "upload piece of fit")                                                               \
  X(FIT_SEGMENT_BYTES, "EG_FIT_SEGMENT_BYTES", "tuning", integer, "device-resident segment of fit")

namespace eg {

#define EG_SW_ID(id, name, cls, kind, purpose) id,
enum class Sw : int { EG_SWITCHES(EG_SW_ID) kCount };
#undef EG_SW_ID

namespace sw {

enum class Kind : unsigned char { flag, integer, real, text };
#define EG_SW_KIND(id, name, cls, kind, purpose) Kind::kind,
constexpr Kind kKinds[] = {EG_SWITCHES(EG_SW_KIND)};
#undef EG_SW_KIND

// What one (re)load of the environment saw.  value[i]: nullptr when the row is unset, or a tuning row without EG_TUNING=1.
struct Snapshot {
  const char* value[(int)Sw::kCount];
  unsigned generation;
};
extern std::atomic<const Snapshot*> g_snapshot;
const Snapshot* first_load();
inline const Snapshot* snapshot() {
  const Snapshot* s = g_snapshot.load(std::memory_order_acquire);
  return s ? s : first_load();
}
inline const char* value(Sw s, Kind k) {
  assert(kKinds[(int)s] == k || (k == Kind::text && kKinds[(int)s] != Kind::flag));
  return snapshot()->value[(int)s];
}

// kind flag: set, not empty, no leading '0'
inline bool on(Sw s) {
  const char* e = value(s, Kind::flag);
  return e && e[0] && e[0] != '0';
}
// the other kinds: the value (nullptr: unset), valid for the life of the process
inline const char* text(Sw s) { return value(s, Kind::text); }
inline bool is_set(Sw s) { return text(s) != nullptr; }
inline long integer(Sw s, long dflt) {
  const char* e = value(s, Kind::integer);
  return e ? atol(e) : dflt;
}
inline double real(Sw s, double dflt) {
  const char* e = value(s, Kind::real);
  return e ? atof(e) : dflt;
}
void reload();
// Bumped by every (re)load of the environment: code that keeps values derived from switches reads them again when it changes.
inline unsigned generation() { return snapshot()->generation; }

}  // namespace sw
}  // namespace eg
