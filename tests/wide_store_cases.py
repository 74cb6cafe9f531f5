"""Products whose tiles leave through LDS as whole rows by default and lane by lane under EG_GEMM_NO_WIDE_STORE=1
(gemm_f32_mfma.hpp, gemm_block_at: the wide-store pass / the per-lane store), shared by tests/test_gpu_ops.py (the two stores agree to the bit)
and tests/test_gemm_plan_cpu.py (the two runs differ in `wide_store` and in nothing else, so it IS the same kernel).

(M, N, K, layout, forced tile or None, what the plan must say for 256 CUs)."""

# both runs: the four-wave tile kernels, one block per tile
SWITCHES = {"EG_GEMM_NO_PAIR": "1", "EG_GEMM_NO_T96": "1", "EG_GEMM_NO_STREAMK": "1"}

CASES = [
    (192, 192, 256, "nn", None, dict(bm=64, bn=64, kb=32)),                      # whole tiles
    (200, 196, 260, "nn", None, dict(bm=64, bn=64, edge=1)),                     # ragged in M, N, K: whole tiles wide, edge tiles direct
    (2048, 2048, 128, "nn", None, dict(bm=64, bn=64, kb=16)),
    (256, 256, 8192, "tn", None, dict(bm=64, bn=64, splits=16, second="split_reduce")),   # wide store into the slabs
    (300, 260, 4096, "tn", None, dict(bm=64, bn=64, splits=10, edge=1)),
    (256, 128, 256, "nn", (128, 32), dict()),
    (384, 192, 512, "tn", (128, 64), dict(splits=4)),
    (512, 128, 256, "tt", (256, 64), dict()),
    (256, 256, 256, "nn", (128, 128), dict()),
    (256, 512, 256, "tn", (256, 256), dict()),                                   # both operands interleaved
    (260, 512, 256, "tn", (256, 256), dict(edge=1)),                             # a ragged tile row
    (784, 512, 16384, "tn", None, dict(route="extra_rows", x_rows=16, splits=40)),
]


def case_id(case):
    M, N, K, layout, tile, _ = case
    return "%dx%dx%d-%s%s" % (M, N, K, layout, "-%dx%d" % tile if tile else "")
