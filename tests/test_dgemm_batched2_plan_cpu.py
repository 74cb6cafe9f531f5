"""The float64 batched planner with two batch indices (csrc/kernels/gemm_plan.cpp: DgemmBatchedProblem::batch1 and the
inner strides, dgemm_batched_vec, plan_dgemm_batched) on the CPU, through a driver of its own
(tests/dgemm_batched2_plan_driver.cpp) built with the host compiler against gemm_plan.cpp alone.  What is checked is what
a wrong answer would break on the GPU: a 16-byte load of a misaligned item (the two-stride VEC rule), an item run twice or
not at all (the cut of batch0 * batch1 items, a launch that starts inside an outer row included), and a second planner
for what is one kernel (batch1 == 1 gives plan_dgemm_batched's figures of tests/dgemm_batched_plan_driver.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exprgrad_amd", "csrc")
MAX_BLOCKS = 1 << 22
TILE = 64


def build(tmp, name):
    exe = str(tmp / name)
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(CSRC, "kernels", "gemm_plan.cpp"),
                          os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dbatched2")
    return build(tmp, "dgemm_batched2_plan_driver"), build(tmp, "dgemm_batched_plan_driver")


def parse(stdout, n):
    result = []
    for line in stdout.splitlines():
        kind, *fields = line.split()
        row = {k: int(v) for k, v in (f.split("=", 1) for f in fields)}
        if kind == "plan":
            result.append((row, []))
        else:
            result[-1][1].append(row)
    assert len(result) == n
    return result


def plans(exe, cases):
    text = "".join(" ".join(str(int(v)) for v in c) + "\n" for c in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    return parse(out.stdout, len(cases))


def call(b0, b1, M, N, K, lda=None, ldb=None, sa=None, sb=None, a_aligned=1, b_aligned=1, cus=256):
    """sa / sb: (outer, inner) strides; None: nested items, one behind the other."""
    lda = K if lda is None else lda
    ldb = N if ldb is None else ldb
    sa = (b1 * M * lda, M * lda) if sa is None else sa
    sb = (b1 * K * ldb, K * ldb) if sb is None else sb
    return (b0, b1, M, N, K, lda, ldb, sa[0], sa[1], sb[0], sb[1], a_aligned, b_aligned, cus)


def test_vec_needs_both_strides_of_both_operands_even(drivers):
    even_a, even_b = (3 * 33 * 18, 33 * 18), (3 * 18 * 20, 18 * 20)
    assert all(s % 2 == 0 for s in even_a + even_b)
    cases = {
        "all even, aligned": (call(2, 3, 33, 20, 18), 1),
        "odd inner stride of A": (call(2, 3, 33, 20, 18, sa=(even_a[0], even_a[1] + 1)), 0),
        "odd inner stride of B": (call(2, 3, 33, 20, 18, sb=(even_b[0], even_b[1] + 1)), 0),
        "odd outer stride of A": (call(2, 3, 33, 20, 18, sa=(even_a[0] + 1, even_a[1])), 0),
        "odd outer stride of B": (call(2, 3, 33, 20, 18, sb=(even_b[0] + 1, even_b[1])), 0),
        "odd inner strides of an inner index of extent 1 are never applied": (call(3, 1, 33, 20, 18, sa=(33 * 18, 7), sb=(18 * 20, 9)), 1),
        "odd outer strides of an outer index of extent 1 are never applied": (call(1, 3, 33, 20, 18, sa=(7, 33 * 18), sb=(9, 18 * 20)), 1),
        "the outer index of extent 1 does not excuse the inner stride": (call(1, 3, 33, 20, 18, sa=(0, 33 * 18 + 1)), 0),
        "A shared by both indices (strides 0)": (call(2, 3, 33, 20, 18, sa=(0, 0)), 1),
        "B shared along the inner index": (call(2, 3, 33, 20, 18, sb=(18 * 20, 0)), 1),
        "B shared, but A's inner stride odd": (call(2, 3, 33, 20, 18, sa=(even_a[0], 595), sb=(0, 0)), 0),
        "head in the row: ld = H * K, inner stride K, K even": (call(2, 3, 33, 20, 16, lda=48, ldb=48, sa=(33 * 48, 16), sb=(20 * 48, 16)), 1),
        "head in the row, K odd": (call(2, 3, 33, 20, 17, lda=51, ldb=51, sa=(33 * 51, 17), sb=(20 * 51, 17)), 0),
        "A base not 16-byte aligned": (call(2, 3, 33, 20, 18, a_aligned=0), 0),
        "B base not 16-byte aligned": (call(2, 3, 33, 20, 18, b_aligned=0), 0),
        "odd lda": (call(2, 3, 33, 20, 17, lda=17, sa=(3 * 33 * 17 + 1, 33 * 17 + 1)), 0),
    }
    got = plans(drivers[0], [c for c, _ in cases.values()])
    for (name, (_, want)), (plan, _) in zip(cases.items(), got):
        assert plan["loop"] == 0 and plan["vec"] == want, (name, plan)


@pytest.mark.parametrize("b0,b1,M,N", [(1, 1, 1, 1), (2, 3, 33, 20), (2, 3, 130, 70), (3, 1398103, 1, 1), (2049, 2048, 1, 1), (1, MAX_BLOCKS + 3, 1, 1),
                                       (MAX_BLOCKS + 3, 1, 1, 1), (5, 299595, 65, 129), (7, 100000, 130, 70)])
def test_launches_cover_every_item_exactly_once(drivers, b0, b1, M, N):
    (plan, launches), = plans(drivers[0], [call(b0, b1, M, N, 8)])
    tiles = -(-M // TILE) * -(-N // TILE)
    items = b0 * b1
    ipl = max(1, MAX_BLOCKS // tiles)
    assert plan["loop"] == 0 and plan["max_blocks"] == MAX_BLOCKS and plan["tiles"] == tiles == plan["tiles_m"] * plan["tiles_n"]
    assert plan["items_per_launch"] == ipl and plan["launches"] == len(launches) == -(-items // ipl)
    nxt = 0
    for n, l in enumerate(launches):
        assert l["index"] == n and l["first"] == nxt and 1 <= l["items"] <= ipl
        assert l["grid"] == l["items"] * tiles and 0 < l["grid"] <= MAX_BLOCKS
        # the item the kernel counts from: o-major, and the 32-bit sum first_inner + (items of the launch) stays below 2^32
        assert l["first_outer"] * b1 + l["first_inner"] == l["first"] and 0 <= l["first_inner"] < b1 and l["first_outer"] < b0
        assert l["first_inner"] + l["items"] < 1 << 32
        nxt += l["items"]
    assert nxt == items
    assert all(l["items"] == ipl for l in launches[:-1])


def test_a_launch_starts_inside_an_outer_row(drivers):
    """3 x 1 398 103 items of one tile: 2^22 + 5 blocks.  The cut's second launch starts at item 2^22, inside outer row 2,
    which only a cut of the flattened range can do.  The (outer, inner) pair is the driver's own first / batch1 and
    first % batch1 — the launcher's arithmetic restated, not the launcher: what the kernel is really handed is checked on the
    GPU (tests/test_gpu_dgemm_batched2.py, the two cases of 2^22 + 5 items)."""
    b0, b1 = 3, 1398103
    assert b0 * b1 == MAX_BLOCKS + 5
    (plan, launches), = plans(drivers[0], [call(b0, b1, 1, 1, 1, sa=(0, 0), sb=(0, 0))])
    assert plan["launches"] == 2
    first, second = launches
    assert (first["first_outer"], first["first_inner"], first["items"]) == (0, 0, MAX_BLOCKS)
    assert second["first"] == MAX_BLOCKS and second["items"] == 5
    assert (second["first_outer"], second["first_inner"]) == (2, MAX_BLOCKS - 2 * b1) and 0 < second["first_inner"] <= b1 - 5


def test_batch1_of_one_is_the_planner_of_one_batch_index(drivers):
    """batch1 == 1 (its strides never applied): every figure of plan_dgemm_batched as the one-index driver prints it."""
    new, old = drivers
    rows = []
    for batch, M, N, K in [(5, 33, 20, 18), (7, 130, 70, 40), (8, 128, 64, 24), (MAX_BLOCKS + 3, 1, 1, 1), (3, 2048, 2048, 64)]:
        for lda_pad, sa_pad, a_al in ((0, 0, 1), (1, 0, 1), (0, 1, 1), (2, 2, 0)):
            lda, ldb = K + lda_pad, N
            rows.append((batch, M, N, K, lda, ldb, M * lda + sa_pad, K * ldb, a_al, 1, 256))
    two = plans(new, [(b, 1, M, N, K, lda, ldb, sa, 77, sb, 99, aa, ba, cus) for b, M, N, K, lda, ldb, sa, sb, aa, ba, cus in rows])
    text = "".join(" ".join(str(v) for v in r) + "\n" for r in rows)
    out = subprocess.run([old], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    one = parse(out.stdout, len(rows))
    seen = set()
    for r, (p2, l2), (p1, l1) in zip(rows, two, one):
        for k in ("loop", "vec", "tiles_m", "tiles_n", "tiles", "items_per_launch", "launches", "max_blocks", "dgemm_vec"):
            assert p2[k] == p1[k], (r, k, p2, p1)
        assert [(l["first"], l["items"], l["grid"]) for l in l2] == [(l["first"], l["items"], l["grid"]) for l in l1], r
        assert all(l["first_inner"] == 0 and l["first_outer"] == l["first"] for l in l2)
        seen.add((p2["loop"], p2["vec"], len(l2) > 1))
    assert seen >= {(0, 1, False), (0, 0, False), (0, 0, True), (1, 0, False)}


@pytest.mark.parametrize("cus", [64, 256])
def test_loop_rule_reads_the_item_alone(drivers, cus):
    for M, N in [(64, 64), (64 * cus, 64), (64 * cus - 64, 64), (2048, 2048)]:
        verdicts = {plans(drivers[0], [call(b0, b1, M, N, 8, cus=cus)])[0][0]["loop"] for b0, b1 in ((1, 1), (2, 3), (1000, 7))}
        assert verdicts == {int(-(-M // TILE) * -(-N // TILE) >= cus)}, (M, N, cus, verdicts)
