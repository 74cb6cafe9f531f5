"""The batched float64 product's planner (csrc/kernels/gemm_plan.cpp: plan_dgemm_batched, dgemm_batched_launch,
dgemm_batched_vec, dgemm_batched_runs_as_loop) on the CPU: a small driver (tests/dgemm_batched_plan_driver.cpp) is built
with the host compiler against gemm_plan.cpp alone and fed one call per line.  What is checked is what a wrong answer
would break on the GPU: a 16-byte load of a misaligned address (the VEC decision), an item run twice or not at all (the
split of a long batch over launches), a block id mapped outside the launch (the remap condition), and bits that depend on
the batch (the loop rule)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exprgrad_amd", "csrc")
MAX_BLOCKS = 1 << 22      # blocks of one launch, the float32 batched launch's limit (kernels/gemm_batched.hip)
TILE = 64


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dbatched") / "dgemm_batched_plan_driver")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(CSRC, "kernels", "gemm_plan.cpp"),
                          os.path.join(ROOT, "tests", "dgemm_batched_plan_driver.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def plans(exe, cases, mode=()):
    """cases: (batch, M, N, K, lda, ldb, stride_a, stride_b, a_aligned, b_aligned, cus) -> [(plan, [launch, ...]), ...]
    mode ("cut",): cases (items, tiles_m, tiles_n) -> [(cut, [launch, ...]), ...]"""
    text = "".join(" ".join(str(int(v)) for v in c) + "\n" for c in cases)
    out = subprocess.run([exe, *mode], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    result = []
    for line in out.stdout.splitlines():
        kind, *fields = line.split()
        row = {k: int(v) for k, v in (f.split("=", 1) for f in fields)}
        if kind in ("plan", "cut"):
            result.append((row, []))
        else:
            result[-1][1].append(row)
    assert len(result) == len(cases)
    return result


def call(batch, M, N, K, lda=None, ldb=None, stride_a=None, stride_b=None, a_aligned=1, b_aligned=1, cus=256):
    lda = K if lda is None else lda
    ldb = N if ldb is None else ldb
    return (batch, M, N, K, lda, ldb, M * lda if stride_a is None else stride_a, K * ldb if stride_b is None else stride_b, a_aligned, b_aligned, cus)


def test_vec_needs_even_rows_even_strides_and_aligned_bases(driver):
    cases = {
        "all even, aligned": (call(5, 33, 20, 18, lda=18, ldb=20), 1),
        "odd lda": (call(5, 33, 20, 17, lda=17, ldb=20, stride_a=33 * 17 + 1), 0),
        "odd ldb": (call(5, 33, 20, 18, lda=18, ldb=21, stride_b=18 * 21), 0),
        "odd stride_a: items 1, 3 are misaligned": (call(5, 33, 20, 18, lda=18, ldb=20, stride_a=33 * 18 + 1), 0),
        "odd stride_b": (call(5, 33, 20, 18, lda=18, ldb=20, stride_b=18 * 20 + 3), 0),
        "odd stride of a batch of one is never used": (call(1, 33, 20, 18, lda=18, ldb=20, stride_a=33 * 18 + 1, stride_b=7), 1),
        "shared A (stride 0)": (call(5, 33, 20, 18, lda=18, ldb=20, stride_a=0), 1),
        "shared B, odd stride_a": (call(5, 33, 20, 18, lda=18, ldb=20, stride_a=595, stride_b=0), 0),
        "A base not aligned": (call(5, 33, 20, 18, lda=18, ldb=20, a_aligned=0), 0),
        "B base not aligned": (call(5, 33, 20, 18, lda=18, ldb=20, b_aligned=0), 0),
        "padded, all even": (call(7, 130, 70, 40, lda=42, ldb=72, stride_a=130 * 42 + 2, stride_b=40 * 72 + 2), 1),
    }
    got = plans(driver, [c for c, _ in cases.values()])
    for (name, (_, want)), (plan, _) in zip(cases.items(), got):
        assert plan["loop"] == 0 and plan["vec"] == want, (name, plan)


@pytest.mark.parametrize("batch,M,N", [(1, 1, 1), (9, 16, 16), (7, 130, 70), (8, 128, 64), (MAX_BLOCKS + 3, 1, 1), (2 * MAX_BLOCKS, 64, 64),
                                       (MAX_BLOCKS // 6 + 1, 130, 70), (MAX_BLOCKS // 3, 65, 129), (3 * (MAX_BLOCKS // 7) + 5, 448, 1)])
def test_launches_cover_every_item_exactly_once(driver, batch, M, N):
    (plan, launches), = plans(driver, [call(batch, M, N, 8)])
    tiles = -(-M // TILE) * -(-N // TILE)
    assert plan["loop"] == 0 and plan["max_blocks"] == MAX_BLOCKS
    assert plan["tiles_m"] * plan["tiles_n"] == tiles == plan["tiles"]
    assert plan["items_per_launch"] == max(1, MAX_BLOCKS // tiles) and plan["launches"] == len(launches) >= 1
    nxt = 0
    for i, l in enumerate(launches):
        assert l["index"] == i and l["first"] == nxt and l["items"] >= 1
        assert l["grid"] == l["items"] * tiles and 0 < l["grid"] <= MAX_BLOCKS
        # the kernel's remap (work = (id & 7) * (grid >> 3) + (id >> 3)) is a permutation of [0, grid) only for a multiple of 8
        assert l["remap"] == int(l["grid"] % 8 == 0 and l["grid"] >= 16), l
        nxt += l["items"]
    assert nxt == batch
    if batch > plan["items_per_launch"]:
        assert len(launches) > 1 and all(l["items"] == plan["items_per_launch"] for l in launches[:-1])


def test_remap_condition(driver):
    cases = [(7, 130, 70), (8, 128, 64), (1, 64, 64), (8, 64, 64), (16, 64, 64), (3, 128, 128), (4, 128, 128), (5, 33, 20), (24, 1, 1), (2, 256, 256)]
    got = plans(driver, [call(b, M, N, 24) for b, M, N in cases])
    want = {(7, 130, 70): 0, (8, 128, 64): 1, (1, 64, 64): 0, (8, 64, 64): 0, (16, 64, 64): 1, (3, 128, 128): 0, (4, 128, 128): 1, (5, 33, 20): 0,
            (24, 1, 1): 1, (2, 256, 256): 1}
    for c, (plan, launches) in zip(cases, got):
        assert len(launches) == 1 and launches[0]["remap"] == want[c], (c, launches)


def remap(block, grid):
    return (block & 7) * (grid >> 3) + (block >> 3)


@pytest.mark.parametrize("grid", [16, 24, 48, 4096])
def test_remap_is_a_permutation_with_contiguous_ranges(grid):
    """The kernel's block id -> work id map, restated: blocks that share an XCD (equal id mod 8) get one contiguous range."""
    work = [remap(b, grid) for b in range(grid)]
    assert sorted(work) == list(range(grid))
    for x in range(8):
        mine = sorted(remap(b, grid) for b in range(x, grid, 8))
        assert mine == list(range(x * grid // 8, (x + 1) * grid // 8))


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_loop_rule_reads_the_item_alone(driver, cus):
    shapes = [(1, 1), (64, 64), (130, 70), (512, 512), (1024, 1024), (960, 1024), (1088, 1024), (2048, 2048), (64 * cus, 64), (64 * cus - 64, 64),
              (64 * cus - 63, 64), (4096, 4096)]
    rows = []
    for M, N in shapes:
        for batch in (1, 1000):
            for K in (1, 64, 4096):
                rows.append(((M, N), call(batch, M, N, K, cus=cus)))
    got = plans(driver, [c for _, c in rows])
    verdict = {}
    for (shape, c), (plan, _) in zip(rows, got):
        verdict.setdefault(shape, set()).add(plan["loop"])
    assert all(len(v) == 1 for v in verdict.values()), verdict
    # the shipped rule: at least one 64 x 64 tile per compute unit
    for (M, N), v in verdict.items():
        assert v == {int(-(-M // TILE) * -(-N // TILE) >= cus)}, (M, N, cus, v)
    assert verdict[(64 * cus, 64)] == {1} and verdict[(64 * cus - 64, 64)] == {0} and verdict[(64 * cus - 63, 64)] == {1}


def test_a_looping_plan_has_no_launches(driver):
    (plan, launches), = plans(driver, [call(8, 2048, 2048, 256)])
    assert plan["loop"] == 1 and plan["launches"] == 0 and launches == []


def test_a_looping_plan_reports_the_workspace_of_its_items(driver):
    """An item with a tile per CU runs as eg_dgemm, and eg_dgemm's model slices many such items (the other block slots of
    a CU are free and K is long): the loop then writes slabs.  The plan carries the plain plan of an item, so a caller can
    see it; the one-launch side never takes workspace."""
    cases = [call(3, 64, 4096, 4096, cus=64), call(3, 512, 512, 65536, cus=64), call(3, 4096, 4096, 4096, cus=256),
             call(1000, 130, 70, 4096, cus=64), call(8, 64, 2048, 65536, cus=256)]
    sliced, sliced_long, unsliced, launch, launch_long = plans(driver, cases)
    assert sliced[0]["loop"] == 1 and (sliced[0]["item_config"], sliced[0]["item_splits"]) == (2, 2)
    assert sliced[0]["item_workspace_doubles"] == 2 * 64 * 4096 > 0
    assert sliced_long[0]["loop"] == 1 and (sliced_long[0]["item_config"], sliced_long[0]["item_splits"]) == (0, 8)
    assert sliced_long[0]["item_workspace_doubles"] == 8 * 512 * 512
    assert unsliced[0]["loop"] == 1 and unsliced[0]["item_splits"] == 1 and unsliced[0]["item_workspace_doubles"] == 0
    for plan, launches in (launch, launch_long):
        assert plan["loop"] == 0 and plan["launches"] == len(launches) == 1 and plan["item_workspace_doubles"] == 0


def test_vec_of_a_batch_of_one_is_the_plain_rule(driver):
    """dgemm_batched_vec is dgemm_vec plus the parity of the strides, which a batch of one never uses."""
    cases = [call(batch, 33, 20, 18, lda=lda, ldb=ldb, stride_a=33 * lda + sa, stride_b=18 * ldb + sb, a_aligned=a, b_aligned=b)
             for batch in (1, 2) for lda in (18, 19) for ldb in (20, 21) for a in (0, 1) for b in (0, 1) for sa in (0, 1) for sb in (0, 1)]
    seen = set()
    for c, (plan, _) in zip(cases, plans(driver, cases)):
        batch, lda, ldb, stride_a, stride_b, a, b = c[0], c[4], c[5], c[6], c[7], c[8], c[9]
        assert plan["loop"] == 0 and plan["dgemm_vec"] == int(lda % 2 == 0 and ldb % 2 == 0 and a and b), c
        if batch == 1:
            assert plan["vec"] == plan["dgemm_vec"], c
        else:
            assert plan["vec"] == int(plan["dgemm_vec"] and stride_a % 2 == 0 and stride_b % 2 == 0), c
        seen.add((batch, plan["vec"], plan["dgemm_vec"]))
    assert seen == {(1, 0, 0), (1, 1, 1), (2, 0, 0), (2, 1, 1), (2, 0, 1)}


def cut_table():
    """(items, tiles_m, tiles_n): for tiles of 1, of a few, of a non-divisor of 2^22, of half a launch, of exactly one launch
    (2^22) and of more than one, `items` of 1 and one below, at and above a multiple of items_per_launch = max(1, 2^22 // tiles)."""
    t = []
    for tm, tn in [(1, 1), (3, 2), (7, 1), (2048, 1024), (2048, 2048), (2049, 2048), (4096, 4096)]:
        ipl = max(1, MAX_BLOCKS // (tm * tn))
        for items in sorted({1, ipl - 1, ipl, ipl + 1, 3 * ipl - 1, 3 * ipl, 3 * ipl + 1} - {0}):
            t.append((items, tm, tn))
    return t


def test_the_item_grids_cut_covers_every_item_once_and_is_the_float64_planners(driver):
    """cut_items / plan_launch (kernels/item_grid.hpp), which the float32 batched products, the attention kernels and — through
    plan_dgemm_batched / dgemm_batched_launch — the float64 batched product all cut their launches with: every item in exactly
    one launch, every grid within BATCHED_MAX_BLOCKS, and the float64 planner's figures equal to the cut's.  An item of more
    than 2^22 tiles fits no launch: the cut still hands out every item once, one per launch, with grid == tiles, which is what
    every launcher refuses ("launch out of range"), and every planner turns such an item away before it cuts (the float64
    planner loops: d_loop); there dgemm_batched_launch is compared on a plan that holds the cut's figures."""
    table = cut_table()
    assert {tm * tn for _, tm, tn in table} >= {1, MAX_BLOCKS} and any(tm * tn > MAX_BLOCKS for _, tm, tn in table)
    for (items, tm, tn), (cut, launches) in zip(table, plans(driver, table, mode=("cut",))):
        tiles = tm * tn
        ipl = max(1, MAX_BLOCKS // tiles)
        want_launches = -(-items // ipl)
        fits = tiles <= MAX_BLOCKS
        assert cut["max_blocks"] == MAX_BLOCKS and cut["tiles"] == tiles, (items, tiles, cut)
        assert cut["items_per_launch"] == ipl and cut["launches"] == want_launches == len(launches), (items, tiles, cut)
        assert cut["d_loop"] == int(not fits), (items, tiles, cut)
        if fits:
            assert (cut["d_tiles"], cut["d_items_per_launch"], cut["d_launches"]) == (tiles, ipl, want_launches), (items, tiles, cut)
        else:
            assert cut["d_launches"] == 0 and ipl == 1, (items, tiles, cut)
        nxt = 0
        for i, l in enumerate(launches):
            assert l["index"] == i and l["first"] == nxt and 1 <= l["items"] <= ipl, (items, tiles, l)
            assert l["grid"] == l["items"] * tiles and l["grid"] > 0, (items, tiles, l)
            assert (l["grid"] <= MAX_BLOCKS) == fits, (items, tiles, l)
            assert (l["d_first"], l["d_items"], l["d_grid"]) == (l["first"], l["items"], l["grid"]), (items, tiles, l)
            nxt += l["items"]
        assert nxt == items, (items, tiles)
        assert all(l["items"] == ipl for l in launches[:-1]), (items, tiles)
