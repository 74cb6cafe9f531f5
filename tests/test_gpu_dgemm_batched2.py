"""GPU parity of eg_dgemm_batched2 (kernels/gemm_f64_mfma.hip, dgemm_batched_kernel on the item grid) against the oracle.

Every item (o, i) is compared with refcpu.dgemm64 on that item's operands within the project's own bound for eg_dgemm
(tests/test_gpu_f64.py, tests/test_gpu_dgemm_batched.py): |got - want| <= 4e-16 * sqrt(K) * (|opA| @ |opB|) + 1e-300
elementwise, an accumulate start or a bias added to the magnitudes.  tests/test_dgemm_batched2_oracle_cpu.py holds the
oracle itself to half of that bound against a numpy.longdouble product, for every case and seed of the table
(tests/dgemm_batched2_cases.py).  The WHOLE C buffer is compared against a poisoned copy, so a store outside the items —
into padding, between interleaved items, behind the last one — shows as a changed value.

Behind the table, bit for bit and without a tolerance: items against batch-1 eg_dgemm_batched calls on their pointers,
nested strides against eg_dgemm_batched with batch0 * batch1 items, a call against itself; then K == 0, a call of two
launches whose second starts inside an outer row, and one item shape each side of the rule that sends items that fill the
chip to a loop of plain products."""
import ctypes

import numpy as np
import pytest

import dgemm_batched2_cases as cases
from dgemm_batched2_cases import POISON, Case
from exprgrad_amd import _lib, ops

pytestmark = pytest.mark.gpu

MAX_BLOCKS = 1 << 22          # blocks of one launch (kernels/item_grid.hpp, BATCHED_MAX_BLOCKS)
TABLE = cases.table()


def dev(ctx, arr):
    arr = np.ascontiguousarray(arr, dtype=np.float64)
    buf = ctx.allocBuffer(arr.nbytes)
    buf.write(arr)
    return buf


def read(buf, n):
    return buf.readInto(np.empty(n, dtype=np.float64))


def free(*bufs):
    for buf in bufs:
        if buf is not None:
            buf.dealloc()


def run(ctx, c):
    """The call of case c -> the whole C buffer."""
    b0, b1, M, N, K = c.dims
    da, db, dc = dev(ctx, c.a), dev(ctx, c.b), dev(ctx, c.c0)
    dbias = dev(ctx, c.bias) if c.bias is not None else None
    o = 8 * c.offset
    ops.dgemm_batched2(ctx, b0, b1, M, N, K, da.ptr + o, c.a_lay[0], c.a_lay[1:], db.ptr + o, c.b_lay[0], c.b_lay[1:], dc.ptr + o, c.c_lay[0],
                       c.c_lay[1:], c.ta, c.tb, c.accumulate, dbias)
    got = read(dc, c.c0.size)
    free(da, db, dc, dbias)
    return got


def check(c, refcpu, got):
    K = c.dims[4]
    want = c.c0.copy()          # everything outside the items' M x N elements must stay as it was
    worst = 0.0
    for o, i in c.items():
        ref, lim = c.oracle_item(refcpu, o, i), cases.bound(K, c.magnitudes(o, i))
        g = c.c_item(got, o, i)
        err = np.abs(g - ref)
        worst = max(worst, float(np.max(err / lim)))
        assert np.all(err <= lim), (c.label(), "item", (o, i), "worst |got - want| / bound", float(np.max(err / lim)))
        c.c_item(want, o, i)[...] = g
    print(c.label(), "worst |got - oracle| / bound", worst)
    assert np.array_equal(got, want), "stored outside the items of C"


def same_bits(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))


@pytest.mark.parametrize("make", [m for _, m in TABLE], ids=[n for n, _ in TABLE])
def test_table(gpu_ctx, refcpu, make):
    """One and 2 x 2 ragged tiles in the four layouts, K of 16 and 17, the head layouts of the scores and the context
    product (C interleaved), each of the four A / B strides 0 in turn, even strides on aligned bases (16-byte loads), the
    same with one odd stride and with every pointer one double off, accumulate with bias, batch0 == 1, batch1 == 1."""
    c = make()
    check(c, refcpu, run(gpu_ctx, c))


def single_call(ctx, c, da, db, o, i):
    """eg_dgemm_batched with batch 1 on the three pointers of item (o, i) -> its M x N result."""
    _, _, M, N, K = c.dims
    at = lambda lay: 8 * (c.offset + o * lay[1] + i * lay[2])
    ldc = c.c_lay[0]
    c0 = np.full(M * ldc, POISON)
    if c.accumulate:
        c0.reshape(M, ldc)[:, :N] = c.c_item(c.c0, o, i)
    dc = dev(ctx, c0)
    dbias = dev(ctx, c.bias) if c.bias is not None else None
    ops.dgemm_batched(ctx, 1, M, N, K, da.ptr + at(c.a_lay), c.a_lay[0], 0, db.ptr + at(c.b_lay), c.b_lay[0], 0, dc, ldc, M * ldc, c.ta, c.tb,
                      c.accumulate, dbias)
    out = np.ascontiguousarray(read(dc, M * ldc).reshape(M, ldc)[:, :N])
    free(dc, dbias)
    return out


# (name, constructor, the three items compared): nested over 2 x 2 ragged tiles, the scores' head layout on 16-byte loads,
# the context's interleaved C on 8-byte loads with accumulate and bias
NAMED = [
    ("nested", lambda: Case(2, 3, 70, 65, 35, seed=3), [(0, 0), (0, 2), (1, 1)]),
    ("scores-in-row", lambda: cases.scores_in_row(16, 20, 0, 4), [(0, 1), (1, 0), (1, 2)]),
    ("context-in-row-accumulate-bias", lambda: Case(2, 3, 33, 17, 19, b=cases.in_row(3, 19, 17), c=cases.in_row(3, 33, 17), offset=1,
                                                    accumulate=True, bias=True, seed=5), [(0, 0), (1, 1), (1, 2)]),
]


@pytest.mark.parametrize("make,items", [(m, it) for _, m, it in NAMED], ids=[n for n, _, _ in NAMED])
def test_items_have_the_bits_of_batch_1_calls(gpu_ctx, make, items):
    c = make()
    got = run(gpu_ctx, c)
    da, db = dev(gpu_ctx, c.a), dev(gpu_ctx, c.b)
    for o, i in items:
        assert same_bits(c.c_item(got, o, i), single_call(gpu_ctx, c, da, db, o, i)), (c.label(), o, i)
    free(da, db)


def test_nested_strides_have_the_bits_of_the_one_index_entry_and_calls_repeat(gpu_ctx, refcpu):
    c = Case(2, 3, 130, 70, 40, a=cases.nested(3, 130, 40, 2, 0), b=cases.nested(3, 40, 70, 2, 0), c=cases.nested(3, 130, 70, 2, 0), seed=6)
    b0, b1, M, N, K = c.dims
    assert all(lay[1] == b1 * lay[2] for lay in (c.a_lay, c.b_lay, c.c_lay))
    first, second = run(gpu_ctx, c), run(gpu_ctx, c)
    check(c, refcpu, first)
    assert same_bits(first, second)
    da, db, dc = dev(gpu_ctx, c.a), dev(gpu_ctx, c.b), dev(gpu_ctx, c.c0)
    ops.dgemm_batched(gpu_ctx, b0 * b1, M, N, K, da, c.a_lay[0], c.a_lay[2], db, c.b_lay[0], c.b_lay[2], dc, c.c_lay[0], c.c_lay[2])
    assert same_bits(read(dc, c.c0.size), first)
    free(da, db, dc)


def raw(ctx, b0, b1, M, N, K, A, lda, sa, B, ldb, sb, C, ldc, sc, bias=None, accumulate=0):
    p = lambda x: ctypes.c_void_p(x.ptr if x is not None else 0)
    return _lib.lib().eg_dgemm_batched2(ctx.handle, 0, 0, b0, b1, M, N, K, p(A), lda, sa[0], sa[1], p(B), ldb, sb[0], sb[1], p(C), ldc, sc[0],
                                        sc[1], accumulate, p(bias))


@pytest.mark.parametrize("with_bias", [False, True])
def test_empty_k_writes_bias_or_zeros(gpu_ctx, with_bias):
    """K == 0 with NULL A and B.  Not accumulating: every item becomes the bias row, or zeros, the padding stays.
    Accumulating without a bias: C stays as it was."""
    b0, b1, M, N = 2, 3, 33, 20
    bias = (np.arange(N, dtype=np.float64) - 7) / 4
    ldc, s1 = N + 3, M * (N + 3) + 5
    s0 = b1 * s1
    n = b0 * s0
    dc, dbias = dev(gpu_ctx, np.full(n, POISON)), dev(gpu_ctx, bias)
    assert raw(gpu_ctx, b0, b1, M, N, 0, None, 1, (0, 0), None, N, (0, 0), dc, ldc, (s0, s1), dbias if with_bias else None) == 0, _lib.last_error()
    got = read(dc, n).reshape(b0 * b1, s1)
    rows = got[:, :M * ldc].reshape(b0 * b1, M, ldc)
    assert np.array_equal(rows[:, :, :N], np.broadcast_to(bias if with_bias else np.zeros(N), (b0 * b1, M, N)))
    assert np.all(rows[:, :, N:] == POISON) and np.all(got[:, M * ldc:] == POISON)
    if not with_bias:
        before = np.random.default_rng(0).random(n) - 0.5
        dc2 = dev(gpu_ctx, before)
        assert raw(gpu_ctx, b0, b1, M, N, 0, None, 1, (0, 0), None, N, (0, 0), dc2, ldc, (s0, s1), accumulate=1) == 0, _lib.last_error()
        assert np.array_equal(read(dc2, n), before)
        free(dc2)
    free(dc, dbias)


def test_a_second_launch_that_starts_inside_an_outer_row(gpu_ctx):
    """3 x 1 398 103 items of 1 x 1 x 1 with A and B shared along both indices: 2^22 + 5 blocks, so the last five items — the
    end of outer row 2 — run in a second launch that starts mid-row.  C has the inner index fastest; a single float64
    product is correctly rounded, so every element is compared with the exact product."""
    b0, b1 = 3, 1398103
    n = b0 * b1
    assert n == MAX_BLOCKS + 5
    a, b = np.array([0.3]), np.array([-0.7])
    da, db, dc = dev(gpu_ctx, a), dev(gpu_ctx, b), dev(gpu_ctx, np.full(n + 3, POISON))
    ops.dgemm_batched2(gpu_ctx, b0, b1, 1, 1, 1, da, 1, (0, 0), db, 1, (0, 0), dc, 1, (b1, 1))
    got = read(dc, n + 3)
    assert np.all(got[n - 5:n] == a[0] * b[0]) and got[MAX_BLOCKS - 1] == a[0] * b[0]      # the second launch; the first one's last item
    assert np.all(got[:n] == a[0] * b[0]) and np.all(got[n:] == POISON)
    free(da, db, dc)


def test_items_are_told_apart_across_the_two_launches(gpu_ctx):
    """The same cut with B stepping along the inner index only (stride_b0 == 0) and the outer index in C's fast position:
    item (o, i) must be a * b[i] at C[i * 3 + o] — a launch that lost count of its first item would shift the tail."""
    b0, b1 = 3, 1398103
    n = b0 * b1
    rng = np.random.default_rng(23)
    a, b = rng.random(1) - 0.5, rng.random(b1) - 0.5
    da, db, dc = dev(gpu_ctx, a), dev(gpu_ctx, b), dev(gpu_ctx, np.full(n + 3, POISON))
    ops.dgemm_batched2(gpu_ctx, b0, b1, 1, 1, 1, da, 1, (0, 0), db, 1, (0, 1), dc, 1, (1, b0))
    got = read(dc, n + 3)
    assert np.array_equal(got[:n].reshape(b1, b0), np.repeat((a[0] * b)[:, None], b0, axis=1)) and np.all(got[n:] == POISON)
    free(da, db, dc)


def compute_units():
    cu, clock, hbm = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    arch = ctypes.create_string_buffer(64)
    _lib.call("eg_device_props", 0, ctypes.byref(cu), ctypes.byref(clock), ctypes.byref(hbm), arch, 64)
    return cu.value


@pytest.mark.parametrize("side", ["loop", "launch"])
def test_both_sides_of_the_loop_rule(gpu_ctx, refcpu, side):
    """The rule of eg_dgemm_batched (gemm_plan.cpp, dgemm_batched_runs_as_loop), decided from the item alone: an item with at
    least one 64 x 64 tile per compute unit runs as a plain product.  Four tile columns; one tile row more or less puts the
    item on either side.  K = 24: eg_dgemm takes no slices, so on both sides item (1, 0) has the bits of the batch-1 call."""
    cus = compute_units()
    rows = -(-cus // 4)
    M = 64 * (rows if side == "loop" else rows - 1)
    assert (M // 64 * 4 >= cus) == (side == "loop") and M > 0
    c = Case(2, 2, M, 256, 24, seed=31 + (side == "loop"))
    got = run(gpu_ctx, c)
    check(c, refcpu, got)
    da, db = dev(gpu_ctx, c.a), dev(gpu_ctx, c.b)
    assert same_bits(c.c_item(got, 1, 0), single_call(gpu_ctx, c, da, db, 1, 0)), side
    free(da, db)
