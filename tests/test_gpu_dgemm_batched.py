"""GPU parity of eg_dgemm_batched (kernels/gemm_f64_mfma.hip, dgemm_batched_kernel) against the oracle.

Every item of a batch is compared with refcpu.dgemm64 on that item's operands within the project's own bound for eg_dgemm
(tests/test_gpu_f64.py): |got - want| <= 4e-16 * sqrt(K) * (|opA| @ |opB|) + 1e-300 elementwise, an accumulate start or a
bias added to the magnitudes.  tests/test_dgemm_batched_oracle_cpu.py holds the oracle itself to half of that bound against
a numpy.longdouble product, for every case and seed of the table (tests/dgemm_batched_cases.py).  Wherever leading
dimensions or strides are padded the WHOLE C buffer is compared, so a store into the padding shows as a changed poison
value.

Behind the table: bit equality with eg_dgemm and across batch sizes, K == 0, empty products, invalid arguments, a batch
that takes more than one launch, and one case each side of the rule that sends items that fill the chip to a loop of plain
products."""
import ctypes

import numpy as np
import pytest

import dgemm_batched_cases as cases
from dgemm_batched_cases import POISON, Case
from exprgrad_amd import _lib, ops

pytestmark = pytest.mark.gpu

EG_ERR_INVALID = 1
MAX_BLOCKS = 1 << 22          # blocks of one launch (kernels/gemm_plan.hpp, BATCHED_MAX_BLOCKS)
TABLE = cases.table()


def dev(ctx, arr):
    arr = np.ascontiguousarray(arr, dtype=np.float64)
    buf = ctx.allocBuffer(arr.nbytes)
    buf.write(arr)
    return buf


def read(buf, n):
    return buf.readInto(np.empty(n, dtype=np.float64))


def run(ctx, c, batch=None, first=0):
    """The call of case c on items [first, first + batch) -> the whole C buffer."""
    nb, M, N, K = c.dims
    batch = nb if batch is None else batch
    da, db, dc = dev(ctx, c.a), dev(ctx, c.b), dev(ctx, c.c0)
    dbias = dev(ctx, c.bias) if c.bias is not None else None
    o = 8 * c.offset
    ops.dgemm_batched(ctx, batch, M, N, K, da.ptr + o + 8 * first * c.stride_a, c.lda, c.stride_a, db.ptr + o + 8 * first * c.stride_b, c.ldb,
                      c.stride_b, dc.ptr + o + 8 * first * c.stride_c, c.ldc, c.stride_c, c.ta, c.tb, c.accumulate, dbias)
    got = read(dc, c.c0.size)
    for buf in (da, db, dc, dbias):
        if buf is not None:
            buf.dealloc()
    return got


def check(c, refcpu, got, items=None):
    batch, M, N, K = c.dims
    want = c.c0.copy()          # everything outside the items' M x N elements must stay as it was
    worst = 0.0
    for i in (range(batch) if items is None else items):
        ref, lim = c.oracle_item(refcpu, i), cases.bound(K, c.magnitudes(i))
        g = c.c_item(got, i)
        err = np.abs(g - ref)
        worst = max(worst, float(np.max(err / lim)))
        assert np.all(err <= lim), (c.label(), "item", i, "worst |got - want| / bound", float(np.max(err / lim)))
        c.c_item(want, i)[...] = g
    print(c.label(), "worst |got - oracle| / bound", worst)
    assert np.array_equal(got, want), "stored outside the items of C"


def dgemm_item(ctx, c, i):
    """eg_dgemm on item i of case c -> its M x N result."""
    _, M, N, K = c.dims
    da, db = dev(ctx, c.a), dev(ctx, c.b)
    c0 = np.full(M * c.ldc, POISON)
    if c.accumulate:
        c0[:] = c.c0[c.offset + i * c.stride_c:][:M * c.ldc]
    dc = dev(ctx, c0)
    dbias = dev(ctx, c.bias) if c.bias is not None else None
    o = 8 * c.offset
    _lib.call("eg_dgemm", ctx.handle, int(c.ta), int(c.tb), M, N, K, ctypes.c_void_p(da.ptr + o + 8 * i * c.stride_a), c.lda,
              ctypes.c_void_p(db.ptr + o + 8 * i * c.stride_b), c.ldb, ctypes.c_void_p(dc.ptr), c.ldc, int(c.accumulate),
              ctypes.c_void_p(dbias.ptr) if dbias is not None else None)
    out = read(dc, M * c.ldc).reshape(M, c.ldc)[:, :N]
    for buf in (da, db, dc, dbias):
        if buf is not None:
            buf.dealloc()
    return np.ascontiguousarray(out)


def same_bits(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))


@pytest.mark.parametrize("kw", [kw for _, kw in TABLE], ids=[name for name, _ in TABLE])
def test_table(gpu_ctx, refcpu, kw):
    c = Case(**kw)
    check(c, refcpu, run(gpu_ctx, c))


@pytest.mark.parametrize("dims", [(5, 33, 20, 17), (7, 130, 70, 40)])
@pytest.mark.parametrize("ta,tb", cases.LAYOUTS, ids=cases.LAYOUT_IDS)
def test_items_have_the_bits_of_eg_dgemm(gpu_ctx, dims, ta, tb):
    """K < 512: eg_dgemm takes no k-slices, so whatever tile it picks, every element is the same k-ascending chain."""
    c = Case(*dims, ta=ta, tb=tb, seed=cases.seed_of(dims, ta, tb))
    got = run(gpu_ctx, c)
    for i in range(dims[0]):
        assert same_bits(c.c_item(got, i), dgemm_item(gpu_ctx, c, i)), (c.label(), i)


def test_bits_do_not_depend_on_the_batch(gpu_ctx):
    """Item 4 of a batch of 9 has the bits of a batch-1 call on its operands; the same call twice gives the same bits."""
    c = Case(9, 130, 70, 40, pad_ld=2, pad_stride=6, seed=3)
    nine, again = run(gpu_ctx, c), run(gpu_ctx, c)
    assert same_bits(nine, again)
    one = run(gpu_ctx, c, batch=1, first=4)
    assert same_bits(c.c_item(one, 4), c.c_item(nine, 4))
    keep = np.ones(one.size, dtype=bool)        # the batch-1 call wrote item 4 and nothing else
    keep.reshape(-1)[c.offset + 4 * c.stride_c:][:130 * c.ldc].reshape(130, c.ldc)[:, :70] = False
    assert np.all(one[keep] == POISON)


@pytest.mark.parametrize("with_bias", [False, True])
def test_empty_k(gpu_ctx, with_bias):
    """K == 0 with NULL A and B.  Not accumulating: every item becomes the bias row, or zeros.  Accumulating without a bias:
    C stays as it was."""
    batch, M, N = 3, 33, 20
    bias = (np.arange(N, dtype=np.float64) - 7) / 4
    null = ctypes.c_void_p(0)
    fn = _lib.lib().eg_dgemm_batched
    dc, dbias = dev(gpu_ctx, np.full(batch * M * N + 5, POISON)), dev(gpu_ctx, bias)
    rc = fn(gpu_ctx.handle, 0, 0, batch, M, N, 0, null, 1, 0, null, N, 0, ctypes.c_void_p(dc.ptr), N, M * N, 0,
            ctypes.c_void_p(dbias.ptr) if with_bias else null)
    assert rc == 0, _lib.last_error()
    got = read(dc, batch * M * N + 5)
    want = np.tile(bias if with_bias else np.zeros(N), batch * M)
    assert np.array_equal(got[:batch * M * N], want) and np.all(got[batch * M * N:] == POISON)
    if not with_bias:
        before = np.random.default_rng(0).random(batch * M * N + 5) - 0.5
        dc2 = dev(gpu_ctx, before)
        assert fn(gpu_ctx.handle, 0, 0, batch, M, N, 0, null, 1, 0, null, N, 0, ctypes.c_void_p(dc2.ptr), N, M * N, 1, null) == 0, _lib.last_error()
        assert np.array_equal(read(dc2, before.size), before)
        dc2.dealloc()
    dc.dealloc()
    dbias.dealloc()


def test_empty_products_launch_nothing(gpu_ctx):
    fn = _lib.lib().eg_dgemm_batched
    buf = dev(gpu_ctx, np.full(4 * 8 * 8, POISON))
    p = ctypes.c_void_p(buf.ptr)
    null = ctypes.c_void_p(0)
    for batch, M, N in ((0, 8, 8), (4, 0, 8), (4, 8, 0)):
        assert fn(gpu_ctx.handle, 0, 0, batch, M, N, 8, p, 8, 64, p, 8, 64, p, 8, 64, 0, null) == 0, _lib.last_error()
        assert fn(gpu_ctx.handle, 0, 0, batch, M, N, 8, null, 8, 64, null, 8, 64, null, 8, 64, 0, null) == 0, _lib.last_error()
    assert np.all(read(buf, 4 * 8 * 8) == POISON)
    buf.dealloc()


def test_invalid_arguments(gpu_ctx):
    fn = _lib.lib().eg_dgemm_batched
    buf = dev(gpu_ctx, np.full(4 * 8 * 8, POISON))
    p = ctypes.c_void_p(buf.ptr)
    null = ctypes.c_void_p(0)
    good = dict(ctx=gpu_ctx.handle, batch=4, M=8, N=8, K=8, A=p, lda=8, stride_a=64, B=p, ldb=8, stride_b=64, C=p, ldc=8, stride_c=64)
    bad = {
        "NULL ctx": dict(ctx=null),
        "negative batch": dict(batch=-1), "negative M": dict(M=-1), "negative N": dict(N=-1), "negative K": dict(K=-1),
        "negative stride_a": dict(stride_a=-64), "negative stride_b": dict(stride_b=-64),
        "lda shorter than a row": dict(lda=7), "ldb shorter than a row": dict(ldb=7), "ldc shorter than a row": dict(ldc=7),
        "items of C overlap": dict(stride_c=63),
        "NULL A": dict(A=null), "NULL B": dict(B=null), "NULL C": dict(C=null),
    }
    for name, change in bad.items():
        a = dict(good, **change)
        rc = fn(a["ctx"], 0, 0, a["batch"], a["M"], a["N"], a["K"], a["A"], a["lda"], a["stride_a"], a["B"], a["ldb"], a["stride_b"], a["C"], a["ldc"],
                a["stride_c"], 0, null)
        assert rc == EG_ERR_INVALID, name
        assert "eg_dgemm_batched" in _lib.last_error(), (name, _lib.last_error())
    assert np.all(read(buf, 4 * 8 * 8) == POISON)
    # a stride_c that would overlap is not looked at for a batch of one
    assert fn(gpu_ctx.handle, 0, 0, 1, 8, 8, 8, p, 8, 64, p, 8, 64, ctypes.c_void_p(buf.ptr + 8 * 128), 8, 0, 0, null) == 0, _lib.last_error()
    buf.dealloc()


def test_more_items_than_one_launch(gpu_ctx):
    """MAX_BLOCKS + 3 items of 1 x 1 x 1 with a shared A (NN, K = 1): one launch holds MAX_BLOCKS blocks, so the last three
    items run in a second one.  A single float64 product is correctly rounded, so every item is compared exactly."""
    n = MAX_BLOCKS + 3
    rng = np.random.default_rng(22)
    a, b = rng.random(1) - 0.5, rng.random(n) - 0.5
    da, db, dc = dev(gpu_ctx, a), dev(gpu_ctx, b), dev(gpu_ctx, np.full(n + 3, POISON))
    ops.dgemm_batched(gpu_ctx, n, 1, 1, 1, da, 1, 0, db, 1, 1, dc, 1, 1)
    got = read(dc, n + 3)
    want = a[0] * b
    assert got[n - 3] == want[n - 3] and got[n - 2] == want[n - 2] and got[n - 1] == want[n - 1]     # the second launch
    assert got[MAX_BLOCKS - 1] == want[MAX_BLOCKS - 1]                                                 # the last item of the first
    assert np.array_equal(got[:n], want) and np.all(got[n:] == POISON)
    for buf in (da, db, dc):
        buf.dealloc()


def compute_units():
    cu, clock, hbm = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    arch = ctypes.create_string_buffer(64)
    _lib.call("eg_device_props", 0, ctypes.byref(cu), ctypes.byref(clock), ctypes.byref(hbm), arch, 64)
    return cu.value


@pytest.mark.parametrize("side", ["loop", "launch"])
def test_both_sides_of_the_loop_rule(gpu_ctx, refcpu, side):
    """The shipped rule (gemm_plan.cpp, dgemm_batched_runs_as_loop): an item with at least one 64 x 64 tile per compute unit
    runs as a plain product.  Four tile columns; one tile row more or less puts the item on either side.  K = 24: eg_dgemm
    takes no slices, so on both sides every item has its bits."""
    cus = compute_units()
    rows = -(-cus // 4)
    M = 64 * (rows if side == "loop" else rows - 1)
    assert (M // 64 * 4 >= cus) == (side == "loop") and M > 0
    c = Case(2, M, 256, 24, seed=31 + (side == "loop"))
    got = run(gpu_ctx, c)
    for i in range(2):
        assert same_bits(c.c_item(got, i), dgemm_item(gpu_ctx, c, i)), (side, i)
    check(c, refcpu, got)
