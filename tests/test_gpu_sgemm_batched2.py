"""GPU parity of eg_sgemm_batched2 (kernels/gemm_batched.hip) against the oracle and a float64 product.

Every item (o, i) is compared with refcpu.sgemm on that item's operands and with the float64 numpy product, within TOL
(1e-5 relative to the item's largest value).  Inputs are U[-0.5, 0.5) and K <= 96 in the table (tests/batched2_cases.py),
where the oracle's own float32 result is within 5e-6 of the float64 product for every shape and seed used here:
tests/test_batched2_oracle_cpu.py asserts that on the CPU.  The WHOLE C buffer is compared against a poisoned copy, so a
store outside the items — into padding, between interleaved items, behind the last one — shows up as a changed value.

The cases behind those of the table reach what K <= 96 cannot: the 16-byte stores through LDS (K >= 128), more items than
one launch holds, and K == 0.  They compare with the float64 product and with batch-1 calls only, never with the oracle.
"""
import ctypes

import numpy as np
import pytest

import batched2_cases as cases
from batched2_cases import POISON, Case
from exprgrad_amd import _lib, ops
from conftest import TOL, rel_err

pytestmark = pytest.mark.gpu

EG_ERR_INVALID = 1
TABLE = cases.table()


def dev(ctx, arr):
    t = ctx.allocTensor(arr.shape)
    t.write(arr)
    return t


def run(ctx, c):
    b0, b1, M, N, K = c.dims
    da, db, dc = dev(ctx, c.a), dev(ctx, c.b), dev(ctx, c.c0)
    dbias = dev(ctx, c.bias) if c.bias is not None else None
    o = 4 * c.offset
    ops.sgemm_batched2(ctx, b0, b1, M, N, K, da.ptr + o, c.a_lay[0], c.a_lay[1:], db.ptr + o, c.b_lay[0], c.b_lay[1:], dc.ptr + o, c.c_lay[0],
                       c.c_lay[1:], c.ta, c.tb, c.accumulate, dbias)
    return dc.read()


def check(c, refcpu, got, oracle=True):
    want = c.c0.copy()          # everything outside the items' M x N elements must stay as it was
    worst = worst64 = 0.0
    for o, i in c.items():
        g = c.c_item(got, o, i)
        if oracle:
            worst = max(worst, rel_err(g, c.oracle(refcpu, o, i), c.label() + " item vs oracle"))
        worst64 = max(worst64, rel_err(g, c.exact(o, i), c.label() + " item vs float64"))
        c.c_item(want, o, i)[...] = g
    print(c.label(), "vs oracle", worst if oracle else "-", "vs float64", worst64)
    assert worst <= TOL and worst64 <= TOL, (c.dims, worst, worst64)
    assert np.array_equal(got, want), "stored outside the items of C"


@pytest.mark.parametrize("make", [m for _, m in TABLE], ids=[n for n, _ in TABLE])
def test_table(gpu_ctx, refcpu, make):
    """Nested strides in the four layouts, the head index inside the row on the 16-byte and on the element path, ragged
    tiles with padding at pointer offsets 0 and 1, operands shared along one or both indices, accumulate with bias."""
    c = make()
    check(c, refcpu, run(gpu_ctx, c))


def lds_store_case():
    """(2, 2, 128, 64, 128): whole tiles, K >= 128, every pointer 16-byte aligned and every stride a multiple of 4, so tiles
    leave through LDS as 16-byte stores.  C keeps the inner index inside its row with 4 floats of padding behind every
    item's row piece (ldc = 2 * 68, stride_c1 = 68) and 8 behind every outer item."""
    return Case(2, 2, 128, 64, 128, c=cases.in_row(2, 128, 64, pad_cols=4, pad_stride=8), tail=4, seed=70)


def test_stores_through_lds_leave_the_gaps(gpu_ctx):
    """Against the float64 product only: an in-order float32 sum of 128 products whose partial sums stay near max|C| is
    off by about sqrt(K) * 2^-24 of it, 7e-7, an order below TOL."""
    c = lds_store_case()
    assert all(s % 4 == 0 for lay in (c.a_lay, c.b_lay, c.c_lay) for s in lay)
    got = run(gpu_ctx, c)
    check(c, None, got, oracle=False)
    same_bits_as_single_calls(gpu_ctx, c, got)


def same_bits_as_single_calls(ctx, c, got):
    """Item (o, i) has the bits of a batch-1 eg_sgemm_batched call on its three pointers."""
    b0, b1, M, N, K = c.dims
    da, db = dev(ctx, c.a), dev(ctx, c.b)
    at = lambda lay, o, i: 4 * (c.offset + o * lay[1] + i * lay[2])
    ldc = c.c_lay[0]
    for o, i in c.items():
        dc = dev(ctx, np.full(M * ldc, POISON, dtype=np.float32))
        ops.sgemm_batched(ctx, 1, M, N, K, da.ptr + at(c.a_lay, o, i), c.a_lay[0], 0, db.ptr + at(c.b_lay, o, i), c.b_lay[0], 0, dc, ldc,
                          M * ldc, c.ta, c.tb)
        one = dc.read().reshape(M, ldc)[:, :N]
        assert np.array_equal(one.view(np.uint32), np.ascontiguousarray(c.c_item(got, o, i)).view(np.uint32)), (o, i)


def test_bits(gpu_ctx, refcpu):
    """The same call twice gives the same bits; every item has the bits of the batch-1 eg_sgemm_batched call on its
    pointers (nested and head-in-row); a call with nested strides has the bits of eg_sgemm_batched with batch0 * batch1 items."""
    c = Case(2, 3, 130, 70, 90, seed=3)
    first, second = run(gpu_ctx, c), run(gpu_ctx, c)
    check(c, refcpu, first)
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))
    same_bits_as_single_calls(gpu_ctx, c, first)
    b0, b1, M, N, K = c.dims
    assert all(lay[1] == b1 * lay[2] for lay in (c.a_lay, c.b_lay, c.c_lay))
    da, db, dc = dev(gpu_ctx, c.a), dev(gpu_ctx, c.b), dev(gpu_ctx, c.c0)
    ops.sgemm_batched(gpu_ctx, b0 * b1, M, N, K, da, c.a_lay[0], c.a_lay[2], db, c.b_lay[0], c.b_lay[2], dc, c.c_lay[0], c.c_lay[2])
    assert np.array_equal(dc.read().view(np.uint32), first.view(np.uint32))
    h = cases.head_in_row(16, 20, 0, 31)
    same_bits_as_single_calls(gpu_ctx, h, run(gpu_ctx, h))


def one_index_cases():
    """(id, constructor) of five items in a row, as both entries can address them.  Ragged: 70 x 66 x 19 is 2 x 2 ragged tiles
    and a k tail, on element loads through an odd lda.  Whole: 64 x 64 x 32 with every stride a multiple of 4, 16-byte loads.
    C is padded behind every row and every item, and poisoned there."""
    t = []
    for ta, tb in cases.LAYOUTS:
        def ragged(ta=ta, tb=tb, **kw):
            ra, ca = (19, 70) if ta else (70, 19)
            rb, cb = (66, 19) if tb else (19, 66)
            c = Case(1, 5, 70, 66, 19, ta, tb, a=cases.nested(5, ra, ca, 3 if ta else 2, 5), b=cases.nested(5, rb, cb, 3, 5),
                     c=cases.nested(5, 70, 66, 3, 5), seed=80 + 2 * ta + tb, **kw)
            assert c.a_lay[0] % 2 == 1
            return c
        t.append(("ragged-%d%d" % (ta, tb), ragged))
    t.append(("ragged-00-accumulate-bias", lambda: t[0][1](accumulate=True, bias=True)))
    t.append(("whole-16-byte", lambda: Case(1, 5, 64, 64, 32, a=cases.nested(5, 64, 32, 4, 8), b=cases.nested(5, 32, 64, 4, 8),
                                            c=cases.nested(5, 64, 64, 4, 8), seed=90)))
    return t


@pytest.mark.parametrize("make", [m for _, m in one_index_cases()], ids=[n for n, _ in one_index_cases()])
def test_one_kernel_behind_both_entries(gpu_ctx, make):
    """eg_sgemm_batched(batch = 5, stride), eg_sgemm_batched2(1, 5, strides (0, stride)) and eg_sgemm_batched2(5, 1, strides
    (stride, 0)) run one kernel through one launcher: the same bits in every element of C, the poisoned padding included.
    The first result is also held to the float64 product (19 or 32 terms in order: well inside TOL)."""
    c = make()
    if c.accumulate:   # Case fills an accumulating C with values throughout: poison what lies between rows and items again
        c0 = np.full_like(c.c0, POISON)
        for o, i in c.items():
            c.c_item(c0, o, i)[...] = c.c_item(c.c0, o, i)
        c.c0 = c0
    _, n, M, N, K = c.dims
    (lda, _, sa), (ldb, _, sb), (ldc, _, sc) = c.a_lay, c.b_lay, c.c_lay
    da, db = dev(gpu_ctx, c.a), dev(gpu_ctx, c.b)
    dbias = dev(gpu_ctx, c.bias) if c.bias is not None else None
    got = []
    for b0, b1 in ((0, 0), (1, n), (n, 1)):   # (0, 0): the entry with one batch index
        dc = dev(gpu_ctx, c.c0)
        if b0 == 0:
            ops.sgemm_batched(gpu_ctx, n, M, N, K, da, lda, sa, db, ldb, sb, dc, ldc, sc, c.ta, c.tb, c.accumulate, dbias)
        else:
            pair = lambda s: (0, s) if b0 == 1 else (s, 0)
            ops.sgemm_batched2(gpu_ctx, b0, b1, M, N, K, da, lda, pair(sa), db, ldb, pair(sb), dc, ldc, pair(sc), c.ta, c.tb, c.accumulate, dbias)
        got.append(dc.read())
    check(c, None, got[0], oracle=False)
    for other in got[1:]:
        assert np.array_equal(got[0].view(np.uint32), other.view(np.uint32))


def test_more_items_than_one_launch(gpu_ctx):
    """2049 x 2048 items of 1 x 1 x 1: one launch holds 2^22 blocks, so the last 2048 items — the whole last outer index —
    run in a second one.  A single float32 product is correctly rounded, so every item is compared exactly."""
    b0, b1 = 2049, 2048
    n = b0 * b1
    assert n > 1 << 22
    rng = np.random.default_rng(22)
    a, b = (rng.random(n, dtype=np.float32) - np.float32(0.5) for _ in range(2))
    da, db, dc = dev(gpu_ctx, a), dev(gpu_ctx, b), dev(gpu_ctx, np.full(n + 3, POISON, dtype=np.float32))
    ops.sgemm_batched2(gpu_ctx, b0, b1, 1, 1, 1, da, 1, (b1, 1), db, 1, (b1, 1), dc, 1, (b1, 1))
    got = dc.read()
    assert np.array_equal(got[:n], a * b) and np.all(got[n:] == POISON)


def raw(ctx, b0, b1, M, N, K, A, lda, sa, B, ldb, sb, C, ldc, sc, bias=None, ta=0, tb=0):
    p = lambda x: ctypes.c_void_p(x.ptr if x is not None else 0)
    return _lib.lib().eg_sgemm_batched2(ctx.handle, ta, tb, b0, b1, M, N, K, p(A), lda, sa[0], sa[1], p(B), ldb, sb[0], sb[1], p(C), ldc, sc[0],
                                        sc[1], 0, p(bias))


@pytest.mark.parametrize("b0,b1", [(0, 3), (2, 0)])
def test_an_empty_batch_succeeds_and_writes_nothing(gpu_ctx, b0, b1):
    buf = dev(gpu_ctx, np.full(2 * 3 * 8 * 8, POISON, dtype=np.float32))
    assert raw(gpu_ctx, b0, b1, 8, 8, 8, buf, 8, (192, 64), buf, 8, (192, 64), buf, 8, (192, 64)) == 0, _lib.last_error()
    assert np.all(buf.read() == POISON)


@pytest.mark.parametrize("with_bias", [False, True])
def test_empty_k_writes_bias_or_zeros(gpu_ctx, with_bias):
    """K == 0 with NULL A and B, not accumulating: every item becomes the bias row, or zeros."""
    b0, b1, M, N = 2, 3, 33, 20
    bias = (np.arange(N, dtype=np.float32) - 7) / 4
    n = b0 * b1 * M * N
    dc, dbias = dev(gpu_ctx, np.full(n + 5, POISON, dtype=np.float32)), dev(gpu_ctx, bias)
    rc = raw(gpu_ctx, b0, b1, M, N, 0, None, 1, (0, 0), None, N, (0, 0), dc, N, (b1 * M * N, M * N), dbias if with_bias else None)
    assert rc == 0, _lib.last_error()
    got = dc.read()
    want = np.tile(bias if with_bias else np.zeros(N, dtype=np.float32), b0 * b1 * M)
    assert np.array_equal(got[:n], want) and np.all(got[n:] == POISON)


def test_error_returns(gpu_ctx):
    """Each invalid argument of the contract returns EG_ERR_INVALID with the function's name, and C stays as it was."""
    buf = dev(gpu_ctx, np.full(2 * 3 * 8 * 8, POISON, dtype=np.float32))
    ok = dict(b0=2, b1=3, M=8, N=8, K=8, A=buf, lda=8, sa=(192, 64), B=buf, ldb=8, sb=(192, 64), C=buf, ldc=8, sc=(192, 64))
    bad = {
        "negative batch0": dict(b0=-1), "negative batch1": dict(b1=-1), "negative M": dict(M=-1), "negative K": dict(K=-1),
        "batch0 of 2^31": dict(b0=1 << 31), "batch1 of 2^31": dict(b1=1 << 31),
        "NULL C": dict(C=None), "NULL A": dict(A=None), "NULL B": dict(B=None),
        "lda below K": dict(lda=7), "ldb below N": dict(ldb=7), "lda below M, transposed": dict(ta=1, M=9, lda=8, sc=(216, 72)),
        "negative stride_a0": dict(sa=(-192, 64)), "negative stride_a1": dict(sa=(192, -64)),
        "negative stride_b0": dict(sb=(-192, 64)), "negative stride_b1": dict(sb=(192, -64)),
        "ldc below N": dict(ldc=7), "items of C overlap": dict(sc=(192, 63)), "outer items of C overlap": dict(sc=(191, 64)),
        "stride_c0 == stride_c1": dict(sc=(64, 64)), "stride_c1 of 0": dict(sc=(192, 0)), "stride_c0 of 0": dict(sc=(0, 64)),
        "interleaved C one short": dict(ldc=24, sc=(192, 7)), "negative stride_c1": dict(sc=(192, -64)),
    }
    for name, change in bad.items():
        assert raw(gpu_ctx, **dict(ok, **change)) == EG_ERR_INVALID, name
        assert "eg_sgemm_batched2" in _lib.last_error(), (name, _lib.last_error())
    gpu_ctx.sync()
    assert np.all(buf.read() == POISON)
    # the interleaved layout itself is fine (and so is the call the table of changes starts from): A and B may alias C's
    # buffer only in a call that is refused, so these run on their own output
    out = dev(gpu_ctx, np.full(2 * 3 * 8 * 8, POISON, dtype=np.float32))
    assert raw(gpu_ctx, **dict(ok, C=out, ldc=24, sc=(192, 8))) == 0, _lib.last_error()
    assert raw(gpu_ctx, **dict(ok, C=out)) == 0, _lib.last_error()
