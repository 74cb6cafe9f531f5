"""GPU parity of eg_sgemm_batched (kernels/gemm_batched.hip) against the oracle and a float64 product.

Every item of a batch is compared with refcpu.sgemm on that item's operands and with the float64 numpy product, within
TOL (1e-5 relative to the item's largest value).  Inputs are U[-0.5, 0.5) and K <= 96, where the oracle's own float32
result is within 5e-6 of the float64 product for every shape and seed used here (checked on the CPU when these cases
were written).  Wherever leading dimensions or strides are padded, the WHOLE C buffer is compared, so a store into the
padding shows up as a changed poison value.

The cases behind those of the table reach what K <= 96 cannot: the 16-byte stores through LDS (K >= 128), a batch that
takes more than one launch, and K == 0.  They compare with the float64 product and with batch-1 calls only, never with
the oracle, whose own float32 error was not checked beyond K = 96.
"""
import ctypes

import numpy as np
import pytest

from exprgrad_amd import _lib, ops
from conftest import TOL, rel_err

pytestmark = pytest.mark.gpu

POISON = np.float32(-777.25)
EG_ERR_INVALID = 1


def dev(ctx, arr):
    t = ctx.allocTensor(arr.shape)
    t.write(arr)
    return t


class Case:
    """Host buffers of one batched call and what the call has to leave in C."""

    def __init__(self, batch, M, N, K, ta=False, tb=False, pad_ld=0, pad_stride=0, offset=0, share_a=False, share_b=False,
                 accumulate=False, bias=False, seed=0):
        rng = np.random.default_rng(seed)
        self.dims = (batch, M, N, K)
        self.ta, self.tb, self.accumulate, self.offset = ta, tb, accumulate, offset
        ra, ca = (K, M) if ta else (M, K)
        rb, cb = (N, K) if tb else (K, N)
        self.lda, self.ldb, self.ldc = ca + pad_ld, cb + pad_ld, N + pad_ld
        self.stride_a = 0 if share_a else ra * self.lda + pad_stride
        self.stride_b = 0 if share_b else rb * self.ldb + pad_stride
        self.stride_c = M * self.ldc + pad_stride
        u = lambda n: (rng.random(n, dtype=np.float32) - np.float32(0.5)).astype(np.float32)
        self.a = u(offset + (batch - 1) * self.stride_a + ra * self.lda)
        self.b = u(offset + (batch - 1) * self.stride_b + rb * self.ldb)
        c_len = offset + batch * self.stride_c
        self.c0 = u(c_len) if accumulate else np.full(c_len, POISON, dtype=np.float32)
        self.bias = u(N) if bias else None
        item = lambda buf, i, stride, rows, ld, cols: buf[offset + i * stride:][:rows * ld].reshape(rows, ld)[:, :cols]
        self.a_items = [np.ascontiguousarray(item(self.a, i, self.stride_a, ra, self.lda, ca)) for i in range(batch)]
        self.b_items = [np.ascontiguousarray(item(self.b, i, self.stride_b, rb, self.ldb, cb)) for i in range(batch)]
        self.c_item = lambda buf, i: item(buf, i, self.stride_c, M, self.ldc, N)

    def run(self, ctx):
        batch, M, N, K = self.dims
        da, db, dc = dev(ctx, self.a), dev(ctx, self.b), dev(ctx, self.c0)
        dbias = dev(ctx, self.bias) if self.bias is not None else None
        o = 4 * self.offset
        ops.sgemm_batched(ctx, batch, M, N, K, da.ptr + o, self.lda, self.stride_a, db.ptr + o, self.ldb, self.stride_b, dc.ptr + o,
                          self.ldc, self.stride_c, self.ta, self.tb, self.accumulate, dbias)
        return dc.read()

    def check(self, refcpu, got, oracle=True):
        batch, M, N, K = self.dims
        label = "eg_sgemm_batched %dx%dx%dx%d %s%s" % (batch, M, N, K, "T" if self.ta else "N", "T" if self.tb else "N")
        want = self.c0.copy()          # everything outside the items' M x N elements must stay as it was
        worst = worst64 = 0.0
        for i in range(batch):
            start = np.ascontiguousarray(self.c_item(self.c0, i)) if self.accumulate else np.zeros((M, N), dtype=np.float32)
            ref = refcpu.sgemm(self.a_items[i], self.b_items[i], self.ta, self.tb, out=start.copy(), threads=1) if oracle else None
            opa = self.a_items[i].T if self.ta else self.a_items[i]
            opb = self.b_items[i].T if self.tb else self.b_items[i]
            exact = opa.astype(np.float64) @ opb.astype(np.float64) + (start.astype(np.float64) if self.accumulate else 0.0)
            if self.bias is not None:
                if oracle:
                    refcpu.bias_add(self.bias, ref)
                exact = exact + self.bias.astype(np.float64)
            g = self.c_item(got, i)
            if oracle:
                worst = max(worst, rel_err(g, ref, label + " item vs oracle"))
            worst64 = max(worst64, rel_err(g, exact, label + " item vs float64"))
            self.c_item(want, i)[...] = self.c_item(got, i)
        print(label, "vs oracle", worst if oracle else "-", "vs float64", worst64)
        assert worst <= TOL and worst64 <= TOL, (self.dims, worst, worst64)
        assert np.array_equal(got, want), "stored outside the items of C"


@pytest.mark.parametrize("dims", [(1, 1, 1, 1), (3, 33, 17, 5), (5, 64, 64, 64), (300, 16, 16, 8), (70000, 4, 4, 4)])
def test_plain_batches(gpu_ctx, refcpu, dims):
    c = Case(*dims, seed=sum(dims))
    c.check(refcpu, c.run(gpu_ctx))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, False), (True, True)])
def test_ragged_padded_layouts(gpu_ctx, refcpu, ta, tb, offset):
    """Ragged over the tile edges in every layout, padded leading dimensions and strides; offset 1: no 16-byte alignment."""
    c = Case(7, 65, 130, 48, ta, tb, pad_ld=3, pad_stride=5, offset=offset, seed=11 + 2 * ta + tb)
    c.check(refcpu, c.run(gpu_ctx))


@pytest.mark.parametrize("share", ["a", "b"])
def test_shared_operand(gpu_ctx, refcpu, share):
    c = Case(4, 96, 96, 40, share_a=share == "a", share_b=share == "b", seed=5)
    c.check(refcpu, c.run(gpu_ctx))


def test_accumulate_and_bias(gpu_ctx, refcpu):
    c = Case(6, 70, 40, 33, accumulate=True, bias=True, seed=9)
    c.check(refcpu, c.run(gpu_ctx))


def same_bits_as_single_calls(ctx, c, got):
    """Item b of the batch has the bits of a batch-1 call on its pointers."""
    batch, M, N, K = c.dims
    da, db = dev(ctx, c.a), dev(ctx, c.b)
    for i in range(batch):
        dc = dev(ctx, np.full(M * c.ldc, POISON, dtype=np.float32))
        ops.sgemm_batched(ctx, 1, M, N, K, da.ptr + 4 * i * c.stride_a, c.lda, c.stride_a, db.ptr + 4 * i * c.stride_b, c.ldb,
                          c.stride_b, dc, c.ldc, c.stride_c)
        one = dc.read().reshape(M, c.ldc)[:, :N]
        assert np.array_equal(one.view(np.uint32), np.ascontiguousarray(c.c_item(got, i)).view(np.uint32)), i


def test_bits_do_not_depend_on_the_batch(gpu_ctx, refcpu):
    """The same call twice gives the same bits, and item b of a batch has the bits of a batch-1 call on its pointers."""
    c = Case(9, 130, 70, 90, seed=3)
    first, second = c.run(gpu_ctx), c.run(gpu_ctx)
    c.check(refcpu, first)
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))
    same_bits_as_single_calls(gpu_ctx, c, first)


@pytest.mark.parametrize("dims", [(3, 128, 64, 128), (5, 130, 72, 160)])
def test_stores_through_lds(gpu_ctx, dims):
    """K >= 128 with 16-byte aligned items and N a multiple of 4: whole tiles leave through LDS as 16-byte stores (the
    first shape: every tile; the second: two of six, the others ragged).  Strides padded by 4 keep the alignment, and the
    poisoned padding must come back untouched.  Against the float64 product only: an in-order float32 sum of K <= 160
    products whose partial sums stay near max|C| is off by about sqrt(K) * 2^-24 of it, 8e-7, an order below TOL."""
    c = Case(*dims, pad_stride=4, seed=sum(dims))
    got = c.run(gpu_ctx)
    c.check(None, got, oracle=False)
    same_bits_as_single_calls(gpu_ctx, c, got)


def test_more_items_than_one_launch(gpu_ctx):
    """2^22 + 5 items of 1 x 1 x 1: one launch holds 2^22 blocks, so the last five items run in a second one.  A single
    float32 product is correctly rounded, so every item is compared exactly."""
    n = (1 << 22) + 5
    rng = np.random.default_rng(22)
    a, b = (rng.random(n, dtype=np.float32) - np.float32(0.5) for _ in range(2))
    da, db, dc = dev(gpu_ctx, a), dev(gpu_ctx, b), dev(gpu_ctx, np.full(n + 3, POISON, dtype=np.float32))
    ops.sgemm_batched(gpu_ctx, n, 1, 1, 1, da, 1, 1, db, 1, 1, dc, 1, 1)
    got = dc.read()
    assert np.array_equal(got[:n], a * b) and np.all(got[n:] == POISON)


@pytest.mark.parametrize("with_bias", [False, True])
def test_empty_k_writes_bias_or_zeros(gpu_ctx, with_bias):
    """K == 0 with NULL A and B, not accumulating: every item becomes the bias row, or zeros."""
    batch, M, N = 3, 33, 20
    bias = (np.arange(N, dtype=np.float32) - 7) / 4
    dc, dbias = dev(gpu_ctx, np.full(batch * M * N + 5, POISON, dtype=np.float32)), dev(gpu_ctx, bias)
    null = ctypes.c_void_p(0)
    rc = _lib.lib().eg_sgemm_batched(gpu_ctx.handle, 0, 0, batch, M, N, 0, null, 1, 0, null, N, 0, ctypes.c_void_p(dc.ptr), N, M * N, 0,
                                     ctypes.c_void_p(dbias.ptr) if with_bias else null)
    assert rc == 0, _lib.last_error()
    got = dc.read()
    want = np.tile(bias if with_bias else np.zeros(N, dtype=np.float32), batch * M)
    assert np.array_equal(got[:batch * M * N], want) and np.all(got[batch * M * N:] == POISON)


def test_error_returns(gpu_ctx):
    fn = _lib.lib().eg_sgemm_batched
    buf = gpu_ctx.allocTensor((4 * 8 * 8,))
    p = ctypes.c_void_p(buf.ptr)
    null = ctypes.c_void_p(0)

    def call(batch, stride_c, a):
        return fn(gpu_ctx.handle, 0, 0, batch, 8, 8, 8, a, 8, 64, p, 8, 64, p, 8, stride_c, 0, null)

    for args in ((4, 63, p), (-1, 64, p), (4, 64, null)):   # items of C overlap, negative batch, NULL A
        assert call(*args) == EG_ERR_INVALID
        assert "eg_sgemm_batched" in _lib.last_error()
    assert call(0, 64, p) == 0
