"""eg_sgemm and eg_dgemm on strided views: padded leading dimensions, bases off their alignment, poison around every view.

The cases are those of tests/gemm_view_cases.py (which says how the buffers are laid out and where the bounds come from);
tests/test_gemm_view_plan_cpu.py states which routes, second passes and load / store forms of the float32 planner they
reach.  Every case uploads its three allocations, passes pointers into them, reads the WHOLE C allocation back and
checks: nothing outside the M x N view changed by a bit, no NaN came in from behind an operand's rows or from C's own
start values, and the view holds the float64 product within the project's bounds.

Every float32 case runs under EG_NO_SPLIT_GEMM=1: the exact path is what the table is about, whatever the shape.  The
split-bf16 path has one test of its own at the end.
"""
import ctypes

import numpy as np
import pytest

import gemm_view_cases as views
from exprgrad_amd import _lib, ops
from conftest import TOL, rel_err

pytestmark = pytest.mark.gpu

F32 = views.f32_table()
F64 = views.f64_table()
F32_BY_NAME = {c.name: c for c in F32}
F64_BY_NAME = {c.name: c for c in F64}


def call(ctx, c):
    """The case's call on fresh device buffers; returns the whole C allocation as it is afterwards."""
    c.build()
    hosts = [c.a, c.b, c.c0] + ([c.bias_buf] if c.bias else [])
    bufs = []
    for h in hosts:
        bufs.append(ctx.allocBuffer(h.nbytes))
        assert bufs[-1].ptr % 16 == 0
        bufs[-1].write(h)
    item = c.dtype.itemsize
    M, N, K = c.dims
    pa, pb, pc = bufs[0].ptr + item * c.a_start, bufs[1].ptr + item * c.b_start, bufs[2].ptr + item * c.c_start
    pbias = bufs[3].ptr + item * c.bias_start if c.bias else None
    if c.dtype == np.float32:
        ops.sgemm(ctx, M, N, K, pa, c.lda, pb, c.ldb, pc, c.ldc, c.ta, c.tb, c.accumulate, pbias)
    else:
        _lib.call("eg_dgemm", ctx.handle, int(c.ta), int(c.tb), M, N, K, ctypes.c_void_p(pa), c.lda, ctypes.c_void_p(pb), c.ldb,
                  ctypes.c_void_p(pc), c.ldc, int(c.accumulate), ctypes.c_void_p(pbias) if c.bias else None)
    got = bufs[2].read(c.dtype)
    for b in bufs:
        b.dealloc()
    return got


def set_env(monkeypatch, c):
    if c.dtype == np.float32:
        monkeypatch.setenv("EG_NO_SPLIT_GEMM", "1")
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("name", [c.name for c in F32])
def test_sgemm_on_a_view(gpu_ctx, monkeypatch, name):
    c = F32_BY_NAME[name]
    set_env(monkeypatch, c)
    try:
        c.check(call(gpu_ctx, c))
    finally:
        c.release()


@pytest.mark.parametrize("name", [c.name for c in F64])
def test_dgemm_on_a_view(gpu_ctx, monkeypatch, name):
    c = F64_BY_NAME[name]
    set_env(monkeypatch, c)
    try:
        c.check(call(gpu_ctx, c))
    finally:
        c.release()


# one padded call per kind of second pass (and the routes without one), twice: a fixed order of summation
DETERMINISTIC = ["1024x1024x256-NN-a",           # pair, no second pass
                 "144x128x8192-TN-a",            # split_reduce, fewer slices on the last tile row
                 "784x512x8192-TN-f",            # split_reduce behind the extra rows
                 "64x200x8192-NN-a",             # split_reduce where the tight call takes the tree
                 "4352x4100x257-NT-a",           # tail_reduce
                 "1792x1792x512-NT-f",           # streamk_fixup
                 "tile2-slices4-130x70x1027-TN-even", "default-64x48x40000-NN"]     # dgemm_reduce_kernel


@pytest.mark.parametrize("name", DETERMINISTIC)
def test_the_same_padded_call_twice_gives_the_same_bits(gpu_ctx, monkeypatch, name):
    c = F32_BY_NAME.get(name) or F64_BY_NAME[name]
    set_env(monkeypatch, c)
    try:
        first, second = call(gpu_ctx, c), call(gpu_ctx, c)
        c.check_outside(first)
        assert np.array_equal(first.view(np.uint8), second.view(np.uint8))
    finally:
        c.release()


@pytest.mark.parametrize("name", [c.name for c in F32 if c.kind == "a"])
def test_aligned_padding_changes_no_bit_of_the_result(gpu_ctx, monkeypatch, name):
    """Layout (a) against the tight call on the same values: the same plan (tests/test_gemm_view_plan_cpu.py), so the same
    order of summation and the same bits.  The exception is a product whose tight call folds its slabs with the tree sum
    (it needs ldc == N): padded, the same slabs are added one after the other by gemm_splitk_reduce_kernel.  Both are
    within TOL * scale of the float64 product (test_sgemm_on_a_view holds the padded call to it, test_gpu_ops.py the
    tight one), so they are within twice that of each other — and that is all that can be said of two orders of one sum."""
    c = F32_BY_NAME[name]
    t = c.tight()
    set_env(monkeypatch, c)
    try:
        padded, tight = c.interior(call(gpu_ctx, c)), t.interior(call(gpu_ctx, t))
        assert np.array_equal(c.a_vals, t.a_vals) and np.array_equal(c.b_vals, t.b_vals)
        M, N, K = c.dims
        if not c.tree_when_tight:
            assert np.array_equal(padded.view(np.uint32), tight.view(np.uint32)), name
        else:
            scale = max(float(np.abs(c.want()).max()), 0.25 * np.sqrt(K) * 0.3)
            assert np.abs(padded.astype(np.float64) - tight).max() <= 2 * TOL * scale, name
    finally:
        c.release()
        t.release()


def test_split_bf16_product_on_a_padded_view(gpu_ctx, monkeypatch):
    """4096 x 4096 x 2048 NN, the smallest product inside the split path's gate, with lda, ldb, ldc padded by 4, 4, 8 and
    aligned bases: the split pass reads A and B through lda and ldb (NaN behind every row: an element read from there
    either reaches C or makes the product stand down), the product kernel stores through ldc.  The padding of C exactly;
    64 fixed rows against the float64 product within TOL, the bound of tests/test_gpu_sgemm_split.py; different bits than the
    exact path (it did run).  Padded by 3 the same call is outside the gate (gemm_split_bf16.hip: lda % 4, ldc % 4): the
    bits of the exact path, and the padding untouched again."""
    M = N = 4096
    K = 2048
    rows = (np.arange(64) * 67 + 5) % M

    def case(pad):
        return views.ViewCase("split-4096x4096x2048-NN-pad%d" % pad[0], np.float32, M, N, K, pad=pad, bias=True, seed=41)

    def rows_error(c, got):
        want = c.a_vals[rows].astype(np.float64) @ c.b_vals.astype(np.float64) + c.bias_vals
        return rel_err(c.interior(got)[rows], want, "split-bf16 product on a padded view against float64")

    c = case((4, 4, 8))
    monkeypatch.delenv("EG_NO_SPLIT_GEMM", raising=False)
    split = call(gpu_ctx, c)
    monkeypatch.setenv("EG_NO_SPLIT_GEMM", "1")
    exact = call(gpu_ctx, c)
    c.check_outside(split)
    c.check_outside(exact)
    assert np.isfinite(c.interior(split)).all()
    assert not np.array_equal(c.interior(split), c.interior(exact))
    e_split, e_exact = rows_error(c, split), rows_error(c, exact)
    print("split-bf16 on a padded view: error %.3g, exact path %.3g" % (e_split, e_exact))
    assert e_split <= TOL and e_exact <= TOL
    c.release()

    c = case((3, 3, 3))
    exact = call(gpu_ctx, c)
    monkeypatch.delenv("EG_NO_SPLIT_GEMM")
    default = call(gpu_ctx, c)
    c.check_outside(default)
    assert np.array_equal(default.view(np.uint32), exact.view(np.uint32))
    assert rows_error(c, default) <= TOL
    c.release()
