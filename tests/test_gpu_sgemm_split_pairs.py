"""eg_sgemm's split-bf16 product with two terms per v_mfma_f32_16x16x32_bf16 (kernels/gemm_split_bf16.hip): lane groups
0-1 and 2-3 of one instruction carry different term pairs of the same 16 k, so products of very different size meet in
one instruction's 32-long sum.  Operands scaled over a wide exponent range, in all four layouts with bias and
accumulate: error against float64 within 1e-5 and within 1.5x the exact path's, row by row, and repeated runs identical
to the bit."""
import numpy as np
import pytest

from exprgrad_amd import ops
from conftest import TOL, rel_err

pytestmark = pytest.mark.gpu


def dev(ctx, arr):
    t = ctx.allocTensor(arr.shape)
    t.write(arr)
    return t


def _scaled(rng, shape, scales):
    """U[-1, 1) times a power of two per index of every axis listed in `scales` ({axis: exponent range})."""
    x = (2 * rng.random(shape, dtype=np.float32) - 1).astype(np.float32)
    for axis, e in scales.items():
        f = np.exp2(rng.integers(-e, e + 1, size=shape[axis])).astype(np.float32)
        x = x * (f[:, None] if axis == 0 else f[None, :])
    return x.astype(np.float32)


def _run(ctx, monkeypatch, split, M, N, K, da, lda, db, ldb, dc, ta, tb, base, dbias):
    if split:
        monkeypatch.delenv("EG_NO_SPLIT_GEMM", raising=False)
    else:
        monkeypatch.setenv("EG_NO_SPLIT_GEMM", "1")
    if base is not None:
        dc.write(base)
    ops.sgemm(ctx, M, N, K, da, lda, db, ldb, dc, N, trans_a=ta, trans_b=tb, accumulate=base is not None, bias=dbias)
    return dc.read()


def _row_errs(got, a, b, rows, ta, tb, base, bias):
    """Error of each sampled row against float64, relative to that row's largest value (rows differ by up to 2^40)."""
    want = (a.T if ta else a).astype(np.float64)[rows] @ (b.T if tb else b).astype(np.float64)
    if base is not None:
        want = want + base[rows].astype(np.float64)
    if bias is not None:
        want = want + bias.astype(np.float64)
    return np.array([rel_err(got[r], w, "split-bf16 pairs against float64, one row") for r, w in zip(rows, want)])


@pytest.mark.parametrize("mode", ["nn", "nt", "tn", "tt"])
@pytest.mark.parametrize("extras", ["plain", "bias_accumulate"])
def test_wide_exponent_range_in_four_layouts(gpu_ctx, monkeypatch, mode, extras):
    """Rows of op(A) and columns of op(B) scaled by 2^-20 .. 2^20, and k scaled by 2^-20 .. 2^20 on the A side, so one
    instruction's sum holds products 2^40 apart.  4096 x 4096 x 2048 is inside the split gate in every layout."""
    ta, tb = mode[0] == "t", mode[1] == "t"
    M = N = 4096
    K = 2048
    rng = np.random.default_rng(17 + 2 * "nn nt tn tt".split().index(mode) + (extras == "plain"))
    opa = _scaled(rng, (M, K), {0: 20, 1: 20})      # op(A): rows and k
    opb = _scaled(rng, (K, N), {1: 20})             # op(B): columns
    a = np.ascontiguousarray(opa.T) if ta else opa
    b = np.ascontiguousarray(opb.T) if tb else opb
    bias = base = dbias = None
    if extras == "bias_accumulate":
        bias = _scaled(rng, (1, N), {1: 20})[0]
        base = _scaled(rng, (M, N), {0: 20, 1: 20})
        dbias = dev(gpu_ctx, bias)
    da, db, dc = dev(gpu_ctx, a), dev(gpu_ctx, b), gpu_ctx.allocTensor((M, N))
    args = (M, N, K, da, a.shape[1], db, b.shape[1], dc, ta, tb, base, dbias)
    split = _run(gpu_ctx, monkeypatch, True, *args)
    again = _run(gpu_ctx, monkeypatch, True, *args)
    exact = _run(gpu_ctx, monkeypatch, False, *args)
    assert np.array_equal(split, again)
    assert not np.array_equal(split, exact)
    rows = np.sort(rng.choice(M, size=24, replace=False))
    e_split = _row_errs(split, a, b, rows, ta, tb, base, bias)
    e_exact = _row_errs(exact, a, b, rows, ta, tb, base, bias)
    assert e_split.max() <= TOL, e_split.max()
    assert e_split.max() <= 1.5 * e_exact.max(), (e_split.max(), e_exact.max())
