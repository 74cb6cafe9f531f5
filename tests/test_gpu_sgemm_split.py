"""eg_sgemm's split-bf16 path (kernels/gemm_split_bf16.hip): large f32 products as six bf16 MFMA terms of an exact
three-way operand split, the device-side fallback to the exact kernel, determinism, the shape gate, and the exact path
under EG_NO_SPLIT_GEMM=1."""
import numpy as np
import pytest

import exprgrad_amd.model as egm
from exprgrad_amd import ops
from conftest import TOL, rel_err
import refcases

pytestmark = pytest.mark.gpu

F32_MAX = np.finfo(np.float32).max


def dev(ctx, arr):
    t = ctx.allocTensor(arr.shape)
    t.write(arr)
    return t


def _set_split(monkeypatch, on):
    if on:
        monkeypatch.delenv("EG_NO_SPLIT_GEMM", raising=False)
    else:
        monkeypatch.setenv("EG_NO_SPLIT_GEMM", "1")


def _run(ctx, monkeypatch, split, M, N, K, da, lda, db, ldb, dc, ta=False, tb=False, base=None, dbias=None):
    _set_split(monkeypatch, split)
    if base is not None:
        dc.write(base)
    ops.sgemm(ctx, M, N, K, da, lda, db, ldb, dc, N, trans_a=ta, trans_b=tb, accumulate=base is not None, bias=dbias)
    return dc.read()


def _err64(got, a, b, rows, ta, tb, base=None, bias=None):
    a64 = (a.T if ta else a).astype(np.float64)[rows]
    b64 = (b.T if tb else b).astype(np.float64)
    want = a64 @ b64
    if base is not None:
        want = want + base[rows].astype(np.float64)
    if bias is not None:
        want = want + bias.astype(np.float64)
    return rel_err(got[rows], want, "split-bf16 product against float64")


@pytest.mark.parametrize("dist", ["u01", "u11"])
def test_split_product_at_4096_meets_the_exact_paths_error(gpu_ctx, monkeypatch, dist):
    """The bench's product (4096^3, U[0,1)) and U[-1,1): error against float64 on sampled rows at most 1e-5 and at most
    1.5x the exact path's on the same inputs; the two results differ (the split path did run) and each repeats to the bit."""
    n = 4096
    rng = np.random.default_rng(2)
    a = rng.random((n, n), dtype=np.float32)
    b = rng.random((n, n), dtype=np.float32)
    if dist == "u11":
        a = (2 * a - 1).astype(np.float32)
        b = (2 * b - 1).astype(np.float32)
    da, db, dc = dev(gpu_ctx, a), dev(gpu_ctx, b), gpu_ctx.allocTensor((n, n))
    split = _run(gpu_ctx, monkeypatch, True, n, n, n, da, n, db, n, dc)
    again = _run(gpu_ctx, monkeypatch, True, n, n, n, da, n, db, n, dc)
    exact = _run(gpu_ctx, monkeypatch, False, n, n, n, da, n, db, n, dc)
    assert np.array_equal(split, again)
    assert not np.array_equal(split, exact)
    rows = np.sort(rng.choice(n, size=32, replace=False))
    e_split, e_exact = _err64(split, a, b, rows, False, False), _err64(exact, a, b, rows, False, False)
    assert e_split <= TOL
    assert e_split <= 1.5 * e_exact, (e_split, e_exact)


@pytest.mark.parametrize("mode", ["nn", "nt", "tn", "tt"])
def test_split_product_in_four_layouts_with_bias_and_accumulate(gpu_ctx, monkeypatch, mode):
    """4096 x 4096 x 2048 and a ragged-free 4096 x 8192 x 2048 are inside the gate in every layout; onto an existing C
    with a bias, against float64 and against the exact path's error."""
    ta, tb = mode[0] == "t", mode[1] == "t"
    rng = np.random.default_rng(5)
    for M, N, K in ((4096, 4096, 2048), (4096, 8192, 2048)):
        a = (rng.random((K, M) if ta else (M, K), dtype=np.float32) - 0.5).astype(np.float32)
        b = (rng.random((N, K) if tb else (K, N), dtype=np.float32) - 0.5).astype(np.float32)
        bias = rng.random((N,), dtype=np.float32)
        base = rng.random((M, N), dtype=np.float32)
        da, db, dbias, dc = dev(gpu_ctx, a), dev(gpu_ctx, b), dev(gpu_ctx, bias), gpu_ctx.allocTensor((M, N))
        args = (M, N, K, da, a.shape[1], db, b.shape[1], dc)
        split = _run(gpu_ctx, monkeypatch, True, *args, ta=ta, tb=tb, base=base, dbias=dbias)
        exact = _run(gpu_ctx, monkeypatch, False, *args, ta=ta, tb=tb, base=base, dbias=dbias)
        assert not np.array_equal(split, exact)
        rows = np.sort(rng.choice(M, size=16, replace=False))
        e_split = _err64(split, a, b, rows, ta, tb, base, bias)
        e_exact = _err64(exact, a, b, rows, ta, tb, base, bias)
        assert e_split <= TOL
        assert e_split <= 1.5 * e_exact, (M, N, K, e_split, e_exact)


@pytest.mark.parametrize("special", ["inf", "nan", "subnormal", "near_max"])
def test_an_operand_that_does_not_split_falls_back_to_the_exact_kernel(gpu_ctx, monkeypatch, special):
    """One element the three bf16 pieces cannot hold: the product kernel stands down on the device and the exact kernel
    behind it runs — the result equals EG_NO_SPLIT_GEMM=1's to the bit (NaN where it has NaN).  A clean call afterwards
    takes the split path again."""
    M = N = 4096
    K = 2048
    rng = np.random.default_rng(9)
    a = (rng.random((M, K), dtype=np.float32) - 0.5).astype(np.float32)
    b = (rng.random((K, N), dtype=np.float32) - 0.5).astype(np.float32)
    value = {"inf": np.inf, "nan": np.nan, "subnormal": 1e-40, "near_max": F32_MAX}[special]
    bad = b.copy()
    bad[777, 1234] = np.float32(value)
    da, db, dbad, dc = dev(gpu_ctx, a), dev(gpu_ctx, b), dev(gpu_ctx, bad), gpu_ctx.allocTensor((M, N))
    split = _run(gpu_ctx, monkeypatch, True, M, N, K, da, K, dbad, N, dc)
    exact = _run(gpu_ctx, monkeypatch, False, M, N, K, da, K, dbad, N, dc)
    assert np.array_equal(split, exact, equal_nan=True)
    clean_split = _run(gpu_ctx, monkeypatch, True, M, N, K, da, K, db, N, dc)
    clean_exact = _run(gpu_ctx, monkeypatch, False, M, N, K, da, K, db, N, dc)
    assert not np.array_equal(clean_split, clean_exact)


@pytest.mark.parametrize("shape", [(2048, 2048, 2048), (3072, 3072, 3072), (4096, 4096, 1024), (4100, 4096, 2048)])
def test_products_outside_the_gate_are_the_exact_paths(gpu_ctx, monkeypatch, shape):
    """Fewer tiles than the chip has CUs, a K too short for the whole-tile launch, ragged rows: bit-identical with and
    without EG_NO_SPLIT_GEMM=1."""
    M, N, K = shape
    rng = np.random.default_rng(M + N + K)
    a = rng.random((M, K), dtype=np.float32)
    b = rng.random((K, N), dtype=np.float32)
    da, db, dc = dev(gpu_ctx, a), dev(gpu_ctx, b), gpu_ctx.allocTensor((M, N))
    split = _run(gpu_ctx, monkeypatch, True, M, N, K, da, K, db, N, dc)
    exact = _run(gpu_ctx, monkeypatch, False, M, N, K, da, K, db, N, dc)
    assert np.array_equal(split, exact)


def test_model_plans_keep_the_exact_path(gpu_ctx, monkeypatch):
    """A compiled model's contraction at a shape inside the gate runs the exact kernel (plans promise bit-identity between
    their variants): the same bits with and without EG_NO_SPLIT_GEMM=1, and the same bits as eg_sgemm's exact path."""
    n = 4096
    rng = np.random.default_rng(3)
    a = rng.random((n, n), dtype=np.float32)
    b = rng.random((n, n), dtype=np.float32)
    model = egm.compile(*refcases.matmul(), gpu=gpu_ctx)
    try:
        _set_split(monkeypatch, True)
        with_split = model.call("c", {"a": a, "b": b})
        _set_split(monkeypatch, False)
        without = model.call("c", {"a": a, "b": b})
    finally:
        model.close()
    assert np.array_equal(with_split, without)
    da, db, dc = dev(gpu_ctx, a), dev(gpu_ctx, b), gpu_ctx.allocTensor((n, n))
    exact = _run(gpu_ctx, monkeypatch, False, n, n, n, da, n, db, n, dc)
    assert np.array_equal(with_split, exact)


@pytest.mark.parametrize("mode", ["nn", "tt"])
def test_exact_path_skew_and_deep_k_loops_still_agree_bit_for_bit(gpu_ctx, monkeypatch, mode):
    """The exact kernel's skewed waves and 32-deep k-tiles at 4096 x 4096 x 2048 (now inside the split gate) under
    EG_NO_SPLIT_GEMM=1: the default, EG_GEMM_NO_SKEW=1 and EG_GEMM_NO_BK32=1 agree to the bit."""
    M = N = 4096
    K = 2048
    ta, tb = mode[0] == "t", mode[1] == "t"
    rng = np.random.default_rng(11)
    a = (rng.random((K, M) if ta else (M, K), dtype=np.float32) - 0.5).astype(np.float32)
    b = (rng.random((N, K) if tb else (K, N), dtype=np.float32) - 0.5).astype(np.float32)
    bias = rng.random((N,), dtype=np.float32)
    base = rng.random((M, N), dtype=np.float32)
    da, db, dbias, dc = dev(gpu_ctx, a), dev(gpu_ctx, b), dev(gpu_ctx, bias), gpu_ctx.allocTensor((M, N))
    outs = []
    for env in ({}, {"EG_GEMM_NO_SKEW": "1"}, {"EG_GEMM_NO_BK32": "1"}):
        for k in ("EG_GEMM_NO_SKEW", "EG_GEMM_NO_BK32"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        outs.append(_run(gpu_ctx, monkeypatch, False, M, N, K, da, a.shape[1], db, b.shape[1], dc, ta=ta, tb=tb, base=base,
                         dbias=dbias))
    for other in outs[1:]:
        assert np.array_equal(outs[0], other)
    rows = np.sort(rng.choice(M, size=16, replace=False))
    assert _err64(outs[0], a, b, rows, ta, tb, base, bias) <= TOL
