"""split_pingpong_kernel, the split-bf16 product's default k loop (kernels/gemm_split_bf16.hip: two barriers per k-tile,
the two waves of a SIMD one barrier apart), against split_gemm_kernel in phase (EG_GEMM_NO_SKEW=1), an independent loop
over the same MFMAs on the same accumulators in the same k order: C must agree bit for bit.  The shapes are the smallest
M x N the gate admits, with K = 2048, 2080 and 2112: 128, 130 and 132 k-tiles, so the three-stage ring ends on each of
its stages.  A race in the schedule would show as a digest that differs or does not repeat; the schedule itself is
checked without a GPU in tests/test_split_schedule_cpu.py."""
import hashlib

import numpy as np
import pytest

from exprgrad_amd import ops

pytestmark = pytest.mark.gpu

M = N = 4096
# name -> K, trans_a, bias and accumulate, seed
CASES = {
    "nn_2048": (2048, False, False, 201),
    "nn_2080": (2080, False, False, 202),
    "nn_2112": (2112, False, False, 203),
    "tn_2080": (2080, True, False, 204),
    "nn_2112_bias_acc": (2112, False, True, 205),
}
PLAIN = [name for name in sorted(CASES) if not CASES[name][2]]


def _dev(ctx, arr):
    t = ctx.allocTensor(arr.shape)
    t.write(arr)
    return t


def digest(c):
    return hashlib.sha256(np.ascontiguousarray(c).tobytes()).hexdigest()


class Product:
    def __init__(self, ctx, name):
        self.K, self.ta, extras, seed = CASES[name]
        rng = np.random.default_rng(seed)
        self.a = (2 * rng.random((self.K, M) if self.ta else (M, self.K), dtype=np.float32) - 1).astype(np.float32)
        self.b = (2 * rng.random((self.K, N), dtype=np.float32) - 1).astype(np.float32)
        self.bias = rng.random((N,), dtype=np.float32) if extras else None
        self.base = rng.random((M, N), dtype=np.float32) if extras else None
        self.ctx = ctx
        self.da, self.db = _dev(ctx, self.a), _dev(ctx, self.b)
        self.dbias = _dev(ctx, self.bias) if extras else None
        self.dc = ctx.allocTensor((M, N))

    def launch(self, db=None):
        if self.base is not None:
            self.dc.write(self.base)
        ops.sgemm(self.ctx, M, N, self.K, self.da, self.a.shape[1], db or self.db, N, self.dc, N, trans_a=self.ta,
                  accumulate=self.base is not None, bias=self.dbias)

    def run(self, monkeypatch, no_split=False, no_skew=False, db=None):
        for name, on in (("EG_NO_SPLIT_GEMM", no_split), ("EG_GEMM_NO_SKEW", no_skew)):
            if on:
                monkeypatch.setenv(name, "1")
            else:
                monkeypatch.delenv(name, raising=False)
        self.launch(db)
        return self.dc.read()


@pytest.mark.parametrize("name", sorted(CASES))
def test_default_loop_has_the_in_phase_loops_bits(gpu_ctx, monkeypatch, name):
    p = Product(gpu_ctx, name)
    c = p.run(monkeypatch)
    in_phase = digest(p.run(monkeypatch, no_skew=True))
    exact = p.run(monkeypatch, no_split=True)
    print(name, digest(c), in_phase)
    assert not np.array_equal(c, exact), "the split route did not run"
    assert digest(c) == in_phase


@pytest.mark.parametrize("name", PLAIN)
def test_ten_launches_back_to_back_end_on_the_same_bits(gpu_ctx, monkeypatch, name):
    """No host synchronise between the launches: each prologue runs behind the launch before it."""
    p = Product(gpu_ctx, name)
    first = digest(p.run(monkeypatch))
    for _ in range(10):
        p.launch()
    last = digest(p.dc.read())
    print(name, first, last)
    assert last == first


def test_a_nan_takes_the_exact_kernel_and_the_next_clean_call_the_split_one(gpu_ctx, monkeypatch):
    p = Product(gpu_ctx, "nn_2048")
    clean = digest(p.run(monkeypatch))
    bad = p.b.copy()
    bad[777, 1234] = np.float32(np.nan)
    dbad = _dev(gpu_ctx, bad)
    stood_down = p.run(monkeypatch, db=dbad)
    exact = p.run(monkeypatch, no_split=True, db=dbad)
    assert np.isnan(stood_down).any()
    assert np.array_equal(stood_down, exact, equal_nan=True)
    assert digest(p.run(monkeypatch)) == clean
