"""The split-bf16 product's two k loops (kernels/gemm_split_bf16.hip): the default, split_pingpong_kernel (two barriers
per k-tile, the two waves of a SIMD one barrier apart), and split_gemm_kernel with EG_GEMM_NO_SKEW=1 (one barrier per
k-tile, every wave in phase).  In both every wave issues the same MFMAs on the same accumulators in the same k order, so
C has the bits the kernel had before its waves ever left phase.  tests/golden/split_product_bits.json holds SHA-256
digests of C recorded from that earlier build (its commit id is in the file) for three products inside the gate; they
must come out again in both modes, and at the end of ten launches queued back to back."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from exprgrad_amd import ops
from conftest import TOL, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "split_product_bits.json")

# name -> M, N, K, trans_a, trans_b, inputs on [-1, 1), bias and accumulate, seed
CASES = {
    "nn_4096_u01": (4096, 4096, 4096, False, False, False, False, 101),          # the bench's product
    "tn_4096x8192x2048_u11_bias_acc": (4096, 8192, 2048, True, False, True, True, 102),   # 512 tiles: two rounds of blocks
    "nt_4096x4096x2080": (4096, 4096, 2080, False, True, False, False, 103),    # 130 k-tiles: the stage rotation ends elsewhere
}


def make_inputs(name):
    M, N, K, ta, tb, signed, extras, seed = CASES[name]
    rng = np.random.default_rng(seed)
    a = rng.random((K, M) if ta else (M, K), dtype=np.float32)
    b = rng.random((N, K) if tb else (K, N), dtype=np.float32)
    if signed:
        a = (2 * a - 1).astype(np.float32)
        b = (2 * b - 1).astype(np.float32)
    bias = rng.random((N,), dtype=np.float32) if extras else None
    base = rng.random((M, N), dtype=np.float32) if extras else None
    return a, b, bias, base


def _dev(ctx, arr):
    t = ctx.allocTensor(arr.shape)
    t.write(arr)
    return t


class Product:
    """One case's operands on the device; launch() queues the product and returns without reading anything back."""

    def __init__(self, ctx, name):
        self.M, self.N, self.K, self.ta, self.tb = CASES[name][:5]
        self.a, self.b, self.bias, self.base = make_inputs(name)
        self.ctx = ctx
        self.da, self.db = _dev(ctx, self.a), _dev(ctx, self.b)
        self.dbias = _dev(ctx, self.bias) if self.bias is not None else None
        self.dc = ctx.allocTensor((self.M, self.N))

    def launch(self, dc=None):
        dc = dc or self.dc
        if self.base is not None:
            dc.write(self.base)
        ops.sgemm(self.ctx, self.M, self.N, self.K, self.da, self.a.shape[1], self.db, self.b.shape[1], dc, self.N,
                  trans_a=self.ta, trans_b=self.tb, accumulate=self.base is not None, bias=self.dbias)

    def run(self):
        self.launch()
        return self.dc.read()


def digest(c):
    return hashlib.sha256(np.ascontiguousarray(c).tobytes()).hexdigest()


def _set(monkeypatch, name, on):
    if on:
        monkeypatch.setenv(name, "1")
    else:
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def golden():
    doc = json.load(open(GOLDEN))
    assert set(doc["cases"]) == set(CASES)
    for name, rec in doc["cases"].items():
        assert rec["seed"] == CASES[name][7]
    return doc


def test_every_case_is_inside_the_gates_planner_predicate(tmp_path):
    """exact_single_launch, the part of the gate the planner decides, on the CPU (256 CUs)."""
    exe = str(tmp_path / "gemm_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "exprgrad_amd", "csrc", "kernels", "gemm_plan.cpp"),
                           os.path.join(ROOT, "tests", "gemm_plan_driver.cpp"), "-o", exe])
    lines = []
    for M, N, K, ta, tb, _, extras, _ in CASES.values():
        lda, ldb = (M if ta else K), (K if tb else N)
        lines.append("single %d %d %d %d %d %d %d %d 1 1 1 %d 0 -" % (M, N, K, ta, tb, lda, ldb, N, int(extras)))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["single=1"] * len(CASES), out.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("no_skew", [False, True], ids=["default", "EG_GEMM_NO_SKEW"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_product_has_the_recorded_bits(gpu_ctx, monkeypatch, golden, name, no_skew):
    _set(monkeypatch, "EG_NO_SPLIT_GEMM", False)
    _set(monkeypatch, "EG_GEMM_NO_SKEW", no_skew)
    p = Product(gpu_ctx, name)
    c = p.run()
    got = digest(c)
    print(name, "no_skew=%d" % no_skew, got)
    _set(monkeypatch, "EG_NO_SPLIT_GEMM", True)
    exact = p.run()
    assert not np.array_equal(c, exact), "the split route did not run"
    assert got == golden["cases"][name]["sha256"]
    rng = np.random.default_rng(CASES[name][7] + 1000)
    rows = np.sort(rng.choice(p.M, size=16, replace=False))
    a64 = (p.a.T if p.ta else p.a).astype(np.float64)[rows]
    want = a64 @ (p.b.T if p.tb else p.b).astype(np.float64)
    if p.base is not None:
        want = want + p.base[rows].astype(np.float64) + p.bias.astype(np.float64)
    err = rel_err(c[rows], want, "split-bf16 product against float64")
    print(name, "error against float64", err)
    assert err <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_ten_launches_back_to_back_end_on_the_recorded_bits(gpu_ctx, monkeypatch, golden, name):
    """No host synchronise between the launches: each prologue runs behind the launch before it."""
    _set(monkeypatch, "EG_NO_SPLIT_GEMM", False)
    _set(monkeypatch, "EG_GEMM_NO_SKEW", False)
    p = Product(gpu_ctx, name)
    first = digest(p.run())
    if p.base is None:
        for _ in range(10):
            p.launch()
        last = digest(p.dc.read())
    else:   # an accumulating product starts from its C: ten buffers filled beforehand, then the ten launches
        outs = [_dev(gpu_ctx, p.base) for _ in range(10)]
        outs[-1].read()
        p.base = None
        for t in outs:
            ops.sgemm(gpu_ctx, p.M, p.N, p.K, p.da, p.a.shape[1], p.db, p.b.shape[1], t, p.N, trans_a=p.ta, trans_b=p.tb,
                      accumulate=True, bias=p.dbias)
        last = digest(outs[-1].read())
    print(name, first, last)
    assert first == golden["cases"][name]["sha256"]
    assert last == first
