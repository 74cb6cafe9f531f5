"""Shapes, operands and the closed form for eg_attention_grad_f64 (tests/test_gpu_attention_grad_f64.py on the device,
tests/test_attention_grad_f64_cases_cpu.py without one).  DIMS is attention_f64_cases.DIMS (one shape per pair of padded head sizes;
the last takes the step of 32) plus many query tiles over one partial key tile, which only the dK/dV loop walks, and D = 1 over four
key tiles.  1x1x1x1x1x1 is not among them: its dQ and dK are exactly 0, and `rel` divides by the largest element."""
import numpy as np

from attention_f64_cases import DIMS as FORWARD_DIMS, SCALE, TOL64, ident, random_operands, rel     # noqa: F401 (for the tests)

DIMS = FORWARD_DIMS + [(1, 1, 200, 7, 8, 40), (3, 2, 7, 200, 33, 1)]


def operands(dims, shared=False):
    """(q, k, v, d_out): attention_f64_cases.random_operands and a U[-0.5, 0.5) d_out [b0, b1, I, D] from a fixed seed"""
    b0, b1, I, J, K, D = dims
    return random_operands(dims, shared=shared) + (np.random.default_rng(2000 + sum(dims)).random((b0, b1, I, D)) - 0.5,)


def closed_form(q, k, v, d_out, scale, dtype):
    """(dq, dk, dv) by the formulas of include/exprgrad_hip.h, as einsums in `dtype`; k and v may have extent 1 along batch0"""
    q, k, v, d_out = (np.asarray(x, dtype) for x in (q, k, v, d_out))
    k, v = np.broadcast_to(k, q.shape[:2] + k.shape[2:]), np.broadcast_to(v, q.shape[:2] + v.shape[2:])
    e = np.exp(np.einsum("abik,abjk->abij", q, k) * dtype(scale))
    p = e / e.sum(-1, keepdims=True)
    o = np.einsum("abij,abjd->abid", p, v)
    delta = np.einsum("abid,abid->abi", d_out, o)[..., None]
    ds = dtype(scale) * p * (np.einsum("abid,abjd->abij", d_out, v) - delta)
    return np.einsum("abij,abjk->abik", ds, k), np.einsum("abij,abik->abjk", ds, q), np.einsum("abij,abid->abjd", p, d_out)
