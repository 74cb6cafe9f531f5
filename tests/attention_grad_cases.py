"""The shapes of the fused attention backward's tests and their references, computed once per shape and shared:
tests/test_attention_grad_oracle_cpu.py holds the oracle to float64 on them, tests/test_gpu_attention_grad.py the device to
both.  The program is attention_programs.attention_training: q, kk, v parameters -> scores -> scale -> softmax -> context ->
mse, whose `fit` target `derive`s the gradients eg_attention_grad computes in closed form."""
import numpy as np

import attention_programs as ap
import refcases

SCALE = ap.SCALE
# (batch0, batch1, I, J, K, D)
SHAPES = [
    (2, 3, 33, 70, 16, 16),      # the training shape of attention_programs.py
    (1, 1, 1, 1, 1, 1),          # the smallest possible
    (1, 2, 65, 63, 20, 12),      # one row past a tile, one key short of one, ragged K and D
    (2, 1, 64, 64, 64, 64),      # exact tiles
    (1, 2, 130, 129, 128, 128),  # the largest instantiation, three tiles each way
    (3, 2, 7, 200, 33, 1),       # D = 1, K padded to 64, four key tiles
    (1, 1, 200, 7, 8, 40),       # many query tiles over one partial key tile: the dK/dV loop has them, the forward never had
    (1, 2, 65, 64, 40, 72),      # K and D padded differently (64, 128); tests/test_gpu_attention_heads.py has the other pairs
]
IDS = ["x".join(map(str, d)) for d in SHAPES]


def u(rng, *shape):
    return (rng.random(shape, dtype=np.float32) - np.float32(0.5)).astype(np.float32)


def inputs(dims, seed=None):
    """q [b0,b1,I,K], k [b0,b1,J,K], v [b0,b1,J,D], labels [b0,b1,I,D] in U[-0.5, 0.5), item-major as the C ABI sees them"""
    b0, b1, I, J, K, D = dims
    rng = np.random.default_rng(sum(dims) if seed is None else seed)
    return u(rng, b0, b1, I, K), u(rng, b0, b1, J, K), u(rng, b0, b1, J, D), u(rng, b0, b1, I, D)


def closed_form(q, k, v, d_out, scale=SCALE):
    """float64: (o, sums, dq, dk, dv) of the formulas in include/exprgrad_hip.h; an extent of 1 along batch0 in k and v is a
    shared operand, whose gradient is still per item"""
    q, k, v, d_out = (np.asarray(x, np.float64) for x in (q, k, v, d_out))
    k, v = np.broadcast_to(k, q.shape[:2] + k.shape[2:]), np.broadcast_to(v, q.shape[:2] + v.shape[2:])
    e = np.exp(np.einsum("obik,objk->obij", q, k) * np.float64(np.float32(scale)))
    sums = e.sum(-1)
    p = e / sums[..., None]
    o = np.einsum("obij,objd->obid", p, v)
    delta = np.einsum("obid,obid->obi", d_out, o)
    dp = np.einsum("obid,objd->obij", d_out, v)
    ds = np.float64(np.float32(scale)) * p * (dp - delta[..., None])
    return o, sums, np.einsum("obij,objk->obik", ds, k), np.einsum("obij,obik->objk", ds, q), np.einsum("obij,obid->objd", p, d_out)


def mse_gradient(o, labels):
    """what the mse of the training program hands back for the context, in float32 on the host: 2 (o - labels) / N, with N the
    mse's divisor — layers.mse divides the sum of squares by the leading extent, batch0"""
    return (np.float32(2.0) * (o.astype(np.float32) - labels) / np.float32(labels.shape[0])).astype(np.float32)


_RUNS = {}


def oracle_run(dims, seed=None):
    """The training program on `inputs(dims, seed)` through the oracle and its float64 shadow, once per (dims, seed):
    {"f32" / "f64": {"out", "q", "kk", "v"}} with the context and the gradients of the three parameters, transposed from the
    oracle's [B,.,H,.] to item-major [b0,b1,.,.]."""
    key = (dims, seed)
    if key not in _RUNS:
        from oracle import kd
        q, k, v, labels = inputs(dims, seed)
        text = refcases.program_text(ap.attention_training(*dims)())
        t = lambda x: np.ascontiguousarray(x.transpose(0, 2, 1, 3))
        res = {}
        for which, model in (("f32", kd.Model(text, threads=4)), ("f64", kd.Model(text, shadow=True))):
            names = {model.prog.tensors[tid]["name"]: tid for tid in model.params}
            for name, x in (("q", q), ("kk", k), ("v", v)):
                model.params[names[name]][...] = t(x)
            r = {"out": np.asarray(model.call("out", {})).transpose(0, 2, 1, 3).copy()}
            model.run_backward("fit", {"labels": t(labels)})
            grads = dict(model.param_grads("fit"))
            for name in ("q", "kk", "v"):
                r[name] = np.asarray(model.last[grads[names[name]]]).transpose(0, 2, 1, 3).copy()
            res[which] = r
        _RUNS[key] = res
    return _RUNS[key]
