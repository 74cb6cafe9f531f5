"""The reference of tests/test_gpu_attention_fused.py, checked on the CPU with the oracle alone: on every shape where the
device is compared with the oracle running the five-statement program (tests/attention_fused_programs.py), inputs
U[-0.5, 0.5), the oracle's float32 arithmetic is within 5e-6 of the float64 shadow of the same kernel list, relative to the
output's largest value — half of the 1e-5 the device is held to against either.  The row sums add at most 200 like-signed exp
terms near 1 (sequential float32: at most about n * 2^-25 of the value, 6e-6 at the very worst, a fraction of it with
rounding errors of both signs); the products add at most 200 terms.  J = 4100 is not here: the device is compared with
float64 only at that width.  A case that missed the bound would get another seed, never a wider bound."""
import numpy as np
import pytest

import attention_fused_programs as fp
import refcases

ORACLE_OWN = 5e-6


def u(rng, *shape):
    return (rng.random(shape, dtype=np.float32) - np.float32(0.5)).astype(np.float32)


def both(graphs):
    from oracle import kd
    text = refcases.program_text(graphs())
    return kd.Model(text, threads=4), kd.Model(text, shadow=True)


def distance(got, exact):
    exact = np.asarray(exact, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - exact)) / np.max(np.abs(exact)))


def inputs(shape, seed):
    B, H, I, J, K, D = shape
    rng = np.random.default_rng(seed)
    return {"q": u(rng, B, I, H, K), "kk": u(rng, B, J, H, K), "v": u(rng, B, J, H, D)}


@pytest.mark.parametrize("shape", fp.ORACLE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_oracle_within_5e6_of_float64(shape):
    ref, exact = both(fp.attention_forward())
    x = inputs(shape, sum(shape))
    worst = distance(ref.call("out", x), exact.call("out", x))
    print(shape, "oracle vs float64", worst)
    assert worst <= ORACLE_OWN, (shape, worst)


@pytest.mark.parametrize("graphs,scale", [(fp.attention_forward_unscaled, 1.0), (fp.attention_forward_scale_first, fp.SCALE)], ids=["unscaled", "scale_first"])
def test_the_other_spellings_of_the_scale(graphs, scale):
    """the program without a scale and with `scale * s`: the oracle against float64 numpy"""
    shape = (2, 3, 33, 70, 16, 16)
    ref, exact = both(graphs)
    x = inputs(shape, 3)
    got = ref.call("out", x)
    assert distance(got, exact.call("out", x)) <= ORACLE_OWN
    q, kk, v = (x[n].astype(np.float64) for n in ("q", "kk", "v"))
    e = np.exp(np.einsum("bihk,bjhk->bhij", q, kk) * np.float64(np.float32(scale)))
    want = np.einsum("bhij,bjhd->bihd", e / e.sum(-1, keepdims=True), v)
    assert distance(got, want) <= ORACLE_OWN
