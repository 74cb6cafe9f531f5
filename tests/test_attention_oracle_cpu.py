"""The reference of tests/test_gpu_attention_rows.py, checked on the CPU with the oracle alone: for every forward shape and
for the training step, on inputs U[-0.5, 0.5), the oracle's float32 arithmetic (oracle/kd.py) is within 5e-6 of the float64
shadow of the same kernel list, relative to the tensor's largest value — half of the 1e-5 the device is held to against
either, so the direct gate of tests/parity.py needs no allow-list entry.  The row sums add at most 257 like-signed exp terms
of magnitude ~1: a sequential float32 sum of n such terms is off by at most about n * 2^-25 of its value, 7.7e-6 at the
very worst and a fraction of that with rounding errors of both signs.  A case that missed the bound would get another seed,
never a wider bound."""
import numpy as np
import pytest

import attention_programs as ap
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


@pytest.mark.parametrize("shape", ap.FORWARD_SHAPES + [ap.RANK3_SHAPE])
def test_forward_oracle_within_5e6_of_float64(shape):
    ref, exact = both(ap.softmax_forward if len(shape) == 4 else ap.softmax_forward_rank3)
    s = u(np.random.default_rng(sum(shape)), *shape)
    worst = distance(ref.call("out", {"s": s}), exact.call("out", {"s": s}))
    print(shape, "oracle vs float64", worst)
    assert worst <= ORACLE_OWN, (shape, worst)


def test_training_step_oracle_within_5e6_of_float64():
    B, H, I, J, K, D = ap.TRAINING_SHAPE
    ref, exact = both(ap.attention_training(*ap.TRAINING_SHAPE))
    rng = np.random.default_rng(2)
    for tid in sorted(ref.params):
        v = u(rng, *ref.params[tid].shape)
        ref.params[tid][...] = v
        exact.params[tid][...] = v
    labels = {"labels": u(rng, B, I, H, D)}
    assert distance(ref.call("out", {}), exact.call("out", {})) <= ORACLE_OWN
    ref.run_backward("fit", labels)
    exact.run_backward("fit", labels)
    for ptid, gtid in ref.param_grads("fit"):
        worst = distance(ref.last[gtid], exact.last[gtid])
        print("gradient of parameter", ptid, "oracle vs float64", worst)
        assert worst <= ORACLE_OWN, (ptid, worst)
