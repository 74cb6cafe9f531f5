"""The references of tests/test_gpu_attention_grad.py, checked on the CPU alone: for every shape of
tests/attention_grad_cases.py the training step of attention_programs.attention_training runs through the oracle
(kd.Model.run_backward("fit", ...), param_grads, last[...]) and through its float64 shadow, on parameters and labels in
U[-0.5, 0.5).  The oracle's context and its gradients of q, kk and v must be within 5e-6 of float64, relative to the tensor's
largest value: the project's condition for holding the device to 1e-5 of either.  A case that missed would get another seed,
never a wider bound.  The closed form the GPU test compares with (attention_grad_cases.closed_form) is held to the float64
shadow as well, at 1e-12: the formulas in the header are the gradients `derive` emits."""
import numpy as np
import pytest

import attention_grad_cases as gc

ORACLE_OWN = 5e-6


def distance(got, exact):
    """relative to the tensor's largest value; a tensor that is exactly zero (one key: p = 1, dS = 0) is held to the bound in
    absolute terms, as conftest.rel_err does"""
    exact = np.asarray(exact, np.float64)
    top = np.max(np.abs(exact))
    return float(np.max(np.abs(np.asarray(got, np.float64) - exact)) / (top if top > 0 else 1.0))


@pytest.mark.parametrize("dims", gc.SHAPES, ids=gc.IDS)
def test_training_step_oracle_within_5e6_of_float64(dims):
    run = gc.oracle_run(dims)
    for name in ("out", "q", "kk", "v"):
        worst = distance(run["f32"][name], run["f64"][name])
        print(dims, name, "oracle vs float64", worst)
        assert worst <= ORACLE_OWN, (dims, name, worst)


@pytest.mark.parametrize("dims", gc.SHAPES, ids=gc.IDS)
def test_closed_form_is_the_derived_gradient(dims):
    q, k, v, labels = gc.inputs(dims)
    exact = gc.oracle_run(dims)["f64"]
    d_out = 2.0 * (exact["out"] - labels.astype(np.float64)) / labels.shape[0]     # layers.mse divides by the leading extent
    o, _, dq, dk, dv = gc.closed_form(q, k, v, d_out)
    for name, got in (("out", o), ("q", dq), ("kk", dk), ("v", dv)):
        worst = distance(got, exact[name])
        print(dims, name, "closed form vs shadow", worst)
        assert worst <= 1e-12, (dims, name, worst)
