"""What tests/attention_exact_cases.py claims, proved on the CPU for every case tests/test_gpu_attention_heads.py runs; no
kernel is touched.  A case is admitted here, never by what a kernel gives on it:

  - every sum of the derivation (O, delta, dP, dP - delta, dQ, dK, dV, the selector's scores) adds terms that are whole
    multiples of a common last bit, and the sum of their absolute values stays below 2^24 of those units: every partial
    sum, in any order, is a float32 number;
  - the float64 closed form gives the stated values: the mean of V and J, or V[sel] and 1;
  - the formulas in float32, summed first to last and last to first, give the same bits, and they are the expected ones;
  - exp(float32(-1024)) is 0 and exp(float32(0)) is 1."""
import numpy as np
import pytest

import attention_exact_cases as ec
import attention_grad_cases as gc

f32, f64 = np.float32, np.float64
LIMIT = float(1 << 24)
FORWARD, BACKWARD = ec.forward_cases(), ec.backward_cases()
CASES = [("forward-" + name, make) for name, make in FORWARD] + [("backward-" + name, make) for name, make in BACKWARD]
OUTPUTS = ("o", "sums", "dq", "dk", "dv")


@pytest.fixture(params=CASES, ids=[name for name, _ in CASES])
def case(request):
    return request.param[1]()


def test_the_exponential_at_the_two_scores():
    with np.errstate(under="ignore"):
        assert np.exp(f32(-1024.0)) == 0 and np.exp(f32(-1024.0)).dtype == f32
    assert np.exp(f32(0.0)) == 1 and f32(ec.SCALE) * f32(ec.B) == 1024 and ec.power_of_two(int(1 / ec.SCALE))


def test_the_tables_hold_what_the_device_test_needs():
    """each family at a diagonal pair of padded head sizes and at least three mixed ones; ragged J over several key tiles;
    I below and above J; backward J a power of two; a selection that crosses 16-key blocks and 64-key tiles"""
    pad = lambda n: 32 if n <= 32 else 64 if n <= 64 else 128
    for table in ([d for d, _ in ec.UNIFORM_FORWARD], [d for d, _ in ec.UNIFORM_BACKWARD], ec.SELECTOR):
        pairs = {(pad(d[4]), pad(d[5])) for d in table}
        assert any(kp == dp for kp, dp in pairs) and len([1 for kp, dp in pairs if kp != dp]) >= 3, pairs
        assert any(d[2] < d[3] for d in table) and any(d[2] > d[3] for d in table), table
    assert {63, 130, 200} <= {d[3] for d, _ in ec.UNIFORM_FORWARD}
    assert all(ec.power_of_two(d[3]) for d, _ in ec.UNIFORM_BACKWARD) and {16, 64, 128} <= {d[3] for d, _ in ec.UNIFORM_BACKWARD}
    assert any(d[3] % 64 and d[3] > 128 for d in ec.SELECTOR)
    assert any(d[2] <= d[3] for d in ec.SELECTOR)           # the dV-only run exists
    rng = np.random.default_rng(0)
    for I, J in ((65, 130), (200, 63)):
        sel = ec.selection(rng, I, J)
        assert len(set(sel[:min(I, J)])) == min(I, J) and (I < J or set(sel) == set(range(J)))
        assert len(set(sel // 16)) == -(-J // 16) and (J <= 64 or np.any(sel[1:] // 64 != sel[:-1] // 64))


def test_every_sum_stays_below_24_bits(case):
    got = ec.sums_in_units(case)
    print(case.family, case.dims, {name: round(float(np.log2(max(x, 1.0))), 1) for name, x in got.items()}, "bits")
    want = {"scores"} if case.family == "selector" else {"o"}
    if case.d_out is not None and case.want["dq"] is not None:
        want |= {"delta", "dp", "dp-delta", "dq", "dk", "dv"}
    assert set(got) == want
    for name, x in got.items():
        assert x < LIMIT, (case.dims, name, x)


def test_the_closed_form_gives_the_stated_values(case):
    b0, b1, I, J, K, D = case.dims
    d_out = case.d_out if case.d_out is not None else np.zeros((b0, b1, I, D))
    o, sums, dq, dk, dv = gc.closed_form(case.q, case.k, case.v, d_out, ec.SCALE)
    if case.family == "uniform":
        assert not case.q.any() or not case.k.any()
        assert np.all(sums == J)
        mean = np.broadcast_to(case.v.astype(f64).sum(2, keepdims=True) / J, o.shape)
        if ec.power_of_two(J):
            assert np.array_equal(o, mean)
        else:       # p = 1 / J is rounded in float64: the closed form is the mean to float64's precision
            assert np.max(np.abs(o - mean)) <= 2.0 ** -50
        assert np.array_equal(mean.astype(f32), case.want["o"]) and np.all(case.want["sums"] == J)
        if case.d_out is not None:
            assert not (dk if not case.q.any() else dq).any() and (dq if not case.q.any() else dk).any()
    else:
        picked = np.take_along_axis(case.v, case.sel[..., None], axis=2)
        assert np.all(sums == 1) and np.array_equal(o, picked.astype(f64)) and np.all(case.want["sums"] == 1)
        assert np.array_equal(case.want["o"].view(np.uint32), picked.view(np.uint32))
        scores = np.einsum("obik,objk->obij", case.q.astype(f64), case.k.astype(f64))
        c, j = case.sel[..., None].astype(f64), np.arange(J, dtype=f64)
        assert np.array_equal(scores, -ec.B * (c - j) ** 2)
        assert np.all((scores == 0) == (j == c)) and np.all(ec.SCALE * scores[scores != 0] <= -1024)
        if case.d_out is not None and case.want["dq"] is not None:
            assert not dq.any() and not dk.any()
    if case.d_out is not None:
        for name, got in (("dq", dq), ("dk", dk), ("dv", dv)):
            if case.want[name] is not None:
                assert np.array_equal(got, case.want[name].astype(f64)), name           # exact in float32: the cast lost nothing
        assert case.want["dv"].any()


def test_float32_in_two_orders_gives_the_expected_bits(case):
    first, last = ec.evaluate32(case, reverse=False), ec.evaluate32(case, reverse=True)
    for name in OUTPUTS:
        if case.want.get(name) is None:
            continue
        ec.same_values(first[name], last[name], "%s %s first to last against last to first" % (case.dims, name))
        ec.same_values(first[name], case.want[name], "%s %s float32 against the expected value" % (case.dims, name))


def test_same_values_sees_one_bit_and_forgives_the_sign_of_zero():
    a = np.array([1.0, 0.0, -0.0, 3.5], f32)
    ec.same_values(a, np.array([1.0, -0.0, 0.0, 3.5], f32), "zeros")
    with pytest.raises(AssertionError):
        ec.same_values(a, np.array([np.nextafter(f32(1), f32(2)), 0, 0, 3.5], f32), "one bit")
