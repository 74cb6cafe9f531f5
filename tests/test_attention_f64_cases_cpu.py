"""What tests/attention_f64_cases.py claims, proved on the CPU for every case tests/test_gpu_attention_f64.py runs; no kernel
is touched.  A case is admitted here, never by what a kernel gives on it:

  - every sum of the derivation (the uniform family's O, the selector's scores) adds terms that are whole multiples of a
    common last bit, and the sum of their absolute values stays below 2^53 of those units: every partial sum, in any order,
    is a float64 number;
  - the closed form gives the stated values: the correctly rounded mean of V (the division held to exact rationals on a
    sample of elements) and J, or V[sel] and 1;
  - the three-statement program in float64, summed first to last and last to first, gives the same bits, and they are the
    expected ones;
  - the double exp(-1024) is 0 and exp(0) is 1."""
from fractions import Fraction

import numpy as np
import pytest

import attention_f64_cases as ec

f64 = np.float64
LIMIT = float(1 << 53)
CASES = ec.forward_cases()


@pytest.fixture(params=CASES, ids=[name for name, _ in CASES])
def case(request):
    return request.param[1]()


def test_the_exponential_at_the_two_scores():
    with np.errstate(under="ignore"):
        assert np.exp(f64(-1024.0)) == 0 and np.exp(f64(-1024.0)).dtype == f64
        assert np.exp(f64(-745.2)) == 0 and np.exp(f64(-744.0)) > 0      # -1024 is far inside the range that gives 0
    assert np.exp(f64(0.0)) == 1 and f64(ec.SCALE) * f64(ec.B) == 1024 and f64(ec.SCALE) == 2.0 ** -2


def test_the_table_holds_what_the_device_test_needs():
    """all nine pairs of padded head sizes once; K, D, I, J and the batch from the sets of the header; J ragged across key
    tiles of 32 and of 64; I below and above J"""
    assert sorted((ec.padded(d[4]), ec.padded(d[5])) for d in ec.DIMS) == [(kp, dp) for kp in (32, 64, 128) for dp in (32, 64, 128)]
    assert {d[4] for d in ec.DIMS} == {20, 33, 65, 32, 64, 128} and {d[5] for d in ec.DIMS} == {12, 33, 65, 32, 64, 128}
    assert {d[2] for d in ec.DIMS} == {33, 65, 70} and {d[3] for d in ec.DIMS} == {31, 33, 63, 65, 130}
    assert {d[:2] for d in ec.DIMS} == {(1, 2), (2, 1)}
    assert all(d[3] % 32 and d[3] % 64 for d in ec.DIMS) and any(d[3] > 64 for d in ec.DIMS) and any(d[3] < 32 for d in ec.DIMS)
    assert any(d[2] < d[3] for d in ec.DIMS) and any(d[2] > d[3] for d in ec.DIMS)
    rng = np.random.default_rng(0)
    for I, J in ((65, 130), (70, 31)):
        sel = ec.selection(rng, I, J)
        assert len(set(sel[:min(I, J)])) == min(I, J) and (I < J or set(sel) == set(range(J)))


def test_the_operands_are_what_the_header_says(case):
    b0, b1, I, J, K, D = case.dims
    assert case.q.dtype == f64 and case.k.dtype == f64 and case.v.dtype == f64
    if case.family == "uniform":
        assert (not case.q.any()) != (not case.k.any())
        assert np.all(np.abs(case.v) <= 1) and np.array_equal(case.v * ec.G, np.rint(case.v * ec.G)) and len(np.unique(case.v)) > case.v.size // 2
    else:       # 53-bit significands: the last fraction bit is set in about half of V, the exponent is that of [1, 2)
        bits = case.v.view(np.uint64)
        assert np.all((np.abs(case.v) >= 1) & (np.abs(case.v) < 2)) and 0.4 < np.mean(bits & np.uint64(1)) < 0.6
        assert 0.4 < np.mean(case.v < 0) < 0.6


def test_every_sum_stays_below_53_bits(case):
    got = ec.sums_in_units(case)
    print(case.family, case.dims, {name: round(float(np.log2(max(x, 1.0))), 1) for name, x in got.items()}, "bits")
    assert set(got) == ({"scores"} if case.family == "selector" else {"o"})
    for name, x in got.items():
        assert x < LIMIT, (case.dims, name, x)


def test_the_closed_form_gives_the_stated_values(case):
    b0, b1, I, J, K, D = case.dims
    scores = np.einsum("obik,objk->obij", case.q, case.k)        # exact: test_every_sum_stays_below_53_bits
    if case.family == "uniform":
        assert not scores.any() and np.all(case.want["sums"] == J)
        total = case.v.sum(2)                                     # exact, in units of 1 / G
        assert np.array_equal(total, np.rint(total * ec.G) / ec.G)
        assert np.array_equal(case.want["o"], np.broadcast_to((total / f64(J))[:, :, None, :], case.want["o"].shape))
        # the division is the correctly rounded one: a sample of elements against exact rationals
        rng = np.random.default_rng(1)
        for _ in range(64):
            o, i1, d = rng.integers(b0), rng.integers(b1), rng.integers(D)
            exact = Fraction(int(round(total[o, i1, d] * ec.G)), ec.G * J)
            got = float(case.want["o"][o, i1, 0, d])
            lo, hi = np.nextafter(got, -np.inf), np.nextafter(got, np.inf)
            assert abs(Fraction(got) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))
    else:
        c, j = case.sel[..., None].astype(f64), np.arange(J, dtype=f64)
        assert np.array_equal(scores, -ec.B * (c - j) ** 2)
        assert np.all((scores == 0) == (j == c)) and np.all(ec.SCALE * scores[scores != 0] <= -1024)
        picked = np.take_along_axis(case.v, case.sel[..., None], axis=2)
        assert np.array_equal(case.want["o"].view(np.uint64), picked.view(np.uint64)) and np.all(case.want["sums"] == 1)


def test_float64_in_two_orders_gives_the_expected_bits(case):
    first, last = ec.evaluate64(case, reverse=False), ec.evaluate64(case, reverse=True)
    for name in ("o", "sums"):
        ec.same_values(first[name], last[name], "%s %s first to last against last to first" % (case.dims, name))
        ec.same_values(first[name], case.want[name], "%s %s float64 against the expected value" % (case.dims, name))


@pytest.mark.parametrize("dims", ec.DIMS, ids=ec.ident)
def test_plain_float64_stays_within_the_bound_of_the_parity_runs(dims):
    """tests/test_gpu_attention_f64.py compares the device with numpy.longdouble on these operands within TOL64 = 1e-12 of the
    largest element.  The bound is attainable: a plain float64 evaluation of the program stays within a tenth of it, and
    longdouble is the wider type here (64 significand bits against 53)."""
    assert np.finfo(np.longdouble).nmant > np.finfo(f64).nmant
    q, k, v = ec.random_operands(dims)
    (o64, s64), (ol, sl) = ec.program(q, k, v, ec.SCALE, f64), ec.program(q, k, v, ec.SCALE, np.longdouble)
    e_o, e_s = ec.rel(o64, ol), ec.rel(s64, sl)
    print(dims, "float64 vs longdouble: O %.3g Sums %.3g of %g" % (e_o, e_s, ec.TOL64))
    assert e_o <= ec.TOL64 / 10 and e_s <= ec.TOL64 / 10


def test_same_values_sees_one_bit_and_forgives_the_sign_of_zero():
    a = np.array([1.0, 0.0, -0.0, 3.5])
    ec.same_values(a, np.array([1.0, -0.0, 0.0, 3.5]), "zeros")
    with pytest.raises(AssertionError):
        ec.same_values(a, np.array([np.nextafter(1.0, 2.0), 0, 0, 3.5]), "one bit")
