"""What tests/exact_cases.py claims, on the CPU: its references are the products they stand for, its emulation of the
split-bf16 arithmetic stays within the bound that tests/test_gpu_exact_products.py asserts while every kept term matters to
it, and its table of exact-route cases reaches every route and second pass of tests/golden/gemm_routes.json."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import exact_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (5, 3, 2), (33, 17, 40), (70, 9, 16)]       # M, N, K: M below, at and above K


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_monomial_references_are_the_float64_product(M, N, K, dtype):
    """One nonzero addend per element: the float64 `@` of float32 operands is the exact product, and that of float64
    operands the correctly rounded one (every other addend is an exact zero)."""
    rng = np.random.default_rng(M + N + K)
    opa, k, a = ec.monomial_rows(M, K, rng, dtype)
    opb = ec.values((K, N), rng, dtype)
    assert opa.dtype == dtype and (np.count_nonzero(opa, axis=1) == 1).all()
    assert M < K or set(k) == set(range(K))
    x, y = ec.rows_factors(k, a, opb)
    assert np.array_equal(opa.astype(np.float64) @ opb.astype(np.float64), ec.exact_product(x, y) if dtype == np.float32 else ec.rounded_product(x, y))

    opa = ec.values((M, K), rng, dtype)
    opb, k, b = ec.monomial_cols(K, N, rng, dtype)
    assert (np.count_nonzero(opb, axis=0) == 1).all()
    assert N < K or set(k) == set(range(K))
    x, y = ec.cols_factors(opa, k, b)
    assert np.array_equal(opa.astype(np.float64) @ opb.astype(np.float64), ec.exact_product(x, y) if dtype == np.float32 else ec.rounded_product(x, y))


@pytest.mark.parametrize("dtype,bits", [(np.float32, 24), (np.float64, 53)])
def test_values_use_every_significand_bit_and_products_round_once(dtype, bits):
    rng = np.random.default_rng(1)
    x, y = ec.values(2000, rng, dtype), ec.values(2000, rng, dtype)
    assert ((np.abs(x) >= 1) & (np.abs(x) < 2)).all() and (x < 0).any() and (x > 0).any()
    for v in x[:200]:
        f = abs(Fraction(float(v))) * 2 ** (bits - 1)
        assert f.denominator == 1 and f.numerator % 2 == 1               # an odd integer of `bits` bits: the last bit is in use
    got = ec.rounded_product(x, y)
    assert got.dtype == dtype
    for v, w, g in zip(x[:500], y[:500], got[:500]):                      # fl(xy) against the exact rational product
        p, g = Fraction(float(v)) * Fraction(float(w)), Fraction(float(g))
        ulp = Fraction(2) ** (int(np.floor(np.log2(float(abs(p))))) - bits + 1)
        assert abs(g - p) <= ulp / 2 and (abs(g - p) < ulp / 2 or (g / ulp).numerator % 2 == 0)
    if dtype == np.float64:                                               # the longdouble product is the bounds' stand-in for ab
        exact = ec.exact_product(x, y)
        for v, w, e in zip(x[:200], y[:200], exact[:200]):
            p = Fraction(float(v)) * Fraction(float(w))
            hi = float(e)
            held = Fraction(hi) + Fraction(float(e - np.longdouble(hi)))         # the longdouble's value, exactly
            assert abs(held - p) <= abs(p) * Fraction(2) ** -min(np.finfo(np.longdouble).nmant, 63)   # (53 where longdouble is double)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_grid_reference_is_the_integer_product_in_any_order(dtype):
    rng = np.random.default_rng(2)
    M, N, K = 37, 29, 4096
    opa, opb = ec.grid((M, K), rng, dtype), ec.grid((K, N), rng, dtype)
    assert set(np.unique(opa * 8)) == set(range(-8, 8))
    ia, ib = np.rint(opa * 8).astype(np.int64), np.rint(opb * 8).astype(np.int64)
    want = ia @ ib
    got = ec.grid_reference(opa, opb)
    assert got.dtype == dtype and np.array_equal(got.astype(np.float64) * 64, want)
    perm = rng.permutation(K)
    ec.same_bits(ec.grid_reference(np.ascontiguousarray(opa[:, perm]), np.ascontiguousarray(opb[perm, :])), got, "permuted k")
    # why any order is exact: a partial sum of up to 2^17 products is n / 64 with |n| <= 2^17 * 64 = 2^23, a float32
    for n in (ec.GRID_MAX_K * 64, ec.GRID_MAX_K * 64 - 1, -(ec.GRID_MAX_K * 64 - 1)):
        assert float(np.float32(n / 64.0)) * 64 == n


def _operand_values():
    """The values the GPU test's split cases draw: 2^20 pairs from the generator."""
    rng = np.random.default_rng(3)
    return ec.values(1 << 20, rng), ec.values(1 << 20, rng)


def test_split3_reproduces_every_generated_value():
    a, b = _operand_values()
    for x in (a, b, ec.grid(1 << 16, np.random.default_rng(4)), np.zeros(4, dtype=np.float32)):
        x0, x1, x2 = ec.split3(x)
        assert np.array_equal(x0.astype(np.float64) + x1.astype(np.float64) + x2.astype(np.float64), x.astype(np.float64))
        for piece in (x0, x1, x2):                                      # each piece is a bf16: the low 16 bits are clear
            assert not (piece.view(np.uint32) & np.uint32(0xFFFF)).any()
    g0, g1, g2 = ec.split3(ec.grid(1 << 16, np.random.default_rng(4)))
    assert not g1.any() and not g2.any()                                # grid values sit in plane 0 alone
    # bf16_round is round-to-nearest-even: ties, and a carry into the exponent
    t = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 2.0 - 2.0 ** -9, 1.0 + 2.0 ** -8 + 2.0 ** -23], dtype=np.float32)
    assert ec.bf16_round(t).tolist() == [1.0, 1.0 + 2.0 ** -6, 2.0, 1.0 + 2.0 ** -7]


@pytest.mark.parametrize("wide", [False, True])
def test_the_split_bound_holds_for_six_terms_and_for_no_five(wide):
    """The teeth of the 8-unit bound.  The emulated product stays within it on the generators' own values, whichever way
    the MFMA rounds; with any ONE of the six kept terms left out, more than half of the elements break it.  The second
    half is a condition on the bound, not a measurement: a bound that ever has to move may only move to a value for which
    it still holds (a product kernel that drops a term, pairs the wrong planes or reads a wrong plane 2 must fail)."""
    a, b = _operand_values()
    ab = ec.exact_product(a, b)
    full = ec.six_term_product(a, b, wide=wide)
    off = ec.units_off(full, ab)
    differ = float((full != ec.rounded_product(a, b)).mean())
    print("six terms, wide=%s: at most %.2f units of 2^-24 |ab|; %.1f %% differ from fl(ab)" % (wide, off.max(), 100 * differ))
    assert (np.abs(full.astype(np.float64) - ab) <= ec.split_bound(ab)).all()
    assert 0.02 <= differ <= 0.30           # the split route shows: the GPU test asserts that some element differs from fl(ab)
    for term in ec.TERMS:
        broken = float((np.abs(ec.six_term_product(a, b, drop=term, wide=wide).astype(np.float64) - ab) > ec.split_bound(ab)).mean())
        print("without %s: %.1f %% of the elements exceed the bound" % (term, 100 * broken))
        assert broken > 0.5, term
    with pytest.raises(AssertionError):
        ec.six_term_product(a[:4], b[:4], drop="a1b2")      # not a kept term


def test_six_term_product_of_grid_values_is_exact():
    rng = np.random.default_rng(5)
    a, b = ec.grid(4096, rng), ec.grid(4096, rng)
    assert np.array_equal(ec.six_term_product(a, b), a * b) and np.array_equal((a * b).astype(np.float64), ec.exact_product(a, b))


def test_table_covers_every_route_and_every_second_pass():
    """In the style of test_gemm_plan_cpu.py::test_table_covers_every_route_and_both_verdicts: the cases of
    tests/test_gpu_exact_products.py are rows of tests/golden/gemm_routes.json, which that module holds to the planner, so
    the route each takes is known here.  Every route name and every second-pass kind the fixture holds — in any mode —
    is reached, each (route, second pass) by its smallest row, and every switch a row names has its environment variable."""
    from test_gemm_plan_cpu import ROUTES
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_routes.json")))["cases"]
    table = ec.sgemm_table()
    assert all(c in cases and c["mode"] == "exact" for c in table)
    assert {c["expect"]["route"] for c in table} == {c["expect"]["route"] for c in cases if "route" in c["expect"]} == ROUTES
    assert {c["expect"]["second"] for c in table if "second" in c["expect"]} == {c["expect"]["second"] for c in cases if "second" in c["expect"]}
    assert {"none", "split_reduce", "tail_reduce", "streamk_fixup", "tree"} == {c["expect"].get("second", "none") for c in table}
    assert any(c["expect"].get("tail_tiles", 0) > 0 for c in table)
    assert len({ec.route_id(c) for c in table}) == len(table)
    for c in table:
        key = (c["expect"]["route"], c["expect"].get("second", "none"))
        rivals = [r for r in ec.route_rows() if (r["expect"]["route"], r["expect"].get("second", "none")) == key]
        assert c["M"] * c["N"] * c["K"] == min(r["M"] * r["N"] * r["K"] for r in rivals)
        assert c["K"] <= ec.GRID_MAX_K
        env = ec.switch_env(c["switches"])
        assert len(env) == (0 if c["switches"] == "-" else len(c["switches"].split(",")))
    # every switch word of the fixture is known, and the variables are the library's (csrc/switches.hpp)
    listed = open(os.path.join(ROOT, "exprgrad_amd", "csrc", "switches.hpp")).read()
    words = {w.split("=")[0] for c in cases for w in c["switches"].split(",")} - {"-"}
    assert words <= set(ec.SWITCH_ENV) and all('"%s"' % v in listed for v in ec.SWITCH_ENV.values())
    assert ec.switch_env("no_pair,force_tile=64x64,streamk_min_ratio=1") == {"EG_GEMM_NO_PAIR": "1", "EG_GEMM_FORCE_TILE": "64,64", "EG_STREAMK_MIN_RATIO": "1"}


def test_a_call_lays_its_operands_out_as_the_row_says():
    """Call / sgemm_call: transposed storage, leading dimensions, one-float offsets, NaN around the operands, SENTINEL around C."""
    rng = np.random.default_rng(6)
    row = dict(ta=1, tb=0, lda=9, ldb=7, ldc=8, a=2, b=1, c=2, bias=2)
    opa, opb = ec.values((5, 3), rng), ec.values((3, 6), rng)
    c = ec.sgemm_call(row, opa, opb, bias=np.zeros(6, dtype=np.float32))
    sa, sb, sc, sbias = c.starts()
    assert (sa, sb, sc, sbias) == (ec.GUARD + 1, ec.GUARD, ec.GUARD + 1, ec.GUARD + 1) and (c.lda, c.ldb, c.ldc) == (9, 7, 8)
    assert all(c.a[sa + k * 9 + m] == opa[m, k] for m in range(5) for k in range(3)) and np.isnan(c.a).sum() == c.a.size - 15
    assert all(c.b[sb + k * 7 + n] == opb[k, n] for k in range(3) for n in range(6))
    assert np.isnan(c.interior(c.c0)).all() and (c.c0 == ec.SENTINEL).sum() == c.c0.size - 30
    got = c.c0.copy()
    c.interior(got)[...] = 1.0
    c.check_outside(got)
    got[sc + 6] = 0.0                 # the padding behind row 0
    with pytest.raises(AssertionError):
        c.check_outside(got)
    with pytest.raises(AssertionError):
        ec.same_bits(np.float32([0.0]), np.float32([-0.0]), "signed zero")
