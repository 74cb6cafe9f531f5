"""tests/generated_cases.py held to itself, without a GPU.

The oracle (oracle/kd.py, float32), its float64 shadow and — for the compile[float64] cases — its float64 form agree with the
plain numpy reference of every case: exactly for the dyadic cases, within 5e-6 of max|reference| otherwise (conftest's
DIRECT_EXCUSE: closer than that, a correct backend meets the direct gate of tests/parity.py against the oracle without an
entry in the allow-list).  Planted errors are caught by the very comparison the GPU module uses, and the table covers the
boundaries its docstring claims.
"""
import numpy as np
import pytest

import generated_cases as gc
from conftest import DIRECT_EXCUSE

_MODELS = {}


def models(case):
    """(oracle, shadow) of the case's program; a float64 case has the oracle's float64 form in both places."""
    from oracle import kd
    key = (case.program, case.f64)
    if key not in _MODELS:
        text = gc.program_text(case.program, case.f64)
        ref = kd.Model(text)
        assert ref.c64 == case.f64
        _MODELS[key] = (ref, ref if case.f64 else kd.Model(text, shadow=True))
    return _MODELS[key]


@pytest.mark.parametrize("name", list(gc.BY_NAME))
def test_oracle_and_shadow_agree_with_the_numpy_reference(name):
    case = gc.BY_NAME[name]
    ref, exact = models(case)
    inputs, want = case.inputs(), case.want()
    got32 = np.array(ref.call(case.target, inputs))
    got64 = np.array(exact.call(case.target, inputs))
    assert got32.dtype == case.dtype and got64.dtype == np.float64
    print("%s: oracle %.3g, shadow %.3g from the numpy reference" % (name, gc.rel(got32, want), gc.rel(got64, want)))
    gc.check_against_numpy(case, got32, want, gc.TOL64 if case.f64 else DIRECT_EXCUSE)
    if case.exact:
        assert np.array_equal(got64, want), name
    else:
        assert gc.rel(got64, want) <= gc.TOL64, (name, gc.rel(got64, want))


def test_inputs_are_what_the_exactness_argument_needs():
    for case in gc.CASES:
        for k, v in case.inputs().items():
            assert v.dtype == case.dtype and np.all(np.isfinite(v)), (case.name, k)
            if case.rtotal is not None and case.rtotal >= 2048 and case.exact:
                assert np.all(np.abs(v) <= 2) and np.array_equal(v * 8, np.round(v * 8)), (case.name, k)
            else:
                assert np.all(np.abs(v) <= 0.5), (case.name, k)
        if case.rtotal is not None and case.rtotal >= 2048:
            assert case.exact or case.name == "SPLIT_EXP", case.name
            assert case.rtotal * 4 * 64 < 2 ** 24       # every partial sum in units of 1/64 fits float32's significand


# name -> the magnitude of one term of the case's middle element (dyadic bodies: the smallest non-zero term there is)
PLANTED = {
    "SPLIT_17x2051": lambda i: 1.0 / 64,
    "F64_SPLIT_64x4099": lambda i: 1.0 / 64,
    "SPLIT_EXP": lambda i: float(np.exp(-0.25)),
    "MAP_LOW": lambda i: abs(float(i["a"][2, 1])),
    "MATVEC_300x100": lambda i: abs(float(i["a"][150, 0]) * float(i["b"][0])),
    "SCATTER": lambda i: abs(float(i["src"][0, 0]) * float(i["b"][0])),
}


@pytest.mark.parametrize("name", list(PLANTED))
def test_planted_errors_are_caught(name):
    """One element off by a term, one stray value outside a bounded region (or in any one place), one NaN."""
    case = gc.BY_NAME[name]
    i, want = case.inputs(), case.want()
    tol = gc.TOL64 if case.f64 else 1e-5
    good = want.astype(case.dtype)
    gc.check_against_numpy(case, good, want, tol)
    term = PLANTED[name](i)
    assert term > 10 * tol * float(np.abs(want).max()) or case.exact, (name, term)     # (an exact case is caught at any size)
    off = good.copy()
    off.flat[off.size // 2] += case.dtype(term)
    with pytest.raises(AssertionError):
        gc.check_against_numpy(case, off, want, tol)
    stray = good.copy()
    where = np.flatnonzero(want == 0)
    stray.flat[where[0] if where.size else 0] += case.dtype(0.01 * max(1.0, float(np.abs(want).max())))
    with pytest.raises(AssertionError):
        gc.check_against_numpy(case, stray, want, tol)
    nan = good.copy()
    nan.flat[-1] = np.nan
    with pytest.raises(AssertionError):
        gc.check_against_numpy(case, nan, want, tol)
    if name == "MAP_LOW":
        assert where.size == 20      # the columns the bounded loop leaves alone


def test_the_table_covers_what_it_claims():
    cases = gc.CASES
    split32 = [c for c in cases if c.mode_b and not c.f64]
    assert {c.tx for c in split32} >= {1, 2, 4, 8, 32, 64}
    assert {c.tx for c in cases if c.mode_b and c.f64} == {1, 64}
    for c in cases:
        if c.total is not None:
            assert c.mode_b == gc.takes_mode_b(c.total, c.rtotal, full_cover=c.name != "PART_COVER"), c.name
            assert not c.mode_b or c.tx == gc.expected_tx(c.total)
    shapes = {(c.total, c.rtotal): c.mode_b for c in cases if c.total is not None and not c.f64 and c.name != "PART_COVER"}
    # either side of rtotal >= 2048, at total = 1 and at total = 32
    assert shapes[1, 2048] and not shapes[1, 2047] and shapes[32, 2048] and not shapes[32, 2047]
    # either side of total * 64 <= rtotal, with rtotal >= 2048 on both
    assert shapes[33, 2112] and not shapes[33, 2111] and shapes[65, 4160]
    # an independent loop that does not cover the tensor keeps a long reduction in mode A
    part = gc.BY_NAME["PART_COVER"]
    assert gc.takes_mode_b(part.total, part.rtotal) and not part.mode_b
    # more than one column tile, the last with one active column (65 = 64 + 1) and with two (130 = 2 * 64 + 2)
    assert any(c.total == 65 for c in split32) and any(c.total == 130 for c in split32)
    # ragged chunks at every tx below 64, a ragged last chunk at 64
    assert {c.tx for c in split32 if c.ragged == "all"} >= {2, 4, 8, 16, 32} and {c.tx for c in cases if c.ragged == "all" and c.f64} == {1}
    assert any(c.tx == 64 and c.ragged == "last" for c in split32)
    # accumulate and overwrite folds, a decode over two independent and two reduction loops
    assert {"SPLIT_TWICE", "SPLIT_TWO_BY_TWO", "SPLIT_EXP"} <= set(gc.BY_NAME)
    # four elements per thread: taken, and every condition that can fail alone does (module docstring of generated_cases)
    maps = [c for c in cases if c.vec4 is not None]
    assert sum(1 for c in maps if not c.vec4 and "vec4" in c.route) >= 4
    for c in maps:
        assert ("vec4" in c.route) == (not c.vec4), c.name
    alone = {next(iter(c.vec4)) for c in maps if len(c.vec4) == 1}
    assert alone == {"last_dim", "bounds", "iterator_value", "operand_order", "float64"}, alone
    together = set().union(*[c.vec4 for c in maps])
    assert {"extent", "total"} <= together
    # every family in float64, every family at all
    assert {c.family for c in cases if c.f64} == set(gc.FAMILIES) == {c.family for c in cases}
    # the narrow body is refused exactly where the kernel computes with Index values
    assert [c.name for c in cases if "wide" in c.route] == ["INDEX_VALUES", "F64_INDEX_VALUES"]
    assert float(21475 * 100000) >= 2.0 ** 31 > float(21474 * 100000)
