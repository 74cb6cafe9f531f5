"""The reference of tests/test_gpu_dgemm_batched2.py, checked on the CPU: for every case and seed of the table
(tests/dgemm_batched2_cases.py) refcpu.dgemm64 per item, from the accumulate start and with the bias added, stays within
HALF of the bound the device is held to (4e-16 * sqrt(K) * (|opA| @ |opB|) + 1e-300, tests/test_gpu_dgemm_batched.py),
measured against a numpy.longdouble product.  A case that missed this would get another seed, never a wider bound."""
import numpy as np
import pytest

import dgemm_batched2_cases as cases

TABLE = cases.table()


def test_longdouble_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps / 1000


def test_table_names_are_unique():
    names = [n for n, _ in TABLE]
    assert len(names) == len(set(names)) == 34


@pytest.mark.parametrize("make", [m for _, m in TABLE], ids=[n for n, _ in TABLE])
def test_oracle_within_half_the_bound(refcpu, make):
    c = make()
    K = c.dims[4]
    for o, i in c.items():
        err = np.abs(c.oracle_item(refcpu, o, i).astype(np.longdouble) - c.longdouble_item(o, i))
        lim = 0.5 * cases.bound(K, c.magnitudes(o, i))
        assert np.all(err <= lim), (c.label(), o, i, float(np.max(err / lim)))


def test_alignment_cases_have_the_parities_they_are_named_for():
    even = lambda lay: all(s % 2 == 0 for s in lay)
    for ta, tb in cases.LAYOUTS:
        c = cases.even_case(ta, tb)
        assert c.offset == 0 and even(c.a_lay) and even(c.b_lay)
        assert cases.even_case(ta, tb, offset=1).offset == 1
    for odd in ("a0", "a1", "b0", "b1"):
        c = cases.even_case(False, False, odd=odd)
        strides = {"a0": c.a_lay[1], "a1": c.a_lay[2], "b0": c.b_lay[1], "b1": c.b_lay[2]}
        assert [k for k, s in strides.items() if s % 2] == [odd], (odd, strides)
        assert c.a_lay[0] % 2 == 0 and c.b_lay[0] % 2 == 0


def test_head_layouts_are_the_models():
    """q[b,i,h,k]: ld = H * K, inner stride K; o[b,i,h,d]: the items of C interleave."""
    c = cases.scores_in_row(16, 20, 0, 1)
    assert c.a_lay == (3 * 16, 33 * 3 * 16, 16) and c.b_lay == (3 * 16, 20 * 3 * 16, 16) and c.tb and not c.ta
    c = cases.context_in_row(20, 16, 0, 1)
    assert c.c_lay == (3 * 16, 33 * 3 * 16, 16) and c.b_lay == (3 * 16, 20 * 3 * 16, 16) and c.c_lay[2] < c.c_lay[0]


def test_an_accumulating_c_is_poisoned_outside_its_items():
    c = cases.Case(2, 3, 7, 5, 3, accumulate=True, c=cases.nested(3, 7, 5, 3, 5), seed=1)
    marks = np.zeros(c.c0.size)          # (float64, as the views of the cases are)
    for o, i in c.items():
        c.c_item(marks, o, i)[...] = 1.0
    inside = marks == 1.0
    assert np.all(c.c0[~inside] == cases.POISON) and not np.any(c.c0[inside] == cases.POISON) and not inside.all()
