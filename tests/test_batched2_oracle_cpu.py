"""The reference of tests/test_gpu_sgemm_batched2.py, checked on the CPU: for every case and seed of the table
(tests/batched2_cases.py, all with K <= 96 and inputs U[-0.5, 0.5)) refcpu.sgemm, from the accumulate start and with the
bias added, is within 5e-6 of the float64 product relative to the item's largest value — half of the 1e-5 the device is
held to against either.  A case that missed this would get another seed, never a wider bound.  The layouts themselves are
checked too: the head-in-row cases have the strides the interface documents."""
import numpy as np
import pytest

import batched2_cases as cases

TABLE = cases.table()
ORACLE_OWN = 5e-6


def test_table_has_every_case():
    names = [n for n, _ in TABLE]
    assert len(names) == len(set(names)) == 4 + 2 + 8 + 4 + 1
    assert all(make().dims[4] <= 96 for _, make in TABLE)


@pytest.mark.parametrize("make", [m for _, m in TABLE], ids=[n for n, _ in TABLE])
def test_oracle_within_5e6_of_float64(refcpu, make):
    c = make()
    worst = 0.0
    for o, i in c.items():
        exact = c.exact(o, i)
        worst = max(worst, float(np.max(np.abs(c.oracle(refcpu, o, i).astype(np.float64) - exact)) / np.max(np.abs(exact))))
    print(c.label(), "oracle vs float64", worst)
    assert worst <= ORACLE_OWN, (c.label(), worst)


def test_head_in_row_layouts_are_the_documented_ones():
    c = cases.head_in_row(16, 20, 0, 31)
    assert c.a_lay == (48, 33 * 48, 16) and c.b_lay == (48, 20 * 48, 16) and c.c_lay == (60, 33 * 60, 20)
    c = cases.head_in_row(17, 19, 1, 32)
    assert c.a_lay == (51, 33 * 51, 17) and c.b_lay == (51, 19 * 51, 17) and c.c_lay == (57, 33 * 57, 19) and c.offset == 1
    # q[b,i,h,k] as numpy sees it: item (b, h) is q4[b, :, h, :]
    q4 = c.a[1:1 + 2 * 33 * 3 * 17].reshape(2, 33, 3, 17)
    assert np.array_equal(c.a_item(1, 2), q4[1, :, 2, :])
