"""The reference of tests/test_gpu_dgemm_batched.py, checked on the CPU: for every case and seed of the table
(tests/dgemm_batched_cases.py) refcpu.dgemm64, from the accumulate start and with the bias added, stays within HALF of the
bound the device is held to, measured against a numpy.longdouble product.  A case that missed this would get another seed,
never a wider bound."""
import numpy as np
import pytest

import dgemm_batched_cases as cases

TABLE = cases.table()


def test_longdouble_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps / 1000


def test_table_has_every_case():
    names = [n for n, _ in TABLE]
    assert len(names) == len(set(names)) == 4 * len(cases.SHAPES) + 2 + 4 * (len(cases.ALIGNMENT) + 2 + len(cases.EPILOGUES))


@pytest.mark.parametrize("kw", [kw for _, kw in TABLE], ids=[name for name, _ in TABLE])
def test_oracle_within_half_the_bound(refcpu, kw):
    c = cases.Case(**kw)
    batch, M, N, K = c.dims
    for i in range(batch):
        err = np.abs(c.oracle_item(refcpu, i).astype(np.longdouble) - c.longdouble_item(i))
        lim = 0.5 * cases.bound(K, c.magnitudes(i))
        assert np.all(err <= lim), (c.label(), i, float(np.max(err / lim)))


def test_alignment_cases_have_the_parities_they_are_named_for():
    for (ta, tb) in cases.LAYOUTS:
        mk = lambda name: cases.Case(*cases.EVEN, ta=ta, tb=tb, **cases.ALIGNMENT[name])
        c = mk("odd_ld")
        assert c.lda % 2 == 1 and c.ldb % 2 == 1
        c = mk("even_ld_odd_stride")
        assert c.lda % 2 == 0 and c.ldb % 2 == 0 and c.stride_a % 2 == 1 and c.stride_b % 2 == 1
        c = mk("offset_1")
        assert c.offset == 1 and c.lda % 2 == 0 and c.ldb % 2 == 0 and c.stride_a % 2 == 0 and c.stride_b % 2 == 0
        c = mk("even_ld_even_stride")
        assert c.offset == 0 and all(v % 2 == 0 for v in (c.lda, c.ldb, c.stride_a, c.stride_b))
        assert c.stride_a > (cases.EVEN[3] if ta else cases.EVEN[1]) * c.lda      # padded behind the last row as well
