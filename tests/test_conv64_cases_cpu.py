"""tests/conv64_cases.py's float64 references against the same sums in np.longdouble: they agree within 1e-13 of the
largest magnitude, an order below the bound the GPU tests hold the kernels to (1e-12), so a GPU result that misses its
bound is the kernel's."""
import numpy as np
import pytest

import conv64_cases as cc


def test_longdouble_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


@pytest.mark.parametrize("role", cc.ROLES)
@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_reference_against_extended_precision(case, role):
    got, want = cc.reference(case, role), cc.reference(case, role, np.longdouble)
    assert got.dtype == np.float64 and want.dtype == np.longdouble and got.shape == want.shape
    scale = float(np.max(np.abs(want)))
    assert scale > 0
    assert float(np.max(np.abs(got.astype(np.longdouble) - want))) <= 1e-13 * scale


def test_longest_chain():
    N, H, W, C, F, FH, FW = cc.SLICED_CASE
    terms = [max(FH * FW * C, FH * FW * F, n * (h - fh + 1) * (w - fw + 1)) for n, h, w, C, F, fh, fw in cc.CASES for FH, FW in [(fh, fw)]]
    assert max(terms) == cc.LONGEST_CHAIN == N * (H - FH + 1) * (W - FW + 1)
    assert cc.LONGEST_CHAIN * 2.0 ** -53 < 1e-12
