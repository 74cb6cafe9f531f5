"""tests/attention_grad_f64_cases.py without a device: at every shape the closed form in float64 stays within a tenth of TOL64 of
the closed form in numpy.longdouble, each output relative to its largest element (the worst seen is 9.1e-16).  So a kernel that
sums in another order has room under TOL64, and a kernel that drops a tile does not."""
import numpy as np
import pytest

import attention_grad_f64_cases as gc


@pytest.mark.parametrize("dims", gc.DIMS, ids=gc.ident)
def test_float64_closed_form_against_longdouble(dims):
    ops = gc.operands(dims)
    for got, ref in zip(gc.closed_form(*ops, gc.SCALE, np.float64), gc.closed_form(*ops, gc.SCALE, np.longdouble)):
        assert np.all(np.isfinite(got)) and np.max(np.abs(ref)) > 0 and gc.rel(got, ref) <= gc.TOL64 / 10, gc.rel(got, ref)
