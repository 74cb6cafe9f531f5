"""eg_conv2_nhwc_f64, eg_conv2_nhwc_grad_filter_f64 and eg_conv2_nhwc_grad_image_f64 on the library's own buffers, every case
of tests/conv64_cases.py through each entry point.

Bound: the project's float64 bound, 1e-12 of the largest magnitude of the expected result (TOL64 / rel of
tests/test_gpu_f64.py).  The longest sum of any case has conv64_cases.LONGEST_CHAIN = 4096 terms of magnitude <= 1, and
4096 * 2^-53 = 4.5e-13 bounds even a worst-case chain; tests/test_conv64_cases_cpu.py holds the numpy reference itself to
1e-13.

Every operand and the destination are carved from a larger allocation filled with NaN (the pattern of
tests/test_gpu_library_ranges.py): the destination's surroundings must be bit-unchanged afterwards, and a NaN in the result
would show a read behind an operand — or, with accumulate == 0, a read of the destination itself, which starts as NaN.
Each case runs once more with every base moved by one double, where no 16-byte load applies."""
import ctypes

import numpy as np
import pytest

import conv64_cases as cc
from exprgrad_amd import _lib

pytestmark = pytest.mark.gpu
TOL64 = 1e-12
GAP = 32          # doubles of NaN in front of and behind every tensor
EG_OK, EG_ERR_INVALID, EG_ERR_SHAPE = 0, 1, 7
ENTRY = {"forward": "eg_conv2_nhwc_f64", "grad_filter": "eg_conv2_nhwc_grad_filter_f64", "grad_image": "eg_conv2_nhwc_grad_image_f64"}
INPUTS = {"forward": ("img", "flt"), "grad_filter": ("img", "gout"), "grad_image": ("flt", "gout")}


def rel(got, want):
    want = np.asarray(want, np.float64)
    scale = max(float(np.max(np.abs(want))) if want.size else 0.0, 1e-300)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want))) / scale if want.size else 0.0


def vp(p):
    return ctypes.c_void_p(int(p))


class Guarded:
    """A tensor inside a NaN-filled allocation: GAP + shift doubles in front, GAP behind."""

    def __init__(self, ctx, values, shift):
        self.first, self.n = GAP + shift, values.size
        self.host = np.full(self.first + self.n + GAP, np.nan)
        self.host[self.first:self.first + self.n] = values.ravel()
        self.buf = ctx.allocBuffer(self.host.nbytes)
        assert self.buf.ptr % 16 == 0
        self.buf.write(self.host)
        self.ptr = self.buf.ptr + 8 * self.first
        assert (self.ptr % 16 == 0) == (shift % 2 == 0)

    def read(self):
        """The tensor as it is now; the surroundings must not have changed by a bit."""
        now = self.buf.read(np.float64)
        outside = np.r_[0:self.first, self.first + self.n:now.size]
        assert np.array_equal(now.view(np.uint64)[outside], self.host.view(np.uint64)[outside]), "written outside the destination"
        return now[self.first:self.first + self.n]

    def free(self):
        self.buf.dealloc()


def run(ctx, case, role, shift=0, start=None, times=1, status=EG_OK):
    """One entry point on guarded buffers.  start: the destination's values before the call (accumulate) or None (NaN,
    accumulate == 0).  Returns the destination after each of `times` calls."""
    o = cc.operands(case)
    want_shape = cc.reference(case, role).shape
    ins = [Guarded(ctx, o[name], shift) for name in INPUTS[role]]
    dst = Guarded(ctx, start if start is not None else np.full(want_shape, np.nan), shift)
    gots = []
    for t in range(times):
        if t:
            dst.buf.write(dst.host)
        rc = getattr(_lib.lib(), ENTRY[role])(ctx.handle, *case, vp(ins[0].ptr), vp(ins[1].ptr), vp(dst.ptr), 0 if start is None else 1)
        assert rc == status, (rc, _lib.last_error())
        gots.append(dst.read().reshape(want_shape))
    for g in ins + [dst]:
        g.free()
    return gots[0] if times == 1 else gots


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "moved-by-one-double"])
@pytest.mark.parametrize("role", cc.ROLES)
@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_against_numpy_on_guarded_ranges(gpu_ctx, case, role, shift):
    want = cc.reference(case, role)
    got = run(gpu_ctx, case, role, shift)                      # accumulate == 0 over a destination of NaN
    print(cc.case_id(case), role, shift, "overwrite", rel(got, want) if np.all(np.isfinite(got)) else "not finite")
    assert np.all(np.isfinite(got)), "NaN from the destination's start values or from behind an operand"
    assert rel(got, want) <= TOL64
    start = np.random.default_rng(7).uniform(-1, 1, want.shape)
    got = run(gpu_ctx, case, role, shift, start=start)         # accumulate != 0
    print(cc.case_id(case), role, shift, "accumulate", rel(got - start, want) if np.all(np.isfinite(got)) else "not finite")
    assert np.all(np.isfinite(got))
    assert float(np.max(np.abs(got - (start + want)))) <= TOL64 * max(float(np.max(np.abs(want))), 1.0)


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_filter_gradient_runs_are_bit_equal(gpu_ctx, case):
    a, b = run(gpu_ctx, case, "grad_filter", times=2)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("role", ["forward", "grad_image"])
def test_an_image_has_the_same_bits_in_any_batch(gpu_ctx, role):
    """Forward and image gradient sum every output element as one chain in tap order, whatever tile the batch's size picks."""
    case = cc.BATCH_CASE
    N = case[0]
    whole = run(gpu_ctx, case, role)
    o = cc.operands(case)
    one = (1,) + case[1:]
    for n in range(N):
        ins = [Guarded(gpu_ctx, o[name][n:n + 1] if name != "flt" else o[name], 0) for name in INPUTS[role]]
        dst = Guarded(gpu_ctx, np.full(whole[n:n + 1].shape, np.nan), 0)
        rc = getattr(_lib.lib(), ENTRY[role])(gpu_ctx.handle, *one, vp(ins[0].ptr), vp(ins[1].ptr), vp(dst.ptr), 0)
        assert rc == EG_OK, _lib.last_error()
        alone = dst.read().reshape(whole[n].shape)
        for g in ins + [dst]:
            g.free()
        assert np.array_equal(alone, whole[n]), (role, n)


def entry(ctx, role, shape, a, b, dst, accumulate=0):
    return getattr(_lib.lib(), ENTRY[role])(ctx.handle, *shape, vp(a.ptr if a else 0), vp(b.ptr if b else 0), vp(dst.ptr if dst else 0), accumulate)


def test_empty_extents(gpu_ctx):
    """N = 0, F = 0 and H = FH - 1 as the header says: empty outputs succeed and launch nothing; a gradient whose sum is
    empty zero-fills with accumulate == 0 and leaves the destination alone otherwise; H = FH - 2 is a shape error."""
    ctx = gpu_ctx
    some = np.linspace(1.0, 2.0, 17 * 3 * 3 * 17)
    a, b = Guarded(ctx, some, 0), Guarded(ctx, some, 0)

    def fresh():
        return Guarded(ctx, some, 0)

    untouched = [("forward", (0, 9, 10, 17, 17, 3, 3)), ("forward", (1, 9, 10, 17, 0, 3, 3)), ("forward", (1, 2, 10, 17, 17, 3, 3)),
                 ("grad_filter", (1, 9, 10, 17, 0, 3, 3)), ("grad_filter", (1, 9, 10, 0, 17, 3, 3)), ("grad_image", (0, 9, 10, 17, 17, 3, 3)),
                 ("grad_image", (1, 9, 10, 0, 17, 3, 3))]
    for role, shape in untouched:
        for acc in (0, 1):
            d = fresh()
            assert entry(ctx, role, shape, a, b, d, acc) == EG_OK, (role, shape, _lib.last_error())
            assert np.array_equal(d.read(), some), (role, shape)
            d.free()
    # empty sums: the whole destination is zero-filled (accumulate == 0) or left as it is
    zero_filled = [("grad_filter", (0, 9, 10, 4, 3, 3, 3), 3 * 3 * 3 * 4), ("grad_filter", (2, 2, 10, 4, 3, 3, 3), 3 * 3 * 3 * 4),
                   ("grad_image", (1, 5, 6, 7, 0, 3, 3), 5 * 6 * 7), ("grad_image", (2, 2, 6, 7, 3, 3, 3), 2 * 2 * 6 * 7)]
    for role, shape, n in zero_filled:
        d = fresh()
        assert entry(ctx, role, shape, a, b, d, 0) == EG_OK, (role, shape, _lib.last_error())
        got = d.read()
        assert np.all(got[:n] == 0.0) and np.array_equal(got[n:], some[n:]), (role, shape)
        assert entry(ctx, role, shape, a, b, d, 1) == EG_OK
        assert np.all(d.read()[:n] == 0.0)
        d.free()
    d = fresh()
    for role in cc.ROLES:
        assert entry(ctx, role, (1, 1, 10, 17, 17, 3, 3), a, b, d) == EG_ERR_SHAPE
        assert ENTRY[role] in _lib.last_error()
        assert entry(ctx, role, (1, 9, 10, 17, 17, 0, 3), a, b, d) == EG_ERR_INVALID
        assert entry(ctx, role, (-1, 9, 10, 17, 17, 3, 3), a, b, d) == EG_ERR_INVALID
        assert entry(ctx, role, (1, 9, 10, 17, 17, 3, 3), None, b, d) == EG_ERR_INVALID
    assert np.array_equal(d.read(), some)
    for g in (a, b, d):
        g.free()


def test_indices_of_2_to_the_31_are_refused(gpu_ctx):
    """The kernels hold pixels and taps in 32 bits (csrc/kernels/gemm_plan.hpp, CONV64_MAX_INDEX): a call whose
    contraction reaches 2^31 rows, columns or terms is refused before anything is launched, and nothing is read or written."""
    some = np.linspace(1.0, 2.0, 64)
    a, b, d = Guarded(gpu_ctx, some, 0), Guarded(gpu_ctx, some, 0), Guarded(gpu_ctx, some, 0)
    lim = 1 << 31
    for role, shape in [("forward", (lim, 1, 2, 17, 17, 1, 2)), ("grad_filter", (lim, 1, 2, 17, 17, 1, 2)), ("grad_image", (lim // 2, 1, 2, 17, 17, 1, 2))]:
        assert entry(gpu_ctx, role, shape, a, b, d) == EG_ERR_INVALID, (role, shape)
        assert "2^31" in _lib.last_error()
    assert np.array_equal(d.read(), some)
    for g in (a, b, d):
        g.free()
