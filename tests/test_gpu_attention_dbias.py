"""GPU parity of eg_attention_bias_dbias (kernels/attention_dbias_f32.hip) against float64 numpy: with p, dP and delta of the
biased forward, g = p * (dP - delta) summed over the axes along which the bias is broadcast, every element within TOL (1e-5 of
the largest value).  The bias comes as [b,h,i,j] (and again from pointers offset by one float), [h,i,j], a causal [i,j] table
of -Inf and a key-padding mask [b,j] (one row per batch: the row fold); dBias has the same form.  Every operand, dBias
included, sits between NaN guards with NaN behind its rows, and the dBias buffer is compared bit for bit with its state before
the call outside the items."""
import ctypes

import numpy as np
import pytest

import attention_grad_cases as gc
from conftest import TOL, rel_err
from exprgrad_amd import _lib, ops
from test_gpu_attention_fused import POISON, View, poisoned, u
from test_gpu_attention_grad import Case, bits, same_outside

pytestmark = pytest.mark.gpu

EG_ERR_INVALID, EG_ERR_UNSUPPORTED = 1, 5
SCALE = gc.SCALE
DIMS = [(2, 3, 33, 70, 16, 16), (1, 2, 65, 63, 20, 12), (2, 2, 70, 129, 128, 128)]
FORMS = ["full", "full_offset", "heads", "causal", "padding"]


def make_bias(dims, form, seed):
    """(host bias broadcastable to [b0, b1, I, J], (ld, s0, s1) of it and of its gradient, pointer offset in floats)"""
    b0, b1, I, J, _, _ = dims
    ld = 4 * (J // 4 + 1)   # NaN behind every row
    if form == "causal":    # key 0 stays for every row
        return np.where(np.arange(J)[None, :] > np.arange(I)[:, None], -np.inf, 0.0).astype(np.float32)[None, None], (ld, 0, 0), 0
    if form == "padding":   # lengths >= 1, one per batch; the row of J floats is every query row's
        lengths = np.array([max(1, J - 7 - 30 * o) for o in range(b0)])
        return np.where(np.arange(J)[None, :] >= lengths[:, None], -np.inf, 0.0).astype(np.float32)[:, None, None, :], (0, J + 5, 0), 0
    if form == "heads":
        return np.float32(2.0) * u(np.random.default_rng(seed), 1, b1, I, J), (ld, 0, I * ld), 0
    return np.float32(2.0) * u(np.random.default_rng(seed), b0, b1, I, J), (ld, b1 * I * ld, I * ld), int(form == "full_offset")


def x(t):
    return (t, t.ld, t.strides)


def dbias(case, B, dB, accumulate):
    ops.attention_bias_dbias(case.ctx, *case.dims, SCALE, *x(case.Q), *x(case.Kk), *x(case.V), *x(case.O), case.S, case.S.strides, *x(case.dO), *x(B),
                             *x(dB), accumulate)
    return dB.dev.read()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "x".join(map(str, d)))
def test_dbias(gpu_ctx, dims, form):
    """dBias with accumulate 0 (twice: equal bits) and 1 against float64, masked entries exactly 0, nothing stored outside"""
    label = "eg_attention_bias_dbias %s %s" % (dims, form)
    bias, (ld, s0, s1), offset = make_bias(dims, form, seed=sum(dims))
    case = Case(gpu_ctx, dims, "bihk", offset=offset)
    B = View(bias, ld, s0, s1, offset).upload(gpu_ctx)
    ops.attention_bias(gpu_ctx, *dims, SCALE, *x(case.Q), *x(case.Kk), *x(case.V), *x(case.O), case.S, case.S.strides, *x(B), False)
    o = case.O.items(case.O.dev.read()).copy()
    d_out = gc.mse_gradient(o, case.labels)
    case.set_d_out(d_out)

    q, k, v, b64, do64 = (np.asarray(t, np.float64) for t in (case.q, case.k, case.v, bias, d_out))
    e = np.exp(np.einsum("obik,objk->obij", q, k) * np.float64(np.float32(SCALE)) + b64)
    p = e / e.sum(-1, keepdims=True)
    o64 = np.einsum("obij,objd->obid", p, v)
    g = p * (np.einsum("obid,objd->obij", do64, v) - np.einsum("obid,obid->obi", do64, o64)[..., None])
    want = g.sum(tuple(a for a in range(3) if bias.shape[a] == 1), keepdims=True)   # the broadcast axes
    assert want.shape == bias.shape and np.all(np.isfinite(want))

    rng = np.random.default_rng(7)
    for accumulate, base in ((0, np.full(bias.shape, np.nan, np.float32)), (1, u(rng, *bias.shape))):
        dB = View(base, ld, s0, s1, offset).upload(gpu_ctx)
        assert (dB.ptr % 16 == 0) == (form != "full_offset")
        buf = dbias(case, B, dB, accumulate)
        got = dB.items(buf).copy()
        err = rel_err(got, want + (base if accumulate else 0.0), label)
        print(label, "accumulate", accumulate, err)
        assert np.all(np.isfinite(got)) and err <= TOL, (label, accumulate, err)
        if not accumulate:
            assert np.all(got[np.isneginf(bias)] == 0), label + ": a masked entry is not 0"
            dB.dev.write(dB.buf)
            assert np.array_equal(bits(dbias(case, B, dB, 0)), bits(buf)), label + ": two calls differ"
        same_outside(dB, buf, label)


def test_refusals_and_empty_extents(gpu_ctx):
    """return codes, messages that name the entry, and dBias zeroed (accumulate 0) or untouched by the empty sums"""
    n = 2 * 3 * 8 * 8
    buf, out = poisoned(gpu_ctx, n), poisoned(gpu_ctx, n + 5)
    p, d = ctypes.c_void_p(buf.ptr), ctypes.c_void_p(out.ptr)
    v, sums = (p, 8, 192, 64), (p, 24, 8)

    def call(dims=(2, 3, 8, 8, 8, 8), b=(p, 8, 192, 64), db=(d, 8, 192, 64), accumulate=0):
        return _lib.lib().eg_attention_bias_dbias(gpu_ctx.handle, *dims, SCALE, *v, *v, *v, *v, *sums, *v, *b, *db, accumulate)

    invalid = [dict(db=(d, 8, 0, 64)), dict(b=(p, 8, 192, 0)), dict(b=(p, 0, 192, 64)), dict(db=(d, 0, 192, 64)),   # steps that are 0 in one only
               dict(b=(p, 7, 192, 64), db=(d, 7, 192, 64)), dict(db=(d, 8, -192, 64)), dict(b=(p, 8, 192, -64)),
               dict(b=(None, 8, 192, 64)), dict(db=(None, 8, 192, 64)), dict(accumulate=2),
               dict(db=(d, 8, 64, 64))]                                                                               # dBias shares addresses
    for kw in invalid:
        assert call(**kw) == EG_ERR_INVALID and "eg_attention_bias_dbias:" in _lib.last_error(), (kw, _lib.last_error())
    for dims in ((2, 3, 8, 8, 129, 8), (2, 3, 8, 8, 8, 129)):
        wide = (p, 129, 192, 64)
        rc = _lib.lib().eg_attention_bias_dbias(gpu_ctx.handle, *dims, SCALE, *wide, *wide, *wide, *wide, *sums, *wide, p, 8, 192, 64, d, 8, 192, 64, 0)
        assert rc == EG_ERR_UNSUPPORTED and "eg_attention_bias_dbias:" in _lib.last_error() and "128" in _lib.last_error(), _lib.last_error()
    assert np.all(out.read() == POISON), "a refused call stored"

    # no element of dBias exists: nothing is launched
    for dims, db in (((0, 3, 8, 8, 8, 8), (d, 8, 192, 64)), ((2, 0, 8, 8, 8, 8), (d, 8, 192, 64)), ((2, 3, 0, 8, 8, 8), (d, 8, 192, 64)),
                     ((2, 3, 8, 0, 8, 8), (d, 8, 192, 64))):
        assert call(dims=dims, db=db) == 0, _lib.last_error()
        assert np.all(out.read() == POISON), dims
    # an empty sum: D == 0, no query rows under the row fold, no item along a summed index
    for dims, b, db, count in (((2, 3, 8, 8, 8, 0), (p, 8, 192, 64), (d, 8, 192, 64), n), ((2, 3, 0, 8, 8, 8), (p, 0, 24, 8), (d, 0, 24, 8), 48),
                               ((0, 3, 8, 8, 8, 8), (p, 8, 0, 64), (d, 8, 0, 64), 192), ((2, 0, 8, 8, 8, 8), (p, 8, 64, 0), (d, 8, 64, 0), 128)):
        assert call(dims=dims, b=b, db=db, accumulate=1) == 0, _lib.last_error()
        assert np.all(out.read() == POISON), (dims, "accumulate")
        assert call(dims=dims, b=b, db=db) == 0, _lib.last_error()
        got = out.read()
        assert np.all(got[:count] == 0) and np.all(got[count:] == POISON), dims
        out.write(np.full(n + 5, POISON, np.float32))
