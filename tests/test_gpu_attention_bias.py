"""GPU parity of eg_attention_bias and eg_attention_bias_grad (kernels/attention_f32.hip, kernels/attention_grad_f32.hip,
BIAS instantiations) against a float64 numpy evaluation of the five statements with the bias added to the scaled scores,

    e = exp(scale * q . k + bias),  L = sum_j e,  O = (e / L) v,  and the closed-form dQ, dK, dV of include/exprgrad_hip.h,

every element within TOL (1e-5 of the largest value).  The bias comes in its broadcast forms: full [b,h,i,j] (16-byte rows, and
again from a pointer offset by one float), a causal [i,j] table of -Inf (both strides 0) and a key-padding mask [b,j]
(ldb = 0, stride_b1 = 0).  Every operand, the bias included, sits between NaN guards with NaN behind its rows, and every
output buffer is compared bit for bit with its state before the call outside the items."""
import ctypes

import numpy as np
import pytest

import attention_grad_cases as gc
from conftest import TOL, rel_err
from exprgrad_amd import _lib, ops
from test_gpu_attention_fused import View, u
from test_gpu_attention_grad import Case, bits, same_outside

pytestmark = pytest.mark.gpu

EG_ERR_INVALID = 1
SCALE = gc.SCALE
DIMS = [(2, 3, 33, 70, 16, 16), (1, 2, 65, 63, 20, 12), (1, 2, 130, 129, 128, 128)]
FORMS = ["full", "causal", "padding", "full_offset"]


def make_bias(ctx, dims, form, seed=0):
    """(host bias broadcastable to [b0, b1, I, J], its View on the device)"""
    b0, b1, I, J, _, _ = dims
    ld = 4 * (J // 4 + 1)   # NaN behind every row; a multiple of 4: 16-byte loads in the dK/dV kernel unless the pointer is offset
    if form == "causal":    # key 0 stays for every row
        x = np.where(np.arange(J)[None, :] > np.arange(I)[:, None], -np.inf, 0.0).astype(np.float32)[None, None]
        return x, View(x, ld, 0, 0).upload(ctx)
    if form == "padding":   # lengths >= 1, one per batch; the row of J floats is every query row's
        lengths = [max(1, J - 7 - 30 * o) for o in range(b0)]
        x = np.where(np.arange(J)[None, :] >= np.array(lengths)[:, None], -np.inf, 0.0).astype(np.float32)[:, None, None, :]
        return x, View(x, 0, J + 5, 0).upload(ctx)
    x = np.float32(2.0) * u(np.random.default_rng(seed + 41), b0, b1, I, J)
    return x, View(x, ld, b1 * I * ld, I * ld, offset=1 if form == "full_offset" else 0).upload(ctx)


def exact(q, k, v, bias, d_out=None):
    """float64: (o, sums) and, with d_out, (dq, dk, dv) too"""
    q, k, v, bias = (np.asarray(x, np.float64) for x in (q, k, v, bias))
    with np.errstate(invalid="ignore"):
        e = np.exp(np.einsum("obik,objk->obij", q, k) * np.float64(np.float32(SCALE)) + bias)
        sums = e.sum(-1)
        p = e / sums[..., None]
    o = np.einsum("obij,objd->obid", p, v)
    if d_out is None:
        return o, sums
    d_out = np.asarray(d_out, np.float64)
    ds = np.float64(np.float32(SCALE)) * p * (np.einsum("obid,objd->obij", d_out, v) - np.einsum("obid,obid->obi", d_out, o)[..., None])
    return o, sums, np.einsum("obij,objk->obik", ds, k), np.einsum("obij,obik->objk", ds, q), np.einsum("obij,obid->objd", p, d_out)


def x(t):
    return (t, t.ld, t.strides) if t is not None else (None, 0, (0, 0))


def forward(case, B, O=None, accumulate=False, sums=True):
    O = O or case.O
    ops.attention_bias(case.ctx, *case.dims, SCALE, *x(case.Q), *x(case.Kk), *x(case.V), *x(O), case.S if sums else None, case.S.strides, *x(B), accumulate)
    return O.dev.read(), case.S.dev.read()


def backward(case, B, accumulate=0):
    ops.attention_bias_grad(case.ctx, *case.dims, SCALE, *x(case.Q), *x(case.Kk), *x(case.V), *x(case.O), case.S, case.S.strides, *x(case.dO),
                            *x(case.dQ), *x(case.dK), *x(case.dV), *x(B), accumulate)
    return case.dQ.dev.read(), case.dK.dev.read(), case.dV.dev.read()


def close(got, want, label):
    err = rel_err(got, want, label)
    print(label, err)
    assert np.all(np.isfinite(got)) and err <= TOL, (label, err)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "x".join(map(str, d)))
def test_forward_and_backward(gpu_ctx, dims, form):
    """O and Sums with accumulate 0 and 1, then dQ, dK and dV with accumulate bits 0 and 7, all against float64"""
    b0, b1, I, J, K, D = dims
    label = "eg_attention_bias %s %s" % (dims, form)
    rng = np.random.default_rng(5)
    bases = {"dq": u(rng, b0, b1, I, K), "dk": u(rng, b0, b1, J, K), "dv": u(rng, b0, b1, J, D)}
    case = Case(gpu_ctx, dims, "bihk")
    acc = Case(gpu_ctx, dims, "bihk", bases=bases)
    bias, B = make_bias(gpu_ctx, dims, form, seed=sum(dims))
    assert (B.ptr % 16 == 0) == (form != "full_offset")
    o_buf, s_buf = forward(case, B)
    o = case.O.items(o_buf).copy()
    d_out = gc.mse_gradient(o, case.labels)
    o64, sums64, dq64, dk64, dv64 = exact(case.q, case.k, case.v, bias, d_out)
    assert np.all(np.isfinite(o64)) and np.all(sums64 > 0), "the masks keep a key in every row"
    close(o, o64, label + " O")
    close(case.S.items(s_buf)[:, :, 0, :], sums64, label + " Sums")
    same_outside(case.O, o_buf, label + " O")
    same_outside(case.S, s_buf, label + " Sums")
    base_o = u(rng, b0, b1, I, D)
    Oa = View(base_o, case.O.ld, *case.O.strides).upload(gpu_ctx)
    oa_buf, _ = forward(case, B, O=Oa, accumulate=True, sums=False)
    close(Oa.items(oa_buf), o64 + base_o, label + " O accumulate")
    same_outside(Oa, oa_buf, label + " O accumulate")
    for c, bit, base in ((case, 0, {}), (acc, 7, bases)):
        c.O, c.S = case.O, case.S
        c.set_d_out(d_out)
        bufs = backward(c, B, bit)
        for name, view, buf, want in (("dq", c.dQ, bufs[0], dq64), ("dk", c.dK, bufs[1], dk64), ("dv", c.dV, bufs[2], dv64)):
            close(view.items(buf), want + base.get(name, 0.0), "%s %s accumulate=%d" % (label, name, bit))
            same_outside(view, buf, "%s %s" % (label, name))


def test_zero_bias_and_null_bias_are_the_unbiased_entries(gpu_ctx):
    """O, Sums, dQ, dK and dV bit for bit as eg_attention_sums and eg_attention_grad give them"""
    dims = (2, 3, 33, 70, 16, 16)
    plain = Case(gpu_ctx, dims, "bihk")
    want = [b.copy() for b in plain.forward() + plain.run()]
    zero = np.zeros((1, 1, dims[2], dims[3]), np.float32)
    for B in (View(zero, dims[3], 0, 0).upload(gpu_ctx), None):
        case = Case(gpu_ctx, dims, "bihk")
        got = list(forward(case, B))
        case.set_d_out(plain.d_out)
        got += backward(case, B)
        for g, w, name in zip(got, want, ("O", "Sums", "dQ", "dK", "dV")):
            assert np.array_equal(bits(g), bits(w)), (name, "NULL" if B is None else "zero bias")


def test_special_rows(gpu_ctx):
    """Row 3 has every key masked: NaN, its neighbours not.  Row 40 has one +Inf: NaN.  Keys 64 .. 127, a whole key tile, are
    -Inf for every row: the other rows are the attention over the remaining keys."""
    dims = (1, 1, 70, 150, 16, 16)
    case = Case(gpu_ctx, dims, "bihk")
    bias = np.zeros((1, 1, 70, 150), np.float32)
    bias[..., 64:128] = -np.inf
    bias[0, 0, 3, :] = -np.inf
    bias[0, 0, 40, 5] = np.inf
    o_buf, s_buf = forward(case, View(bias, 152, 0, 0).upload(gpu_ctx))
    o, sums = case.O.items(o_buf)[0, 0], case.S.items(s_buf)[0, 0, 0]
    assert np.all(np.isnan(o[[3, 40]])) and sums[3] == 0 and np.isnan(sums[40]), (o[[3, 40]], sums[[3, 40]])
    rows, keys = np.setdiff1d(np.arange(70), [3, 40]), np.r_[0:64, 128:150]
    o64, sums64 = exact(case.q[:, :, rows], case.k[:, :, keys], case.v[:, :, keys], 0.0)
    close(o[rows], o64[0, 0], "eg_attention_bias without the masked keys O")
    close(sums[rows], sums64[0, 0], "eg_attention_bias without the masked keys Sums")


def test_refusals(gpu_ctx):
    """a negative bias stride and 0 < ldb < J: EG_ERR_INVALID, and the message names the entry"""
    dims = (2, 3, 8, 8, 8, 8)
    buf = gpu_ctx.allocTensor((2 * 3 * 8 * 8,))
    p = ctypes.c_void_p(buf.ptr)
    v = (p, 8, 192, 64)
    for ldb, sb0, sb1 in ((8, -192, 64), (8, 192, -64), (7, 192, 64), (1, 0, 0)):
        rc = _lib.lib().eg_attention_bias(gpu_ctx.handle, *dims, SCALE, *v, *v, *v, *v, 0, p, 24, 8, p, ldb, sb0, sb1)
        assert rc == EG_ERR_INVALID and "eg_attention_bias:" in _lib.last_error(), (ldb, sb0, sb1, rc, _lib.last_error())
        rc = _lib.lib().eg_attention_bias_grad(gpu_ctx.handle, *dims, SCALE, *v, *v, *v, *v, p, 24, 8, *v, *v, *v, *v, 0, p, ldb, sb0, sb1)
        assert rc == EG_ERR_INVALID and "eg_attention_bias_grad:" in _lib.last_error(), (ldb, sb0, sb1, rc, _lib.last_error())
