"""GPU parity of eg_attention_stable and eg_attention_stable_grad (kernels/attention_stable_f32.hip, the STABLE kernels of
kernels/attention_grad_stable_f32.hip) against a float64 numpy evaluation with the row maximum,

    x = scale * q . k + bias,  m = max_j x,  e = exp(x - m),  L = sum_j e,  O = (e / L) v,  and the closed-form dQ, dK, dV,

every element within TOL (1e-5 of the largest value): on moderate scores, where eg_attention_bias must agree too; on scores
far outside the window of the as-written entries, built so that every x is exact in float32; and on the special rows of the
header's table.  Operands sit between NaN guards and every output buffer is compared bit for bit outside its items."""
import ctypes

import numpy as np
import pytest

import attention_grad_cases as gc
from conftest import TOL
from exprgrad_amd import _lib, ops
from test_gpu_attention_bias import close, make_bias, x
from test_gpu_attention_fused import View, u
from test_gpu_attention_grad import Case, same_outside

pytestmark = pytest.mark.gpu

EG_ERR_INVALID, EG_ERR_UNSUPPORTED = 1, 5
DIMS = [(2, 3, 33, 70, 16, 16), (1, 2, 65, 63, 20, 12), (1, 2, 130, 129, 128, 128)]
FORMS = ["none", "full", "causal", "full_offset"]


def stats_view(ctx, dims, vec=True):
    """[b0, b1, 2, I] of NaN: the two rows lds apart, with NaN behind each; lds and the strides multiples of 4 when `vec`"""
    b0, b1, I = dims[:3]
    lds = 4 * (I // 4 + 1) if vec else I + 1
    return View(np.full((b0, b1, 2, I), np.nan, np.float32), lds, b1 * 2 * lds + (0 if vec else 3), 2 * lds).upload(ctx)


def exact(q, k, v, bias, scale, d_out=None):
    """float64: (o, maxima, sums) and, with d_out, (dq, dk, dv) too"""
    q, k, v, bias = (np.asarray(t, np.float64) for t in (q, k, v, bias))
    xs = np.einsum("obik,objk->obij", q, k) * np.float64(np.float32(scale)) + bias
    mx = xs.max(-1)
    e = np.exp(xs - mx[..., None])
    sums = e.sum(-1)
    p = e / sums[..., None]
    o = np.einsum("obij,objd->obid", p, v)
    if d_out is None:
        return o, mx, sums
    d_out = np.asarray(d_out, np.float64)
    ds = np.float64(np.float32(scale)) * p * (np.einsum("obid,objd->obij", d_out, v) - np.einsum("obid,obid->obi", d_out, o)[..., None])
    return o, mx, sums, np.einsum("obij,objk->obik", ds, k), np.einsum("obij,obik->objk", ds, q), np.einsum("obij,obid->objd", p, d_out)


def forward(case, St, B, O=None, accumulate=False):
    O = O or case.O
    ops.attention_stable(case.ctx, *case.dims, case.scale, *x(case.Q), *x(case.Kk), *x(case.V), *x(O), *x(St), *x(B), accumulate)
    return O.dev.read(), St.dev.read() if St else None


def backward(case, St, B, accumulate=0):
    ops.attention_stable_grad(case.ctx, *case.dims, case.scale, *x(case.Q), *x(case.Kk), *x(case.V), *x(case.O), *x(St), *x(case.dO), *x(case.dQ),
                              *x(case.dK), *x(case.dV), *x(B), accumulate)
    return case.dQ.dev.read(), case.dK.dev.read(), case.dV.dev.read()


def as_written(case, B):
    """O of eg_attention_bias on the same operands, into a buffer of its own"""
    O = View(np.full(case.O.shape, np.nan, np.float32), case.O.ld, *case.O.strides).upload(case.ctx)
    ops.attention_bias(case.ctx, *case.dims, case.scale, *x(case.Q), *x(case.Kk), *x(case.V), *x(O), None, (0, 0), *x(B))
    return O.items(O.dev.read()).copy()


def check_all(ctx, case, acc, bases, bias, B, label, vec):
    """O, both Stats rows, O accumulate, then dQ, dK and dV with accumulate bits 0 and 7, all against float64; the device's O"""
    b0, b1, I, J, K, D = case.dims
    St = stats_view(ctx, case.dims, vec)
    o_buf, s_buf = forward(case, St, B)
    o = case.O.items(o_buf).copy()
    d_out = gc.mse_gradient(o, case.labels)
    o64, mx64, sums64, dq64, dk64, dv64 = exact(case.q, case.k, case.v, bias, case.scale, d_out)
    close(o, o64, label + " O")
    close(St.items(s_buf)[:, :, 0], mx64, label + " Max")
    close(St.items(s_buf)[:, :, 1], sums64, label + " Sum")
    same_outside(case.O, o_buf, label + " O")
    same_outside(St, s_buf, label + " Stats")
    base_o = u(np.random.default_rng(6), b0, b1, I, D)
    Oa = View(base_o, case.O.ld, *case.O.strides).upload(ctx)
    oa_buf, _ = forward(case, None, B, O=Oa, accumulate=True)
    close(Oa.items(oa_buf), o64 + base_o, label + " O accumulate")
    same_outside(Oa, oa_buf, label + " O accumulate")
    for c, bit, base in ((case, 0, {}), (acc, 7, bases)):
        c.O = case.O
        c.set_d_out(d_out)
        bufs = backward(c, St, B, bit)
        for name, view, buf, want in (("dq", c.dQ, bufs[0], dq64), ("dk", c.dK, bufs[1], dk64), ("dv", c.dV, bufs[2], dv64)):
            close(view.items(buf), want + base.get(name, 0.0), "%s %s accumulate=%d" % (label, name, bit))
            same_outside(view, buf, "%s %s" % (label, name))
    return o, mx64


def two_cases(ctx, dims, **kw):
    b0, b1, I, J, K, D = dims
    rng = np.random.default_rng(5)
    bases = {"dq": u(rng, b0, b1, I, K), "dk": u(rng, b0, b1, J, K), "dv": u(rng, b0, b1, J, D)}
    return Case(ctx, dims, "bihk", **kw), Case(ctx, dims, "bihk", bases=bases, **kw), bases


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "x".join(map(str, d)))
def test_moderate_scores(gpu_ctx, dims, form):
    """inside the window of the as-written entries: float64 parity of everything, and O within TOL of eg_attention_bias' O"""
    case, acc, bases = two_cases(gpu_ctx, dims)
    bias, B = (0.0, None) if form == "none" else make_bias(gpu_ctx, dims, form, seed=sum(dims))
    o, _ = check_all(gpu_ctx, case, acc, bases, bias, B, "eg_attention_stable %s %s" % (dims, form), vec=form != "none")
    close(o, as_written(case, B), "eg_attention_stable %s %s against eg_attention_bias" % (dims, form))


@pytest.mark.parametrize("biased", [False, True], ids=["no_bias", "row_bias"])
def test_scores_outside_the_window(gpu_ctx, biased):
    """q and k are multiples of 1/4 in [-2, 2], K = 16 and scale = 8: scale * s is a multiple of 1/2 of magnitude <= 512, and the
    bias a constant per row from {0, -1000, 1000, -300}: every x is exact in float32, so TOL holds as it does inside the window.
    Rows with a score above 89 (NaN in eg_attention_bias) and rows that first reach their maximum in key tile 1 or 2 exist in
    both runs; a row whose every score is below -104 (0 / 0 as written) needs the bias and is asserted in that run."""
    dims = (1, 2, 70, 150, 16, 16)
    b0, b1, I, J, K, D = dims
    rng = np.random.default_rng(29)
    quarter = lambda *shape: (rng.integers(-8, 9, shape) / 4.0).astype(np.float32)
    given = (quarter(b0, b1, I, K), quarter(b0, b1, J, K), u(rng, b0, b1, J, D), u(rng, b0, b1, I, D))
    case, acc, bases = two_cases(gpu_ctx, dims, given=given, scale=8.0)
    bias, B = 0.0, None
    if biased:
        bias = np.broadcast_to(np.float32([0, -1000, 1000, -300])[np.arange(I) % 4][None, None, :, None], (b0, b1, I, J)).copy()
        B = View(bias, J + 2, b1 * I * (J + 2), I * (J + 2)).upload(gpu_ctx)
    xs = np.einsum("obik,objk->obij", given[0].astype(np.float64), given[1].astype(np.float64)) * 8.0 + bias
    assert np.array_equal(xs, xs.astype(np.float32)) and np.abs(xs).max() <= 1512, "every score is exact in float32"
    above = xs.max(-1) > 89
    assert above.any() and (xs.argmax(-1) >= 64).any() and (not biased or (xs.max(-1) < -104).any())
    o, _ = check_all(gpu_ctx, case, acc, bases, bias, B, "eg_attention_stable out of the window, %s" % ("row bias" if biased else "no bias"), vec=True)
    assert np.all(np.isnan(as_written(case, B)[above])), "eg_attention_bias is NaN where a score passes 89: the case is outside its window"


def test_special_rows(gpu_ctx):
    """The header's table at (1, 1, 70, 150, 16, 16).  Key tile 0 (keys 0 .. 63) is -Inf for every row, so the maximum stays
    -Inf through a whole tile (the subtrahend is 0 there); row 3 has every key masked; row 40 one +Inf; row 50 one NaN.  The
    other rows are the attention over keys 64 .. 149.  The backward: the named rows are NaN in dQ, the others finite."""
    dims = (1, 1, 70, 150, 16, 16)
    case = Case(gpu_ctx, dims, "bihk")
    bias = np.zeros((1, 1, 70, 150), np.float32)
    bias[..., :64] = -np.inf
    bias[0, 0, 3, :] = -np.inf
    bias[0, 0, 40, 140] = np.inf
    bias[0, 0, 50, 5] = np.nan
    B, St = View(bias, 152, 0, 0).upload(gpu_ctx), stats_view(gpu_ctx, dims)
    o_buf, s_buf = forward(case, St, B)
    o, (mx, sums) = case.O.items(o_buf)[0, 0], St.items(s_buf)[0, 0]
    assert np.all(np.isnan(o[[3, 40, 50]])), o[[3, 40, 50]]
    assert mx[3] == -np.inf and sums[3] == 0 and mx[40] == np.inf and np.isnan(sums[40]) and np.isnan(sums[50]), (mx[[3, 40, 50]], sums[[3, 40, 50]])
    rows, keys = np.setdiff1d(np.arange(70), [3, 40, 50]), np.r_[64:150]
    o64, mx64, sums64 = exact(case.q[:, :, rows], case.k[:, :, keys], case.v[:, :, keys], 0.0, case.scale)
    close(o[rows], o64[0, 0], "eg_attention_stable without the masked keys O")
    close(mx[rows], mx64[0, 0], "eg_attention_stable without the masked keys Max")
    close(sums[rows], sums64[0, 0], "eg_attention_stable without the masked keys Sum")
    case.set_d_out(gc.mse_gradient(np.nan_to_num(o)[None, None], case.labels))
    dq = case.dQ.items(backward(case, St, B)[0])[0, 0]
    assert np.all(np.isnan(dq[[3, 40, 50]])) and np.all(np.isfinite(dq[rows]))


def test_a_masked_tile_between_live_tiles_and_no_keys(gpu_ctx):
    """keys 64 .. 127, a whole key tile, at -Inf for every row: the attention over the other keys; and J == 0: O = 0, Sum = 0,
    Max = -Inf, O left alone when accumulating"""
    dims = (1, 1, 70, 150, 16, 16)
    case = Case(gpu_ctx, dims, "bihk")
    bias = np.zeros((1, 1, 1, 150), np.float32)
    bias[..., 64:128] = -np.inf
    St = stats_view(gpu_ctx, dims)
    o_buf, s_buf = forward(case, St, View(bias, 0, 0, 0).upload(gpu_ctx))
    keys = np.r_[0:64, 128:150]
    o64, mx64, sums64 = exact(case.q, case.k[:, :, keys], case.v[:, :, keys], 0.0, case.scale)
    close(case.O.items(o_buf), o64, "eg_attention_stable around a masked tile O")
    close(St.items(s_buf)[:, :, 0], mx64, "eg_attention_stable around a masked tile Max")
    close(St.items(s_buf)[:, :, 1], sums64, "eg_attention_stable around a masked tile Sum")
    case.dims, before = (1, 1, 70, 0, 16, 16), case.O.items(o_buf).copy()
    for accumulate, want in ((True, before), (False, np.zeros_like(before))):
        o_buf, s_buf = forward(case, St, None, accumulate=accumulate)
        assert np.array_equal(case.O.items(o_buf), want) and np.all(St.items(s_buf)[:, :, 0] == -np.inf) and np.all(St.items(s_buf)[:, :, 1] == 0)
        same_outside(case.O, o_buf, "eg_attention_stable J == 0")


def test_refusals(gpu_ctx):
    """every refusal of the header, once per entry: the return code, and the entry's name in the message"""
    dims = (2, 3, 8, 8, 8, 8)
    buf = gpu_ctx.allocTensor((2 * 3 * 8 * 129,))
    p = ctypes.c_void_p(buf.ptr)
    v, lib = (p, 8, 192, 64), _lib.lib()
    ok = dict(dims=dims, st=(p, 8, 48, 16), b=(p, 8, 192, 64), big=False)
    changes = {"lds < I": dict(st=(p, 7, 48, 16)), "overlapping stats": dict(st=(p, 8, 48, 15)), "negative stride_s0": dict(st=(p, 8, -48, 16)),
               "negative stride_b1": dict(b=(p, 8, 192, -64)), "0 < ldb < J": dict(b=(p, 7, 192, 64)),
               "K of 129": dict(dims=(2, 3, 8, 8, 129, 8), big=True), "D of 129": dict(dims=(2, 3, 8, 8, 8, 129), big=True)}
    for name, change in changes.items():
        c = dict(ok, **change)
        w = (p, 129, 3096, 1032) if c["big"] else v
        want = EG_ERR_UNSUPPORTED if c["big"] else EG_ERR_INVALID
        rc = lib.eg_attention_stable(gpu_ctx.handle, *c["dims"], 0.125, *w, *w, *w, *w, 0, *c["st"], *c["b"])
        assert rc == want and "eg_attention_stable:" in _lib.last_error(), (name, rc, _lib.last_error())
        rc = lib.eg_attention_stable_grad(gpu_ctx.handle, *c["dims"], 0.125, *w, *w, *w, *w, *c["st"], *w, *w, *w, *w, 0, *c["b"])
        assert rc == want and "eg_attention_stable_grad:" in _lib.last_error(), (name, rc, _lib.last_error())
