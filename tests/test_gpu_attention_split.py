"""GPU parity of eg_attention_stable_split (kernels/attention_split_f32.hip: the partial kernels of the 64-row and the 16-row
mode and the combine kernel) against the float64 numpy evaluation with the row maximum of test_gpu_attention_stable.py, every
element within TOL: on moderate scores at every mode, bias form and split count; on scores whose weights between splits
underflow, built so that every x is exact in float32; on the special rows of the header's table; through
eg_attention_stable_grad; and bit for bit where the header promises bits.  Operands sit between NaN guards and every output
buffer is compared bit for bit outside its items."""
import ctypes

import numpy as np
import pytest

import attention_grad_cases as gc
from exprgrad_amd import _lib, ops
from test_gpu_attention_bias import close, make_bias, x
from test_gpu_attention_fused import View, u
from test_gpu_attention_grad import Case, bits, same_outside
from test_gpu_attention_stable import exact, stats_view

pytestmark = pytest.mark.gpu

EG_ERR_INVALID = 1
ROWS64 = [((1, 2, 70, 200, 20, 12), 2), ((1, 2, 70, 200, 20, 12), 3), ((1, 2, 70, 200, 20, 12), 4), ((1, 1, 65, 129, 128, 128), 2)]
ROWS16 = [((1, 2, I, 150, 20, 12), s) for I in (1, 5, 16) for s in (1, 3)] + [((1, 1, 16, 129, 128, 128), 2)]


def split(case, St, B, splits, O=None, accumulate=False, entry=ops.attention_stable_split):
    O = O or case.O
    extra = (splits,) if entry is ops.attention_stable_split else ()
    entry(case.ctx, *case.dims, case.scale, *x(case.Q), *x(case.Kk), *x(case.V), *x(O), *x(St), *x(B), accumulate, *extra)
    return O.dev.read(), St.dev.read() if St else None


def check_forward(ctx, case, bias, B, splits, label):
    """O, both Stats rows and O accumulate against float64; (Stats view, the device's O)"""
    b0, b1, I, J, K, D = case.dims
    St = stats_view(ctx, case.dims)
    o_buf, s_buf = split(case, St, B, splits)
    o64, mx64, sums64 = exact(case.q, case.k, case.v, bias, case.scale)
    close(case.O.items(o_buf), o64, label + " O")
    close(St.items(s_buf)[:, :, 0], mx64, label + " Max")
    close(St.items(s_buf)[:, :, 1], sums64, label + " Sum")
    same_outside(case.O, o_buf, label + " O")
    same_outside(St, s_buf, label + " Stats")
    base_o = u(np.random.default_rng(6), b0, b1, I, D)
    Oa = View(base_o, case.O.ld, *case.O.strides).upload(ctx)
    oa_buf, _ = split(case, None, B, splits, O=Oa, accumulate=True)
    close(Oa.items(oa_buf), o64 + base_o, label + " O accumulate")
    same_outside(Oa, oa_buf, label + " O accumulate")
    return St, case.O.items(o_buf).copy()


@pytest.mark.parametrize("form", ["none", "full", "causal"])
@pytest.mark.parametrize("dims,splits", ROWS64 + ROWS16, ids=lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else "s%d" % d)
def test_moderate_scores(gpu_ctx, dims, splits, form):
    """both modes; uneven ranges (4 tiles in 3), a ragged last tile (16-row mode: wave 1 with six live keys, waves 2 and 3 with
    none), the largest heads; `causal`: the later splits are wholly -Inf for the early rows"""
    bias, B = (0.0, None) if form == "none" else make_bias(gpu_ctx, dims, form, seed=sum(dims))
    check_forward(gpu_ctx, Case(gpu_ctx, dims, "bihk"), bias, B, splits, "eg_attention_stable_split %s splits=%d %s" % (dims, splits, form))


@pytest.mark.parametrize("I", [70, 16])
def test_weights_that_underflow(gpu_ctx, I):
    """q and k multiples of 1/4 in [-2, 2], K = 16, scale 8, and a bias of {0, -1000, 1000, -300} that changes with the row and
    the key tile: every x is exact in float32, and with one key tile per split every row has splits whose weight expf(m_s - M)
    is 0 in float32"""
    dims = (1, 2, I, 200, 16, 16)
    b0, b1, _, J, K, D = dims
    rng = np.random.default_rng(29)
    quarter = lambda *shape: (rng.integers(-8, 9, shape) / 4.0).astype(np.float32)
    given = (quarter(b0, b1, I, K), quarter(b0, b1, J, K), u(rng, b0, b1, J, D), u(rng, b0, b1, I, D))
    bias = np.float32([0, -1000, 1000, -300])[(np.arange(I)[:, None] + np.arange(J)[None, :] // 64) % 4][None, None]
    B = View(bias, J + 4, 0, 0).upload(gpu_ctx)
    xs = np.einsum("obik,objk->obij", given[0].astype(np.float64), given[1].astype(np.float64)) * 8.0 + bias
    assert np.array_equal(xs, xs.astype(np.float32)), "every score is exact in float32"
    tile_max = np.stack([xs[..., t:t + 64].max(-1) for t in range(0, J, 64)], -1)
    assert np.all(tile_max.min(-1) < xs.max(-1) - 104), "every row has a split more than 104 below its maximum"
    check_forward(gpu_ctx, Case(gpu_ctx, dims, "bihk", given=given, scale=8.0), bias, B, 4, "eg_attention_stable_split underflow I=%d" % I)


@pytest.mark.parametrize("I", [16, 70])
def test_special_rows(gpu_ctx, I):
    """The header's table at splits = 3: key tile 0, the whole first split, is -Inf for every row; one row has every key masked,
    one a +Inf score, one a NaN score.  The other rows are the attention over keys 64 .. 149."""
    dims = (1, 1, I, 150, 16, 16)
    masked, inf, nan = 3, 4 * I // 7, 5 * I // 7
    case = Case(gpu_ctx, dims, "bihk")
    bias = np.zeros((1, 1, I, 150), np.float32)
    bias[..., :64] = -np.inf
    bias[0, 0, masked, :] = -np.inf
    bias[0, 0, inf, 140] = np.inf
    bias[0, 0, nan, 5] = np.nan
    St = stats_view(gpu_ctx, dims)
    o_buf, s_buf = split(case, St, View(bias, 152, 0, 0).upload(gpu_ctx), 3)
    o, (mx, sums) = case.O.items(o_buf)[0, 0], St.items(s_buf)[0, 0]
    named = [masked, inf, nan]
    assert np.all(np.isnan(o[named])), o[named]
    assert mx[masked] == -np.inf and sums[masked] == 0 and mx[inf] == np.inf and np.isnan(sums[inf]) and np.isnan(sums[nan]), (mx[named], sums[named])
    rows, keys = np.setdiff1d(np.arange(I), named), np.r_[64:150]
    o64, mx64, sums64 = exact(case.q[:, :, rows], case.k[:, :, keys], case.v[:, :, keys], 0.0, case.scale)
    close(o[rows], o64[0, 0], "eg_attention_stable_split without the masked keys O")
    close(mx[rows], mx64[0, 0], "eg_attention_stable_split without the masked keys Max")
    close(sums[rows], sums64[0, 0], "eg_attention_stable_split without the masked keys Sum")


def test_backward_from_the_split_forward(gpu_ctx):
    """eg_attention_stable_grad on O and Stats of the split forward"""
    dims = (1, 2, 16, 150, 20, 12)
    case = Case(gpu_ctx, dims, "bihk")
    St, o = check_forward(gpu_ctx, case, 0.0, None, 3, "eg_attention_stable_split before the backward")
    d_out = gc.mse_gradient(o, case.labels)
    case.set_d_out(d_out)
    ops.attention_stable_grad(gpu_ctx, *dims, case.scale, *x(case.Q), *x(case.Kk), *x(case.V), *x(case.O), *x(St), *x(case.dO), *x(case.dQ), *x(case.dK),
                              *x(case.dV))
    want = exact(case.q, case.k, case.v, 0.0, case.scale, d_out)[3:]
    for name, view, w in zip(("dq", "dk", "dv"), (case.dQ, case.dK, case.dV), want):
        buf = view.dev.read()
        close(view.items(buf), w, "eg_attention_stable_grad after the split forward " + name)
        same_outside(view, buf, name)


@pytest.mark.parametrize("I", [16, 70])
def test_bits(gpu_ctx, I):
    """two runs agree; splits above the key tiles are splits = nt; above 16 rows one split is eg_attention_stable"""
    dims = (1, 2, I, 200, 20, 12)
    case = Case(gpu_ctx, dims, "bihk")
    run = lambda splits, **kw: [bits(b).copy() for b in split(case, stats_view(gpu_ctx, dims), None, splits, **kw)]
    for a, b in ((run(3), run(3)), (run(1000), run(4))) + (((run(1), run(0, entry=ops.attention_stable)),) if I > 16 else ()):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_refusals(gpu_ctx):
    """a negative split count, and one refusal of eg_attention_stable's under this entry's name"""
    buf = gpu_ctx.allocTensor((2 * 3 * 8 * 8,))
    p = ctypes.c_void_p(buf.ptr)
    v, lib = (p, 8, 192, 64), _lib.lib()
    for st, splits in (((p, 8, 48, 16), -1), ((p, 7, 48, 16), 2)):
        rc = lib.eg_attention_stable_split(gpu_ctx.handle, 2, 3, 8, 8, 8, 8, 0.125, *v, *v, *v, *v, 0, *st, *v, splits)
        assert rc == EG_ERR_INVALID and "eg_attention_stable_split:" in _lib.last_error(), (st, splits, rc, _lib.last_error())
