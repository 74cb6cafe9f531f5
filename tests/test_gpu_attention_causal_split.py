"""GPU parity of eg_attention_causal_split (kernels/attention_causal_split_f32.hip: the partial kernels of the 64-row and the
16-row mode and the combine kernel) against the float64 numpy evaluation on the table of -Inf where j > i + offset, every element
within TOL; that keys no row sees are never loaded; bit for bit where the header promises bits; and through
eg_attention_causal_grad.  Operands sit between NaN guards and every output buffer is compared bit for bit outside its items."""
import ctypes

import numpy as np
import pytest

import attention_grad_cases as gc
from exprgrad_amd import _lib, ops
from test_gpu_attention_bias import close, make_bias, x
from test_gpu_attention_causal import table
from test_gpu_attention_fused import View, u
from test_gpu_attention_grad import Case, bits, same_outside
from test_gpu_attention_stable import exact, stats_view

pytestmark = pytest.mark.gpu

EG_ERR_INVALID = 1
SELF = (1, 2, 200, 200, 20, 12)   # n_t = 1, 2, 3, 4; the last row tile has 8 rows
# (dims, offset, chunk).  SELF: chunk 2 -> pieces 1, 1, 2, 2, chunk 3 -> 1, 1, 1, 2: direct finish and combine in one launch, the diagonal
# tile the last of the last piece.  70 x 300: n_t = 5, 5 in three pieces, two cut tiles in the last, a ragged key tile.  130 x 200 offset 37:
# 167 visible keys, waves above a cut tile.  65 x 129: the largest heads.  16-row mode: three tiles in 3 and 2 pieces, the mask in the last
# tile's waves; offset 40: one tile, wave 3 partly beyond the visible keys.
ROWS64 = [(SELF, 0, 1), (SELF, 0, 2), (SELF, 0, 3), ((1, 2, 70, 300, 20, 12), 230, 2), ((1, 2, 130, 200, 20, 12), 37, 1),
          ((1, 1, 65, 129, 128, 128), 64, 1)]
ROWS16 = [((1, 2, I, 150, 20, 12), 150 - I, c) for I in (1, 5, 16) for c in (1, 2)] + [((1, 2, 16, 150, 20, 12), 40, 1), ((1, 1, 16, 129, 128, 128), 113, 1)]


def run(case, St, B, offset, chunk, O=None, accumulate=False):
    O = O or case.O
    kw = {"offset": offset} if chunk is None else {"offset": offset, "chunk": chunk}
    entry = ops.attention_causal if chunk is None else ops.attention_causal_split
    entry(case.ctx, *case.dims, case.scale, *x(case.Q), *x(case.Kk), *x(case.V), *x(O), *x(St), *x(B), accumulate, **kw)
    return O.dev.read(), St.dev.read() if St else None


def check_forward(ctx, case, bias, B, offset, chunk, label):
    """O, both Stats rows and O accumulate against float64 on the table; (Stats view, the device's O)"""
    b0, b1, I, J, K, D = case.dims
    St = stats_view(ctx, case.dims)
    o_buf, s_buf = run(case, St, B, offset, chunk)
    o64, mx64, sums64 = exact(case.q, case.k, case.v, table(case.dims, offset, bias)[0], case.scale)
    close(case.O.items(o_buf), o64, label + " O")
    close(St.items(s_buf)[:, :, 0], mx64, label + " Max")
    close(St.items(s_buf)[:, :, 1], sums64, label + " Sum")
    same_outside(case.O, o_buf, label + " O")
    same_outside(St, s_buf, label + " Stats")
    base_o = u(np.random.default_rng(6), b0, b1, I, D)
    Oa = View(base_o, case.O.ld, *case.O.strides).upload(ctx)
    oa_buf, _ = run(case, None, B, offset, chunk, O=Oa, accumulate=True)
    close(Oa.items(oa_buf), o64 + base_o, label + " O accumulate")
    same_outside(Oa, oa_buf, label + " O accumulate")
    return St, case.O.items(o_buf).copy()


@pytest.mark.parametrize("form", ["none", "full"])
@pytest.mark.parametrize("dims,offset,chunk", ROWS64 + ROWS16, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_values(gpu_ctx, dims, offset, chunk, form):
    bias, B = (0.0, None) if form == "none" else make_bias(gpu_ctx, dims, form, seed=sum(dims))
    check_forward(gpu_ctx, Case(gpu_ctx, dims, "bihk"), bias, B, offset, chunk, "eg_attention_causal_split %s offset %d chunk %d %s" % (dims, offset, chunk, form))


@pytest.mark.parametrize("I", [33, 16])
def test_keys_that_no_row_sees_are_never_loaded(gpu_ctx, I):
    """offset 0 < J - I with V NaN at keys >= I: O is finite and is the attention over the first I keys"""
    dims = (2, 3, I, 200, 16, 16)
    q, k, v, labels = gc.inputs(dims, None)
    v = v.copy()
    v[:, :, I:] = np.nan
    case = Case(gpu_ctx, dims, "bihk", given=(q, k, v, labels))
    o_buf, _ = run(case, stats_view(gpu_ctx, dims), None, 0, 1)
    t, _ = table((2, 3, I, I, 16, 16), 0, 0.0)
    close(case.O.items(o_buf), exact(q, k[:, :, :I], v[:, :, :I], t, case.scale)[0], "eg_attention_causal_split with NaN in V beyond the visible keys")


def test_bits(gpu_ctx):
    """two runs agree; a chunk above every row tile is eg_attention_causal; the row tiles with one piece have its bits"""
    case = Case(gpu_ctx, SELF, "bihk")

    def both(chunk, c=case, offset=0):
        St = stats_view(gpu_ctx, c.dims)
        o_buf, s_buf = run(c, St, None, offset, chunk)
        return bits(c.O.items(o_buf)).copy(), bits(St.items(s_buf)).copy()

    causal, two = both(None), both(2)
    for a, b in zip(two, both(2)):
        assert np.array_equal(a, b)
    for a, b in zip(causal, both(1000)):
        assert np.array_equal(a, b)
    assert np.array_equal(two[0][:, :, :128], causal[0][:, :, :128]) and np.array_equal(two[1][..., :128], causal[1][..., :128])
    small = Case(gpu_ctx, (1, 2, 16, 150, 20, 12), "bihk")
    for a, b in zip(both(1, small, 134), both(1, small, 134)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("dims,offset,chunk", [(SELF, 0, 2), ((1, 2, 16, 150, 20, 12), 134, 1)], ids=["rows64", "rows16"])
def test_backward_from_it(gpu_ctx, dims, offset, chunk):
    """eg_attention_causal_grad on O and Stats of this forward"""
    case = Case(gpu_ctx, dims, "bihk")
    St, o = check_forward(gpu_ctx, case, 0.0, None, offset, chunk, "eg_attention_causal_split before the backward")
    d_out = gc.mse_gradient(o, case.labels)
    case.set_d_out(d_out)
    ops.attention_causal_grad(gpu_ctx, *dims, case.scale, *x(case.Q), *x(case.Kk), *x(case.V), *x(case.O), *x(St), *x(case.dO), *x(case.dQ), *x(case.dK),
                              *x(case.dV), offset=offset)
    want = exact(case.q, case.k, case.v, table(dims, offset, 0.0)[0], case.scale, d_out)[3:]
    for name, view, w in zip(("dq", "dk", "dv"), (case.dQ, case.dK, case.dV), want):
        buf = view.dev.read()
        close(view.items(buf), w, "eg_attention_causal_grad after the chunked forward " + name)
        same_outside(view, buf, name)


def test_refusals(gpu_ctx):
    """a negative chunk, a negative offset, and one refusal of eg_attention_causal's under this entry's name"""
    buf = gpu_ctx.allocTensor((2 * 3 * 8 * 8,))
    p = ctypes.c_void_p(buf.ptr)
    v, lib = (p, 8, 192, 64), _lib.lib()
    for st, offset, chunk in (((p, 8, 48, 16), 0, -1), ((p, 8, 48, 16), -1, 1), ((p, 7, 48, 16), 0, 2)):
        rc = lib.eg_attention_causal_split(gpu_ctx.handle, 2, 3, 8, 8, 8, 8, 0.125, *v, *v, *v, *v, 0, *st, *v, offset, chunk)
        assert rc == EG_ERR_INVALID and "eg_attention_causal_split:" in _lib.last_error(), (st, offset, chunk, rc, _lib.last_error())
