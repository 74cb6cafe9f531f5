"""GPU parity of eg_attention_causal and eg_attention_causal_grad (kernels/attention_causal_f32.hip, attention_grad_causal_f32.hip,
attention_grad_causal_bias_f32.hip): key j is visible to row i iff j <= i + offset, and key tiles without a visible key are never
visited.  The reference is eg_attention_stable / eg_attention_stable_grad on the same operands with a bias table of -Inf at the
masked pairs and the given bias (or +0) elsewhere: O, both Stats rows, dQ, dK and dV must have its bits (np.array_equal: a sign
of zero aside), and be within TOL of the float64 evaluation with that table.  Operands sit between NaN guards and every output
buffer is compared bit for bit outside its items."""
import ctypes

import numpy as np
import pytest

import attention_grad_cases as gc
from exprgrad_amd import _lib, ops
from test_gpu_attention_bias import close, make_bias, x
from test_gpu_attention_fused import View
from test_gpu_attention_grad import Case, same_outside
from test_gpu_attention_stable import exact, stats_view, two_cases

pytestmark = pytest.mark.gpu

EG_ERR_INVALID = 1
# per shape: one cut tile, two cut tiles, a cut off the multiples of 16 and 64, the ragged key tile as a row tile's last, nothing masked
CASES = [((2, 3, 33, 70, 16, 16), (0, 40, 75)), ((1, 2, 130, 129, 20, 12), (0, 1, 65)), ((1, 2, 130, 200, 128, 128), (0, 40, 70))]


def table(dims, offset, bias):
    """the reference's bias [b0 or 1, b1 or 1, I, J]: -Inf where j > i + offset, the given bias or +0 elsewhere; and its View"""
    b0, b1, I, J, _, _ = dims
    masked = np.arange(J)[None, :] > np.arange(I)[:, None] + offset
    t = np.where(masked, -np.inf, bias).astype(np.float32) + np.zeros((1, 1, 1, 1), np.float32)
    ld = 4 * (J // 4 + 1)
    return t, (View(t, ld, b1 * I * ld, I * ld) if t.shape[:2] == (b0, b1) else View(t, ld, 0, 0))


def run(case, St, B, offset=None, accumulate=0):
    """forward into case.O and St, dO from that O, backward: eg_attention_causal and its grad, or with offset None the stable pair"""
    kw = {} if offset is None else {"offset": offset}
    fwd, bwd = (ops.attention_stable, ops.attention_stable_grad) if offset is None else (ops.attention_causal, ops.attention_causal_grad)
    fwd(case.ctx, *case.dims, case.scale, *x(case.Q), *x(case.Kk), *x(case.V), *x(case.O), *x(St), *x(B), **kw)
    o_buf, s_buf = case.O.dev.read(), St.dev.read()
    case.set_d_out(gc.mse_gradient(case.O.items(o_buf).copy(), case.labels))
    bwd(case.ctx, *case.dims, case.scale, *x(case.Q), *x(case.Kk), *x(case.V), *x(case.O), *x(St), *x(case.dO), *x(case.dQ), *x(case.dK), *x(case.dV),
        *x(B), accumulate, **kw)
    return [(case.O, o_buf), (St, s_buf), (case.dQ, case.dQ.dev.read()), (case.dK, case.dK.dev.read()), (case.dV, case.dV.dev.read())]


@pytest.mark.parametrize("form", ["none", "full"])
@pytest.mark.parametrize("dims,offset", [(d, o) for d, offsets in CASES for o in offsets], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_same_bits_as_the_masked_table(gpu_ctx, dims, offset, form):
    bias, B = (0.0, None) if form == "none" else make_bias(gpu_ctx, dims, form, seed=sum(dims))
    t, T = table(dims, offset, bias)
    T.upload(gpu_ctx)
    mine, mine_acc, bases = two_cases(gpu_ctx, dims)
    ref, ref_acc, _ = two_cases(gpu_ctx, dims)
    for bit, base, a, b in ((0, {}, mine, ref), (7, bases, mine_acc, ref_acc)):
        label = "eg_attention_causal %s offset %d %s accumulate=%d" % (dims, offset, form, bit)
        got = run(a, stats_view(gpu_ctx, dims), B, offset, bit)
        want = run(b, stats_view(gpu_ctx, dims), T, None, bit)
        o64, mx64, sums64, dq64, dk64, dv64 = exact(a.q, a.k, a.v, t, a.scale, a.d_out)
        stats64 = np.stack([mx64, sums64], 2)
        for name, (view, buf), (rview, rbuf), w64 in zip(("O", "Stats", "dq", "dk", "dv"), got, want, (o64, stats64, dq64, dk64, dv64)):
            assert np.array_equal(view.items(buf), rview.items(rbuf)), "%s %s: not the bits of the stable entry on the table" % (label, name)
            same_outside(view, buf, "%s %s" % (label, name))
            for row in range(2 if name == "Stats" else 1):   # the maxima and the sums each against their own largest value
                part = (lambda z: z[:, :, row]) if name == "Stats" else (lambda z: z)
                close(part(view.items(buf)), part(w64) + base.get(name, 0.0), "%s %s" % (label, name))


def test_keys_that_no_row_sees_are_never_loaded(gpu_ctx):
    """offset 0 < J - I: keys j > I - 1 are visible to no row.  With V NaN there, O is finite and is the attention over the first I keys:
    those keys are not loaded.  The table of -Inf computes 0 * NaN for them."""
    dims = (2, 3, 33, 70, 16, 16)
    q, k, v, labels = gc.inputs(dims, None)
    v = v.copy()
    v[:, :, 33:] = np.nan
    case, St = Case(gpu_ctx, dims, "bihk", given=(q, k, v, labels)), stats_view(gpu_ctx, dims)
    ops.attention_causal(gpu_ctx, *dims, case.scale, *x(case.Q), *x(case.Kk), *x(case.V), *x(case.O), *x(St), offset=0)
    t, _ = table((2, 3, 33, 33, 16, 16), 0, 0.0)
    close(case.O.items(case.O.dev.read()), exact(q, k[:, :, :33], v[:, :, :33], t, case.scale)[0], "eg_attention_causal with NaN in V beyond the visible keys")


def test_refusals(gpu_ctx):
    """a negative offset and one inherited refusal per entry: the return code, and the entry's name in the message"""
    buf = gpu_ctx.allocTensor((2 * 3 * 8 * 8,))
    p, lib = ctypes.c_void_p(buf.ptr), _lib.lib()
    v, st = (p, 8, 192, 64), (p, 8, 48, 16)
    for name, offset, stats, b in (("offset", -1, st, v), ("lds < I", 0, (p, 7, 48, 16), v), ("0 < ldb < J", 0, st, (p, 7, 192, 64))):
        rc = lib.eg_attention_causal(gpu_ctx.handle, 2, 3, 8, 8, 8, 8, 0.125, *v, *v, *v, *v, 0, *stats, *b, offset)
        assert rc == EG_ERR_INVALID and "eg_attention_causal:" in _lib.last_error(), (name, rc, _lib.last_error())
        rc = lib.eg_attention_causal_grad(gpu_ctx.handle, 2, 3, 8, 8, 8, 8, 0.125, *v, *v, *v, *v, *stats, *v, *v, *v, *v, 0, *b, offset)
        assert rc == EG_ERR_INVALID and "eg_attention_causal_grad:" in _lib.last_error(), (name, rc, _lib.last_error())
