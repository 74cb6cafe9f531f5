"""The fused attention kernels (kernels/attention_f32.hip, kernels/attention_grad_f32.hip) at every pair of padded head sizes,
element by element, and across a cut into two launches.

a. The head table.  Each of the four kernels is compiled once per (kp, dp) with kp, dp in {32, 64, 128}
   (attention_tile.hpp dispatch_heads).  Where kp != dp a mix-up of the two — an LDS row stride, a tile's base offset, an
   unroll count, the LDS bytes of the launch — shows; on the diagonal it cannot.  HEADS has one small shape per pair, with K
   and D at the edges of the instantiations, a second query tile and, on the pairs no other test reaches, three key tiles
   with a ragged last one.  test_the_table_reaches_every_instantiation holds the table to the two planners without a device.
   Each row runs eg_attention, eg_attention_sums and eg_attention_grad against float64 within conftest.TOL, in both layouts,
   and with every pointer one float off 16-byte alignment.  The oracle is not consulted: it has not been held to float64 on
   these shapes.
b. The exact cases of tests/attention_exact_cases.py: every element of O, Sums, dQ, dK and dV to its own bits
   (tests/test_attention_exact_cases_cpu.py proves the expected values without a kernel).
c. (2051, 2047) items of one block each: 2^22 + 4093 blocks, so a second launch that starts at item 2^22 = (2049, 1), with
   first_inner != 0, for the forward with sums and for both backward kernels.

As in tests/test_gpu_attention_grad.py every operand sits between NaN guards and every output buffer keeps its bits outside
the items."""
import numpy as np
import pytest

import attention_exact_cases as ec
import attention_grad_cases as gc
from conftest import TOL, rel_err
from test_attention_grad_plan_cpu import driver as grad_plan_driver, plan as grad_plan     # noqa: F401 (a fixture)
from test_attention_plan_cpu import driver as forward_plan_driver, plan as forward_plan     # noqa: F401 (a fixture)
from test_gpu_attention_fused import View, check
from test_gpu_attention_grad import Case, bits, check_grads, out_view, same_outside

gpu = pytest.mark.gpu
LAYOUTS = ["bihk", "bhik"]
ident = ec.ident

# (kp, dp) -> (batch0, batch1, I, J, K, D)
HEADS = {
    (32, 64): (1, 2, 65, 130, 32, 33),
    (32, 128): (1, 2, 65, 130, 17, 65),
    (64, 128): (1, 2, 65, 130, 64, 128),
    (128, 32): (1, 2, 65, 130, 65, 32),
    (128, 64): (1, 2, 65, 130, 128, 40),
    (64, 32): (1, 2, 65, 63, 33, 20),
    (32, 32): (2, 1, 66, 63, 32, 32),
    (64, 64): (1, 2, 65, 63, 40, 64),
    (128, 128): (1, 1, 70, 65, 100, 65),
}
ROWS = sorted(HEADS.items())
ROW_IDS = ["kp%d-dp%d-%s" % (kp, dp, ident(d)) for (kp, dp), d in ROWS]


def test_the_table_reaches_every_instantiation(forward_plan_driver, grad_plan_driver):
    """no device: both planners pad each row's K and D to the pair it is listed under, and the pairs are all nine"""
    assert sorted(HEADS) == [(kp, dp) for kp in (32, 64, 128) for dp in (32, 64, 128)]
    for (kp, dp), dims in ROWS:
        fwd, bwd = forward_plan(forward_plan_driver, *dims), grad_plan(grad_plan_driver, *dims)
        assert (fwd["supported"], fwd["kp"], fwd["dp"]) == (1, kp, dp), (dims, fwd)
        assert (bwd["supported"], bwd["kp"], bwd["dp"]) == (1, kp, dp), (dims, bwd)
    for table in ([d for d, _ in ec.UNIFORM_FORWARD], [d for d, _ in ec.UNIFORM_BACKWARD], ec.SELECTOR):
        pairs = set()
        for dims in table:
            fwd, bwd = forward_plan(forward_plan_driver, *dims), grad_plan(grad_plan_driver, *dims)
            assert (fwd["kp"], fwd["dp"]) == (bwd["kp"], bwd["dp"])
            pairs.add((fwd["kp"], fwd["dp"]))
        assert any(kp == dp for kp, dp in pairs) and sum(kp != dp for kp, dp in pairs) >= 3, pairs


# ---- a. the head table ------------------------------------------------------------------------------------------------------
def run_row(ctx, pair, dims, layout, what, **kw):
    """eg_attention, eg_attention_sums and eg_attention_grad on one Case: each against float64 within TOL, O of the two forward
    entries bit-equal, nothing stored outside the items; prints the errors"""
    b0, b1, I, J, K, D = dims
    case = Case(ctx, dims, layout, **kw)
    label = "heads kp=%d dp=%d %s %s %s" % (pair + (ident(dims), layout, what))
    plain = out_view(ctx, layout, (b0, b1, I, D), case.offset, None)
    o_plain, _ = case.forward(sums=False, O=plain)
    check(dims, label + " eg_attention", (case.q, case.k, case.v), plain, o_plain, with_oracle=False)
    bufs = case.run()       # eg_attention_sums, dO = 2 (O - labels) / N, eg_attention_grad
    o_sums, s_buf = case.O.dev.read(), case.S.dev.read()
    assert np.array_equal(bits(o_sums), bits(o_plain)), label + ": O of eg_attention_sums differs from eg_attention's"
    o64, sums64, dq64, dk64, dv64 = case.exact()
    sums = case.S.items(s_buf)[:, :, 0, :]
    errs = {"O": rel_err(case.O.items(o_sums), o64, label + " O vs float64"), "Sums": rel_err(sums, sums64, label + " Sums vs float64")}
    for name, view, buf, want in (("dQ", case.dQ, bufs[0], dq64), ("dK", case.dK, bufs[1], dk64), ("dV", case.dV, bufs[2], dv64)):
        errs[name] = rel_err(view.items(buf), want, "%s %s vs float64" % (label, name))
    print(label, "vs float64:", " ".join("%s %.3g" % kv for kv in errs.items()), "| largest %.3g of TOL %g" % (max(errs.values()), TOL))
    assert np.all(np.isfinite(sums)) and errs["Sums"] <= TOL, (label, errs)
    same_outside(case.S, s_buf, label + " Sums")
    same_outside(case.O, o_sums, label + " O")
    check_grads(case, label + " eg_attention_grad", bufs, with_oracle=False)
    return case


@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("pair,dims", ROWS, ids=ROW_IDS)
def test_head_table(gpu_ctx, pair, dims, layout):
    """outputs of NaN, operands between NaN guards, at aligned pointers"""
    run_row(gpu_ctx, pair, dims, layout, "aligned")


@gpu
@pytest.mark.parametrize("pair,dims", ROWS, ids=ROW_IDS)
def test_head_table_with_pointers_offset_by_one_float(gpu_ctx, pair, dims):
    """no operand is 16-byte aligned: the element path of load_rows<WP> and of every store of that instantiation"""
    case = run_row(gpu_ctx, pair, dims, "bhik", "offset 1", offset=1)
    assert all(x.ptr % 16 != 0 for x in (case.Q, case.Kk, case.V, case.O, case.S, case.dO, case.dQ, case.dK, case.dV))


@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_keys_and_values_shared_along_the_inner_batch_index(gpu_ctx, layout):
    """stride1 = 0 for Kk and V on a mixed pair; dK and dV stay distinct per item"""
    pair = (64, 128)
    case = run_row(gpu_ctx, pair, HEADS[pair], layout, "shared inner", shared="inner")
    assert case.Kk.strides[1] == 0 and case.V.strides[1] == 0 and case.Kk.strides[0] > 0 and case.dK.strides[1] > 0 and case.dV.strides[1] > 0


# ---- b. the exact cases -----------------------------------------------------------------------------------------------------
FORWARD, BACKWARD = ec.forward_cases(), ec.backward_cases()


def exact_forward(ctx, ex, layout, label):
    """eg_attention_sums and eg_attention on the case's operands: O and Sums to their bits, by both entries"""
    b0, b1, I, J, K, D = ex.dims
    case = Case(ctx, ex.dims, layout, given=(ex.q, ex.k, ex.v, None), scale=ec.SCALE)
    o_buf, s_buf = case.forward()
    ec.same_values(case.O.items(o_buf), ex.want["o"], label + " O")
    ec.same_values(case.S.items(s_buf)[:, :, 0, :], ex.want["sums"], label + " Sums")
    same_outside(case.O, o_buf, label + " O")
    same_outside(case.S, s_buf, label + " Sums")
    plain = out_view(ctx, layout, (b0, b1, I, D), 0, None)
    o_plain, _ = case.forward(sums=False, O=plain)
    assert np.array_equal(bits(o_plain), bits(o_buf)), label + ": eg_attention differs from eg_attention_sums"
    return case


@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("make", [m for _, m in FORWARD], ids=[n for n, _ in FORWARD])
def test_exact_forward(gpu_ctx, make, layout):
    ex = make()
    exact_forward(gpu_ctx, ex, layout, "exact forward %s %s %s" % (ex.family, ident(ex.dims), layout))


@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("make", [m for _, m in BACKWARD], ids=[n for n, _ in BACKWARD])
def test_exact_backward(gpu_ctx, make, layout):
    """the forward's O and Sums (held to their bits first) and the case's dO into eg_attention_grad: the gradients the case
    claims to their bits, the others finite"""
    ex = make()
    label = "exact backward %s %s %s" % (ex.family, ident(ex.dims), layout)
    case = exact_forward(gpu_ctx, ex, layout, label)
    case.set_d_out(ex.d_out)
    bufs = case.backward()
    for name, view, buf in (("dq", case.dQ, bufs[0]), ("dk", case.dK, bufs[1]), ("dv", case.dV, bufs[2])):
        got = view.items(buf)
        if ex.want[name] is None:
            assert np.all(np.isfinite(got)), (label, name)
        else:
            ec.same_values(got, ex.want[name], "%s %s" % (label, name))
        same_outside(view, buf, "%s %s" % (label, name))


# ---- c. a cut with two launches ---------------------------------------------------------------------------------------------
CUT = (2051, 2047, 1, 2, 1, 1)
NAMED = {"2^22 - 1": (2049, 0), "2^22": (2049, 1), "the last": (2050, 2046)}


def cut_case(ctx):
    """Q and the labels (dO, in the backward) distinct per item, Kk and V shared along both batch indices; tight row sums (two floats per item)"""
    b0, b1, I, J, K, D = CUT
    assert b0 * b1 == (1 << 22) + 4093 and all(o * b1 + i == n for n, (o, i) in zip(((1 << 22) - 1, 1 << 22, b0 * b1 - 1), NAMED.values()))
    rng = np.random.default_rng(22)
    q, labels = gc.u(rng, b0, b1, I, K) * np.float32(8), gc.u(rng, b0, b1, I, D)
    k, v = np.array([0.75, -0.5], np.float32).reshape(1, 1, J, K), np.array([1.0, -0.25], np.float32).reshape(1, 1, J, D)
    case = Case(ctx, CUT, "bihk", given=(q, k, v, labels), shared="both")
    case.S = View(np.full((b0, b1, 1, I), np.nan, np.float32), I, 2 * b1 + 1, 2).upload(ctx)
    assert case.Kk.strides == (0, 0) and case.V.strides == (0, 0)
    return case


def held(got, want, label):
    """every item within TOL of float64, relative to the largest value; the three named items on their own"""
    err = rel_err(got, want, label + " vs float64")
    print(label, "vs float64", err, "over", got.shape[0] * got.shape[1], "items")
    assert np.all(np.isfinite(got)) and err <= TOL, (label, err)
    top = np.max(np.abs(want))
    for name, (o, i) in NAMED.items():
        assert np.all(np.abs(got[o, i] - want[o, i]) <= TOL * top), "%s: item %s = (%d, %d): got %r, want %r" % (label, name, o, i, got[o, i], want[o, i])


@gpu
def test_sums_across_a_cut(gpu_ctx):
    """eg_attention_sums: the second launch starts at outer index 2049, inner index 1"""
    case = cut_case(gpu_ctx)
    o_buf, s_buf = case.forward()
    o64, sums64, _, _, _ = gc.closed_form(case.q, case.k, case.v, np.zeros(case.q.shape[:3] + (1,)), case.scale)
    held(case.O.items(o_buf), o64, "eg_attention_sums across a cut O")
    held(case.S.items(s_buf), sums64[:, :, None, :], "eg_attention_sums across a cut Sums")
    same_outside(case.O, o_buf, "O")
    same_outside(case.S, s_buf, "Sums")


@gpu
def test_grad_across_a_cut(gpu_ctx):
    """eg_attention_grad on O and Sums computed on the host (float64, rounded): both kernels' second launches"""
    case = cut_case(gpu_ctx)
    o64, sums64, _, _, _ = gc.closed_form(case.q, case.k, case.v, np.zeros(case.q.shape[:3] + (1,)), case.scale)
    for view, x in ((case.O, o64), (case.S, sums64[:, :, None, :])):
        view.items(view.buf)[...] = x.astype(np.float32)
        view.dev.write(view.buf)
    case.set_d_out(case.labels)
    bufs = case.backward()
    _, _, dq, dk, dv = case.exact()
    for name, view, buf, want in (("dQ", case.dQ, bufs[0], dq), ("dK", case.dK, bufs[1], dk), ("dV", case.dV, bufs[2], dv)):
        held(view.items(buf), want, "eg_attention_grad across a cut " + name)
        same_outside(view, buf, name)
