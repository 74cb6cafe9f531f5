"""GPU parity of eg_attention_sums and eg_attention_grad (kernels/attention_f32.hip, kernels/attention_grad_f32.hip) on the
shapes of tests/attention_grad_cases.py, in both layouts of tests/test_gpu_attention_fused.py:

  - eg_attention_sums: O bit-equal to eg_attention on the same views, Sums within TOL (1e-5 of the largest value) of float64;
  - eg_attention_grad on that O, those Sums and dO = 2 (O - labels) / N computed on the host in float32 (what the mse of the
    training program hands back): dQ, dK and dV within TOL of the float64 closed form on the same inputs, and within TOL of the
    oracle's gradients of q, kk and v (`last[gtid]` after run_backward("fit")) on the same parameters and labels.
    tests/test_attention_grad_oracle_cpu.py holds the oracle itself to 5e-6 of float64 on these shapes.

Every operand sits between NaN guards in a larger allocation (a read outside a view shows up as NaN), and every output buffer
is compared bit for bit with its state before the call outside the items."""
import ctypes

import numpy as np
import pytest

import attention_grad_cases as gc
from conftest import TOL, rel_err
from exprgrad_amd import _lib, ops
from test_gpu_attention_fused import POISON, View, lay, poisoned, u

pytestmark = pytest.mark.gpu

EG_ERR_INVALID, EG_ERR_UNSUPPORTED = 1, 5
SCALE = gc.SCALE
LAYOUTS = ["bihk", "bhik"]
OFFSET_SHAPES = [(2, 3, 33, 70, 16, 16), (2, 1, 64, 64, 64, 64), (3, 2, 7, 200, 33, 1)]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def same_outside(view, got_buf, label):
    """everything of the buffer but the items has the bits it was uploaded with"""
    want = view.buf.copy()
    view.items(want)[...] = view.items(got_buf)
    assert np.array_equal(bits(got_buf), bits(want)), label + ": stored outside the items"


def out_view(ctx, layout, shape, offset, pad, init=None):
    """An output [b0, b1, R, C] filled with NaN (or `init`): rows padded by 3 floats in "bihk" (no 16-byte stores), to the next
    multiple of 4 above C in "bhik" (16-byte stores at offset 0), or by `pad` when given."""
    b0, b1, R, C = shape
    if pad is None:
        pad = 3 if layout == "bihk" else 4 - C % 4
    ld, s0, s1 = lay(layout, b1, R, C, pad)
    x = np.full(shape, np.nan, np.float32) if init is None else init
    return View(x, ld, s0, s1, offset).upload(ctx)


def sums_view(ctx, layout, b0, b1, I, offset):
    """[b0, b1, 1, I]: items of I floats with NaN between them; strides multiples of 4 in "bhik" only"""
    s1 = I + 3 if layout == "bihk" else 4 * (I // 4 + 1)
    s0 = b1 * s1 + (2 if layout == "bihk" else 0)
    return View(np.full((b0, b1, 1, I), np.nan, np.float32), I, s0, s1, offset).upload(ctx)


class Case:
    """The operands of one call on the device: inputs from attention_grad_cases.inputs (or `given`: q, k, v, labels), outputs of
    NaN.  shared: Kk and V have stride 0 along batch0 (True), along batch1 ("inner") or along both ("both")."""

    def __init__(self, ctx, dims, layout, seed=None, offset=0, pad=0, shared=False, out_pad=None, bases=None, given=None, scale=SCALE):
        b0, b1, I, J, K, D = dims
        self.ctx, self.dims, self.layout, self.scale = ctx, dims, layout, scale
        self.q, self.k, self.v, self.labels = given or gc.inputs(dims, seed)
        outer, inner = shared in (True, "both"), shared in ("inner", "both")
        if outer:
            self.k, self.v = self.k[:1], self.v[:1]
        if inner:
            self.k, self.v = self.k[:, :1], self.v[:, :1]
        ldq, q0, q1 = lay(layout, b1, I, K, pad)
        ldk, k0, k1 = lay(layout, b1, J, K, pad)
        ldv, v0, v1 = lay(layout, b1, J, D, pad)
        self.layo = lay(layout, b1, I, D, pad)
        self.offset = offset
        self.Q = View(self.q, ldq, q0, q1, offset).upload(ctx)
        self.Kk = View(self.k, ldk, 0 if outer else k0, 0 if inner else k1, offset).upload(ctx)
        self.V = View(self.v, ldv, 0 if outer else v0, 0 if inner else v1, offset).upload(ctx)
        self.O = out_view(ctx, layout, (b0, b1, I, D), offset, out_pad)
        self.S = sums_view(ctx, layout, b0, b1, I, offset)
        bases = bases or {}
        self.dQ = out_view(ctx, layout, (b0, b1, I, K), offset, out_pad, bases.get("dq"))
        self.dK = out_view(ctx, layout, (b0, b1, J, K), offset, out_pad, bases.get("dk"))
        self.dV = out_view(ctx, layout, (b0, b1, J, D), offset, out_pad, bases.get("dv"))
        self.dO = None

    def forward(self, sums=True, O=None, accumulate=False):
        """eg_attention_sums (or eg_attention) into O; the O and Sums buffers as read back"""
        O = O or self.O
        args = (self.ctx,) + self.dims + (self.scale, self.Q, self.Q.ld, self.Q.strides, self.Kk, self.Kk.ld, self.Kk.strides, self.V, self.V.ld,
                                          self.V.strides, O, O.ld, O.strides)
        if sums:
            ops.attention_sums(*args, self.S, self.S.strides, accumulate)
        else:
            ops.attention(*args, accumulate)
        return O.dev.read(), self.S.dev.read()

    def set_d_out(self, d_out):
        ld, s0, s1 = self.layo
        self.d_out = d_out
        self.dO = View(d_out, ld, s0, s1, self.offset).upload(self.ctx)

    def backward(self, accumulate=0, O=None):
        O = O or self.O
        x = lambda t: (t, t.ld, t.strides)
        ops.attention_grad(self.ctx, *self.dims, self.scale, *x(self.Q), *x(self.Kk), *x(self.V), *x(O), self.S, self.S.strides, *x(self.dO), *x(self.dQ),
                           *x(self.dK), *x(self.dV), accumulate)
        return self.dQ.dev.read(), self.dK.dev.read(), self.dV.dev.read()

    def run(self, accumulate=0):
        """forward with sums, dO from the device's O and the labels on the host, backward; the three output buffers"""
        o_buf, _ = self.forward()
        self.o = self.O.items(o_buf).copy()
        self.set_d_out(gc.mse_gradient(self.o, self.labels))
        return self.backward(accumulate)

    def exact(self):
        return gc.closed_form(self.q, self.k, self.v, self.d_out, self.scale)


def check_grads(case, label, bufs, with_oracle, bases=None):
    """dQ, dK and dV against the float64 closed form (and the oracle), relative to the largest value; where the exact gradient
    is zero everywhere (one key: p = 1, dS = 0) rel_err holds the device, and its distance from the oracle, to TOL in absolute
    terms.  Everything else of the three buffers bit-unchanged."""
    _, _, dq, dk, dv = case.exact()
    oracle = gc.oracle_run(case.dims) if with_oracle else None
    for name, oname, view, buf, want64 in (("dQ", "q", case.dQ, bufs[0], dq), ("dK", "kk", case.dK, bufs[1], dk), ("dV", "v", case.dV, bufs[2], dv)):
        got = view.items(buf).copy()
        base = (bases or {}).get(name.lower())
        if base is not None:
            want64 = want64 + base.astype(np.float64)
        e64 = rel_err(got, want64, "%s %s vs float64" % (label, name))
        e_or = 0.0
        if with_oracle and np.any(want64):
            e_or = rel_err(got, oracle["f32"][oname], "%s %s vs oracle" % (label, name))
        elif with_oracle:   # a gradient that is exactly zero: the oracle's own value is rounding noise with no largest value to
            e_or = rel_err(got - oracle["f32"][oname], want64, "%s %s vs oracle" % (label, name))   # relate to; absolute, as rel_err does
        print(label, name, "vs float64", e64, "vs oracle", e_or if with_oracle else "-")
        assert np.all(np.isfinite(got)), (label, name)
        assert e64 <= TOL and e_or <= TOL, (label, name, e64, e_or)
        same_outside(view, buf, "%s %s" % (label, name))


# ---- eg_attention_sums ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", gc.SHAPES, ids=gc.IDS)
def test_sums_table(gpu_ctx, dims, layout):
    """O has eg_attention's bits with and without Sums; Sums is within TOL of float64 and nothing else of its buffer changes"""
    b0, b1, I, J, K, D = dims
    case = Case(gpu_ctx, dims, layout)
    o_sums, s_buf = case.forward()
    plain = out_view(gpu_ctx, layout, (b0, b1, I, D), 0, None)
    o_plain, _ = case.forward(sums=False, O=plain)
    assert np.array_equal(bits(o_sums), bits(o_plain)), "O differs from eg_attention's"
    null = out_view(gpu_ctx, layout, (b0, b1, I, D), 0, None)
    ops.attention_sums(gpu_ctx, *dims, SCALE, case.Q, case.Q.ld, case.Q.strides, case.Kk, case.Kk.ld, case.Kk.strides, case.V, case.V.ld,
                       case.V.strides, null, null.ld, null.strides, None, (0, 0))
    assert np.array_equal(bits(null.dev.read()), bits(o_plain)), "Sums = NULL differs from eg_attention"
    o64, sums64, _, _, _ = gc.closed_form(case.q, case.k, case.v, np.zeros((b0, b1, I, D)))
    got = case.S.items(s_buf)[:, :, 0, :]
    err = rel_err(got, sums64, "eg_attention_sums %s %s vs float64" % (dims, layout))
    print("eg_attention_sums", dims, layout, "vs float64", err, "O", rel_err(case.O.items(o_sums), o64))
    assert np.all(np.isfinite(got)) and err <= TOL, err
    same_outside(case.S, s_buf, "Sums")
    same_outside(case.O, o_sums, "O")


def test_sums_are_overwritten_while_o_accumulates(gpu_ctx):
    dims = (1, 2, 65, 63, 20, 12)
    case = Case(gpu_ctx, dims, "bihk")
    first, s_first = case.forward()
    base = u(np.random.default_rng(3), 1, 2, 65, 12)
    acc = View(base, case.O.ld, case.O.strides[0], case.O.strides[1]).upload(gpu_ctx)
    got, s_second = case.forward(O=acc, accumulate=True)
    plain = View(base, case.O.ld, case.O.strides[0], case.O.strides[1]).upload(gpu_ctx)
    want, _ = case.forward(sums=False, O=plain, accumulate=True)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(s_first), bits(s_second))


# ---- eg_attention_grad ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", gc.SHAPES, ids=gc.IDS)
def test_grad_table(gpu_ctx, dims, layout):
    """all bits clear over outputs of NaN, operands between NaN guards, at aligned pointers"""
    case = Case(gpu_ctx, dims, layout)
    check_grads(case, "eg_attention_grad %s %s" % (dims, layout), case.run(), with_oracle=True)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", OFFSET_SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_pointers_offset_by_one_float(gpu_ctx, dims, layout):
    """no operand is 16-byte aligned: the element path of every load and store"""
    case = Case(gpu_ctx, dims, layout, offset=1)
    assert all(x.ptr % 16 != 0 for x in (case.Q, case.Kk, case.V, case.O, case.S, case.dQ, case.dK, case.dV))
    check_grads(case, "eg_attention_grad %s %s offset 1" % (dims, layout), case.run(), with_oracle=True)


def test_sixteen_byte_rows_with_a_ragged_last_chunk(gpu_ctx, layout="bhik"):
    """K = 33 and D = 1 in rows padded to a multiple of 4: 16-byte accesses whose last chunk of a row goes element by element"""
    dims = (3, 2, 7, 200, 33, 1)
    case = Case(gpu_ctx, dims, layout, pad=3, out_pad=3)
    bufs = case.run()
    assert all(x.ld % 4 == 0 and all(s % 4 == 0 for s in x.strides) and x.ptr % 16 == 0
               for x in (case.Q, case.Kk, case.V, case.O, case.dO, case.dQ, case.dK, case.dV))
    check_grads(case, "eg_attention_grad %s %s padded rows" % (dims, layout), bufs, with_oracle=True)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_shared_keys_and_values(gpu_ctx, layout):
    """strides 0 along batch0 for Kk and V; dK and dV stay distinct per item"""
    dims = (2, 3, 33, 70, 16, 16)
    case = Case(gpu_ctx, dims, layout, seed=7, shared=True)
    assert case.Kk.strides[0] == 0 and case.V.strides[0] == 0 and case.dK.strides[0] > 0 and case.dV.strides[0] > 0
    check_grads(case, "eg_attention_grad %s %s shared" % (dims, layout), case.run(), with_oracle=False)


@pytest.mark.parametrize("accumulate", [1, 2, 4, 7])
def test_accumulate_bits(gpu_ctx, accumulate):
    """each bit alone and all three: an output whose bit is set adds to a random base, one whose bit is clear starts as NaN and
    ends finite"""
    dims = (1, 2, 65, 63, 20, 12)
    b0, b1, I, J, K, D = dims
    rng = np.random.default_rng(20 + accumulate)
    shapes = {"dq": (b0, b1, I, K), "dk": (b0, b1, J, K), "dv": (b0, b1, J, D)}
    bases = {name: u(rng, *shapes[name]) for bit, name in ((1, "dq"), (2, "dk"), (4, "dv")) if accumulate & bit}
    case = Case(gpu_ctx, dims, "bhik" if accumulate & 2 else "bihk", seed=31, bases=bases)
    check_grads(case, "eg_attention_grad %s accumulate %d" % (dims, accumulate), case.run(accumulate), with_oracle=False, bases=bases)


def test_twice_the_same_bits(gpu_ctx):
    dims = (2, 3, 130, 200, 20, 12)
    case = Case(gpu_ctx, dims, "bihk", seed=13)
    first = case.run()
    for x in (case.dQ, case.dK, case.dV):
        x.dev.write(x.buf)
    second = case.backward()
    check_grads(case, "eg_attention_grad %s twice" % (dims,), first, with_oracle=False)
    for a, b in zip(first, second):
        assert np.array_equal(bits(a), bits(b))


def test_delta_comes_from_o(gpu_ctx):
    """the same call with another O: dV does not depend on delta and keeps its bits, dQ and dK change"""
    dims = (1, 2, 65, 63, 20, 12)
    case = Case(gpu_ctx, dims, "bihk", seed=41)
    first = case.run()
    other = View(case.o + u(np.random.default_rng(42), *case.o.shape), case.O.ld, case.O.strides[0], case.O.strides[1]).upload(gpu_ctx)
    for x in (case.dQ, case.dK, case.dV):
        x.dev.write(x.buf)
    second = case.backward(O=other)
    assert np.array_equal(bits(first[2]), bits(second[2])), "dV depends on O"
    assert not np.array_equal(bits(first[0]), bits(second[0])), "dQ does not depend on O"
    assert not np.array_equal(bits(first[1]), bits(second[1])), "dK does not depend on O"
    assert np.all(np.isfinite(case.dQ.items(second[0]))) and np.all(np.isfinite(case.dK.items(second[1])))


# ---- raw calls: errors and empty extents -------------------------------------------------------------------------------------
NAMES = ("q", "k", "v", "o", "s", "do", "dq", "dk", "dv")


def raw(ctx, dims, bufs, ld, st, accumulate=0):
    """eg_attention_grad itself: bufs / ld / st map an operand's name to its tensor (None: NULL), leading dimension, strides"""
    p = lambda x: ctypes.c_void_p(x.ptr if x is not None else 0)
    args = []
    for name in NAMES:
        args += [p(bufs[name])] + ([] if name == "s" else [ld[name]]) + list(st[name])
    return _lib.lib().eg_attention_grad(ctx.handle, *dims, SCALE, *args, accumulate)


def raw_sums(ctx, dims, bufs, ld, st, accumulate=0):
    p = lambda x: ctypes.c_void_p(x.ptr if x is not None else 0)
    args = []
    for name in ("q", "k", "v", "o"):
        args += [p(bufs[name]), ld[name]] + list(st[name])
    return _lib.lib().eg_attention_sums(ctx.handle, *dims, SCALE, *args, accumulate, p(bufs["s"]), *st["s"])


def dense_call(ctx, dims, n=2 * 3 * 8 * 8):
    """a valid call on nested [2, 3, 8, 8] operands of eight-float rows, every operand its own poisoned buffer"""
    bufs = {name: poisoned(ctx, n) for name in NAMES}
    ld = {name: 8 for name in NAMES if name != "s"}
    st = {name: (192, 64) for name in NAMES}
    st["s"] = (24, 8)
    return dict(dims=dims, bufs=bufs, ld=ld, st=st)


def changed(call, **kw):
    new = dict(call, bufs=dict(call["bufs"]), ld=dict(call["ld"]), st=dict(call["st"]))
    for key, value in kw.items():
        if key in ("dims", "accumulate"):
            new[key] = value
        else:
            which, name = key.split("_", 1)
            new[{"buf": "bufs", "ld": "ld", "st": "st"}[which]][name] = value
    return new


def test_error_returns(gpu_ctx):
    """the invalid and the unsupported calls of the contract, each with the function's name; nothing is written"""
    ok = dense_call(gpu_ctx, (2, 3, 8, 8, 8, 8))
    invalid = {
        "negative batch0": dict(dims=(-1, 3, 8, 8, 8, 8)), "negative J": dict(dims=(2, 3, 8, -1, 8, 8)), "batch1 of 2^31": dict(dims=(2, 1 << 31, 8, 8, 8, 8)),
        "accumulate of 8": dict(accumulate=8),
        "NULL Q": dict(buf_q=None), "NULL V": dict(buf_v=None), "NULL O": dict(buf_o=None), "NULL Sums": dict(buf_s=None), "NULL dO": dict(buf_do=None),
        "NULL dQ": dict(buf_dq=None), "NULL dK": dict(buf_dk=None), "NULL dV": dict(buf_dv=None),
        "ldq below K": dict(ld_q=7), "ldo below D": dict(ld_o=7), "lddo below D": dict(ld_do=7), "lddq below K": dict(ld_dq=7),
        "lddk below K": dict(ld_dk=7), "lddv below D": dict(ld_dv=7),
        "negative stride_q0": dict(st_q=(-192, 64)), "negative stride_o1": dict(st_o=(192, -64)), "negative stride_s0": dict(st_s=(-24, 8)),
        "negative stride_do1": dict(st_do=(192, -64)), "negative stride_dq1": dict(st_dq=(192, -64)),
        "dQ aliases itself": dict(st_dq=(64, 64)), "stride_dk1 of 0": dict(st_dk=(192, 0)), "items of dV overlap": dict(st_dv=(192, 63)),
    }
    for name, change in invalid.items():
        assert raw(gpu_ctx, **changed(ok, **change)) == EG_ERR_INVALID, name
        assert "eg_attention_grad" in _lib.last_error(), (name, _lib.last_error())
    big = {name: poisoned(gpu_ctx, 2 * 3 * 8 * 129) for name in ("a", "b", "c", "d")}
    wide = dict(ld=129, st=(3096, 1032))
    for name, change in {
            "K of 129": dict(dims=(2, 3, 8, 8, 129, 8), **{"%s_%s" % (f, o): (big[b] if f == "buf" else wide[f])
                                                         for o, b in (("q", "a"), ("k", "b"), ("dq", "c"), ("dk", "d")) for f in ("buf", "ld", "st")}),
            "D of 129": dict(dims=(2, 3, 8, 8, 8, 129), **{"%s_%s" % (f, o): (big[b] if f == "buf" else wide[f])
                                                         for o, b in (("v", "a"), ("o", "b"), ("do", "c"), ("dv", "d")) for f in ("buf", "ld", "st")})}.items():
        assert raw(gpu_ctx, **changed(ok, **change)) == EG_ERR_UNSUPPORTED, (name, _lib.last_error())
        assert "eg_attention_grad" in _lib.last_error() and "128" in _lib.last_error(), (name, _lib.last_error())
    # the row sums of eg_attention_sums: items of I floats that overlap, and a tie
    for name, st in {"stride_s1 below I": (24, 7), "stride_s0 == stride_s1": (8, 8), "stride_s1 of 0": (24, 0), "negative stride_s1": (24, -8)}.items():
        assert raw_sums(gpu_ctx, ok["dims"], ok["bufs"], ok["ld"], dict(ok["st"], s=st)) == EG_ERR_INVALID, name
        assert "eg_attention_sums" in _lib.last_error() and "Sums" in _lib.last_error(), (name, _lib.last_error())
    assert raw_sums(gpu_ctx, (2, 3, 8, 8, 129, 8), dict(ok["bufs"], q=big["a"], k=big["b"]), dict(ok["ld"], q=129, k=129),
                    dict(ok["st"], q=wide["st"], k=wide["st"])) == EG_ERR_UNSUPPORTED
    assert "eg_attention_sums" in _lib.last_error() and "128" in _lib.last_error(), _lib.last_error()
    gpu_ctx.sync()
    assert all(np.all(t.read() == POISON) for t in list(ok["bufs"].values()) + list(big.values()))
    # the calls the tables of changes start from
    fresh = dense_call(gpu_ctx, (2, 3, 8, 8, 8, 8))
    for name in ("q", "k", "v"):
        fresh["bufs"][name].write(u(np.random.default_rng(1), 2 * 3 * 8 * 8))
    assert raw_sums(gpu_ctx, fresh["dims"], fresh["bufs"], fresh["ld"], fresh["st"]) == 0, _lib.last_error()
    assert raw(gpu_ctx, **fresh) == 0, _lib.last_error()


@pytest.mark.parametrize("dims", [(0, 3, 8, 8, 8, 8), (2, 0, 8, 8, 8, 8)], ids=lambda d: "x".join(map(str, d)))
def test_an_empty_batch_launches_nothing(gpu_ctx, dims):
    call = dense_call(gpu_ctx, dims)
    assert raw(gpu_ctx, **call) == 0, _lib.last_error()
    assert raw_sums(gpu_ctx, call["dims"], call["bufs"], call["ld"], call["st"]) == 0, _lib.last_error()
    assert all(np.all(t.read() == POISON) for t in call["bufs"].values())


@pytest.mark.parametrize("accumulate", [0, 7])
@pytest.mark.parametrize("dims", [(2, 3, 0, 8, 8, 8), (2, 3, 8, 0, 8, 8), (2, 3, 8, 8, 8, 0)], ids=lambda d: "x".join(map(str, d)))
def test_empty_sums_are_zeros_or_nothing(gpu_ctx, dims, accumulate):
    """I == 0: dK and dV; J == 0: dQ; D == 0: dQ and dK — zeros where the bit is clear, untouched where it is set; every other
    buffer untouched; inputs of an empty sum may be NULL"""
    b0, b1, I, J, K, D = dims
    call = dense_call(gpu_ctx, dims)
    zeroed = {0: ("dk", "dv"), 1: ("dq",), 2: ("dq", "dk")}[[I, J, D].index(0)]
    if I == 0 or J == 0:
        call = changed(call, buf_q=None, buf_k=None, buf_v=None, buf_o=None, buf_s=None, buf_do=None)
    else:
        call["bufs"]["s"].write(np.full(2 * 3 * 8 * 8, 8.0, np.float32))
        for name in ("q", "k"):
            call["bufs"][name].write(u(np.random.default_rng(2), 2 * 3 * 8 * 8))
        call = changed(call, buf_v=None, buf_o=None, buf_do=None)
    assert raw(gpu_ctx, accumulate=accumulate, **call) == 0, _lib.last_error()
    for name in ("dq", "dk", "dv"):
        got = call["bufs"][name].read()
        want = 0.0 if name in zeroed and not accumulate else POISON
        assert np.all(got == want), (name, got[:8])


def test_no_head_dimension(gpu_ctx):
    """K == 0 with NULL Q, Kk, dQ and dK: every score is 0, every probability 1 / J, dV_j = sum_i dO_i / J"""
    I, J, D = 70, 9, 12
    rng = np.random.default_rng(19)
    v, d_out = u(rng, J, D), u(rng, I, D)
    o = np.broadcast_to(v.mean(0), (I, D)).astype(np.float32)
    dev = {}
    for name, x in (("v", v), ("o", o), ("do", d_out), ("s", np.full(I, J, np.float32))):
        dev[name] = gpu_ctx.allocTensor(x.shape)
        dev[name].write(x)
    dev["dv"] = poisoned(gpu_ctx, 2 * J * D + 3)
    bufs = dict({name: None for name in NAMES}, **dev)
    ld = {name: (D if name in ("v", "o", "do", "dv") else 0) for name in NAMES if name != "s"}
    st = dict({name: (0, 0) for name in NAMES}, dv=(J * D, J * D))
    assert raw(gpu_ctx, (2, 1, I, J, 0, D), bufs, ld, st) == 0, _lib.last_error()
    got = dev["dv"].read()
    want = np.broadcast_to(d_out.astype(np.float64).sum(0) / J, (2 * J, D))
    assert rel_err(got[:2 * J * D].reshape(2 * J, D), want, "eg_attention_grad K == 0 vs float64") <= TOL
    assert np.all(got[2 * J * D:] == POISON)


def test_sums_without_a_value_dimension(gpu_ctx):
    """eg_attention_sums with D == 0 and NULL V and O still writes the row sums; J == 0 writes zeros and leaves an accumulating O"""
    dims = (2, 3, 8, 8, 8, 0)
    call = dense_call(gpu_ctx, dims)
    q, k = u(np.random.default_rng(5), 2, 3, 8, 8), u(np.random.default_rng(6), 2, 3, 8, 8)
    call["bufs"]["q"].write(q.ravel())
    call["bufs"]["k"].write(k.ravel())
    bufs = dict(call["bufs"], v=None, o=None)
    assert raw_sums(gpu_ctx, dims, bufs, call["ld"], call["st"]) == 0, _lib.last_error()
    _, sums64, _, _, _ = gc.closed_form(q, k, np.zeros((2, 3, 8, 1)), np.zeros((2, 3, 8, 1)))
    got = call["bufs"]["s"].read()
    assert rel_err(got[:48].reshape(2, 3, 8), sums64, "eg_attention_sums D == 0 vs float64") <= TOL and np.all(got[48:] == POISON)
    empty = dense_call(gpu_ctx, (2, 3, 8, 0, 8, 8))
    assert raw_sums(gpu_ctx, (2, 3, 8, 0, 8, 8), dict(empty["bufs"], k=None, v=None), empty["ld"], empty["st"], accumulate=1) == 0, _lib.last_error()
    got = empty["bufs"]["s"].read()
    assert np.all(got[:48] == 0) and np.all(got[48:] == POISON) and np.all(empty["bufs"]["o"].read() == POISON)
