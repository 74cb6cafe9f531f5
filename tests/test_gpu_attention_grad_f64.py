"""eg_attention_grad_f64 (kernels/attention_grad_f64.hip) on the device, against the numpy.longdouble closed form of
tests/attention_grad_f64_cases.py within TOL64 of each output's largest element.  O and Sums come from eg_attention_sums_f64 with
accumulate = 0 on the same operands.  Every operand sits inside a NaN-filled allocation with guards (a read outside a view shows up
as NaN), and every output buffer is compared bit for bit with its state before the call outside its items' elements."""
import ctypes
import functools

import numpy as np
import pytest

import attention_grad_f64_cases as gc
from attention_grad_f64_cases import SCALE, TOL64
from exprgrad_amd import _lib, ops
from test_gpu_attention_f64 import EG_ERR_INVALID, EG_ERR_UNSUPPORTED, LAYOUTS, POISON, Poisoned, View, bits, lay

pytestmark = pytest.mark.gpu

OUTPUTS = ("dQ", "dK", "dV")


@functools.lru_cache(None)
def reference(dims, shared=False):
    """(q, k, v, d_out, dq, dk, dv): operands and their longdouble gradients, computed once per shape and left unchanged"""
    operands = gc.operands(dims, shared)
    out = tuple(operands) + tuple(gc.closed_form(*operands, SCALE, np.longdouble))
    for x in out:
        x.setflags(write=False)
    return out


class Run:
    """The nine operands of one call on the device.  rows: "even" / "odd" pads every row (and the stride of Sums) to that parity;
    offset: doubles every pointer is moved by; Kk and V with extent 1 along batch0 are shared along it (stride 0)."""

    def __init__(self, ctx, dims, layout, q, k, v, d_out, rows=None, offset=0):
        b0, b1, I, J, K, D = dims
        self.ctx, self.dims = ctx, dims
        par = lambda n: n if rows is None else n + (n + (rows == "odd")) % 2

        def view(x, R, C, extra=0):
            ld = lay(layout, b1, R, C)[0]
            ld, s0, s1 = lay(layout, b1, R, C, par(ld) - ld + extra)
            return View(x, ld, 0 if x.shape[0] < b0 else s0, s1, offset).upload(ctx)

        nan = lambda *shape: np.full((b0, b1) + shape, np.nan)
        self.inputs = [view(q, I, K), view(k, J, K), view(v, J, D), view(nan(I, D), I, D, 2)]      # Q, Kk, V, O
        self.S, self.dO = View(nan(1, I), I, b1 * par(I + 5), par(I + 5), offset).upload(ctx), view(d_out, I, D)
        self.out = {"dQ": view(nan(I, K), I, K, 2), "dK": view(nan(J, K), J, K, 2), "dV": view(nan(J, D), J, D, 2)}
        self.views = self.inputs + [self.S, self.dO] + list(self.out.values())
        ops.attention_sums_f64(ctx, *dims, SCALE, *(y for x in self.inputs for y in (x.ptr, x.ld, x.strides)), self.S.ptr, self.S.strides)

    def grad(self, accumulate=0, base=None):
        """-> {name: the output's items}; an output whose bit is set starts as base[name], the others as NaN"""
        for i, x in enumerate(self.out.values()):
            x.items(x.buf)[...] = base[OUTPUTS[i]] if accumulate >> i & 1 else np.nan
            x.dev.write(x.buf)
        operand = lambda x: (x.ptr, x.ld, x.strides)
        ops.attention_grad_f64(self.ctx, *self.dims, SCALE, *(y for x in self.inputs for y in operand(x)), self.S.ptr, self.S.strides, *operand(self.dO),
                               *(y for x in self.out.values() for y in operand(x)), accumulate)
        got = {}
        for name, x in self.out.items():
            buf = x.read()
            x.same_outside(buf, name)
            got[name] = x.items(buf).copy()
        return got

    def free(self):
        for x in self.views:
            x.free()


def held(label, got, want):
    for name, ref in zip(OUTPUTS, want):
        if ref.size == 0:      # K == 0: dQ and dK have no elements
            continue
        err = gc.rel(got[name], ref)
        print(label, name, "vs longdouble: %.3g of TOL64 %g" % (err, TOL64))
        assert np.all(np.isfinite(got[name])) and err <= TOL64, (label, name, err)


def same_bits(a, b, what):
    assert all(np.array_equal(bits(a[name]), bits(b[name])) for name in OUTPUTS), what


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims,shared", [(d, False) for d in gc.DIMS + [(2, 1, 5, 70, 0, 12)]] + [((2, 3, 33, 70, 20, 12), True)], ids=lambda x: gc.ident(x) if type(x) is tuple else str(x))
def test_parity(gpu_ctx, dims, shared, layout):
    """every shape in both layouts; K = 0, which still computes dV; Kk and V shared along batch0 (stride 0) with dK and dV per item"""
    ref = reference(dims, shared)
    run = Run(gpu_ctx, dims, layout, *ref[:4])
    assert (run.inputs[2].strides[0] == 0) == shared and run.out["dV"].strides[0] > 0      # V (and Kk with it) shared, dV per item
    got = run.grad()
    run.free()
    held("eg_attention_grad_f64 %s %s" % (gc.ident(dims), layout), got, ref[4:])


@pytest.mark.parametrize("dims", [gc.DIMS[0], gc.DIMS[4], gc.DIMS[8]], ids=gc.ident)
def test_the_eight_byte_path_has_the_bits_of_the_sixteen_byte_path(gpu_ctx, dims):
    """The same values three times: rows of even length at aligned pointers (16-byte accesses of all nine operands), odd leading
    dimensions, every pointer one double off.  The accesses differ, the arithmetic does not."""
    ref = reference(dims)
    results = {}
    for name, rows, offset in (("16-byte", "even", 0), ("odd ld", "odd", 0), ("offset 1", "even", 1)):
        run = Run(gpu_ctx, dims, "bhik", *ref[:4], rows=rows, offset=offset)
        vec = [(x is run.S or x.ld % 2 == 0) and x.strides[0] % 2 == 0 and x.strides[1] % 2 == 0 and x.ptr % 16 == 0 for x in run.views]
        assert vec == [name == "16-byte"] * 9, (name, vec)
        results[name] = run.grad()
        run.free()
    held("eg_attention_grad_f64 %s even rows" % gc.ident(dims), results["16-byte"], ref[4:])
    same_bits(results["odd ld"], results["16-byte"], "odd ld")
    same_bits(results["offset 1"], results["16-byte"], "offset 1")


def test_accumulate_twice_and_an_item_alone(gpu_ctx):
    """Two calls give the same bits.  An output whose bit is set is base + fresh to the bit; one whose bit is clear starts as NaN, is
    not read, and is fresh.  An item run alone has the bits it has inside the batch."""
    dims = gc.DIMS[8]      # both kernels on the step of 32
    ref = reference(dims)
    rng = np.random.default_rng(11)
    base = {name: rng.random(x.shape) - 0.5 for name, x in zip(OUTPUTS, ref[4:])}
    run = Run(gpu_ctx, dims, "bihk", *ref[:4])
    fresh = run.grad()
    same_bits(fresh, run.grad(), "the second call")
    for accumulate in (1, 2, 4, 7):
        same_bits(run.grad(accumulate, base), {name: base[name] + fresh[name] if accumulate >> i & 1 else fresh[name] for i, name in enumerate(OUTPUTS)}, accumulate)
    run.free()
    for i1 in range(dims[1]):
        alone = Run(gpu_ctx, (1, 1) + dims[2:], "bhik", *(x[:, i1:i1 + 1] for x in ref[:4]))
        same_bits({n: x[0, 0] for n, x in alone.grad().items()}, {n: fresh[n][0, i1] for n in OUTPUTS}, "item %d alone" % i1)
        alone.free()


# ---- empty extents and refusals: raw calls on poisoned buffers -----------------------------------------------------------------
NAMES = ("Q", "Kk", "V", "O", "S", "dO", "dQ", "dK", "dV")
N, SMALL = 2 * 3 * 8 * 129 + 5, 0.125


def raw(ctx, dims, bufs, ld=8, accumulate=0, null=(), **changed):
    """every operand [2, 3, 8, ld] dense unless `changed` gives its (ld, stride0, stride1); `null`: names passed as NULL"""
    args = [ctx.handle] + list(dims) + [SCALE]
    for name in NAMES:
        l, s0, s1 = changed.get(name, (ld, 24 * ld, 8 * ld) if name != "S" else (0, 24, 8))
        args += [ctypes.c_void_p(0 if name in null else bufs[name].ptr)] + ([l] if name != "S" else []) + [s0, s1]
    return _lib.lib().eg_attention_grad_f64(*(args + [accumulate]))


@pytest.fixture()
def bufs(gpu_ctx):
    """outputs of POISON with five doubles behind the items; inputs of a small finite value, so that a call that runs stays finite"""
    out = {name: Poisoned(gpu_ctx, N) for name in NAMES}
    for name in NAMES[:6]:
        out[name].dev.write(np.full(N, SMALL))
    return out


def untouched(bufs):
    return all(np.all(b.read() == (POISON if name in OUTPUTS else SMALL)) for name, b in bufs.items())


@pytest.mark.parametrize("accumulate", [0, 7])
def test_empty_extents(gpu_ctx, bufs, accumulate):
    """a zero batch extent writes nothing; I = 0, J = 0 or D = 0 writes zeros where the bit is clear and nothing otherwise, NULL inputs allowed"""
    for dims in ((0, 3, 8, 8, 8, 8), (2, 0, 8, 8, 8, 8)):
        assert raw(gpu_ctx, dims, bufs, accumulate=accumulate) == 0 and untouched(bufs), (dims, _lib.last_error())
    for dims, null, zeroed in (((2, 3, 0, 8, 8, 8), NAMES[:7], ("dK", "dV")), ((2, 3, 8, 0, 8, 8), NAMES[:6] + ("dK", "dV"), ("dQ",)),
                               ((2, 3, 8, 8, 8, 0), ("V", "O", "dO", "dV"), ("dQ", "dK"))):
        assert raw(gpu_ctx, dims, bufs, accumulate=accumulate, null=null) == 0, (dims, _lib.last_error())
        for name in zeroed:
            got = bufs[name].read()
            assert np.all(got[:384] == (0 if accumulate == 0 else POISON)) and np.all(got[384:] == POISON), (dims, name)
            bufs[name].dev.write(np.full(N, POISON))
        assert untouched(bufs), dims


def test_error_returns(gpu_ctx, bufs):
    """each invalid call of the contract returns its code and names the entry; the buffers stay as they were"""
    ok = (2, 3, 8, 8, 8, 8)
    invalid = {
        "negative batch0": dict(dims=(-1, 3, 8, 8, 8, 8)), "negative I": dict(dims=(2, 3, -1, 8, 8, 8)), "negative D": dict(dims=(2, 3, 8, 8, 8, -1)),
        "negative stride_q0": dict(Q=(8, -192, 64)), "negative stride_s1": dict(S=(0, 24, -8)), "negative stride_do0": dict(dO=(8, -192, 64)),
        "ldk below K": dict(Kk=(7, 192, 64)), "ldo below D": dict(O=(7, 192, 64)), "lddv below D": dict(dV=(7, 192, 64)),
        "dQ aliases itself": dict(dQ=(8, 64, 64)), "items of dK overlap": dict(dK=(8, 192, 63)), "stride_dv1 of 0": dict(dV=(8, 192, 0)),
        "NULL Q": dict(null=("Q",)), "NULL Sums": dict(null=("S",)), "NULL dO": dict(null=("dO",)), "NULL dK": dict(null=("dK",)),
        "accumulate of 8": dict(accumulate=8),
    }
    for name, change in invalid.items():
        assert raw(gpu_ctx, change.pop("dims", ok), bufs, **change) == EG_ERR_INVALID, name
        assert "eg_attention_grad_f64" in _lib.last_error(), (name, _lib.last_error())
    for dims in ((2, 3, 8, 8, 129, 8), (2, 3, 8, 8, 8, 129)):
        assert raw(gpu_ctx, dims, bufs, ld=129) == EG_ERR_UNSUPPORTED, dims
        assert "eg_attention_grad_f64" in _lib.last_error() and "128" in _lib.last_error(), (dims, _lib.last_error())
    gpu_ctx.sync()
    assert untouched(bufs) and raw(gpu_ctx, ok, bufs) == 0, _lib.last_error()      # and the call the table of changes starts from runs
