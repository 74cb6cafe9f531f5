"""eg_attention_f64 and eg_attention_sums_f64 (kernels/attention_f64.hip) on the device.

a. The exact cases of tests/attention_f64_cases.py at all nine pairs of padded head sizes: every element of O and of Sums to
   its own bits (tests/test_attention_f64_cases_cpu.py proves the expected values without a kernel).
b. Parity at the same shapes: random operands against a numpy.longdouble evaluation of the three-statement program within
   TOL64 = 1e-12 of the largest element, the project's float64 bound (tests/test_gpu_f64.py); the CPU test above holds a
   plain float64 evaluation of the same operands to a tenth of it.
c. The contract: [b,i,h,*] interleaved and nested strides, zero strides, the 8-byte load path against the 16-byte path on the
   same values, accumulate, Sums and the bits of O with and without them, a call against itself, an item alone against the
   item inside a batch, the empty extents, the refusals, the special values of the header.

Every operand sits inside a larger device allocation filled with NaN: a read in front of a view, behind a row's end, behind
the last row or of a key j >= J shows up as a NaN row, and the whole O and Sums buffers are compared bit for bit with their
state before the call outside the items' elements."""
import ctypes

import numpy as np
import pytest

import attention_f64_cases as ec
from attention_f64_cases import SCALE, TOL64
from exprgrad_amd import _lib, ops

pytestmark = pytest.mark.gpu

EG_ERR_INVALID, EG_ERR_UNSUPPORTED = 1, 5
GUARD = 64      # doubles of NaN in front of and behind every operand; even, so that offset 0 stays 16-byte aligned
LAYOUTS = ["bihk", "bhik"]
f64 = np.float64
bits = lambda x: np.ascontiguousarray(x, f64).view(np.uint64)


class View:
    """A [b0, b1, R, C] float64 operand placed in a NaN-filled host buffer at `offset` doubles behind the guard: row step ld,
    strides (s0, s1) of the two batch indices; a stride of 0 shares the operand along that index (x then has extent 1 there)."""

    def __init__(self, x, ld, s0, s1, offset=0, fill=np.nan):
        b0, b1, R, C = x.shape
        self.shape, self.ld, self.strides, self.offset = x.shape, ld, (s0, s1), offset
        span = (b0 - 1) * s0 + (b1 - 1) * s1 + (R - 1) * ld + C
        self.buf = np.full(GUARD + offset + span + GUARD, fill, dtype=f64)
        self.items(self.buf)[...] = x

    def items(self, buf):
        b0, b1, R, C = self.shape
        return np.lib.stride_tricks.as_strided(buf[GUARD + self.offset:], (b0, b1, R, C), (8 * self.strides[0], 8 * self.strides[1], 8 * self.ld, 8))

    def upload(self, ctx):
        self.dev = ctx.allocBuffer(self.buf.nbytes)
        self.dev.write(self.buf)
        return self

    def read(self):
        return self.dev.readInto(np.empty(self.buf.size, dtype=f64))

    def free(self):
        self.dev.dealloc()

    @property
    def ptr(self):
        return self.dev.ptr + 8 * (GUARD + self.offset)

    def same_outside(self, got_buf, what):
        """everything of the buffer but the items' elements has the bits it was uploaded with"""
        want = self.buf.copy()
        self.items(want)[...] = self.items(got_buf)
        assert np.array_equal(bits(got_buf), bits(want)), what + ": stored outside the items"


def lay(layout, b1, R, C, pad=0):
    """(ld, s0, s1) of a [b0, b1, R, C] operand: heads inside the row ([b,i,h,*]) or nested ([b,h,i,*])"""
    if layout == "bihk":
        ld = b1 * C + pad
        return ld, R * ld, C
    ld = C + pad
    return ld, b1 * R * ld, R * ld


class Run:
    """The operands of one call on the device.  rows: the parity of the row lengths of Q, Kk and V; offset: doubles every
    pointer is moved by; Kk and V with extent 1 along batch0 are shared along it (stride 0)."""

    def __init__(self, ctx, dims, layout, q, k, v, rows=None, offset=0, o_init=None):
        b0, b1, I, J, K, D = dims
        self.ctx, self.dims = ctx, dims
        shared = k.shape[0] == 1 and b0 > 1
        # rows: None (dense), "even" or "odd": each row of Q, Kk and V padded by at most one double to that parity
        pad = lambda R, C: 0 if rows is None else (lay(layout, b1, R, C)[0] + (rows == "odd")) % 2
        ldq, q0, q1 = lay(layout, b1, I, K, pad(I, K))
        ldk, k0, k1 = lay(layout, b1, J, K, pad(J, K))
        ldv, v0, v1 = lay(layout, b1, J, D, pad(J, D))
        ldo, o0, o1 = lay(layout, b1, I, D, 3)      # ldo > D in either layout
        self.Q = View(q, ldq, q0, q1, offset).upload(ctx)
        self.Kk = View(k, ldk, 0 if shared else k0, k1, offset).upload(ctx)
        self.V = View(v, ldv, 0 if shared else v0, v1, offset).upload(ctx)
        self.O = View(np.full((b0, b1, I, D), np.nan) if o_init is None else o_init, ldo, o0, o1, offset).upload(ctx)
        self.S = View(np.full((b0, b1, 1, I), np.nan), I, b1 * (I + 5), I + 5, offset).upload(ctx)   # five doubles between the items

    def call(self, sums, accumulate=False, scale=SCALE):
        """-> (O's items, the Sums [b0, b1, I] or None); both buffers checked outside their items"""
        b0, b1, I, J, K, D = self.dims
        Q, Kk, V, O, S = self.Q, self.Kk, self.V, self.O, self.S
        O.dev.write(O.buf)
        S.dev.write(S.buf)
        args = (self.ctx, b0, b1, I, J, K, D, scale, Q.ptr, Q.ld, Q.strides, Kk.ptr, Kk.ld, Kk.strides, V.ptr, V.ld, V.strides, O.ptr, O.ld, O.strides)
        if sums:
            ops.attention_sums_f64(*(args + (S.ptr, S.strides, accumulate)))
        else:
            ops.attention_f64(*(args + (accumulate,)))
        o_buf, s_buf = O.read(), S.read()
        O.same_outside(o_buf, "O")
        if sums:
            S.same_outside(s_buf, "Sums")
        else:
            assert np.array_equal(bits(s_buf), bits(S.buf)), "eg_attention_f64 touched another buffer"
        return O.items(o_buf).copy(), (S.items(s_buf)[:, :, 0, :].copy() if sums else None)

    def both(self, accumulate=False):
        """eg_attention_sums_f64 and eg_attention_f64: O bit-equal -> (o, sums)"""
        o, sums = self.call(True, accumulate)
        plain, _ = self.call(False, accumulate)
        assert np.array_equal(bits(plain), bits(o)), "O of eg_attention_f64 differs from eg_attention_sums_f64's"
        return o, sums

    def free(self):
        for x in (self.Q, self.Kk, self.V, self.O, self.S):
            x.free()


# ---- a. the exact cases -----------------------------------------------------------------------------------------------------
EXACT = ec.forward_cases()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("make", [m for _, m in EXACT], ids=[n for n, _ in EXACT])
def test_exact_cases(gpu_ctx, make, layout):
    ex = make()
    label = "exact %s %s %s" % (ex.family, ec.ident(ex.dims), layout)
    run = Run(gpu_ctx, ex.dims, layout, ex.q, ex.k, ex.v)
    o, sums = run.both()
    run.free()
    ec.same_values(sums, ex.want["sums"], label + " Sums")
    ec.same_values(o, ex.want["o"], label + " O")


# ---- b. parity at the same shapes -------------------------------------------------------------------------------------------
_REFERENCE = {}


def reference(dims, shared=False):
    """operands and their numpy.longdouble evaluation, computed once per shape"""
    key = dims + (shared,)
    if key not in _REFERENCE:
        q, k, v = ec.random_operands(dims, shared=shared)
        o, sums = ec.program(q, k, v, SCALE, np.longdouble)
        for x in (q, k, v, o, sums):
            x.setflags(write=False)
        _REFERENCE[key] = (q, k, v, o, sums)
    return _REFERENCE[key]


def held(label, o, sums, want_o, want_sums):
    e_o, e_s = ec.rel(o, want_o), (ec.rel(sums, want_sums) if sums is not None else 0.0)
    print(label, "vs longdouble: O %.3g Sums %.3g of TOL64 %g" % (e_o, e_s, TOL64))
    assert np.all(np.isfinite(o)) and e_o <= TOL64 and e_s <= TOL64, (label, e_o, e_s)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", ec.DIMS, ids=ec.ident)
def test_parity(gpu_ctx, dims, layout):
    q, k, v, want_o, want_sums = reference(dims)
    run = Run(gpu_ctx, dims, layout, q, k, v)
    o, sums = run.both()
    run.free()
    held("eg_attention_sums_f64 %s %s" % (ec.ident(dims), layout), o, sums, want_o, want_sums)


# ---- c. the contract --------------------------------------------------------------------------------------------------------
LOAD_PATHS = [(ec.DIMS[0], "bhik"), (ec.DIMS[4], "bhik"), (ec.DIMS[4], "bihk"), (ec.DIMS[5], "bhik"), (ec.DIMS[8], "bhik")]


@pytest.mark.parametrize("dims,layout", LOAD_PATHS, ids=["%s-%s" % (ec.ident(d), l) for d, l in LOAD_PATHS])
def test_the_eight_byte_path_has_the_bits_of_the_sixteen_byte_path(gpu_ctx, dims, layout):
    """The same values three times: rows of even length at aligned pointers (16-byte loads of every operand; where K or D is
    odd, a row's last element alone), rows of odd length, and every pointer one double off 16-byte alignment.  The loads
    differ, the arithmetic does not.  (The nested layout, and the interleaved one where K and D are even: with the heads
    inside the row an odd K is itself the odd stride.)"""
    q, k, v, want_o, want_sums = reference(dims)
    even = lambda n: n % 2 == 0
    results = {}
    for name, rows, offset in (("16-byte", "even", 0), ("odd ld", "odd", 0), ("offset 1", "even", 1)):
        run = Run(gpu_ctx, dims, layout, q, k, v, rows=rows, offset=offset)
        vec = [even(x.ld) and even(x.strides[0]) and even(x.strides[1]) and x.ptr % 16 == 0 for x in (run.Q, run.Kk, run.V)]
        assert vec == [name == "16-byte"] * 3, (name, vec)
        results[name] = run.both()
        run.free()
    o, sums = results["16-byte"]
    held("eg_attention_sums_f64 %s %s even rows" % (ec.ident(dims), layout), o, sums, want_o, want_sums)
    for name in ("odd ld", "offset 1"):
        assert np.array_equal(bits(results[name][0]), bits(o)) and np.array_equal(bits(results[name][1]), bits(sums)), name


@pytest.mark.parametrize("layout", LAYOUTS)
def test_shared_keys_and_values(gpu_ctx, layout):
    """strides 0 along batch0 for Kk and V"""
    dims = (2, 3, 33, 70, 20, 12)
    q, k, v, want_o, want_sums = reference(dims, shared=True)
    run = Run(gpu_ctx, dims, layout, q, k, v)
    assert run.Kk.strides[0] == 0 and run.V.strides[0] == 0 and run.Q.strides[0] > 0
    o, sums = run.both()
    run.free()
    held("eg_attention_sums_f64 %s %s shared" % (ec.ident(dims), layout), o, sums, want_o, want_sums)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_accumulate_adds_to_o(gpu_ctx, layout):
    dims = ec.DIMS[2]
    b0, b1, I, J, K, D = dims
    q, k, v, want_o, want_sums = reference(dims)
    base = np.random.default_rng(11).random((b0, b1, I, D)) - 0.5
    run = Run(gpu_ctx, dims, layout, q, k, v, o_init=base)
    o, sums = run.both(accumulate=True)
    fresh, fresh_sums = run.both(accumulate=False)
    run.free()
    held("eg_attention_sums_f64 %s %s accumulate" % (ec.ident(dims), layout), o, sums, want_o + base.astype(np.longdouble), want_sums)
    assert np.array_equal(bits(o), bits(base + fresh)) and np.array_equal(bits(sums), bits(fresh_sums))      # one addition; Sums overwritten


def test_twice_the_same_bits_and_an_item_alone_has_its_bits_in_the_batch(gpu_ctx):
    dims = (2, 3, 70, 130, 65, 65)      # the key tile of 32
    b0, b1, I, J, K, D = dims
    q, k, v, want_o, want_sums = reference(dims)
    run = Run(gpu_ctx, dims, "bihk", q, k, v)
    first, second = run.both(), run.both()
    run.free()
    held("eg_attention_sums_f64 %s twice" % ec.ident(dims), first[0], first[1], want_o, want_sums)
    assert np.array_equal(bits(first[0]), bits(second[0])) and np.array_equal(bits(first[1]), bits(second[1]))
    for o, i1 in ((0, 0), (1, 2)):
        alone = Run(gpu_ctx, (1, 1, I, J, K, D), "bhik", q[o:o + 1, i1:i1 + 1], k[o:o + 1, i1:i1 + 1], v[o:o + 1, i1:i1 + 1])
        got_o, got_s = alone.both()
        alone.free()
        assert np.array_equal(bits(got_o[0, 0]), bits(first[0][o, i1])) and np.array_equal(bits(got_s[0, 0]), bits(first[1][o, i1])), (o, i1)


def run_special(ctx, q, k, v):
    """one item, dense operands -> (device rows, device sums)"""
    I, K = q.shape
    J, D = v.shape
    run = Run(ctx, (1, 1, I, J, K, D), "bhik", q[None, None], k[None, None], v[None, None])
    o, sums = run.both()
    run.free()
    return o[0, 0], sums[0, 0]


def test_special_rows(gpu_ctx):
    """Special scores against the three-statement program in float64.  Every key has 1 in column 1, and only key 3 an entry
    (1) in column 0; the rows of q:
      0  (0, +Inf, 0, 0): every score +Inf           -> NaN        1  a NaN in q                  -> NaN
      2  (0, -1e300, 0, 0): every term underflows     -> 0 / 0      3  (709 / scale, 0, 0, 0): one term exp(709), finite
      4  ordinary"""
    I, J, K, D = 5, 70, 4, 4
    rng = np.random.default_rng(17)
    q, k, v = rng.random((I, K)) - 0.5, rng.random((J, K)) - 0.5, rng.random((J, D)) + 0.5
    k[:, 0] = 0.0
    k[3, 0] = 1.0
    k[:, 1] = 1.0
    q[0] = (0.0, np.inf, 0.0, 0.0)
    q[1, 2] = np.nan
    q[2] = (0.0, -1e300, 0.0, 0.0)
    q[3] = (709.0 / SCALE, 0.0, 0.0, 0.0)
    got, sums = run_special(gpu_ctx, q, k, v)
    want, want_sums = (x[0, 0] for x in ec.program(q[None, None], k[None, None], v[None, None], SCALE, f64))
    print("special rows: device", got, sums, "float64 program", want, want_sums)
    assert np.all(np.isnan(want[:3])) and np.all(np.isfinite(want[3:])), want
    assert np.all(np.isnan(got[:3])) and np.all(np.isfinite(got[3:]))
    assert np.all(np.abs(got[3:] - want[3:]) <= TOL64 * np.abs(want[3:]))      # each value to itself: V is positive, nothing cancels
    assert np.isnan(sums[0]) and np.isnan(sums[1]) and sums[2] == 0 and np.all(np.abs(sums[3:] - want_sums[3:]) <= TOL64 * want_sums[3:])


def test_a_minus_infinity_score_adds_nothing(gpu_ctx):
    """key 5 has -Inf in column 1 and every row of q has 1 there: one score of -Inf per row, whose term is exactly 0"""
    I, J, K, D = 5, 70, 4, 4
    rng = np.random.default_rng(18)
    q, k, v = rng.random((I, K)) - 0.5, rng.random((J, K)) - 0.5, rng.random((J, D)) + 0.5
    q[:, 1] = 1.0
    k[5, 1] = -np.inf
    got, sums = run_special(gpu_ctx, q, k, v)
    live = np.arange(J) != 5
    want, want_sums = (x[0, 0] for x in ec.program(q[None, None], k[None, None][:, :, live], v[None, None][:, :, live], SCALE, np.longdouble))
    print("-Inf score: device", got, sums, "longdouble without that key", want, want_sums)
    assert np.all(np.isfinite(got)) and ec.rel(got, want) <= TOL64 and ec.rel(sums, want_sums) <= TOL64


def test_a_sum_that_overflows_is_nan_where_the_program_gives_zero(gpu_ctx):
    """The one departure the header states.  Row 0 has 70 scores of 709 / scale: every term is exp(709) = 8.2e307, finite, and
    their sum overflows.  The program divides each finite term by Inf and gives 0; this entry turns an infinite denominator
    into NaN, in O and in Sums.  Row 1 is ordinary and agrees."""
    I, J, K, D = 2, 70, 4, 4
    rng = np.random.default_rng(23)
    q, k, v = rng.random((I, K)) - 0.5, rng.random((J, K)) - 0.5, rng.random((J, D)) + 0.5
    k[:, 0] = 1.0
    q[0] = (709.0 / SCALE, 0.0, 0.0, 0.0)
    q[1, 0] = 0.0
    got, sums = run_special(gpu_ctx, q, k, v)
    want, want_sums = (x[0, 0] for x in ec.program(q[None, None], k[None, None], v[None, None], SCALE, f64))
    print("overflowing sum: device", got, sums, "float64 program", want, want_sums)
    assert np.all(want[0] == 0) and np.isinf(want_sums[0]) and np.all(np.isfinite(want[1])), want
    assert np.all(np.isnan(got[0])) and np.isnan(sums[0])
    assert np.all(np.abs(got[1] - want[1]) <= TOL64 * np.abs(want[1])) and abs(sums[1] - want_sums[1]) <= TOL64 * want_sums[1]


# ---- empty extents and refusals: raw calls on poisoned buffers --------------------------------------------------------------
POISON = -77.25


class Poisoned:
    def __init__(self, ctx, n):
        self.n, self.dev = n, ctx.allocBuffer(8 * n)
        self.dev.write(np.full(n, POISON))
        self.ptr = self.dev.ptr

    def read(self):
        return self.dev.readInto(np.empty(self.n, dtype=f64))


def raw(ctx, dims, Q, Kk, V, O, ld, sq, sk, sv, so, accumulate=0, scale=SCALE, S=None, ss=None):
    p = lambda x: ctypes.c_void_p(x.ptr if x is not None else 0)
    b0, b1, I, J, K, D = dims
    args = (ctx.handle, b0, b1, I, J, K, D, scale, p(Q), ld[0], sq[0], sq[1], p(Kk), ld[1], sk[0], sk[1], p(V), ld[2], sv[0], sv[1], p(O), ld[3],
            so[0], so[1], accumulate)
    if ss is None:
        return _lib.lib().eg_attention_f64(*args)
    return _lib.lib().eg_attention_sums_f64(*(args + (p(S), ss[0], ss[1])))


@pytest.mark.parametrize("dims", [(0, 3, 8, 8, 8, 8), (2, 0, 8, 8, 8, 8), (2, 3, 0, 8, 8, 8), (2, 3, 8, 8, 8, 0)], ids=ec.ident)
def test_empty_extents_launch_nothing(gpu_ctx, dims):
    buf = Poisoned(gpu_ctx, 2 * 3 * 8 * 8)
    rc = raw(gpu_ctx, dims, buf, buf, buf, buf, (8, 8, 8, 8), (192, 64), (192, 64), (192, 64), (192, 64))
    assert rc == 0, _lib.last_error()
    assert np.all(buf.read() == POISON)


@pytest.mark.parametrize("accumulate", [0, 1])
def test_no_keys(gpu_ctx, accumulate):
    """J == 0: zeros when not accumulating, nothing otherwise; Kk and V may be NULL; the sums are zeros either way"""
    q = Poisoned(gpu_ctx, 2 * 3 * 8 * 8)
    for with_sums in (False, True):
        out, sums = Poisoned(gpu_ctx, 2 * 3 * 8 * 8 + 5), Poisoned(gpu_ctx, 2 * 3 * 8 + 3)
        rc = raw(gpu_ctx, (2, 3, 8, 0, 8, 8), q, None, None, out, (8, 8, 8, 8), (192, 64), (0, 0), (0, 0), (192, 64), accumulate,
                 S=sums if with_sums else None, ss=(24, 8) if with_sums else None)
        assert rc == 0, _lib.last_error()
        got, s = out.read(), sums.read()
        assert np.all(got[:384] == (POISON if accumulate else 0)) and np.all(got[384:] == POISON)
        assert np.all(s[:48] == (0 if with_sums else POISON)) and np.all(s[48:] == POISON)


def test_no_head_dimension_is_the_mean_of_v(gpu_ctx):
    """K == 0 with NULL Q and Kk: every score is 0, every weight 1 / J"""
    J, D = 70, 12
    v = np.random.default_rng(19).random((J, D)) - 0.5
    dv, out = gpu_ctx.allocBuffer(v.nbytes), Poisoned(gpu_ctx, 2 * 5 * D + 3)
    dv.write(v)
    rc = raw(gpu_ctx, (2, 1, 5, J, 0, D), None, None, dv, out, (0, 0, D, D), (0, 0), (0, 0), (0, 0), (5 * D, 5 * D))
    assert rc == 0, _lib.last_error()
    got = out.read()
    want = np.broadcast_to(v.astype(np.longdouble).mean(0), (10, D))
    assert ec.rel(got[:10 * D].reshape(10, D), want) <= TOL64
    assert np.all(got[10 * D:] == POISON)


def test_no_value_columns_still_stores_the_sums(gpu_ctx):
    """D == 0 with NULL V and O: eg_attention_sums_f64 writes the denominators, eg_attention_f64 launches nothing"""
    dims = (1, 2, 65, 63, 20, 0)
    b0, b1, I, J, K, _ = dims
    q, k, _, _, want_sums = reference((1, 2, 65, 63, 20, 1))
    Q, Kk = View(q, K, b1 * I * K, I * K).upload(gpu_ctx), View(k, K, b1 * J * K, J * K).upload(gpu_ctx)
    S = View(np.full((b0, b1, 1, I), np.nan), I, b1 * (I + 5), I + 5).upload(gpu_ctx)
    ops.attention_sums_f64(gpu_ctx, b0, b1, I, J, K, 0, SCALE, Q.ptr, Q.ld, Q.strides, Kk.ptr, Kk.ld, Kk.strides, None, 0, (0, 0), None, 0, (0, 0),
                           S.ptr, S.strides)
    s_buf = S.read()
    S.same_outside(s_buf, "Sums")
    assert ec.rel(S.items(s_buf)[:, :, 0, :], want_sums) <= TOL64
    ops.attention_f64(gpu_ctx, b0, b1, I, J, K, 0, SCALE, Q.ptr, Q.ld, Q.strides, Kk.ptr, Kk.ld, Kk.strides, None, 0, (0, 0), None, 0, (0, 0))
    for x in (Q, Kk, S):
        x.free()


def test_error_returns(gpu_ctx):
    """the invalid and the unsupported calls of the contract, each with the entry's name; the buffers stay as they were"""
    buf = Poisoned(gpu_ctx, 2 * 3 * 8 * 8)
    big = Poisoned(gpu_ctx, 2 * 3 * 8 * 129)
    ok = dict(dims=(2, 3, 8, 8, 8, 8), Q=buf, Kk=buf, V=buf, O=buf, ld=(8, 8, 8, 8), sq=(192, 64), sk=(192, 64), sv=(192, 64), so=(192, 64))
    invalid = {
        "negative batch0": dict(dims=(-1, 3, 8, 8, 8, 8)), "negative J": dict(dims=(2, 3, 8, -1, 8, 8)), "negative D": dict(dims=(2, 3, 8, 8, 8, -1)),
        "batch0 of 2^31": dict(dims=(1 << 31, 3, 8, 8, 8, 8)), "batch1 of 2^31": dict(dims=(2, 1 << 31, 8, 8, 8, 8)),
        "NULL O": dict(O=None), "NULL Q": dict(Q=None), "NULL Kk": dict(Kk=None), "NULL V": dict(V=None),
        "ldq below K": dict(ld=(7, 8, 8, 8)), "ldk below K": dict(ld=(8, 7, 8, 8)), "ldv below D": dict(ld=(8, 8, 7, 8)),
        "ldo below D": dict(ld=(8, 8, 8, 7)),
        "negative stride_q0": dict(sq=(-192, 64)), "negative stride_k1": dict(sk=(192, -64)), "negative stride_v0": dict(sv=(-192, 64)),
        "stride_o0 == stride_o1": dict(so=(64, 64)), "stride_o1 of 0": dict(so=(192, 0)), "items of O overlap": dict(so=(192, 63)),
        "negative stride_o1": dict(so=(192, -64)),
    }
    for name, change in invalid.items():
        assert raw(gpu_ctx, **dict(ok, **change)) == EG_ERR_INVALID, name
        assert "eg_attention_f64" in _lib.last_error(), (name, _lib.last_error())
    sums = Poisoned(gpu_ctx, 2 * 3 * 8)
    for name, ss in {"stride_s0 == stride_s1": (8, 8), "items of Sums overlap": (24, 7), "stride_s1 of 0": (24, 0)}.items():
        assert raw(gpu_ctx, **dict(ok, S=sums, ss=ss)) == EG_ERR_INVALID, name
        assert "eg_attention_sums_f64" in _lib.last_error(), (name, _lib.last_error())
    for name, change in {"K of 129": dict(dims=(2, 3, 8, 8, 129, 8), ld=(129, 129, 8, 8), sq=(3096, 1032), sk=(3096, 1032), Q=big, Kk=big),
                         "D of 129": dict(dims=(2, 3, 8, 8, 8, 129), ld=(8, 8, 129, 129), sv=(3096, 1032), so=(3096, 1032), V=big, O=big)}.items():
        assert raw(gpu_ctx, **dict(ok, **change)) == EG_ERR_UNSUPPORTED, name
        assert "eg_attention_f64" in _lib.last_error() and "128" in _lib.last_error(), (name, _lib.last_error())
    gpu_ctx.sync()
    assert np.all(buf.read() == POISON) and np.all(big.read() == POISON) and np.all(sums.read() == POISON)
    out = Poisoned(gpu_ctx, 2 * 3 * 8 * 8)
    assert raw(gpu_ctx, **dict(ok, O=out)) == 0, _lib.last_error()     # the call the table of changes starts from
