"""GPU parity of eg_attention (kernels/attention_f32.hip) against a float64 numpy evaluation of

    O[i,:] = (sum_j exp(scale * q_i . k_j) * V[j,:]) / (sum_j exp(scale * q_i . k_j))

and, for J <= 200, against the oracle running the five-statement program (tests/attention_fused_programs.py), within TOL
(1e-5 of the largest value).  tests/test_attention_fused_oracle_cpu.py holds the oracle itself to 5e-6 on those shapes; the
oracle's serial sum of 4100 terms has not been held to that, so J = 4100 is compared with float64 only.

Every operand sits inside a larger device allocation filled with NaN: a read in front of a view, behind a row's end, behind
the last row or of a key j >= J shows up as a NaN row, and the whole O buffer is compared bit for bit with its state before
the call outside the items' I x D elements."""
import ctypes

import numpy as np
import pytest

import attention_fused_programs as fp
import refcases
from conftest import TOL, rel_err
from exprgrad_amd import _lib, ops
from test_gpu_special_values import same_special

pytestmark = pytest.mark.gpu

EG_ERR_INVALID, EG_ERR_UNSUPPORTED = 1, 5
GUARD = 64      # floats of NaN in front of and behind every operand; a multiple of 4, so that offset 0 stays 16-byte aligned
SCALE = fp.SCALE
# (batch0, batch1, I, J, K, D)
DIMS = [(2, 3, 33, 70, 16, 16), (1, 1, 1, 1, 1, 1), (1, 2, 65, 63, 20, 12), (2, 1, 64, 64, 64, 64), (1, 2, 130, 129, 128, 128),
        (3, 2, 7, 200, 33, 1), (1, 1, 5, 4100, 8, 8)]
LAYOUTS = ["bihk", "bhik"]


def u(rng, *shape):
    return (rng.random(shape, dtype=np.float32) - np.float32(0.5)).astype(np.float32)


class View:
    """A [b0, b1, R, C] operand placed in a NaN-filled host buffer at `offset` floats behind the guard: row step ld, strides
    (s0, s1) of the two batch indices; a stride of 0 shares the operand along that index (x then has extent 1 there)."""

    def __init__(self, x, ld, s0, s1, offset=0, fill=np.nan):
        b0, b1, R, C = x.shape
        self.shape, self.ld, self.strides, self.offset = x.shape, ld, (s0, s1), offset
        span = (b0 - 1) * s0 + (b1 - 1) * s1 + (R - 1) * ld + C
        self.buf = np.full(GUARD + offset + span + GUARD, fill, dtype=np.float32)
        self.items(self.buf)[...] = x

    def items(self, buf):
        b0, b1, R, C = self.shape
        return np.lib.stride_tricks.as_strided(buf[GUARD + self.offset:], (b0, b1, R, C), (4 * self.strides[0], 4 * self.strides[1], 4 * self.ld, 4))

    def upload(self, ctx):
        self.dev = ctx.allocTensor(self.buf.shape)
        self.dev.write(self.buf)
        return self

    @property
    def ptr(self):
        return self.dev.ptr + 4 * (GUARD + self.offset)


def lay(layout, b1, R, C, pad=0):
    """(ld, s0, s1) of a [b0, b1, R, C] operand: heads inside the row ([b,i,h,*]) or nested ([b,h,i,*])"""
    if layout == "bihk":
        ld = b1 * C + pad
        return ld, R * ld, C
    ld = C + pad
    return ld, b1 * R * ld, R * ld


def exact(q, k, v, scale):
    """float64, item by item; q [b0,b1,I,K] (an extent of 1 in k, v: shared)"""
    q, k, v = (np.asarray(x, np.float64) for x in (q, k, v))
    e = np.exp(np.einsum("obik,objk->obij", q, np.broadcast_to(k, q.shape[:2] + k.shape[2:])) * np.float64(np.float32(scale)))
    return np.einsum("obij,objd->obid", e, np.broadcast_to(v, q.shape[:2] + v.shape[2:])) / e.sum(-1, keepdims=True)


_ORACLES = {}


def oracle(q, k, v, graphs=None, key="scaled"):
    """the oracle on the program: its tensors are [B,I,H,K], [B,J,H,K], [B,J,H,D] -> [B,I,H,D]"""
    from oracle import kd
    if key not in _ORACLES:
        _ORACLES[key] = kd.Model(refcases.program_text((graphs or fp.attention_forward())()), threads=4)
    t = lambda x: np.ascontiguousarray(np.broadcast_to(x, q.shape[:2] + x.shape[2:]).transpose(0, 2, 1, 3))
    with np.errstate(all="ignore"):
        out = _ORACLES[key].call("out", {"q": t(q), "kk": t(k), "v": t(v)})
    return np.asarray(out).transpose(0, 2, 1, 3)


def attention(ctx, Q, Kk, V, O, dims, scale=SCALE, accumulate=False):
    b0, b1, I, J, K, D = dims
    ops.attention(ctx, b0, b1, I, J, K, D, scale, Q.ptr, Q.ld, Q.strides, Kk.ptr, Kk.ld, Kk.strides, V.ptr, V.ld, V.strides, O.ptr, O.ld, O.strides,
                  accumulate)
    return O.dev.read()


def operands(ctx, dims, layout, seed, offset=0, shared=False, pad=0, o_fill=np.nan, o_init=None):
    b0, b1, I, J, K, D = dims
    rng = np.random.default_rng(seed)
    q, k, v = u(rng, b0, b1, I, K), u(rng, 1 if shared else b0, b1, J, K), u(rng, 1 if shared else b0, b1, J, D)
    ldq, q0, q1 = lay(layout, b1, I, K, pad)
    ldk, k0, k1 = lay(layout, b1, J, K, pad)
    ldv, v0, v1 = lay(layout, b1, J, D, pad)
    ldo, o0, o1 = lay(layout, b1, I, D, 3)      # ldo > D in either layout
    Q = View(q, ldq, q0, q1, offset).upload(ctx)
    Kk = View(k, ldk, 0 if shared else k0, k1, offset).upload(ctx)
    V = View(v, ldv, 0 if shared else v0, v1, offset).upload(ctx)
    O = View(np.full((b0, b1, I, D), o_fill, np.float32) if o_init is None else o_init, ldo, o0, o1, offset, fill=o_fill).upload(ctx)
    return (q, k, v), (Q, Kk, V, O)


def check(dims, label, host, O, got_buf, with_oracle, base=None):
    """the items against float64 (and the oracle); everything else of the O buffer bit-unchanged"""
    q, k, v = host
    got = O.items(got_buf).copy()
    want64 = exact(q, k, v, SCALE)
    if base is not None:
        want64 = want64 + base.astype(np.float64)
    e64 = rel_err(got, want64, label + " vs float64")
    e_or = 0.0
    if with_oracle:
        want32 = oracle(q, k, v)
        if base is not None:
            want32 = want32 + base
        e_or = rel_err(got, want32, label + " vs oracle")
    print(label, "vs float64", e64, "vs oracle", e_or if with_oracle else "-")
    assert np.all(np.isfinite(got)), label
    assert e64 <= TOL and e_or <= TOL, (label, e64, e_or)
    want_buf = O.buf.copy()
    O.items(want_buf)[...] = got
    assert np.array_equal(got_buf.view(np.uint32), want_buf.view(np.uint32)), label + ": stored outside the items of O"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "x".join(map(str, d)))
def test_table(gpu_ctx, dims, layout):
    """accumulate = 0 over an O of NaN, operands between NaN guards, at aligned pointers"""
    host, (Q, Kk, V, O) = operands(gpu_ctx, dims, layout, seed=sum(dims))
    got = attention(gpu_ctx, Q, Kk, V, O, dims)
    check(dims, "eg_attention %s %s" % (dims, layout), host, O, got, with_oracle=dims[3] <= 200)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dims", [(2, 3, 33, 70, 16, 16), (2, 1, 64, 64, 64, 64), (3, 2, 7, 200, 33, 1)], ids=lambda d: "x".join(map(str, d)))
def test_pointers_offset_by_one_float(gpu_ctx, dims, layout):
    """no operand is 16-byte aligned: the element-load path"""
    host, (Q, Kk, V, O) = operands(gpu_ctx, dims, layout, seed=1 + sum(dims), offset=1)
    got = attention(gpu_ctx, Q, Kk, V, O, dims)
    check(dims, "eg_attention %s %s offset 1" % (dims, layout), host, O, got, with_oracle=True)


def test_sixteen_byte_rows_with_a_ragged_last_chunk(gpu_ctx, layout="bhik"):
    """K = 33 and D = 1 in rows padded to a multiple of 4: 16-byte loads whose last chunk of a row is read element by element"""
    dims = (3, 2, 7, 200, 33, 1)
    host, (Q, Kk, V, O) = operands(gpu_ctx, dims, layout, seed=5, pad=3)
    assert all(x.ld % 4 == 0 and all(s % 4 == 0 for s in x.strides) and x.ptr % 16 == 0 for x in (Q, Kk, V))
    got = attention(gpu_ctx, Q, Kk, V, O, dims)
    check(dims, "eg_attention %s %s padded rows" % (dims, layout), host, O, got, with_oracle=True)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_shared_keys_and_values(gpu_ctx, layout):
    """strides 0 along batch0 for Kk and V"""
    dims = (2, 3, 33, 70, 16, 16)
    host, (Q, Kk, V, O) = operands(gpu_ctx, dims, layout, seed=7, shared=True)
    assert Kk.strides[0] == 0 and V.strides[0] == 0
    got = attention(gpu_ctx, Q, Kk, V, O, dims)
    check(dims, "eg_attention %s %s shared" % (dims, layout), host, O, got, with_oracle=True)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_accumulate_adds_to_o(gpu_ctx, layout):
    dims = (1, 2, 65, 63, 20, 12)
    base = u(np.random.default_rng(11), 1, 2, 65, 12)
    host, (Q, Kk, V, O) = operands(gpu_ctx, dims, layout, seed=12, o_init=base)
    got = attention(gpu_ctx, Q, Kk, V, O, dims, accumulate=True)
    check(dims, "eg_attention %s %s accumulate" % (dims, layout), host, O, got, with_oracle=True, base=base)


def test_twice_the_same_bits(gpu_ctx):
    dims = (2, 3, 130, 200, 20, 12)
    host, (Q, Kk, V, O) = operands(gpu_ctx, dims, "bihk", seed=13)
    first = attention(gpu_ctx, Q, Kk, V, O, dims)
    O.dev.write(O.buf)
    second = attention(gpu_ctx, Q, Kk, V, O, dims)
    check(dims, "eg_attention %s twice" % (dims,), host, O, first, with_oracle=False)
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))


def run_special(ctx, q, k, v):
    """one item, dense operands; (device rows, oracle rows)"""
    I, K = q.shape
    J, D = v.shape
    q4, k4, v4 = q[None, None], k[None, None], v[None, None]
    Q, Kk, V = View(q4, K, I * K, I * K).upload(ctx), View(k4, K, J * K, J * K).upload(ctx), View(v4, D, J * D, J * D).upload(ctx)
    O = View(np.full((1, 1, I, D), np.nan, np.float32), D + 3, I * (D + 3), I * (D + 3)).upload(ctx)
    got = O.items(attention(ctx, Q, Kk, V, O, (1, 1, I, J, K, D)))[0, 0].copy()
    return got, oracle(q4, k4, v4)[0, 0]


def test_special_rows(gpu_ctx):
    """Special scores against the oracle on the program, through same_special (NaN where it has NaN, finite values within TOL
    of each value itself — so V is U[0.5, 1.5) here: a weighted mean of like-signed values does not cancel).  Every key has
    1 in column 1, and only key 3 an entry (1) in column 0; the rows of q:
      0  (0, +Inf, 0, 0): every score +Inf           -> NaN        1  a NaN in q                  -> NaN
      2  (0, -1e30, 0, 0): every term underflows      -> 0 / 0      3  (88 / scale, 0, 0, 0): one term exp(88), finite
      4  ordinary"""
    I, J, K, D = 5, 70, 4, 4
    rng = np.random.default_rng(17)
    q, k, v = u(rng, I, K), u(rng, J, K), u(rng, J, D) + np.float32(1.0)
    k[:, 0] = 0.0
    k[3, 0] = 1.0
    k[:, 1] = 1.0
    q[0] = (0.0, np.inf, 0.0, 0.0)
    q[1, 2] = np.nan
    q[2] = (0.0, -1e30, 0.0, 0.0)
    q[3] = (88.0 / SCALE, 0.0, 0.0, 0.0)
    got, want = run_special(gpu_ctx, q, k, v)
    print("special rows: device", got, "oracle", want)
    assert np.all(np.isnan(want[:3])) and np.all(np.isfinite(want[3:])), want
    same_special(got, want, "eg_attention special rows")


def test_a_minus_infinity_score_adds_nothing(gpu_ctx):
    """key 5 has -Inf in column 1 and every row of q has 1 there: one score of -Inf per row, whose term is exactly 0"""
    I, J, K, D = 5, 70, 4, 4
    rng = np.random.default_rng(18)
    q, k, v = u(rng, I, K), u(rng, J, K), u(rng, J, D) + np.float32(1.0)
    q[:, 1] = 1.0
    k[5, 1] = -np.inf
    got, want = run_special(gpu_ctx, q, k, v)
    print("-Inf score: device", got, "oracle", want)
    assert np.all(np.isfinite(want)), want
    same_special(got, want, "eg_attention -Inf score")
    live = np.arange(J) != 5
    assert rel_err(got, exact(q[None, None][:, :, :, :], k[None, None][:, :, live], v[None, None][:, :, live], SCALE)[0, 0], "-Inf score vs float64 without that key") <= TOL


def test_a_sum_that_overflows_is_nan_where_the_program_gives_zero(gpu_ctx):
    """The one departure the header states.  Row 0 has 70 scores of 88 / scale: every term is exp(88) = 1.65e38, finite, and
    their sum overflows.  The program divides each finite term by Inf and gives 0; this entry turns an infinite denominator
    into NaN.  Row 1 is ordinary and agrees."""
    I, J, K, D = 2, 70, 4, 4
    rng = np.random.default_rng(23)
    q, k, v = u(rng, I, K), u(rng, J, K), u(rng, J, D) + np.float32(1.0)
    k[:, 0] = 1.0
    q[0] = (88.0 / SCALE, 0.0, 0.0, 0.0)
    q[1, 0] = 0.0
    got, want = run_special(gpu_ctx, q, k, v)
    print("overflowing sum: device", got, "oracle", want)
    assert np.all(want[0] == 0) and np.all(np.isfinite(want[1])), want
    assert np.all(np.isnan(got[0])), got
    same_special(got[1], want[1], "eg_attention row next to an overflowing sum")


def raw(ctx, dims, Q, Kk, V, O, ld, sq, sk, sv, so, accumulate=0, scale=SCALE):
    p = lambda x: ctypes.c_void_p(x.ptr if x is not None else 0)
    b0, b1, I, J, K, D = dims
    return _lib.lib().eg_attention(ctx.handle, b0, b1, I, J, K, D, scale, p(Q), ld[0], sq[0], sq[1], p(Kk), ld[1], sk[0], sk[1], p(V), ld[2], sv[0],
                                   sv[1], p(O), ld[3], so[0], so[1], accumulate)


POISON = np.float32(-77.25)


def poisoned(ctx, n):
    t = ctx.allocTensor((n,))
    t.write(np.full(n, POISON, np.float32))
    return t


@pytest.mark.parametrize("dims", [(0, 3, 8, 8, 8, 8), (2, 0, 8, 8, 8, 8), (2, 3, 0, 8, 8, 8), (2, 3, 8, 8, 8, 0)], ids=lambda d: "x".join(map(str, d)))
def test_empty_extents_launch_nothing(gpu_ctx, dims):
    buf = poisoned(gpu_ctx, 2 * 3 * 8 * 8)
    rc = raw(gpu_ctx, dims, buf, buf, buf, buf, (8, 8, 8, 8), (192, 64), (192, 64), (192, 64), (192, 64))
    assert rc == 0, _lib.last_error()
    assert np.all(buf.read() == POISON)


@pytest.mark.parametrize("accumulate", [0, 1])
def test_no_keys(gpu_ctx, accumulate):
    """J == 0: zeros when not accumulating, nothing otherwise; Kk and V may be NULL"""
    out = poisoned(gpu_ctx, 2 * 3 * 8 * 8 + 5)
    q = poisoned(gpu_ctx, 2 * 3 * 8 * 8)
    rc = raw(gpu_ctx, (2, 3, 8, 0, 8, 8), q, None, None, out, (8, 8, 8, 8), (192, 64), (0, 0), (0, 0), (192, 64), accumulate)
    assert rc == 0, _lib.last_error()
    got = out.read()
    assert np.all(got[:384] == (POISON if accumulate else 0)) and np.all(got[384:] == POISON)


def test_no_head_dimension_is_the_mean_of_v(gpu_ctx):
    """K == 0 with NULL Q and Kk: every score is 0, every weight 1 / J"""
    J, D = 70, 12
    v = u(np.random.default_rng(19), J, D)
    dv, out = gpu_ctx.allocTensor(v.shape), poisoned(gpu_ctx, 2 * 5 * D + 3)
    dv.write(v)
    rc = raw(gpu_ctx, (2, 1, 5, J, 0, D), None, None, dv, out, (0, 0, D, D), (0, 0), (0, 0), (0, 0), (5 * D, 5 * D))
    assert rc == 0, _lib.last_error()
    got = out.read()
    want = np.broadcast_to(v.astype(np.float64).mean(0), (10, D))
    assert rel_err(got[:10 * D].reshape(10, D), want, "eg_attention K == 0 vs float64") <= TOL
    assert np.all(got[10 * D:] == POISON)


def test_error_returns(gpu_ctx):
    """the invalid and the unsupported calls of the contract, each with the function's name; O stays as it was"""
    buf = poisoned(gpu_ctx, 2 * 3 * 8 * 8)
    big = poisoned(gpu_ctx, 2 * 3 * 8 * 129)
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
        assert "eg_attention" in _lib.last_error(), (name, _lib.last_error())
    for name, change in {"K of 129": dict(dims=(2, 3, 8, 8, 129, 8), ld=(129, 129, 8, 8), sq=(3096, 1032), sk=(3096, 1032), Q=big, Kk=big),
                         "D of 129": dict(dims=(2, 3, 8, 8, 8, 129), ld=(8, 8, 129, 129), sv=(3096, 1032), so=(3096, 1032), V=big, O=big)}.items():
        assert raw(gpu_ctx, **dict(ok, **change)) == EG_ERR_UNSUPPORTED, name
        assert "eg_attention" in _lib.last_error() and "128" in _lib.last_error(), (name, _lib.last_error())
    gpu_ctx.sync()
    assert np.all(buf.read() == POISON) and np.all(big.read() == POISON)
    out = poisoned(gpu_ctx, 2 * 3 * 8 * 8)
    assert raw(gpu_ctx, **dict(ok, O=out)) == 0, _lib.last_error()     # the call the table of changes starts from
