"""Operands whose attention results are known exactly, for tests/test_gpu_attention_heads.py (the fused kernels on the
device) and tests/test_attention_exact_cases_cpu.py (what this file claims, on the CPU).  No GPU, no HIP.

The other attention tests compare with float64 under a bound normalised by the LARGEST element of the output: a wrong key
picked among rows of like magnitude, a lost low bit of V or dO, an element that is wrong only where the output is small all
pass it.  The operands here hold EVERY element to its own value, as tests/exact_cases.py does for the contractions.  The
scale is 0.25, a power of two.  With s_ij = q_i . k_j, e_ij = expf(scale * s_ij), L_i = sum_j e_ij, p_ij = e_ij / L_i:

  uniform    Q = 0 or Kk = 0: every score is exactly 0, every e is expf(0) = 1 and L = J.
             Forward, any J: V holds multiples of 1/g in [-1, 1), so sum_j v_j is exact in any order, and O = fl(sum / J) is
             ONE correctly rounded division (the float64 quotient of two float32 numbers, rounded to float32, is that value:
             53 >= 2 * 24 + 2 bits make the double rounding harmless).  Sums == J.
             Backward, J a power of two: 1 / L, p and O are exact.  dO and V are multiples of 1/g, the operand that is not
             zero lies in {-1, 0, 1}: delta_i = dO_i . o_i, dP_ij = dO_i . v_j, dP - delta, dS = (scale * p) (dP - delta)
             and the three gradients are sums of numbers on a common binary grid that stay below 2^24 of its units.  Q = 0
             gives an informative dQ and dK = 0, Kk = 0 an informative dK and dQ = 0: both are in the tables.
  selector   row i attends to exactly one key c = sel(i).  Three columns of Q and Kk (the first, the middle, the last: an
             unroll count that ends early loses one) hold q_i = (-B c^2, 2 B c, -B) and k_j = (1, j, j^2), B = 2^12; the
             others are zero.  s_ij = -B (c - j)^2 is a sum of integers in units of B: 0 at j = c, and scale * s <= -1024
             elsewhere, where expf is exactly 0.  So L = 1, Sums == 1 and O[i, :] has the bits of V[sel(i), :], whatever V
             holds (full 24-bit significands, exact_cases.values).  Backward with dO and V on the 1/8 grid: delta_i and
             dP_i,sel(i) are the same exact number, dS is exactly 0 everywhere, dQ = dK = 0 and dV_j is the exact sum of the
             dO rows that selected j.  With a dO of full significands and an injective sel, dV alone is exact: its row
             sel(i) has the bits of dO's row i, every other row is 0.

g is chosen per shape (the tables below); tests/test_attention_exact_cases_cpu.py admits a shape: it holds, for every sum
above, the sum of the absolute values of its terms below 2^24 units of their common last bit, the float64 closed form to
the stated values, and a float32 evaluation in two summation orders to the same bits.  Zeros are compared by value: the
sign of a zero is not part of the contract."""
import numpy as np

import attention_grad_cases as gc
from exact_cases import values

f32, f64 = np.float32, np.float64
SCALE = 0.25
B = 4096.0      # 2^12: scale * B = 1024, and expf(-1024) is 0 in float32


# ---- the tables: (batch0, batch1, I, J, K, D) and what else a case needs -------------------------------------------------------
# uniform forward: ragged J over one to four key tiles; g = 4096 gives V thirteen significand bits (200 keys: 2^20 units)
UNIFORM_FORWARD = [
    ((1, 2, 33, 130, 20, 12), 4096),     # (kp, dp) = (32, 32)
    ((1, 2, 65, 200, 32, 33), 4096),     # (32, 64)
    ((1, 2, 65, 130, 17, 65), 4096),     # (32, 128)
    ((2, 1, 70, 63, 65, 32), 4096),      # (128, 32)
    ((1, 1, 65, 130, 64, 128), 4096),    # (64, 128)
]
# uniform backward: J a power of two, I below and above J; g as large as dQ and dK allow (their terms are in units of
# scale / (g^2 J^2) and there are J or I of them)
UNIFORM_BACKWARD = [
    ((1, 2, 65, 64, 20, 12), 8),         # (32, 32)
    ((1, 2, 65, 64, 32, 33), 8),         # (32, 64)
    ((1, 2, 70, 128, 17, 65), 8),        # (32, 128), two key tiles
    ((2, 1, 65, 16, 65, 32), 8),         # (128, 32)
    ((1, 1, 33, 64, 64, 128), 8),        # (64, 128)
    ((1, 1, 66, 128, 128, 40), 8),       # (128, 64)
]
# selector: I below and above J, ragged J over several key tiles
SELECTOR = [
    (1, 2, 66, 63, 20, 12),              # (32, 32), I > J
    (1, 2, 65, 130, 32, 33),             # (32, 64)
    (1, 2, 200, 63, 17, 65),             # (32, 128), I > J, four query tiles
    (2, 1, 65, 130, 65, 32),             # (128, 32)
    (1, 1, 70, 200, 128, 40),            # (128, 64)
]
ident = lambda d: "x".join(map(str, d))


class Exact:
    """One case: q [b0,b1,I,K], k [b0,b1,J,K], v [b0,b1,J,D], d_out [b0,b1,I,D] or None (forward only), and `want`: the
    float32 values of o, sums and — with a d_out — dq, dk, dv (None where the case makes no claim)."""

    def __init__(self, family, dims, q, k, v, d_out, want, g=None, sel=None):
        self.family, self.dims, self.q, self.k, self.v, self.d_out, self.want, self.g, self.sel = family, dims, q, k, v, d_out, want, g, sel


def grid(rng, g, *shape):
    """multiples of 1/g in [-1, 1)"""
    return (rng.integers(-g, g, size=shape) / f64(g)).astype(f32)


def signs(rng, *shape):
    return rng.integers(-1, 2, size=shape).astype(f32)


def power_of_two(n):
    return n > 0 and n & (n - 1) == 0


# ---- uniform ------------------------------------------------------------------------------------------------------------------
def uniform(dims, g, zero, backward, seed=None):
    """zero: "q" or "k", the operand that is all zeros; the other one lies in {-1, 0, 1}"""
    b0, b1, I, J, K, D = dims
    rng = np.random.default_rng(sum(dims) + g + (zero == "k") if seed is None else seed)
    q = np.zeros((b0, b1, I, K), f32) if zero == "q" else signs(rng, b0, b1, I, K)
    k = np.zeros((b0, b1, J, K), f32) if zero == "k" else signs(rng, b0, b1, J, K)
    v = grid(rng, g, b0, b1, J, D)
    mean = (v.astype(f64).sum(2, keepdims=True) / f64(J)).astype(f32)       # one division, rounded once
    want = {"o": np.broadcast_to(mean, (b0, b1, I, D)).copy(), "sums": np.full((b0, b1, I), J, f32)}
    d_out = None
    if backward:
        assert power_of_two(J), dims
        d_out = grid(rng, g, b0, b1, I, D)
        _, _, dq, dk, dv = gc.closed_form(q, k, v, d_out, SCALE)
        want.update(dq=dq.astype(f32), dk=dk.astype(f32), dv=dv.astype(f32))
    return Exact("uniform", dims, q, k, v, d_out, want, g=g)


# ---- selector -----------------------------------------------------------------------------------------------------------------
def columns(K):
    """where the three live columns of Q and Kk sit: the first, the middle and the last"""
    assert K >= 3
    return 0, K // 2, K - 1


def selection(rng, I, J):
    """sel(i) = perm[i mod J] for a random permutation of the keys: injective for I <= J, onto for I >= J, and neighbouring
    rows land in different 16-key blocks and 64-key tiles"""
    return rng.permutation(J)[np.arange(I) % J]


def selector(dims, v_kind="full", d_out_kind=None, seed=None):
    """v_kind / d_out_kind: "full" (24-bit significands in +-[1, 2)) or "grid" (multiples of 1/8); d_out_kind None: forward only.
    A "full" d_out claims dV alone and needs I <= J."""
    b0, b1, I, J, K, D = dims
    rng = np.random.default_rng(sum(dims) + 7 if seed is None else seed)
    sel = np.stack([np.stack([selection(rng, I, J) for _ in range(b1)]) for _ in range(b0)])       # [b0, b1, I]
    c0, c1, c2 = columns(K)
    q, k = np.zeros((b0, b1, I, K), f64), np.zeros((b0, b1, J, K), f64)
    c, j = sel.astype(f64), np.arange(J, dtype=f64)
    q[..., c0], q[..., c1], q[..., c2] = -B * c * c, 2 * B * c, -B
    k[..., c0], k[..., c1], k[..., c2] = 1.0, j, j * j
    assert np.array_equal(q.astype(f32), q) and np.array_equal(k.astype(f32), k)
    draw = lambda kind, *shape: values(shape, rng) if kind == "full" else grid(rng, 8, *shape)
    v = draw(v_kind, b0, b1, J, D)
    want = {"o": np.take_along_axis(v, sel[..., None], axis=2), "sums": np.ones((b0, b1, I), f32)}
    d_out = None
    if d_out_kind:
        d_out = draw(d_out_kind, b0, b1, I, D)
        dv = np.zeros((b0, b1, J, D), f64)
        for o in range(b0):
            for i1 in range(b1):
                np.add.at(dv[o, i1], sel[o, i1], d_out[o, i1].astype(f64))
        if d_out_kind == "full":
            assert I <= J, dims         # injective: every row of dV is one row of dO or zero
            want.update(dq=None, dk=None, dv=dv.astype(f32))
        else:
            want.update(dq=np.zeros((b0, b1, I, K), f32), dk=np.zeros((b0, b1, J, K), f32), dv=dv.astype(f32))
    return Exact("selector", dims, q.astype(f32), k.astype(f32), v, d_out, want, sel=sel)


# ---- what the CPU test holds --------------------------------------------------------------------------------------------------
def units(terms, unit, axis):
    """The sum over `axis` of |terms| in units of `unit`, at its largest; every term must be a whole number of units."""
    t = np.abs(np.asarray(terms, f64)) / f64(unit)
    assert np.array_equal(t, np.rint(t)), "a term off its grid of %r" % unit
    return float(t.sum(axis).max()) if t.size else 0.0


def sums_in_units(case):
    """{name of a sum in the derivation: the largest sum of |terms| in units of the terms' common last bit}.  float64 holds
    every term exactly (products of two float32 numbers).  For a selector case the sums that have one nonzero term (O, the
    gradients through p in {0, 1}) are in the list with their unit; dQ and dK have no nonzero term at all."""
    q, k, v, d_out = (None if x is None else x.astype(f64) for x in (case.q, case.k, case.v, case.d_out))
    b0, b1, I, J, K, D = case.dims
    out = {}
    if case.family == "selector":
        out["scores"] = units(q[:, :, :, None, :] * k[:, :, None, :, :], B, -1)
        if d_out is None or case.want["dq"] is None:
            return out
        g, o = 8, case.want["o"].astype(f64)
        p = (np.arange(J)[None, None, None, :] == case.sel[..., None]).astype(f64)
        pj = 1
    else:
        g = case.g
        out["o"] = units(v, 1.0 / g, 2)
        if d_out is None:
            return out
        o = v.sum(2, keepdims=True) / J + np.zeros((b0, b1, I, D))
        p = np.full((b0, b1, I, J), 1.0 / J)
        pj = J
    delta_t = d_out * o                                                            # [.., I, D], units 1 / (g^2 J)
    dp_t = d_out[:, :, :, None, :] * v[:, :, None, :, :]                           # [.., I, J, D], units 1 / g^2
    out["delta"] = units(delta_t, 1.0 / (g * g * pj), -1)
    out["dp"] = units(dp_t, 1.0 / (g * g), -1)
    delta, dp = delta_t.sum(-1), dp_t.sum(-1)
    out["dp-delta"] = units(np.stack([dp, np.broadcast_to(delta[..., None], dp.shape)]), 1.0 / (g * g * pj), 0)
    ds = SCALE * p * (dp - delta[..., None])                                       # power-of-two factors: units scale / (g^2 J^2)
    u_ds = SCALE / (g * g * pj * pj)
    out["dq"] = units(ds[..., None] * k[:, :, None, :, :], u_ds, 3)
    out["dk"] = units(ds[..., None] * q[:, :, :, None, :], u_ds, 2)
    out["dv"] = units(p[..., None] * d_out[:, :, :, None, :], 1.0 / (g * pj), 2)
    return out


def sum32(terms, axis, reverse):
    """float32, one addition after the other along `axis`, first to last or last to first"""
    terms = np.moveaxis(np.asarray(terms, f32), axis, 0)
    acc = np.zeros(terms.shape[1:], f32)
    for t in (terms[::-1] if reverse else terms):
        acc = (acc + t).astype(f32)
    return acc


def evaluate32(case, reverse):
    """The formulas of the kernels' headers in float32, every sum in one of two orders: {o, sums, dq, dk, dv}."""
    q, k, v, scale = case.q, case.k, case.v, f32(SCALE)
    s = sum32(q[:, :, :, None, :] * k[:, :, None, :, :], -1, reverse)
    with np.errstate(under="ignore"):
        e = np.exp((s * scale).astype(f32)).astype(f32)
    sums = sum32(e, -1, reverse)
    o = (sum32(e[..., None] * v[:, :, None, :, :], 3, reverse) / sums[..., None]).astype(f32)
    got = {"o": o, "sums": sums}
    if case.d_out is not None:
        d = case.d_out
        delta = sum32(d * o, -1, reverse)
        dp = sum32(d[:, :, :, None, :] * v[:, :, None, :, :], -1, reverse)
        p = (e * (f32(1.0) / sums)[..., None]).astype(f32)
        ds = ((scale * p) * (dp - delta[..., None])).astype(f32)
        got.update(dq=sum32(ds[..., None] * k[:, :, None, :, :], 3, reverse), dk=sum32(ds[..., None] * q[:, :, :, None, :], 2, reverse),
                   dv=sum32(p[..., None] * d[:, :, :, None, :], 2, reverse))
    return got


def same_values(got, want, what):
    """bit for bit, except that a zero may have either sign; the first difference named"""
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~((got == 0) & (want == 0)))
    assert bad.size == 0, "%s: %d of %d elements differ from the exact value; the first is %s: got %r, want %r" % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


# ---- every case the GPU test runs ---------------------------------------------------------------------------------------------
def forward_cases():
    """(id, make): uniform with either operand zero at any J, the selector with a V of full significands"""
    rows = [("uniform-%s-zero-%s" % (ident(d), z), lambda d=d, g=g, z=z: uniform(d, g, z, backward=False)) for d, g in UNIFORM_FORWARD for z in "qk"]
    return rows + [("selector-%s" % ident(d), lambda d=d: selector(d, "full")) for d in SELECTOR]


def backward_cases():
    """(id, make): uniform with either operand zero, the selector on the 1/8 grid, and the selector with a dO of full
    significands where sel is injective (dV alone)"""
    rows = [("uniform-%s-zero-%s" % (ident(d), z), lambda d=d, g=g, z=z: uniform(d, g, z, backward=True)) for d, g in UNIFORM_BACKWARD for z in "qk"]
    rows += [("selector-%s-grid" % ident(d), lambda d=d: selector(d, "grid", "grid")) for d in SELECTOR]
    return rows + [("selector-%s-full-dO" % ident(d), lambda d=d: selector(d, "grid", "full")) for d in SELECTOR if d[2] <= d[3]]
