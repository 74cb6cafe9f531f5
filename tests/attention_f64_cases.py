"""Float64 operands whose attention results are known exactly — the forward families of tests/attention_exact_cases.py in
doubles — for tests/test_gpu_attention_f64.py (eg_attention_f64 on the device) and tests/test_attention_f64_cases_cpu.py
(what this file claims, on the CPU).  No GPU, no HIP.

A bound relative to the LARGEST element of the output passes a wrong key picked among rows of like magnitude, a lost low bit
of V, an element that is wrong only where the output is small.  The operands here hold EVERY element of O and of Sums to
its own bits.  The scale is 0.25, a power of two.  With s_ij = q_i . k_j, e_ij = exp(scale * s_ij) (the double exp),
L_i = sum_j e_ij:

  uniform    Q = 0 or Kk = 0: every score is exactly 0, every e is exp(0) = 1 and L = J.  V holds multiples of 1/g in
             [-1, 1), g = 2^40: sum_j v_j is exact in any order (J < 2^12 terms below 2^40 units each), and
             O = fl(sum / J) is ONE correctly rounded double division.  Sums == J.
  selector   row i attends to exactly one key c = sel(i).  Three columns of Q and Kk (the first, the middle, the last: an
             unroll count that ends early loses one) hold q_i = (-B c^2, 2 B c, -B) and k_j = (1, j, j^2), B = 2^12; the
             others are zero.  s_ij = -B (c - j)^2 is a sum of integers in units of B: 0 at j = c, and scale * s <= -1024
             elsewhere, where the double exp is exactly 0 (its smallest positive result, 2^-1074, is exp(-744.4)).  So
             L = 1, Sums == 1 and O[i, :] = 1 * V[sel(i), :] + 0 + ... has the bits of V[sel(i), :], whatever V holds: here
             full 53-bit significands.

DIMS has one shape per pair of padded head sizes (kp, dp) in {32, 64, 128}^2: (K, D) from {20, 33, 65} x {12, 33, 65} and the
edges 32, 64, 128; I in {33, 65, 70} crosses a query tile; J in {31, 33, 63, 65, 130} is ragged across both key tiles the
planner may choose, 32 and 64; batch is (1, 2) or (2, 1).  tests/test_attention_f64_cases_cpu.py admits each row: the sum of
the absolute values of a sum's terms stays below 2^53 units of their common last bit, the closed form gives the stated
values, and a float64 evaluation in two summation orders gives the same bits.  Zeros are compared by value: the sign of a
zero is not part of the contract."""
import numpy as np

f64 = np.float64
SCALE = 0.25
B = 4096.0          # 2^12: scale * B = 1024, and exp(-1024.0) is 0 in float64
G = 2 ** 40         # the uniform family's grid

# (batch0, batch1, I, J, K, D), one per (kp, dp)
DIMS = [
    (1, 2, 33, 31, 20, 12),      # (32, 32)
    (2, 1, 65, 33, 32, 33),      # (32, 64), K at the edge
    (1, 2, 70, 63, 20, 65),      # (32, 128)
    (2, 1, 33, 65, 33, 12),      # (64, 32)
    (1, 2, 65, 130, 64, 64),     # (64, 64), both at the edge
    (2, 1, 70, 31, 33, 128),     # (64, 128), D at the edge
    (1, 2, 33, 63, 65, 32),      # (128, 32), D at the edge
    (2, 1, 65, 65, 128, 33),     # (128, 64), K at the edge
    (1, 2, 70, 130, 65, 65),     # (128, 128): the key tile of 32, five of them
]
ident = lambda d: "x".join(map(str, d))
padded = lambda n: 32 if n <= 32 else 64 if n <= 64 else 128


class Exact:
    """One case: q [b0,b1,I,K], k [b0,b1,J,K], v [b0,b1,J,D] and `want`: the float64 values of o [b0,b1,I,D] and sums [b0,b1,I]"""

    def __init__(self, family, dims, q, k, v, want, sel=None):
        self.family, self.dims, self.q, self.k, self.v, self.want, self.sel = family, dims, q, k, v, want, sel


def grid(rng, *shape):
    """multiples of 1/G in [-1, 1)"""
    return rng.integers(-G, G, size=shape).astype(f64) / f64(G)


def full(rng, *shape):
    """+-[1, 2) with all 52 fraction bits random: full 53-bit significands"""
    frac = rng.integers(0, 1 << 52, size=shape, dtype=np.uint64)
    x = (frac | np.uint64(1023 << 52)).view(f64)
    return np.where(rng.integers(0, 2, size=shape) == 1, -x, x)


def signs(rng, *shape):
    return rng.integers(-1, 2, size=shape).astype(f64)


def uniform(dims, zero, seed=None):
    """zero: "q" or "k", the operand that is all zeros; the other one lies in {-1, 0, 1}"""
    b0, b1, I, J, K, D = dims
    rng = np.random.default_rng(sum(dims) + (zero == "k") if seed is None else seed)
    q = np.zeros((b0, b1, I, K)) if zero == "q" else signs(rng, b0, b1, I, K)
    k = np.zeros((b0, b1, J, K)) if zero == "k" else signs(rng, b0, b1, J, K)
    v = grid(rng, b0, b1, J, D)
    mean = v.sum(2, keepdims=True) / f64(J)         # an exact sum, then one division, rounded once
    return Exact("uniform", dims, q, k, v, {"o": np.broadcast_to(mean, (b0, b1, I, D)).copy(), "sums": np.full((b0, b1, I), f64(J))})


def columns(K):
    """where the three live columns of Q and Kk sit: the first, the middle and the last"""
    assert K >= 3
    return 0, K // 2, K - 1


def selection(rng, I, J):
    """sel(i) = perm[i mod J] for a random permutation of the keys: injective for I <= J, onto for I >= J"""
    return rng.permutation(J)[np.arange(I) % J]


def selector(dims, seed=None):
    b0, b1, I, J, K, D = dims
    rng = np.random.default_rng(sum(dims) + 7 if seed is None else seed)
    sel = np.stack([np.stack([selection(rng, I, J) for _ in range(b1)]) for _ in range(b0)])       # [b0, b1, I]
    c0, c1, c2 = columns(K)
    q, k = np.zeros((b0, b1, I, K)), np.zeros((b0, b1, J, K))
    c, j = sel.astype(f64), np.arange(J, dtype=f64)
    q[..., c0], q[..., c1], q[..., c2] = -B * c * c, 2 * B * c, -B
    k[..., c0], k[..., c1], k[..., c2] = 1.0, j, j * j
    v = full(rng, b0, b1, J, D)
    return Exact("selector", dims, q, k, v, {"o": np.take_along_axis(v, sel[..., None], axis=2), "sums": np.ones((b0, b1, I))}, sel=sel)


# ---- what the CPU test holds --------------------------------------------------------------------------------------------------
def units(terms, unit, axis):
    """The sum over `axis` of |terms| in units of `unit`, at its largest; every term must be a whole number of units."""
    t = np.abs(np.asarray(terms, f64)) / f64(unit)
    assert np.array_equal(t, np.rint(t)), "a term off its grid of %r" % unit
    return float(t.sum(axis).max()) if t.size else 0.0


def sums_in_units(case):
    """{name of a sum in the derivation: the largest sum of |terms| in units of the terms' common last bit}"""
    if case.family == "selector":
        return {"scores": units(case.q[:, :, :, None, :] * case.k[:, :, None, :, :], B, -1)}
    return {"o": units(case.v, 1.0 / G, 2)}


def sum64(terms, axis, reverse):
    """float64, one addition after the other along `axis`, first to last or last to first"""
    terms = np.moveaxis(np.asarray(terms, f64), axis, 0)
    acc = np.zeros(terms.shape[1:], f64)
    for t in (terms[::-1] if reverse else terms):
        acc = acc + t
    return acc


def evaluate64(case, reverse):
    """The three-statement program in float64, every sum in one of two orders: {o, sums}"""
    q, k, v = case.q, case.k, case.v
    s = sum64(q[:, :, :, None, :] * k[:, :, None, :, :], -1, reverse)
    with np.errstate(under="ignore"):
        e = np.exp(s * f64(SCALE))
    sums = sum64(e, -1, reverse)
    return {"o": sum64(e[..., None] * v[:, :, None, :, :], 3, reverse) / sums[..., None], "sums": sums}


def same_values(got, want, what):
    """bit for bit, except that a zero may have either sign; the first difference named"""
    got, want = np.ascontiguousarray(got, f64), np.ascontiguousarray(want, f64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got.view(np.uint64) != want.view(np.uint64)) & ~((got == 0) & (want == 0)))
    assert bad.size == 0, "%s: %d of %d elements differ from the exact value; the first is %s: got %r, want %r" % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


# ---- the parity runs at the same shapes -----------------------------------------------------------------------------------------
TOL64 = 1e-12       # the project's float64 bound, relative to the largest element (tests/test_gpu_f64.py)


def random_operands(dims, seed=None, shared=False):
    """U[-0.5, 0.5) operands; shared: Kk and V have extent 1 along batch0"""
    b0, b1, I, J, K, D = dims
    rng = np.random.default_rng(1000 + sum(dims) if seed is None else seed)
    return rng.random((b0, b1, I, K)) - 0.5, rng.random((1 if shared else b0, b1, J, K)) - 0.5, rng.random((1 if shared else b0, b1, J, D)) - 0.5


def program(q, k, v, scale, dtype):
    """The three-statement program (scale, row sum of exp, exp / sum) around the two products, in `dtype`: (o, sums).  Per
    item, as matrix products: numpy.longdouble has no BLAS and takes numpy's own loops."""
    q, k, v = (np.asarray(x, dtype) for x in (q, k, v))
    k, v = np.broadcast_to(k, q.shape[:2] + k.shape[2:]), np.broadcast_to(v, q.shape[:2] + v.shape[2:])
    o = np.empty(q.shape[:3] + v.shape[3:], dtype)
    sums = np.empty(q.shape[:3], dtype)
    with np.errstate(all="ignore"):
        for a in range(q.shape[0]):
            for b in range(q.shape[1]):
                e = np.exp((q[a, b] @ k[a, b].T) * dtype(scale))
                sums[a, b] = e.sum(-1)
                o[a, b] = (e / sums[a, b][:, None]) @ v[a, b]
    return o, sums


def rel(got, want):
    """max|got - want| / max|want|, in the wider of the two types"""
    want = np.asarray(want)
    return float(np.max(np.abs(np.asarray(got, want.dtype) - want)) / np.max(np.abs(want)))


def forward_cases():
    """(id, make): uniform with either operand zero, the selector with a V of full significands, at every row of DIMS"""
    rows = [("uniform-%s-zero-%s" % (ident(d), z), lambda d=d, z=z: uniform(d, z)) for d in DIMS for z in "qk"]
    return rows + [("selector-%s" % ident(d), lambda d=d: selector(d)) for d in DIMS]
