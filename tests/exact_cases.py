"""Operands whose product is known exactly, for tests/test_gpu_exact_products.py (every contraction route of the library
on the device) and tests/test_exact_cases_cpu.py (what this file claims, on the CPU).  No GPU, no HIP.

The suite's other contraction tests compare with a float64 product under a bound normalised by the LARGEST element of C
(tests/gemm_view_cases.py), or bit for bit with a sibling that shares the arithmetic.  Neither sees an error that is small
against max|C|: an operand that lost its low significand bits, one wrong element in a row of small values, a split-bf16
product that dropped one of its 2^-16 terms.  The operands here hold EVERY element of C to its own value:

  monomial   op(A) has one nonzero per row (monomial_rows), or op(B) one per column (monomial_cols), the other operand
             is dense: C[i,j] is ONE product, every other addend is an exact zero.  All values are +-[1, 2) with every
             significand bit in use (the last one is always set), so nothing is zero, subnormal or overflows, and a lost
             low bit of either operand changes the product.
  grid       multiples of 1/8 in [-1, 1): every product is a multiple of 1/64, and a sum of up to 2^17 of them is an
             integer multiple of 1/64 below 2^17 in size, 24 bits: exact in float32 in any order of summation.

Bounds.  None is measured on a kernel.  u = 2^-24 for float32, 2^-53 for float64; ab is the exact product.

  exact routes, monomial, no start values, no bias:  the bits of fl(ab).
      The f32 and f64 matrix instructions are fused-multiply-add chains: 0 + ab rounds once, fl(ab) + (+-0) is fl(ab), and
      a second pass (slab sums, stream-K fix-up, tail tiles) adds slabs that are exact zeros.  A bias of zeros, where a
      fixture row needs a bias for its plan, adds +0 to a nonzero number: no bit changes.
  exact routes, grid:  the bits of numpy's own product in the same type (exact, whatever the order).
  exact routes, monomial with start values and a bias:  |got - (old + ab + bias)| <= 3u (|old| + |ab| + |bias|).
      One rounding of the product and one per addition, each at most u of a partial sum that is at most
      |old| + |ab| + |bias| (to first order; the second-order terms are 2^-24 of the bound).  Where the kernel's header
      states the order — the second passes of gemm_f32_mfma.hpp, split-K and tail tiles: C = (old + sum of slabs) + bias —
      the test asserts the bits of fl(fl(old + fl(ab)) + bias) as well.  (The float64 kernels compute old + (ab + bias);
      their headers leave the order open, so they are held to the bound alone.)
  split-bf16 product, monomial:  |got - ab| <= 8 * 2^-24 |ab|  (SPLIT_UNITS).
      Kept: a0b0 + (a0b1 + a1b0) + (a0b2 + a1b1 + a2b0).  Each piece is the rounding of a remainder to 8 bits, so
      |x1| <= 2^-8 |x| and |x2| <= 2^-16 |x|: the dropped a1b2 + a2b1 + a2b2 are at most (2 * 2^-24 + 2^-32) |ab|, which
      is (2 + 2^-8) units.
      Six terms onto one accumulator that starts at zero are at most five roundings to nearest of a partial sum of about
      |ab|: half an ulp of that sum each, which is at most one unit (it is one when |ab| is just above a power of two,
      half of one just below the next): at most 7.01 units, under 8.  six_term_product emulates it: 2.5 units at most on
      2^20 pairs when every term rounds, 1.6 when an MFMA rounds once.  With any kept term left out at least 72 % of the
      elements exceed 8 units (tests/test_exact_cases_cpu.py holds the bound to "more than half" for each of the six).
      On the MI355X the kernels reach 3.3 to 3.7 units and 31.6 % of the elements differ from fl(ab), against 2.5 units
      and 4 to 24 % in the emulation: the inner arithmetic of v_mfma_f32_16x16x32_bf16 is neither of the two
      emulations (nor truncation per term or per MFMA, which give 50 % and 86 %).  The bound is the derivation's, not
      that figure's.
      With start values and a bias the 3u term above is added.
  split-bf16 product, grid:  the bits of numpy's float32 product.  A multiple of 1/8 in [-1, 1) has at most 4 significand
      bits: plane 0 holds it, planes 1 and 2 are zero, and every sum is exact.
"""
import json
import math
import os

import numpy as np

from gemm_view_cases import GUARD, SENTINEL, _embed, _view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, U64 = 2.0 ** -24, 2.0 ** -53
SPLIT_UNITS = 8                     # the split-bf16 bound in units of 2^-24 |ab|
TERMS = ("a0b2", "a1b1", "a0b1", "a1b0", "a0b0", "a2b0")      # the kept terms in the kernel's order, two per MFMA


def unit(dtype):
    return U32 if np.dtype(dtype) == np.float32 else U64


# ---- operand generators --------------------------------------------------------------------------------------------------
def values(shape, rng, dtype=np.float32):
    """+-[1, 2) with a random significand of 24 (53) bits whose last bit is set."""
    bits = 23 if np.dtype(dtype) == np.float32 else 52
    m = rng.integers(0, 1 << (bits - 1), size=shape, dtype=np.int64) * 2 + 1
    sign = rng.integers(0, 2, size=shape) * 2 - 1
    return (sign * (1.0 + m * 2.0 ** -bits)).astype(dtype)       # exact in float64, and in float32 for 23 bits


def _positions(n, K, rng):
    """k(i) = (i * p + c) % K with p odd and coprime to K: consecutive i hit different k, and n >= K covers every k."""
    p = 2 * int(rng.integers(0, max(K, 2))) + 1
    while math.gcd(p, K) != 1:
        p += 2
    c = int(rng.integers(0, K))
    return (np.arange(n, dtype=np.int64) * p + c) % K


def monomial_rows(M, K, rng, dtype=np.float32):
    """op(A), M x K, with one nonzero per row -> (op(A), k, a): op(A)[i, k[i]] = a[i]."""
    k, a = _positions(M, K, rng), values(M, rng, dtype)
    op = np.zeros((M, K), dtype=dtype)
    op[np.arange(M), k] = a
    return op, k, a


def monomial_cols(K, N, rng, dtype=np.float32):
    """op(B), K x N, with one nonzero per column -> (op(B), k, b): op(B)[k[j], j] = b[j]."""
    k, b = _positions(N, K, rng), values(N, rng, dtype)
    op = np.zeros((K, N), dtype=dtype)
    op[k, np.arange(N)] = b
    return op, k, b


def grid(shape, rng, dtype=np.float32):
    """Multiples of 1/8 in [-1, 1), as range_cases._grid draws them for the convolutions."""
    return (rng.integers(-8, 8, size=shape) / 8.0).astype(dtype)


GRID_MAX_K = 1 << 17


# ---- references ----------------------------------------------------------------------------------------------------------
def rows_factors(k, a, opb):
    """The two factors of every element of C for monomial_rows: a[i] and op(B)[k[i], j], broadcast to M x N."""
    return a[:, None], opb[k, :]


def cols_factors(opa, k, b):
    return opa[:, k], b[None, :]


def exact_product(x, y):
    """float32 factors: the exact product, in float64 (48 bits).  float64 factors: numpy.longdouble, whose 64 bits hold
    the 106-bit product to 2^-64 — for bounds only; the bits come from rounded_product."""
    if x.dtype == np.float32:
        return x.astype(np.float64) * y.astype(np.float64)
    return x.astype(np.longdouble) * y.astype(np.longdouble)


def rounded_product(x, y):
    """fl(xy), the product rounded once to the factors' type: a gather and one multiplication.  For float32 the exact
    float64 product is rounded by the cast; for float64 it is IEEE multiplication itself
    (tests/test_exact_cases_cpu.py checks it against Python fractions)."""
    if x.dtype == np.float32:
        return exact_product(x, y).astype(np.float32)
    return x * y


def grid_reference(opa, opb):
    """numpy's own product in the operands' type: exact for grid operands up to K = 2^17.  A sum that is zero is +0, as
    every chain that starts from +0 leaves it, whatever sign numpy's own order of summation gives it."""
    assert opa.shape[1] <= GRID_MAX_K and opa.dtype == opb.dtype
    return (opa @ opb) + opa.dtype.type(0)


def epilogue_bound(old, ab, bias, dtype):
    wide = np.float64 if np.dtype(dtype) == np.float32 else np.longdouble
    return 3 * unit(dtype) * (np.abs(old).astype(wide) + np.abs(ab) + np.abs(bias).astype(wide))


def epilogue_in_order(old, fl_ab, bias):
    """fl(fl(old + fl(ab)) + bias) in the operands' type: the order the second passes' headers state."""
    return (old + fl_ab) + bias


def split_bound(ab):
    return SPLIT_UNITS * U32 * np.abs(ab)


# ---- the split-bf16 product's arithmetic in numpy ------------------------------------------------------------------------
def bf16_round(x):
    """float32 -> the nearest value with 8 significand bits (ties to even), as float32: on the uint32 view."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def split3(x):
    """split_elem of kernels/gemm_split_pass.hip: x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1), as float32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    x0 = bf16_round(x)
    r1 = x - x0
    x1 = bf16_round(r1)
    x2 = bf16_round(r1 - x1)
    return x0, x1, x2


def six_term_product(a, b, drop=None, wide=False):
    """One element of the split product whose only nonzero products are those of a and b: the six kept terms onto one
    float32 accumulator that starts at zero, in the order of kernels/gemm_split_bf16.hip's `multiply` — the MFMAs
    (a0b2 + a1b1), (a0b1 + a1b0), (a0b0 + a2b0).  Every bf16 x bf16 product is exact (16 bits) and float64 holds the
    accumulator plus two of them exactly, so a cast is one rounding: after every term, or with wide=True once per MFMA
    (the instruction's inner rounding is not documented; the bound must hold either way).  drop: one of TERMS, left out."""
    assert drop is None or drop in TERMS
    pa, pb = split3(a), split3(b)
    acc = np.zeros(np.broadcast(pa[0], pb[0]).shape, dtype=np.float32)
    for pair in (TERMS[0:2], TERMS[2:4], TERMS[4:6]):
        s = acc.astype(np.float64)
        for t in pair:
            if t == drop:
                continue
            s = s + pa[int(t[1])].astype(np.float64) * pb[int(t[3])].astype(np.float64)
            if not wide:
                s = s.astype(np.float32).astype(np.float64)
        acc = s.astype(np.float32)
    return acc


def units_off(got, ab):
    """|got - ab| in units of 2^-24 |ab|, elementwise."""
    return np.abs(got.astype(np.float64) - ab) / (U32 * np.abs(ab))


# ---- one call on guarded views -------------------------------------------------------------------------------------------
class Call:
    """One eg_sgemm / eg_dgemm call: op(A) (M x K) and op(B) (K x N) stored in the layout asked for, inside guarded
    allocations as gemm_view_cases._embed lays them out — NaN in everything of A, B and the bias that is no operand
    element, SENTINEL around C's M x N interior, NaN inside it unless the call accumulates."""

    def __init__(self, opa, opb, ta=False, tb=False, lda=None, ldb=None, ldc=None, off=(0, 0, 0), start=None, bias=None, off_bias=0):
        self.dtype = opa.dtype
        M, K = opa.shape
        N = opb.shape[1]
        assert opb.shape[0] == K and opb.dtype == self.dtype
        self.dims, self.ta, self.tb = (M, N, K), ta, tb
        a, b = (opa.T if ta else opa), (opb.T if tb else opb)
        self.lda, self.ldb, self.ldc = lda or a.shape[1], ldb or b.shape[1], ldc or N
        assert self.lda >= a.shape[1] and self.ldb >= b.shape[1] and self.ldc >= N
        self.off_a, self.off_b, self.off_c = off
        self.off_bias, self.accumulate = off_bias, start is not None
        nan = self.dtype.type(np.nan)
        self.a, self.b = _embed(a, self.lda, self.off_a, nan), _embed(b, self.ldb, self.off_b, nan)
        self.c0 = _embed(start if self.accumulate else np.full((M, N), nan, dtype=self.dtype), self.ldc, self.off_c, self.dtype.type(SENTINEL))
        self.bias = _embed(bias[None, :], N, off_bias, nan) if bias is not None else None

    def starts(self):
        """Element offsets of the pointers that are passed: A, B, C, bias."""
        return GUARD + self.off_a, GUARD + self.off_b, GUARD + self.off_c, GUARD + self.off_bias

    def interior(self, got):
        M, N, _ = self.dims
        return _view(got, GUARD + self.off_c, M, N, self.ldc)

    def check_outside(self, got):
        """Every element of the C allocation outside the M x N interior has the bits that were uploaded."""
        M, N, _ = self.dims
        assert got.shape == self.c0.shape and got.dtype == self.dtype
        outside = np.ones(self.c0.shape, dtype=bool)
        _view(outside, GUARD + self.off_c, M, N, self.ldc)[...] = False
        bits = np.uint32 if self.dtype == np.float32 else np.uint64
        changed = np.flatnonzero((got.view(bits) != self.c0.view(bits)) & outside)
        assert changed.size == 0, "%d elements of C outside the %d x %d view were written; the first is element %d of the allocation, now %r" % (
            changed.size, M, N, changed[0], got[changed[0]])


def same_bits(got, want, what):
    """got and want hold the same bits everywhere: compared whole, and the first difference named."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bits = np.uint32 if got.dtype == np.float32 else np.uint64
    bad = np.argwhere(got.view(bits) != want.view(bits))
    assert bad.size == 0, "%s: %d of %d elements differ from the exact value; the first is %s: got %r, want %r" % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def within(got, want, limit, what):
    """|got - want| <= limit elementwise (want and limit in a wider type); returns the largest ratio."""
    assert np.isfinite(got).all(), "%s: NaN or Inf in the result" % what
    ratio = np.abs(got.astype(want.dtype) - want) / limit
    worst = float(ratio.max())
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert worst <= 1.0, "%s: off by %.3g of the bound at %s: got %r, want %r" % (what, worst, at, got[at], want[at])
    return worst


# ---- the table of eg_sgemm's exact routes --------------------------------------------------------------------------------
# A planner switch in the words of tests/gemm_plan_driver.cpp -> the environment variable gemm_f32_mfma.hip reads it from
SWITCH_ENV = {
    "no_small": "EG_NO_SMALL_GEMM", "no_skinny": "EG_NO_SKINNY_GEMM", "no_pair": "EG_GEMM_NO_PAIR", "no_t96": "EG_GEMM_NO_T96",
    "no_streamk": "EG_GEMM_NO_STREAMK", "no_xrow": "EG_GEMM_NO_XROW", "no_bk32": "EG_GEMM_NO_BK32", "no_wide_store": "EG_GEMM_NO_WIDE_STORE",
    "no_skew": "EG_GEMM_NO_SKEW", "old_tile_model": "EG_GEMM_OLD_TILE_MODEL", "small_bk32": "EG_GEMM_SMALL_BK32",
    "force_tile": "EG_GEMM_FORCE_TILE", "force_splits": "EG_GEMM_FORCE_SPLITS", "streamk_blocks": "EG_STREAMK_BLOCKS_PER_CU",
    "streamk_min_ratio": "EG_STREAMK_MIN_RATIO",
}


def switch_env(switches):
    """'no_pair,force_tile=64x64' -> {'EG_GEMM_NO_PAIR': '1', 'EG_GEMM_FORCE_TILE': '64,64'}."""
    env = {}
    for item in switches.split(","):
        if item == "-":
            continue
        name, _, value = item.partition("=")
        env[SWITCH_ENV[name]] = value.replace("x", ",") if value else "1"
    return env


def route_rows():
    """The rows of tests/golden/gemm_routes.json that eg_sgemm can reach (mode `exact`).  tests/test_gemm_plan_cpu.py holds
    the fixture to the planner on 256 CUs, so the route of each is known without a GPU."""
    with open(os.path.join(ROOT, "tests", "golden", "gemm_routes.json")) as f:
        return [c for c in json.load(f)["cases"] if c["mode"] == "exact"]


def route_id(c):
    e = c["expect"]
    return "%s-%s-%dx%dx%d-%s%s" % (e["route"], e.get("second", "none"), c["M"], c["N"], c["K"], "NT"[c["ta"]], "NT"[c["tb"]])


def sgemm_table():
    """For every (route, second pass) of the fixture the row with the smallest M * N * K (the first of equals), with its
    switches, leading dimensions and alignments.  Routes without a second-pass field (small, skinny, remainder) count as
    `none`; `tail_reduce` is the pass behind tail tiles."""
    best = {}
    for c in route_rows():
        key = (c["expect"]["route"], c["expect"].get("second", "none"))
        if key not in best or c["M"] * c["N"] * c["K"] < best[key]["M"] * best[key]["N"] * best[key]["K"]:
            best[key] = c
    return [best[k] for k in sorted(best)]


def sgemm_call(row, opa, opb, start=None, bias=None):
    """The fixture row's call on these operands: its layout, leading dimensions and base alignments (1: 16-byte aligned, 2:
    one float off)."""
    off = tuple(0 if row[x] == 1 else 1 for x in "abc")
    return Call(opa, opb, bool(row["ta"]), bool(row["tb"]), row["lda"], row["ldb"], row["ldc"], off, start, bias, off_bias=int(row["bias"] == 2))


def dgemm_table():
    """The float64 planner's fixture (tests/golden/dgemm_routes.json, held to plan_dgemm by tests/test_dgemm_plan_cpu.py) on
    256 CUs: for every (tile config, sliced or not, XCD remap, 16-byte loads) it holds, the row with the smallest M * N * K
    among those with every extent above 1.  A row's `tile` is EG_DGEMM_TILE's text ('-': unset)."""
    with open(os.path.join(ROOT, "tests", "golden", "dgemm_routes.json")) as f:
        rows = [c for c in json.load(f)["cases"] if c["cus"] == 256 and min(c["M"], c["N"], c["K"]) >= 2]
    best = {}
    for c in rows:
        e = c["expect"]
        key = (e["config"], e["splits"] > 1, e["remap"], e["vec"])
        if key not in best or c["M"] * c["N"] * c["K"] < best[key]["M"] * best[key]["N"] * best[key]["K"]:
            best[key] = c
    return [best[k] for k in sorted(best)]


def dgemm_id(c):
    e = c["expect"]
    return "tile%d-%s-%s-%dx%dx%d" % (e["config"], "sliced" if e["splits"] > 1 else "whole", "remap" if e["remap"] else "plain", c["M"], c["N"], c["K"])


def dgemm_call(row, opa, opb, start=None, bias=None):
    """The row's call, NN (the fixture's lda >= K and ldb >= N are NN's; the plan does not depend on the layout); a / b: 1 =
    16-byte aligned base, otherwise one double off."""
    return Call(opa, opb, False, False, row["lda"], row["ldb"], None, (int(row["a"] != 1), int(row["b"] != 1), 0), start, bias)


# ---- batched calls -------------------------------------------------------------------------------------------------------
class Batch:
    """batch0 x batch1 products of one shape in strided buffers (eg_sgemm_batched2's addressing; batch0 = 1 with stride 0 is
    eg_sgemm_batched's and eg_dgemm_batched's).  A layout is (ld, stride0, stride1) in elements, as tests/batched2_cases.py
    builds them; a stride of 0 shares the operand along that index.  A and B are NaN wherever no item lies, C holds
    SENTINEL there and NaN inside the items, and `tail` more sentinels behind the last one."""

    def __init__(self, b0, b1, M, N, K, ta, tb, a_lay, b_lay, c_lay, offset=0, dtype=np.float32, tail=8):
        self.dims, self.ta, self.tb, self.offset, self.dtype = (b0, b1, M, N, K), ta, tb, offset, np.dtype(dtype)
        self.a_lay, self.b_lay, self.c_lay = a_lay, b_lay, c_lay
        self.ra, self.ca = (K, M) if ta else (M, K)
        self.rb, self.cb = (N, K) if tb else (K, N)
        size = lambda rows, cols, lay: offset + (b0 - 1) * lay[1] + (b1 - 1) * lay[2] + (rows - 1) * lay[0] + cols
        self.a = np.full(size(self.ra, self.ca, a_lay), np.nan, dtype=dtype)
        self.b = np.full(size(self.rb, self.cb, b_lay), np.nan, dtype=dtype)
        self.c0 = np.full(size(M, N, c_lay) + tail, SENTINEL, dtype=dtype)
        self.want = {}

    def items(self):
        return [(o, i) for o in range(self.dims[0]) for i in range(self.dims[1])]

    def _item(self, buf, lay, o, i, rows, cols):
        return _view(buf, self.offset + o * lay[1] + i * lay[2], rows, cols, lay[0])

    def c_item(self, buf, o, i):
        return self._item(buf, self.c_lay, o, i, self.dims[2], self.dims[3])

    def fill(self, make):
        """make(o, i) -> (op(A), op(B), want) for every item.  Items that share an operand (a stride of 0) must get the
        same values for it: `make` is handed the item it shares with through Batch.source."""
        for o, i in self.items():
            opa, opb, want = make(o, i)
            self._item(self.a, self.a_lay, o, i, self.ra, self.ca)[...] = opa.T if self.ta else opa
            self._item(self.b, self.b_lay, o, i, self.rb, self.cb)[...] = opb.T if self.tb else opb
            self.c_item(self.c0, o, i)[...] = np.nan
            self.want[o, i] = want
        return self

    def source(self, lay, o, i):
        """The first item whose operand with layout `lay` is the one item (o, i) reads."""
        return (o if lay[1] else 0, i if lay[2] else 0)

    def check(self, got, what):
        expect = self.c0.copy()
        for o, i in self.items():
            same_bits(self.c_item(got, o, i), self.want[o, i], "%s item (%d, %d)" % (what, o, i))
            self.c_item(expect, o, i)[...] = self.want[o, i]
        same_bits(got, expect, what + ": outside the items of C")


def fill_batch(batch, kind, seed):
    """kind: `rows`, `cols` (monomial) or `grid`.  Operands are drawn per item, a shared one once."""
    b0, b1, M, N, K = batch.dims
    rng = np.random.default_rng(seed)
    dt = batch.dtype
    drawn_a, drawn_b = {}, {}

    def draw_a():
        return monomial_rows(M, K, rng, dt) if kind == "rows" else ((grid if kind == "grid" else values)((M, K), rng, dt),)

    def draw_b():
        return monomial_cols(K, N, rng, dt) if kind == "cols" else ((grid if kind == "grid" else values)((K, N), rng, dt),)

    def make(o, i):
        sa, sb = batch.source(batch.a_lay, o, i), batch.source(batch.b_lay, o, i)
        if sa not in drawn_a:
            drawn_a[sa] = draw_a()
        if sb not in drawn_b:
            drawn_b[sb] = draw_b()
        a, b = drawn_a[sa], drawn_b[sb]
        if kind == "rows":
            want = rounded_product(*rows_factors(a[1], a[2], b[0]))
        elif kind == "cols":
            want = rounded_product(*cols_factors(a[0], b[1], b[2]))
        else:
            want = grid_reference(a[0], b[0])
        return a[0], b[0], want

    return batch.fill(make)
