"""The cases of tests/test_gpu_gemm_views.py (eg_sgemm and eg_dgemm called on strided views) and of
tests/test_gemm_view_plan_cpu.py and tests/test_dgemm_view_plan_cpu.py (which routes of kernels/gemm_plan.cpp those cases reach).  No GPU, no HIP.

A ViewCase is one call with its host buffers.  The contract of include/exprgrad_hip.h is lda >= K, ldb >= N, ldc >= N and
any base pointer, so every buffer here is a view into a larger allocation:

    [ guard | gap of `off` elements | row 0 | padding | row 1 | padding | ... | last row | guard ]

The pointer that is passed is the one behind the gap; the last row has no padding behind it.  In A, B and the bias
everything that is not an operand element is NaN: an element read from there reaches the result.  In C everything outside
the M x N interior holds SENTINEL and must come back bit for bit; the interior starts as NaN unless the call accumulates,
so a kernel that reads C when it must only write it shows as well.  GUARD elements on either side make an over-read or a
stray store a wrong number in the allocation, not a fault.

Bounds (the project's own):
    f32  max|got - want| <= TOL * max(max|want|, 0.25 * sqrt(K) * 0.3)            (test_random_contraction_shapes)
    f64  |got - want| <= 4e-16 * sqrt(K) * (|opA| @ |opB| + |start| + |bias|) + 1e-300, elementwise  (test_dgemm_against_numpy)
against the float64 numpy product of the unpadded operands.
"""
import numpy as np

from conftest import TOL

GUARD = 1024                 # elements; a multiple of 4, so the alignment of a pointer is that of its offset
SENTINEL = -777.25
LAYOUTS = {"NN": (False, False), "NT": (False, True), "TN": (True, False), "TT": (True, True)}


def _view(buf, start, rows, cols, ld):
    return np.lib.stride_tricks.as_strided(buf[start:], shape=(rows, cols), strides=(ld * buf.itemsize, buf.itemsize))


def _embed(vals, ld, off, fill):
    rows, cols = vals.shape
    buf = np.full(GUARD + off + (rows - 1) * ld + cols + GUARD, fill, dtype=vals.dtype)
    _view(buf, GUARD + off, rows, cols, ld)[...] = vals
    return buf


class ViewCase:
    """One call to eg_sgemm (dtype float32) or eg_dgemm (float64): layout parameters, host buffers, expected result."""

    def __init__(self, name, dtype, M, N, K, ta=False, tb=False, pad=(0, 0, 0), off=(0, 0, 0), off_bias=0, accumulate=False,
                 bias=False, seed=0, env=None, switches="-", kind=""):
        self.name, self.dtype, self.dims, self.ta, self.tb = name, np.dtype(dtype), (M, N, K), ta, tb
        self.pad_a, self.pad_b, self.pad_c = pad
        self.off_a, self.off_b, self.off_c = off
        self.off_bias, self.accumulate, self.bias, self.seed = off_bias, accumulate, bias, seed
        self.env = dict(env or {})       # tuning aids the GPU test sets (EG_TUNING=1 is the suite's default) ...
        self.switches = switches         # ... and the same in the planner driver's words
        self.kind = kind                 # which of the layouts (a) .. (f) of the table
        self.ra, self.ca = (K, M) if ta else (M, K)
        self.rb, self.cb = (N, K) if tb else (K, N)
        self.lda, self.ldb, self.ldc = self.ca + self.pad_a, self.cb + self.pad_b, N + self.pad_c
        self._built = False

    # ---- the planner driver's line (tests/gemm_plan_driver.cpp): 1 = 16-byte aligned base, 2 = not ----
    def driver_line(self):
        assert self.dtype == np.float32
        al = lambda off: 1 if off % 4 == 0 else 2
        M, N, K = self.dims
        return "exact %d %d %d %d %d %d %d %d %d %d %d %d 0 %s" % (
            M, N, K, self.ta, self.tb, self.lda, self.ldb, self.ldc, al(self.off_a), al(self.off_b), al(self.off_c),
            (al(self.off_bias) if self.bias else 0), self.switches)

    # ---- the float64 planner driver's case (tests/test_dgemm_plan_cpu.py, dgemm_plans): offsets are in doubles ----
    def dgemm_driver_case(self, cus=256):
        assert self.dtype == np.float64
        M, N, K = self.dims
        return dict(M=M, N=N, K=K, lda=self.lda, ldb=self.ldb, a=int(self.off_a % 2 == 0), b=int(self.off_b % 2 == 0), cus=cus,
                    tile=self.env.get("EG_DGEMM_TILE", "-"))

    def tight(self):
        """The same call on the same values with tight leading dimensions and aligned bases."""
        return ViewCase(self.name + "-tight", self.dtype, *self.dims, ta=self.ta, tb=self.tb, accumulate=self.accumulate, bias=self.bias,
                        seed=self.seed, env=self.env, switches=self.switches, kind="tight")

    # ---- host buffers: the values depend on the shape, the flags and the seed only, never on the padding ----
    def build(self):
        if self._built:
            return self
        M, N, K = self.dims
        rng = np.random.default_rng(self.seed)
        u = lambda *shape: (rng.random(shape) - 0.5).astype(self.dtype)     # U[-0.5, 0.5)
        self.a_vals, self.b_vals = u(self.ra, self.ca), u(self.rb, self.cb)
        self.c_vals = u(M, N) if self.accumulate else None
        self.bias_vals = u(N) if self.bias else None
        nan = self.dtype.type(np.nan)
        self.a = _embed(self.a_vals, self.lda, self.off_a, nan)
        self.b = _embed(self.b_vals, self.ldb, self.off_b, nan)
        start = self.c_vals if self.accumulate else np.full((M, N), nan, dtype=self.dtype)
        self.c0 = _embed(start, self.ldc, self.off_c, self.dtype.type(SENTINEL))
        self.bias_buf = _embed(self.bias_vals[None, :], N, self.off_bias, nan) if self.bias else None
        self._built = True
        return self

    def release(self):
        """Drop the host buffers (the large cases hold a few hundred MB)."""
        for k in ("a_vals", "b_vals", "c_vals", "bias_vals", "a", "b", "c0", "bias_buf", "_want", "_mags"):
            self.__dict__.pop(k, None)
        self._built = False

    # element offsets of the pointers that are passed
    @property
    def a_start(self):
        return GUARD + self.off_a

    @property
    def b_start(self):
        return GUARD + self.off_b

    @property
    def c_start(self):
        return GUARD + self.off_c

    @property
    def bias_start(self):
        return GUARD + self.off_bias

    def want(self):
        """The float64 product of the unpadded operands, plus start values and bias; computed once."""
        if "_want" not in self.__dict__:
            self.build()
            opa = (self.a_vals.T if self.ta else self.a_vals).astype(np.float64)
            opb = (self.b_vals.T if self.tb else self.b_vals).astype(np.float64)
            w = opa @ opb
            if self.dtype == np.float64:
                mags = np.abs(opa) @ np.abs(opb)
            if self.accumulate:
                w = w + self.c_vals
                if self.dtype == np.float64:
                    mags = mags + np.abs(self.c_vals)
            if self.bias:
                w = w + self.bias_vals[None, :]
                if self.dtype == np.float64:
                    mags = mags + np.abs(self.bias_vals)[None, :]
            self._want = w
            self._mags = mags if self.dtype == np.float64 else None
        return self._want

    def interior(self, got):
        M, N, _ = self.dims
        return _view(got, self.c_start, M, N, self.ldc)

    def _where(self, i):
        M, N, _ = self.dims
        if i < GUARD:
            return "front guard, element %d" % i
        if i < self.c_start:
            return "gap in front of C"
        j = i - self.c_start
        if j >= (M - 1) * self.ldc + N:
            return "back guard, %d elements behind the last row" % (j - ((M - 1) * self.ldc + N))
        return "row %d, column %d (row padding, ldc = %d, N = %d)" % (j // self.ldc, j % self.ldc, self.ldc, N)

    def check_outside(self, got):
        """Every element of the C allocation outside the M x N interior is bit-identical to what was uploaded."""
        self.build()
        M, N, K = self.dims
        assert got.shape == self.c0.shape and got.dtype == self.dtype
        bits = np.uint32 if self.dtype == np.float32 else np.uint64
        outside = np.ones(self.c0.shape, dtype=bool)
        _view(outside, self.c_start, M, N, self.ldc)[...] = False
        changed = np.flatnonzero((got.view(bits) != self.c0.view(bits)) & outside)
        assert changed.size == 0, "%s: %d elements of C outside the %d x %d view were written; the first is %s, now %r" % (
            self.name, changed.size, M, N, self._where(int(changed[0])), got[changed[0]])

    def check(self, got):
        """got: the WHOLE C allocation as read back.  Returns the error figure that was compared with the bound."""
        self.check_outside(got)
        M, N, K = self.dims
        g = self.interior(got)
        bad = np.argwhere(~np.isfinite(g))
        assert bad.size == 0, "%s: %d elements of C are NaN or Inf; the first is (%d, %d)" % (self.name, len(bad), bad[0][0], bad[0][1])
        want = self.want()
        diff = np.abs(g.astype(np.float64) - want)
        if self.dtype == np.float32:
            scale = max(float(np.abs(want).max()), 0.25 * np.sqrt(K) * 0.3)
            err, bound = float(diff.max()) / scale, TOL
        else:   # elementwise: the figure is the largest ratio to the bound's own magnitude term
            limit = 4e-16 * np.sqrt(K) * self._mags + 1e-300
            err, bound = float((diff / limit).max()), 1.0
        print("%s: error %.3g of a bound of %.3g" % (self.name, err, bound))
        at = np.unravel_index(int(np.argmax(diff)), diff.shape)
        assert err <= bound, "%s: error %.3g exceeds %.3g; largest difference at (%d, %d): got %r, want %r" % (
            self.name, err, bound, at[0], at[1], g[at], want[at])
        return err


# ---- the float32 table ---------------------------------------------------------------------------------------------------
# kind -> (pad_a, pad_b, pad_c), (off_a, off_b, off_c), off_bias, bias, accumulate.  About half accumulate.
#   a   padded by 4, every base aligned: the plan of the tight call (tests/test_gemm_view_plan_cpu.py asserts it)
#   b   padded by 3: no 16-byte loads, no 16-byte stores
#   c   padded by 4, A, B and C one float off
#   d   padded by 4, C alone one float off: 16-byte loads with direct stores
#   e   padded by 4, A alone one float off: scalar loads, and 16-byte stores where the route has them
#   f   a bias, three different pads (a kernel that takes the wrong one of the three leading dimensions shows);
#   g   the bias one float off
F32_KINDS = {
    "a": ((4, 4, 4), (0, 0, 0), 0, False, False),
    "b": ((3, 3, 3), (0, 0, 0), 0, False, True),
    "c": ((4, 4, 4), (1, 1, 1), 0, False, False),
    "d": ((4, 4, 4), (0, 0, 1), 0, False, True),
    "e": ((4, 4, 4), (1, 0, 0), 0, False, False),
    "f": ((8, 4, 12), (0, 0, 0), 0, True, True),
    "g": ((4, 8, 12), (0, 0, 0), 1, True, False),
}
ALL_KINDS = "abcdefg"
BIG_KINDS = "abd"      # the 4100-class shapes and 4352 x 4100: the smallest that reach their routes on 256 CUs

# (route the tight and the (a) call take, M, N, K, {layout: kinds}, keyword arguments of every case of the shape).
# The first layout of a shape runs every kind, a further one (a), (b) and (c): the route does not depend on the layout
# except where noted, and every route that accepts them is seen in two layouts at least.
F32_SHAPES = [
    ("small", 33, 17, 40, {"NN": ALL_KINDS, "NT": "abc", "TN": "abc", "TT": "abc"}, {}),
    ("skinny", 4096, 10, 64, {"NN": ALL_KINDS}, {}),                                    # NN only
    ("kw8", 96, 96, 512, {"NN": ALL_KINDS, "TT": "abc"}, {}),                           # whole 32 x 32 tiles
    ("kw8", 300, 700, 900, {"NT": ALL_KINDS, "TN": "abc"}, {}),                         # ragged in M, N and K
    ("kw8", 1000, 24, 400, {"NN": ALL_KINDS, "TN": ALL_KINDS}, {}),
    ("t96", 1344, 1440, 512, {"NN": ALL_KINDS}, {}),
    ("t96", 1440, 1344, 512, {"TN": ALL_KINDS, "NT": "abc"}, {}),
    ("remainder", 4100, 4100, 128, {"NN": BIG_KINDS, "TT": "a"}, {}),                   # whole tiles + rows + columns
    ("remainder", 4104, 4096, 128, {"NT": BIG_KINDS + "e"}, {}),                        # whole tiles + rows
    ("extra_rows", 260, 256, 8192, {"TN": ALL_KINDS}, {}),                              # TN only; x_rows = 4, one tile row
    ("extra_rows", 784, 512, 8192, {"TN": ALL_KINDS}, {}),                              # x_rows = 16, 40 / 47 slices
    ("generic", 144, 128, 8192, {"TN": ALL_KINDS, "NN": "abc"}, {}),                    # split_reduce, fewer slices on the last tile row
    ("generic", 4352, 4100, 257, {"NT": BIG_KINDS, "TN": "a"}, {}),                     # tail_reduce; NT: scalar loads (K % 4), 16-byte stores
    ("pair", 1024, 1024, 256, {"NN": ALL_KINDS, "TT": "abc"}, {}),                      # 32-deep k-tiles
    ("pair", 1024, 960, 128, {"TN": ALL_KINDS, "NT": "abc"}, {}),                       # 16-deep
    ("generic", 2560, 2560, 256, {"NN": ALL_KINDS, "TN": "abc"}, {"bias": True}),       # whole tiles, 16-byte stores, a bias throughout
    # tight and without a bias these fold their slabs with the tree sum, which needs ldc == N; padded: split_reduce
    ("generic", 64, 200, 8192, {"NN": ALL_KINDS, "NT": "abc"}, {"tree_when_tight": True}),
    ("generic", 2, 4, 8192, {"TN": ALL_KINDS}, {"tree_when_tight": True}),
    ("generic", 4, 1, 8192, {"TN": ALL_KINDS}, {"tree_when_tight": True}),              # A alone takes 16-byte loads (vec = 41)
    # stream-K: the planner's balance model does not choose it at K = 512; test_stream_k_blocks_against_the_exact_product_
    # and_one_block_per_tile reaches it at this shape with EG_STREAMK_MIN_RATIO=0, and so do these cases
    ("streamk", 1792, 1792, 512, {"NT": ALL_KINDS, "TN": "abc"},
     {"env": {"EG_STREAMK_MIN_RATIO": "0"}, "switches": "streamk_min_ratio=0"}),
    # bk32: the planner returns it by default from 4096 x 4096 x 2048 on (the first shape with whole 256 x 256 tiles for
    # every CU); once at that size, and in every kind on a small output with the tile and the slice count forced, the way
    # tests/golden/gemm_routes.json reaches routes (force_tile / force_splits)
    ("bk32", 4096, 4096, 2048, {"NN": BIG_KINDS}, {}),
    ("bk32", 512, 512, 2048, {"TN": ALL_KINDS, "NT": "abc"},
     {"env": {"EG_GEMM_FORCE_TILE": "256,256", "EG_GEMM_FORCE_SPLITS": "1"}, "switches": "force_tile=256x256,force_splits=1"}),
]


def f32_table():
    """Every float32 case: ViewCase objects without their buffers (build() makes them)."""
    cases = []
    for n, (route, M, N, K, layouts, kw) in enumerate(F32_SHAPES):
        kw = dict(kw)
        always_bias, tree = kw.pop("bias", False), kw.pop("tree_when_tight", False)
        for lid, kinds in layouts.items():
            ta, tb = LAYOUTS[lid]
            for kind in kinds:
                pad, off, off_bias, bias, acc = F32_KINDS[kind]
                cases.append(ViewCase("%dx%dx%d-%s-%s" % (M, N, K, lid, kind), np.float32, M, N, K, ta, tb, pad, off, off_bias, acc,
                                      bias or always_bias, seed=100 * n + 10 * ta + tb, kind=kind, **kw))
                cases[-1].route = route
                cases[-1].tree_when_tight = tree and not cases[-1].bias
    return cases


# ---- the float64 table -----------------------------------------------------------------------------------------------------
# Left alone, plan_dgemm (kernels/gemm_plan.cpp) gives every shape here one tile and one slice count, so EG_DGEMM_TILE=
# <config>,<slices> (a measurement aid) takes the table through every tile (0: 128 x 128, 1: 128 x 64, 2: 64 x 64), unsliced
# and sliced; tests/test_dgemm_view_plan_cpu.py asserts through the planner that each case ends where its name says.
# 16-byte loads need even lda and ldb and aligned bases, whatever the extents: with pad 2 and an odd K or M the second
# double of a row's last pair is the NaN behind the row.
F64_SHAPES = [(65, 63, 17), (130, 70, 1027), (257, 129, 1000)]     # odd extents; K = 1027: four slices of at least 256
F64_KINDS = {
    "even": ((2, 2, 2), (0, 0, 0)),       # 16-byte loads
    "odd": ((1, 1, 1), (0, 0, 0)),        # 8-byte loads
    "ab_off": ((2, 2, 2), (1, 1, 0)),     # even leading dimensions, A and B one double off: 8-byte loads
    "c_off": ((2, 2, 2), (0, 0, 1)),
}
F64_EPILOGUES = [(False, False), (True, False), (False, True), (True, True)]     # (accumulate, bias)


def f64_table():
    cases = []
    for tile in (0, 1, 2):
        for slices in (1, 4):
            for s, (M, N, K) in enumerate(F64_SHAPES):
                for l, (lid, (ta, tb)) in enumerate(LAYOUTS.items()):
                    for k, (kind, (pad, off)) in enumerate(F64_KINDS.items()):
                        acc, bias = F64_EPILOGUES[(s + l + k + tile + slices) % 4]
                        cases.append(ViewCase("tile%d-slices%d-%dx%dx%d-%s-%s" % (tile, slices, M, N, K, lid, kind), np.float64, M, N, K, ta, tb,
                                              pad, off, off_bias=k % 2, accumulate=acc, bias=bias, seed=1000 * s + 10 * l + k,
                                              env={"EG_DGEMM_TILE": "%d,%d" % (tile, slices)}, kind=kind))
    # the default path: few tiles and a long K slice by themselves, and dgemm_reduce_kernel sees ldc != N
    cases.append(ViewCase("default-64x48x40000-NN", np.float64, 64, 48, 40000, pad=(0, 0, 2), accumulate=True, bias=True, seed=7, kind="default"))
    return cases
