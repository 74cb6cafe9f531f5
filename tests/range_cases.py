"""The cases of tests/test_gpu_library_ranges.py (every group-2 library entry except the contractions, called on ranges inside
larger allocations) and of tests/test_range_cases_cpu.py (which holds this file to the oracle).  No GPU, no HIP.

A RangeCase is one library call with its host buffers.  include/exprgrad_hip.h promises "any base pointer", and every
entry picks a kernel, or a branch inside it, from the low four bits of its pointers.  So every operand lives in an
allocation of its own:

    [ GUARD | gap of `off` elements | the operand, tight | GUARD ]

and the pointer that is passed is the one behind the gap.  GUARD is a multiple of 4 elements, so the alignment of a pointer
is that of its offset (f32: 0 aligned, 1 .. 3 not; f64: 0 aligned, 1 not).  A read-only operand is NaN everywhere outside
the operand: an element read from there reaches the result.  A written operand holds SENTINEL outside the result, and
inside NaN when the call overwrites (a kernel that reads what it must only write shows) or start values when it
accumulates; eg_axpy's y and an accumulating eg_bias_add's out are read-write like every accumulate=True target.  GUARD
elements on either side make an over-read or a stray store a wrong number in the allocation, not a fault.

References are float64 numpy, written plainly from the formulas of include/exprgrad_hip.h (enum eg_map_op) and the
closed-form derivatives; tests/test_range_cases_cpu.py compares them with oracle/refcpu.c.  Values depend on the call's
shape only, never on the offsets or on accumulate: the same shape at another alignment is the same problem.

Bounds (the project's own or derived; none measured on the kernels):
    rel      rel_err(got, want) <= TOL: maps, bias add, axpy, convolutions (conftest.TOL, relative to max|want|)
    sum      max|got - want| <= TOL * (max over outputs of sum|x|) + TOL * max|start| when accumulating: f32 reductions
             (test_bias_colsum_rowsum's normalisation)
    f64sum   |got - want| <= rows * 2**-53 * (sum|x| + |start|) elementwise: the textbook bound of any order of a sum
    exact    fills

The route of a column sum (reduce.hip: colsum_with_scratch) is restated in colsum_route() for 256 compute units, and the
table COLSUM_ROUTES says by hand where every case ends; the CPU test holds one to the other.
"""
import functools
import zlib

import numpy as np

from conftest import TOL, rel_err

GUARD = 1024                 # elements; a multiple of 4 (and of 2 doubles): pointer alignment = offset alignment
SENTINEL = -777.25

MAPS = [("identity", 0.0), ("relu", 0.0), ("leaky_relu", 0.01), ("sigmoid", 0.0), ("tanh", 0.0),
        ("scale", 2.5), ("sin", 0.0), ("xor_leaky", 0.1), ("exp", 0.0)]
MAP_PARAM = dict(MAPS)
FEW_MAPS = ["relu", "tanh", "xor_leaky"]       # one select, one transcendental, one with a parameter


def aligned(off, dtype=np.float32):
    return (off * np.dtype(dtype).itemsize) % 16 == 0


def embed(vals, off, fill):
    """The flat allocation [GUARD | off | vals | GUARD] with `fill` everywhere outside vals."""
    vals = np.ascontiguousarray(vals).reshape(-1)
    buf = np.full(GUARD + off + vals.size + GUARD, fill, dtype=vals.dtype)
    buf[GUARD + off:GUARD + off + vals.size] = vals
    return buf


# ---- float64 references ------------------------------------------------------------------------------------------------------
def map_forward(op, x, p):
    x = np.asarray(x, np.float64)
    if op == "identity":
        return x.copy()
    if op == "relu":
        return np.where(x >= 0, x, 0.0)
    if op == "leaky_relu":
        return np.where(x >= 0, 1.0, p) * x
    if op == "sigmoid":
        return 1.0 / (1.0 + np.exp(-x))
    if op == "tanh":                                 # the naive quotient (dnn.nim:35-40)
        return (np.exp(x) - np.exp(-x)) / (np.exp(x) + np.exp(-x))
    if op == "scale":
        return x * p
    if op == "sin":
        return np.sin(x)
    if op == "xor_leaky":
        return np.where(x <= 0, p * x, x)
    if op == "exp":
        return np.exp(x)
    raise KeyError(op)


def map_backward(op, x, g, p):
    """d out / d x * g in closed form."""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    if op == "identity":
        return g.copy()
    if op == "relu":
        return np.where(x >= 0, g, 0.0)
    if op == "leaky_relu":
        return g * np.where(x >= 0, 1.0, p)
    if op == "sigmoid":
        s = 1.0 / (1.0 + np.exp(-x))
        return g * s * (1.0 - s)
    if op == "tanh":
        t = np.tanh(x)
        return g * (1.0 - t * t)
    if op == "scale":
        return g * p
    if op == "sin":
        return np.cos(x) * g
    if op == "xor_leaky":
        return np.where(x <= 0, g * p, g)
    if op == "exp":
        return g * np.exp(x)
    raise KeyError(op)


def conv2_forward(img, flt):
    img, flt = np.asarray(img, np.float64), np.asarray(flt, np.float64)
    F, FH, FW, C = flt.shape
    win = np.lib.stride_tricks.sliding_window_view(img, (FH, FW), axis=(1, 2))     # [N, Ho, Wo, C, FH, FW]
    return np.einsum("nyxcij,fijc->nyxf", win, flt, optimize=True)


def conv2_grad_filter(img, gout, flt_shape):
    from parity import exact_conv2_grad_filter
    return exact_conv2_grad_filter(img, gout, flt_shape)


def conv2_grad_image(flt, gout, img_shape):
    """Every output pixel scatters gout[n, y, x, :] @ flt[:, dy, dx, :] onto image pixel (y + dy, x + dx)."""
    flt, gout = np.asarray(flt, np.float64), np.asarray(gout, np.float64)
    F, FH, FW, C = flt.shape
    _, Ho, Wo, _ = gout.shape
    g = np.zeros(img_shape)
    for dy in range(FH):
        for dx in range(FW):
            g[:, dy:dy + Ho, dx:dx + Wo, :] += gout @ flt[:, dy, dx, :]
    return g


# ---- values: a function of the family and the shape only ---------------------------------------------------------------------
def _u(rng, shape, lo, hi, dtype=np.float32):
    return (lo + (hi - lo) * rng.random(shape)).astype(dtype)


def _grid(rng, shape, lo, hi):
    """Multiples of 1/8 in [lo/8, hi/8): products are multiples of 1/64, and a sum of 2^17 of them is exact in float32
    in any order."""
    return (rng.integers(lo, hi, size=shape) / 8.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _values(family, key):
    a = dict(key)
    rng = np.random.default_rng(zlib.crc32(repr((family, key)).encode()))
    if family in ("map", "map_grad"):
        # test_maps_and_their_gradients' ranges.  The gradient of tanh on a handful of elements draws x from U[-2, 2)
        # instead: the derived gradient of the naive quotient adds g / t and -d g / t^2, which cancel to eps * t / 2b
        # relative (1e-4 at |x| = 4) in the oracle's float32 as well, and with n = 1 there is no larger element for that
        # error to be relative to (the CPU test had the oracle at 0.96 of the bound there)
        n = a["n"]
        r = 2 if (family, a["op"]) == ("map_grad", "tanh") and n <= 5 else 4
        v = {"in": _u(rng, n, -r, r), "gout": _u(rng, n, -0.5, 0.5), "start": _u(rng, n, 0, 1)}
    elif family == "axpy":
        v = {"x": _u(rng, a["n"], 0, 1), "start": _u(rng, a["n"], 0, 1)}
    elif family == "fill":
        v = {"start": _u(rng, a["n"], 0, 1, a["dtype"])}
    elif family == "bias_add":
        v = {"bias": _u(rng, a["cols"], 0, 1), "start": _u(rng, (a["rows"], a["cols"]), -0.5, 0.5)}
    elif family == "sum":
        v = {"in": _u(rng, a["n"], -0.5, 0.5), "start": _u(rng, 1, -0.5, 0.5)}
    elif family == "rowsum":
        v = {"in": _u(rng, (a["rows"], a["cols"]), -0.5, 0.5), "start": _u(rng, a["rows"], -0.5, 0.5)}
    elif family == "colsum":
        v = {"in": _u(rng, (a["rows"], a["cols"]), -0.5, 0.5), "start": _u(rng, a["cols"], -0.5, 0.5)}
    elif family == "colsum_f64":
        v = {"in": _u(rng, (a["rows"], a["cols"]), -0.5, 0.5, np.float64), "start": _u(rng, a["cols"], -0.5, 0.5, np.float64)}
    elif family in ("conv_fwd", "conv_gf", "conv_gi"):
        # one set of arrays per shape, shared by the three calls: the ranges of tests/test_gpu_conv_grad.py
        return _values("conv", tuple(sorted({"shape": a["shape"], "grid": a["grid"]}.items())))
    elif family == "conv":
        N, H, W, C, F, FH, FW = a["shape"]
        Ho, Wo = H - FH + 1, W - FW + 1
        if a["grid"]:
            v = {"img": _grid(rng, (N, H, W, C), 0, 8), "flt": _grid(rng, (F, FH, FW, C), -8, 8), "gout": _grid(rng, (N, Ho, Wo, F), -4, 4)}
        else:
            v = {"img": _u(rng, (N, H, W, C), 0, 1), "flt": _u(rng, (F, FH, FW, C), -1, 1), "gout": _u(rng, (N, Ho, Wo, F), -0.5, 0.5)}
        v["start_out"] = _u(rng, (N, Ho, Wo, F), 0, 1)
        v["start_gflt"] = _u(rng, (F, FH, FW, C), 0, 1)
        v["start_gimg"] = _u(rng, (N, H, W, C), 0, 1)
    else:
        raise KeyError(family)
    for arr in v.values():
        arr.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _reference(family, key):
    """(float64 result without start values, magnitude term of the bound or None); computed once per shape."""
    a, v = dict(key), _values(family, key)
    if family == "map":
        return map_forward(a["op"], v["in"], float(np.float32(a["param"]))), None
    if family == "map_grad":
        return map_backward(a["op"], v["in"], v["gout"], float(np.float32(a["param"]))), None
    if family == "axpy":
        return float(np.float32(a["alpha"])) * v["x"].astype(np.float64), None
    if family == "fill":
        return np.full(a["n"], np.dtype(a["dtype"]).type(a["value"]), dtype=np.float64), None
    if family == "bias_add":
        return np.broadcast_to(v["bias"].astype(np.float64), (a["rows"], a["cols"])).copy(), None
    x = v["in"].astype(np.float64) if "in" in v else None
    if family == "sum":
        return np.array([x.sum()]), np.array([np.abs(x).sum()])
    if family == "rowsum":
        return x.sum(axis=1), np.abs(x).sum(axis=1)
    if family in ("colsum", "colsum_f64"):
        return x.sum(axis=0), np.abs(x).sum(axis=0)
    if family == "conv_fwd":
        return conv2_forward(v["img"], v["flt"]), None
    if family == "conv_gf":
        return conv2_grad_filter(v["img"], v["gout"], v["flt"].shape), None
    if family == "conv_gi":
        return conv2_grad_image(v["flt"], v["gout"], v["img"].shape), None
    raise KeyError(family)


# family -> (read-only operands in call order, written operand, key of its start values, bound)
FAMILIES = {
    "map": (("in",), "out", "start", "rel"),
    "map_grad": (("in", "gout"), "gin", "start", "rel"),
    "axpy": (("x",), "y", "start", "rel"),
    "fill": ((), "out", "start", "exact"),
    "bias_add": (("bias",), "out", "start", "rel"),
    "sum": (("in",), "out", "start", "sum"),
    "rowsum": (("in",), "out", "start", "sum"),
    "colsum": (("in",), "out", "start", "sum"),
    "colsum_f64": (("in",), "out", "start", "f64sum"),
    "conv_fwd": (("img", "flt"), "out", "start_out", "rel"),
    "conv_gf": (("img", "gout"), "gflt", "start_gflt", "rel"),
    "conv_gi": (("flt", "gout"), "gimg", "start_gimg", "rel"),
}
ALWAYS_READ_WRITE = ("axpy",)          # y = y + alpha * x whatever `accumulate` says


class RangeCase:
    """One call: family, shape arguments, one element offset per pointer, overwrite or accumulate, switches."""

    def __init__(self, family, offs, accumulate=False, env=None, pattern="", **args):
        self.family, self.args, self.accumulate, self.pattern = family, args, bool(accumulate), pattern
        self.inputs, self.written, self._start_key, self.bound = FAMILIES[family]
        if family in ALWAYS_READ_WRITE:
            self.accumulate = True
        self.offs = dict(zip(self.inputs + (self.written,), offs))
        assert len(self.offs) == len(self.inputs) + 1 == len(offs), (family, offs)
        self.env = dict(env or {})
        self.dtype = np.dtype(args.get("dtype", np.float64 if family.endswith("f64") else np.float32))
        self.key = tuple(sorted(args.items()))
        shape = "x".join(str(s) for s in args["shape"]) if "shape" in args else "-".join(
            str(args[k]) for k in ("op", "rows", "cols", "n") if k in args)
        self.name = "%s-%s-%s-%s" % (family, shape, pattern or "o" + "".join(str(o) for o in offs), "acc" if self.accumulate else "ovw")
        if self.env:
            self.name += "-" + "+".join(k[3:].lower() for k in sorted(self.env))

    def __repr__(self):
        return self.name

    def is_aligned(self, operand):
        return aligned(self.offs[operand], self.dtype)

    # ---- host side -----------------------------------------------------------------------------------------------------
    def values(self):
        return _values(self.family, self.key)

    def start(self):
        """What the result range holds before the call: start values when the call accumulates, else NaN."""
        s = self.values()[self._start_key]
        return s if self.accumulate else np.full(s.shape, np.nan, dtype=self.dtype)

    def buffers(self):
        """{operand: whole host allocation}, inputs in call order and the written operand last."""
        nan = self.dtype.type(np.nan)
        out = {name: embed(self.values()[name], self.offs[name], nan) for name in self.inputs}
        out[self.written] = embed(self.start(), self.offs[self.written], self.dtype.type(SENTINEL))
        return out

    def first(self, operand):
        """Element index of the operand's first element in its allocation."""
        return GUARD + self.offs[operand]

    def want(self):
        w, _ = _reference(self.family, self.key)
        if self.accumulate:
            w = w + self.values()[self._start_key].astype(np.float64)
        return w

    def result_size(self):
        return self.values()[self._start_key].size

    def interior(self, got):
        lo = self.first(self.written)
        return got[lo:lo + self.result_size()].reshape(self.values()[self._start_key].shape)

    # ---- checks --------------------------------------------------------------------------------------------------------
    def _where(self, i):
        lo = self.first(self.written)
        if i < GUARD:
            return "front guard, %d elements in front of the range" % (lo - i)
        if i < lo:
            return "gap in front of the range, %d elements in front of it" % (lo - i)
        return "back guard, %d elements behind the end of the range" % (i - (lo + self.result_size()) + 1)

    def check_outside(self, got):
        """Every element of the written allocation outside the result is bit-identical to what was uploaded."""
        sent = embed(self.start(), self.offs[self.written], self.dtype.type(SENTINEL))
        assert got.shape == sent.shape and got.dtype == self.dtype, (self.name, got.shape, sent.shape, got.dtype)
        bits = np.uint32 if self.dtype == np.float32 else np.uint64
        lo = self.first(self.written)
        outside = np.ones(sent.shape, dtype=bool)
        outside[lo:lo + self.result_size()] = False
        changed = np.flatnonzero((got.view(bits) != sent.view(bits)) & outside)
        assert changed.size == 0, "%s: %d elements outside the result range of %s were written; the first is in the %s, now %r" % (
            self.name, changed.size, self.written, self._where(int(changed[0])), got[changed[0]])

    def check(self, got):
        """got: the WHOLE written allocation as read back.  Returns the error figure that was compared with the bound."""
        self.check_outside(got)
        g, want = self.interior(got), self.want()
        bad = np.argwhere(~np.isfinite(g) & np.isfinite(want))
        assert bad.size == 0, "%s: %d elements of %s are NaN or Inf where the reference is finite; the first is %s" % (
            self.name, len(bad), self.written, tuple(int(i) for i in bad[0]))
        diff = np.abs(g.astype(np.float64) - want)
        if self.bound == "rel":
            err, bound = rel_err(g, want, self.name), TOL
        elif self.bound == "sum":
            _, mags = _reference(self.family, self.key)
            limit = TOL * float(mags.max()) + (TOL * float(np.abs(self.values()[self._start_key]).max()) if self.accumulate else 0.0)
            err, bound = float(diff.max()) / max(limit, 1e-300) * TOL, TOL
        elif self.bound == "f64sum":
            _, mags = _reference(self.family, self.key)
            limit = self.args["rows"] * 2.0 ** -53 * (mags + (np.abs(self.values()[self._start_key]) if self.accumulate else 0.0))
            err, bound = float((diff / np.maximum(limit, 1e-300)).max()), 1.0
        else:
            err, bound = float(np.count_nonzero(g != want.astype(self.dtype))), 0.0
        print("%s: error %.3g of a bound of %.3g" % (self.name, err, bound))
        at = np.unravel_index(int(np.argmax(diff)), diff.shape)
        assert err <= bound, "%s: error %.3g exceeds %.3g; largest difference at %s: got %r, want %r" % (
            self.name, err, bound, tuple(int(i) for i in at), g[at], want[at])
        return err


# ==== elementwise =================================================================================================================
# elementwise.hip: the 16-byte chunked path needs every pointer aligned and n >= 4; anything else is the grid-stride scalar
# path.  4099 = one 1024-group chunk and a 3-element tail; 12289 = three blocks of the chunked launch and a tail; 70001 on
# the scalar path = 274 blocks.
LENGTHS = [1, 3, 4, 5, 1023, 4099, 12289, 70001]
MAP_PATTERNS = {"aligned": (0, 0), "all1": (1, 1), "in1": (1, 0), "out1": (0, 1)}
GRAD_PATTERNS = {"aligned": (0, 0, 0), "all1": (1, 1, 1), "in1": (1, 0, 0), "gin1": (0, 0, 1), "gout1": (0, 1, 0), "o123": (1, 2, 3)}
AXPY_PATTERNS = {"aligned": (0, 0), "all1": (1, 1), "x1": (1, 0), "y1": (0, 1)}


def _map_like(family, patterns, out_alone):
    cases = []
    for op, param in MAPS:
        for n in LENGTHS:
            for pat, offs in patterns.items():
                every_op = n in (4099, 70001) and pat in ("aligned", out_alone)
                if not every_op and op not in FEW_MAPS:
                    continue
                for acc in (False, True):
                    cases.append(RangeCase(family, offs, acc, pattern=pat, op=op, param=param, n=n))
    return cases


def map_cases():
    return _map_like("map", MAP_PATTERNS, "out1")


def map_grad_cases():
    return _map_like("map_grad", GRAD_PATTERNS, "gin1")


def axpy_cases():
    return [RangeCase("axpy", offs, pattern=pat, n=n, alpha=-0.1) for n in LENGTHS for pat, offs in AXPY_PATTERNS.items()]


def fill_cases():
    return [RangeCase("fill", (off,), n=n, value=1.5, dtype="float32") for n in LENGTHS for off in (0, 1, 2, 3)]


def fill_f64_cases():
    return [RangeCase("fill", (off,), n=n, value=-2.75, dtype="float64") for n in (1, 5, 1000, 70001) for off in (0, 1)]


# eg_fill_uniform / eg_fill_uniform_f64: one grid-stride form each, element i a function of (state, stream, i) alone
UNIFORM_LENGTHS = [1, 5, 1000, 70001]
UNIFORM_OFFSETS = (0, 1)
UNIFORM_RANGE = (-2.0, 3.0)


def uniform_cases(dtype):
    """The guarded output ranges of the uniform fills (a fill case supplies layout and guard check; the values are drawn)."""
    return {(n, off): RangeCase("fill", (off,), n=n, value=0.0, dtype=np.dtype(dtype).name) for n in UNIFORM_LENGTHS for off in UNIFORM_OFFSETS}


# eg_bias_add: the chunked path needs cols % 4 == 0 and both pointers aligned
BIAS_SHAPES = [(1, 4), (37, 8), (300, 132), (64, 33), (1025, 16)]
BIAS_PATTERNS = {"aligned": (0, 0), "bias1": (1, 0), "out2": (0, 2)}


def bias_cases():
    return [RangeCase("bias_add", offs, acc, pattern=pat, rows=r, cols=c)
            for r, c in BIAS_SHAPES for pat, offs in BIAS_PATTERNS.items() for acc in (False, True)]


def elementwise_vector_path(c):
    """Whether elementwise.hip takes the 16-byte chunked path for this case."""
    every = all(c.is_aligned(o) for o in c.offs)
    if c.family == "bias_add":
        return every and c.args["cols"] % 4 == 0
    return every and c.args["n"] >= 4


# ==== reductions ==================================================================================================================
SUM_LENGTHS = [1, 3, 4, 7, 1027, 70001]            # eg_sum: the vector form needs n >= 4 and an aligned input


def sum_cases():
    return [RangeCase("sum", (i, o), acc, n=n) for n in SUM_LENGTHS for i in (0, 1) for o in (0, 1) for acc in (False, True)]


# eg_rowsum: which kernel takes the aligned call / the call with `in` one float off
ROWSUM_SHAPES = {
    (5, 1): ("thread", "thread"),
    (1000, 32): ("thread", "thread"),             # cols <= 32: the edge of one thread per row
    (70, 36): ("vec", "wave"),                    # the same matrix must take the scalar wave kernel off alignment
    (70, 37): ("wave", "wave"),                   # cols % 4
    (3, 260): ("vec", "wave"),                    # a row longer than one pass of 64 lanes x 4
    (1030, 64): ("vec", "wave"),
}
REDUCE_PATTERNS = {"aligned": (0, 0), "in1": (1, 0), "out1": (0, 1)}


def rowsum_route(rows, cols, in_aligned):
    if cols <= 32:
        return "thread"
    return "vec" if cols % 4 == 0 and in_aligned else "wave"


def rowsum_cases():
    return [RangeCase("rowsum", offs, acc, pattern=pat, rows=r, cols=c)
            for r, c in ROWSUM_SHAPES for pat, offs in REDUCE_PATTERNS.items() for acc in (False, True)]


# eg_colsum on 256 compute units, "first pass + second pass (partials)".  First pass: vec (colsum_vec_kernel) needs
# cols % 4 == 0, rows >= 64 and an aligned input, else scalar (colsum_partial_kernel).  Second pass: slab (slab_sum_kernel)
# needs more than one partial, cols % 4 == 0 and an aligned output; else tree (one block per column) when cols <= 256 and
# there are more than 64 partials; else thread (one thread per column).  both1 is not one of the three patterns every
# shape must see, but the only way to the tree final behind a scalar first pass on a cols % 4 == 0 matrix.
COLSUM_PATTERNS = dict(REDUCE_PATTERNS, both1=(1, 1))
COLSUM_ROUTES = {
    (63, 8): {"aligned": "scalar+thread(1)", "in1": "scalar+thread(1)", "out1": "scalar+thread(1)", "both1": "scalar+thread(1)"},  # rows = 63: below the vector gate
    (64, 8): {"aligned": "vec+thread(1)", "in1": "scalar+thread(1)", "out1": "vec+thread(1)", "both1": "scalar+thread(1)"},
    (1000, 4): {"aligned": "vec+thread(1)", "in1": "scalar+slab(16)", "out1": "vec+thread(1)", "both1": "scalar+thread(16)"},
    (4096, 12): {"aligned": "vec+slab(13)", "in1": "scalar+slab(64)", "out1": "vec+thread(13)", "both1": "scalar+thread(64)"},
    (777, 512): {"aligned": "vec+slab(98)", "in1": "scalar+slab(13)", "out1": "vec+thread(98)", "both1": "scalar+thread(13)"},
    (300, 130): {"aligned": "scalar+thread(5)", "in1": "scalar+thread(5)", "out1": "scalar+thread(5)", "both1": "scalar+thread(5)"},
    (70000, 8): {"aligned": "vec+slab(137)", "in1": "scalar+slab(1015)", "out1": "vec+tree(137)", "both1": "scalar+tree(1015)"},
    (65536, 1): {"aligned": "scalar+tree(1024)", "in1": "scalar+tree(1024)", "out1": "scalar+tree(1024)", "both1": "scalar+tree(1024)"},
    (20000, 260): {"aligned": "vec+slab(1667)", "in1": "scalar+slab(205)", "out1": "vec+thread(1667)", "both1": "scalar+thread(205)"},
}


def colsum_route(rows, cols, in_aligned, out_aligned, cus=256, no_slab=False):
    """reduce.hip (colsum_vec, colsum_geometry, colsum_with_scratch) restated; the workspace is 16-byte aligned."""
    ceil = lambda a, b: (a + b - 1) // b
    vec = cols >= 4 and cols % 4 == 0 and rows >= 64 and in_aligned
    if vec:
        cg = min(cols // 4, 256)
        phases, col_tiles = 256 // cg, ceil(cols // 4, cg)
        nparts, trip = ceil(8 * cus, col_tiles), phases * 4
        rpb = max(ceil(ceil(rows, nparts), trip) * trip, trip)
        nparts = max(ceil(rows, rpb), 1)
    else:
        col_tiles = ceil(cols, 64)
        nparts = max(min(ceil(4 * cus, col_tiles), ceil(rows, 64)), 1)
        rpb = ceil(rows, nparts)
        nparts = max(ceil(rows, rpb), 1) if rpb > 0 else 1
    if nparts > 1 and not no_slab and cols % 4 == 0 and out_aligned:
        final = "slab"
    elif cols <= 256 and nparts > 64:
        final = "tree"
    else:
        final = "thread"
    return "%s+%s(%d)" % ("vec" if vec else "scalar", final, nparts)


def colsum_cases(patterns=COLSUM_PATTERNS, env=None):
    return [RangeCase("colsum", COLSUM_PATTERNS[pat], acc, env=env, pattern=pat, rows=r, cols=c)
            for r, c in COLSUM_ROUTES for pat in patterns for acc in (False, True)]


def colsum_no_slab_cases():
    """The aligned patterns again with the slab sum switched off (a child process that starts with the switch set runs them)."""
    return colsum_cases(("aligned",), {"EG_NO_SLAB_SUM": "1"})


# eg_colsum_f64 (gemm_f64_mfma.hip) has one form: a scalar first pass and one thread per column, whatever the alignment
COLSUM_F64_SHAPES = [s for s in COLSUM_ROUTES if s != (70000, 8)]


def colsum_f64_cases():
    return [RangeCase("colsum_f64", (i, o), acc, rows=r, cols=c)
            for r, c in COLSUM_F64_SHAPES for i in (0, 1) for o in (0, 1) for acc in (False, True)]


# (family, rows, cols, pattern): run twice, bit for bit.  One float32 case per second-pass form on each of the three shapes
# that have partials, the tree behind either first pass, and the float64 form.
TWICE = [("colsum", 777, 512, "aligned"), ("colsum", 777, 512, "out1"), ("colsum", 4096, 12, "aligned"), ("colsum", 4096, 12, "out1"),
         ("colsum", 20000, 260, "aligned"), ("colsum", 20000, 260, "out1"), ("colsum", 70000, 8, "out1"), ("colsum", 65536, 1, "aligned"),
         ("colsum_f64", 777, 512, "aligned"), ("colsum_f64", 4096, 12, "aligned"), ("colsum_f64", 20000, 260, "aligned")]


# ==== convolutions ================================================================================================================
# The dispatch of eg_conv2_nhwc, eg_conv2_nhwc_grad_filter and eg_conv2_nhwc_grad_image (kernels/gemm_f32_mfma.hip) and of the
# _try functions they ask in turn, read for 256 compute units.  Operands per call: forward (img, flt, out); filter gradient
# (img, gout, gflt); image gradient (flt, gout, gimg).
#
# Patterns:  aligned   everything 16-byte aligned
#            out1      the written operand alone one float off
#            a1, b1    the first / the second input alone one float off
#            o123      the three pointers 1, 2 and 3 floats off
CONV_PATTERNS = {"aligned": (0, 0, 0), "out1": (0, 0, 1), "a1": (1, 0, 0), "b1": (0, 1, 0), "o123": (1, 2, 3)}
CONV_CALLS = ("conv_fwd", "conv_gf", "conv_gi")
NO_TINY, NO_BAND = {"EG_CONV_NO_TINY": "1"}, {"EG_CONV_NO_BAND": "1"}


class ConvShape:
    def __init__(self, row, shape, env=None, grid=False, same_bits=(), note=""):
        self.row, self.shape, self.env, self.grid, self.same_bits, self.note = row, shape, dict(env or {}), grid, same_bits, note
        self.id = "x".join(str(s) for s in shape) + ("-" + "+".join(k[3:].lower() for k in sorted(self.env)) if self.env else "")

    def cases(self, call):
        return {(pat, acc): RangeCase(call, offs, acc, env=self.env, pattern=pat, shape=self.shape, grid=self.grid)
                for pat, offs in CONV_PATTERNS.items() for acc in (False, True)}


# same_bits: the calls whose "out1" pattern runs the kernel of the aligned pattern on the same loads in the same order and
# differs in the form of the stores only (or not at all): bit-identical results.
#
# Where every pattern of a call ends, by the dispatch code:
CONV_SHAPES = [
    # ---- tiny (conv2_tiny.hip): forward and image gradient have no alignment branch (one thread per output element,
    # scalar loads and stores): all five patterns run the tiny kernel.  The filter gradient folds its slabs with the slab
    # sum, which needs an aligned gflt and F * FH * FW * C % 4 == 0 (168 and 72 here): out1 and o123 -> tiny declines ->
    # too few pixels for band / direct -> the contraction (conv = 2) with scalar loads (C % 4) at a shape its own tests
    # reach only under EG_CONV_NO_TINY.
    ConvShape("tiny", (5, 9, 11, 3, 7, 2, 4), same_bits=("conv_fwd", "conv_gi")),
    ConvShape("tiny", (1, 3, 3, 2, 4, 3, 3), same_bits=("conv_fwd", "conv_gi")),
    # ---- band (conv2_band.cpp).  3 x 70 x 90 x 3 -> 5 is 2.4 M multiply-adds forward and 2.6 M for the image gradient:
    # below the tiny kernels' 6 Mi limit, so left alone those two calls are tiny ones; under EG_CONV_NO_TINY they reach the
    # band kernel, 5 (3) outputs per pixel: element-wise stores whatever the alignment.  Its filter gradient has 135
    # outputs (135 % 4: no slab sum anywhere): band first pass, 21 partial rows, eg::colsum_with_scratch scalar + thread.
    # 130 x 16 x 20 x 16 -> 16: forward and image gradient leave as 16-byte pieces through LDS when out / gimg is aligned
    # ("_w" kernels) and element by element otherwise (out1, o123); the inputs are staged element by element either way.
    # Filter gradient: 2304 outputs (more than the tiny kernel's 2048), band first pass with 130 partial rows; gflt aligned
    # -> slab sum, gflt off -> colsum_with_scratch vec first pass (the partials are aligned) + one thread per column.
    ConvShape("band", (3, 70, 90, 3, 5, 3, 3), env=NO_TINY, same_bits=("conv_fwd", "conv_gi")),
    ConvShape("band", (130, 16, 20, 16, 16, 3, 3), same_bits=("conv_fwd", "conv_gi")),
    # ---- direct (conv2_direct.cpp), values on a grid of 1/8: the filter gradient sums 147 456 terms, which the oracle's
    # sequential float32 loop cannot do within TOL on random values (tests/test_gpu_conv_grad.py excuses it there); on the
    # grid every order of the sum is exact.  64 x 50 x 50 x 3 -> 4 under EG_CONV_NO_BAND: forward = the per-pixel kernel,
    # 16-byte stores ("_v4") for an aligned out, element-wise for out1 / o123; loads are scalar always.  Filter gradient =
    # conv2_direct_grad_filter_try (72 partial rows of 108) + colsum_with_scratch: vec first pass, 2 partials, slab sum for
    # an aligned gflt, one thread per column otherwise.  Image gradient: F = 4 is no multiple of 16 -> the padded copy
    # (16-byte copies for an aligned gout, scalar for b1 / o123) -> eg_conv2_nhwc on 52 x 52 x 4 -> 3 -> the per-pixel
    # kernel with 3 outputs per pixel: element-wise stores whatever gimg's alignment.
    # 64 x 50 x 50 x 2 -> 20 without a switch (F > 16: no band): forward = the per-pixel kernel, "_v4" for an aligned
    # out.  Filter gradient: 360 outputs x 147 456 pixels is past tiny, F > 16 past band, 360 > 224 past direct -> the
    # contraction (conv = 2), scalar loads always (C % 4).  Image gradient: padded copy (F = 20: 16-byte copies for an
    # aligned gout) -> eg_conv2_nhwc on 52 x 52 x 20 -> 2 -> implicit GEMM with 16-byte loads (its operands are the
    # library's own aligned scratch); gimg's alignment picks the contraction's store form.
    ConvShape("direct", (64, 50, 50, 3, 4, 3, 3), env=NO_BAND, grid=True, same_bits=("conv_fwd", "conv_gi")),
    ConvShape("direct", (64, 50, 50, 2, 20, 3, 3), grid=True, same_bits=("conv_fwd",)),
    # ---- halo forward / image gradient (conv2_halo.hip).  conv2_halo_suits wants at least compute_units / 2 = 128 patches
    # of 8 x 32 pixels x 64 filters that are 70 % full.  The two shapes the halo tests of tests/test_gpu_conv_grad.py are
    # named after do not pass that on 256 compute units: 2 x 130 x 70 x 32 -> 64 has 96 patches forward and 102 for the
    # image gradient, 3 x 100 x 120 x 48 -> 48 fills 66 % and 68 % of its patches (48 of 64 filters).  Both therefore run
    # on the implicit GEMM forward (16-byte loads when img and flt are aligned, scalar for a1 / b1 / o123; C stores by
    # out's alignment), the contraction (conv = 2) for the filter gradient (128 x 68 and 99 x 118 output pixels fail the
    # filter-gradient halo's segment fill or its 3 x 3 test) and padded copy -> implicit GEMM for the image gradient.  They
    # stay in the table as large implicit-GEMM problems.  The two shapes behind them do reach the halo kernel:
    # 8 x 66 x 66 x 16 -> 64 forward = 128 full patches: halo with 16-byte stores through LDS for an aligned out
    # (overwrite), element-wise stores for out1; a1 / b1 / o123 -> the halo kernel declines -> implicit GEMM with scalar
    # loads on a 66 x 66 x 16 -> 64 image.  Its image gradient fills a quarter of the filter block: padded copy.
    # 8 x 64 x 64 x 64 -> 16 image gradient = halo kernel with virtual padding on gout (128 full patches), the flipped bank
    # in the library's aligned scratch, so flt's alignment (a1) changes nothing; gimg off (out1) -> the same kernel,
    # element-wise stores; gout off (b1, o123) -> no virtual padding: scalar padded copy -> eg_conv2_nhwc on 66 x 66 x 16
    # -> 64 -> the halo kernel on the copy.
    ConvShape("halo", (2, 130, 70, 32, 64, 3, 3)),
    ConvShape("halo", (3, 100, 120, 48, 48, 2, 3)),
    ConvShape("halo", (8, 66, 66, 16, 64, 3, 3), same_bits=("conv_fwd",)),
    ConvShape("halo", (8, 64, 64, 64, 16, 3, 3), same_bits=("conv_gi",)),
    # ---- filter-gradient halo (conv2_gradf_halo.hip): 3 x 3, C and F multiples of 32, img, gout and gflt all aligned
    # (2 and 10 pixel ranges, folded by the slab sum); out1 / a1 / b1 / o123 -> it declines -> the contraction (conv = 2),
    # 16-byte loads only when img and gout are both aligned (out1).  Forward and image gradient of these shapes have too few
    # patches for the halo kernel: implicit GEMM.
    ConvShape("gradf_halo", (1, 34, 34, 64, 64, 3, 3)),
    ConvShape("gradf_halo", (2, 40, 70, 32, 96, 3, 3)),
    # ---- implicit GEMM / contraction (gemm_f32_mfma.hip, conv = 1, 2): 16-byte loads need C % 4 == 0 (filter gradient: and
    # F % 4 == 0) and both inputs aligned; the second shape (C = 5) has scalar loads always and needs EG_CONV_NO_TINY to get
    # here.  The stores follow the planner (aligned16(C), ldc % 4), as in tests/test_gemm_view_plan_cpu.py.
    ConvShape("gemm", (2, 20, 20, 32, 64, 3, 3)),
    ConvShape("gemm", (2, 7, 9, 5, 6, 3, 2), env=NO_TINY),
    # ---- 1 x 1: the three calls are plain sgemm_exact products (NT, TN, NN) on the pointers as they come
    ConvShape("1x1", (3, 6, 6, 4, 8, 1, 1)),
]
# Branches named by the issue that no row reaches: conv2_direct.cpp's switch of its LOADS on aligned16(img) (vec_in) is in
# conv2_direct_f64_try, the float64 kernel of the model route; the float32 per-pixel kernel that group 2 reaches loads
# element by element whatever the alignment.  The band kernels likewise stage their inputs element by element.
