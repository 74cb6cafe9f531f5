"""The case table of the generated-kernel emitter (csrc/host/codegen.cpp: generate_mode_a, generate_mode_b), route by route.

Every case names a program of the Python DSL mirror, one of its targets, the inputs, the route the plain launch list
(EG_NO_ROWFUSE=1 EG_NO_INLINE=1) must take for it — as words of the launch line, Model.launch_plan — and a float64 numpy
reference written as loops and slices from the statement itself.  The reference does not go through oracle/kd.py: kd.py and
csrc/host/kd.cpp restate the same rules and could share a misreading.  tests/test_generated_cases_cpu.py holds the oracle to
these references; tests/test_gpu_generated_routes.py the backend, with fusion off, with the 64-bit body forced, and with
default settings (where csrc/host/rowfuse_small.cpp emits many of the same kernels a second time).

Boundaries, read from csrc/host/plan.cpp as it stands:
    Vec4 (fill_params, Slot::Vec4; the slot exists only if generate_mode_a found the kernel eligible: float32, no reduction,
        no scatter, the fastest loop unbounded, every operand ending in the bare fastest iterator, no instruction using it):
        start 0, extent % 4 == 0, total % 4 == 0, every operand's last dimension % 4 == 0.  An unbounded loop takes its extent
        from the last dimension of an operand, and total is a multiple of that extent, so of the four only "a last dimension"
        can fail alone (MAP_LONG_B: b one element longer than the rows of a); the extent fails together with a last dimension
        (5 x 7, 6 x 6) and total with both (5 x 7).  The conditions of generate_mode_a fail alone: bounds, a value that uses
        the iterator, an operand that does not end in it (transposed read), float64.
    mode B: b_capable && !scatter && rtotal >= 2048 && total <= 8192 && total * 64 <= rtotal && full_cover;
        tx = the power of two at or above total, at most 64; ty = 256 / tx; chunks = min(ceil(4 * CUs / column tiles),
        ceil(rtotal / (8 * ty))), then chunk = ceil(rtotal / chunks) and chunks = ceil(rtotal / chunk).  On 256 compute units
        the second bound decides for every shape here, so a full chunk is 8 * ty terms or one or two more; at tx = 64 it is
        exactly 32 = 8 * ty for every rtotal >= 2048 (chunk = 32 - floor((32 - s) / (q + 1)) with rtotal = 32 q + s, q >= 64):
        there only the LAST chunk can be ragged.  `ragged` says what the GPU test asserts from the plan line's chunks=:
        "all" — last chunk shorter, and ty divides neither the full nor the last chunk's length; "last" — last chunk shorter
        and ty does not divide its length; None — the shape sits exactly on a gate and cannot be ragged.
    Narrow: off for a kernel that computes with Index values (INDEX_VALUES), on for every other case here.

Inputs: maps and reductions under 2048 terms take U[-0.5, 0.5) float32 values.  Reductions of 2048 terms or more take dyadic
values — multiples of 1/8 in [-2, 2] — under bodies of `*`, `+`, `-` and select only: products are multiples of 1/64 in
[-4, 4], every partial sum is below 8323 * 4 * 64 = 2.2e6 < 2^24 units of 1/64, so every order of summation is exact in float32
and backend, oracle and numpy must be EQUAL (`exact`).  SPLIT_EXP keeps an inexact body (exp of a bounded value, all terms
positive).
"""
import numpy as np

from exprgrad_amd import dsl
from exprgrad_amd.dsl import Fun, iters, select

FAMILIES = ("map", "shared", "displaced", "computed", "reduce", "split", "index")


def wrap(a, b):
    """wrap(a, b) = ((a mod b) + b) mod b (llvmgen.nim:227-230); the mirror has the instruction but no builder for it."""
    return dsl.Expr("instr", dsl.INDEX, instr="wrap", children=[dsl.literal(a), dsl.literal(b)])


def split_body(a, b):
    """The body of the dyadic reductions: select, -, * (exact on multiples of 1/8 in [-2, 2])."""
    return select(b < 0.0, a - b, a * b)


def np_split_body(a, b):
    return np.where(b < 0, a - b, a * b)


# ---- programs: one model each, several targets, so that a handful of hiprtc programs serve the whole table --------------------------------
def maps_program():
    y, x, z, it = iters("y x z it")
    a, b, c = dsl.input("a"), dsl.input("b"), dsl.input("c")
    out = []
    m = Fun()
    m[y, x] += a[y, x] * b[x] + a[y, x]
    m.copy_shape(a)
    out.append(m.target("map"))
    two = Fun()                                              # first writer stores, the second accumulates: old + res
    two[y, x] += a[y, x] * b[x]
    two[y, x] += a[y, x] - b[x]
    two.copy_shape(a)
    out.append(two.target("map_twice"))
    lo = Fun()
    xl = dsl.iter_in("x", 0, 4)
    lo[y, xl] += a[y, xl] * b[xl] + a[y, xl]
    lo.copy_shape(a)
    out.append(lo.target("map_low"))
    hi = Fun()
    xh = dsl.iter_in("x", 4, 8)
    hi[y, xh] += a[y, xh] * b[xh] + a[y, xh]
    hi.copy_shape(a)
    out.append(hi.target("map_high"))
    raw = Fun()
    raw.raw[it] += a.raw[it] * 2.0 - b.raw[it]
    raw.copy_shape(a)
    out.append(raw.target("map_raw"))
    three = Fun()
    three[z, y, x] += a[z, y, x] * b[y, x] + c[x]
    three.copy_shape(a)
    out.append(three.target("map_three"))
    pos = Fun()
    pos[y, x] += a[y, x] * dsl.to_scalar(x) + dsl.to_scalar(y)
    pos.copy_shape(a)
    out.append(pos.target("map_position"))
    tr = Fun()
    tr[y, x] += a[y, x] + b[x, y]
    tr.copy_shape(a)
    out.append(tr.target("map_transposed"))
    return out


def shared_program():
    n, y, x, c = iters("n y x c")
    a, b = dsl.input("a"), dsl.input("b")
    same = Fun()
    same[n, y, x, c] += a[n, y, x, c] * b[n, y, x, c]
    same.copy_shape(a)
    xb = dsl.iter_in("x", 0, 5)
    other = Fun()
    other[n, y, xb, c] += a[n, y, xb, c] * b[n, y, xb, c]
    other.copy_shape(a)
    return [same.target("shared"), other.target("shared_else")]


def displaced_program():
    img, flt = dsl.input("img"), dsl.input("flt")
    y, x = dsl.iter_in("y", 0, 7), dsl.iter_in("x", 0, 9)      # img is 9 x 11
    st = Fun()
    st[y, x] += img[y, x] + img[y + 1, x + 2] - img[y + 2, x]
    st.with_shape(7, 9)
    yn, xn = dsl.iter_in("y", 2, 9), dsl.iter_in("x", 2, 10)
    neg = Fun()
    neg[yn, xn] += img[yn, xn] - img[yn - 1, xn - 2] + img[yn - 2, xn + 1]
    neg.copy_shape(img)
    xc, dx = iters("x dx")
    conv = Fun()
    conv[xc] += dsl.input("line")[xc + dx] * flt[dx]
    return [st.target("stencil"), neg.target("stencil_negative"), conv.target("conv1")]


def computed_program():
    y, x, dx = iters("y x dx")
    src, b, flt = dsl.input("src"), dsl.input("b"), dsl.input("flt")
    gather = Fun()
    gather[y, x] += src[y // 2, x // 2]
    gather.with_shape(10, 14)                                  # src is 5 x 7
    scatter = Fun()
    scatter[y // 2, x % 3] += src[y, x] * b[x]
    scatter.with_shape(3, 3)
    rows = Fun()                                               # one thread per x, a read-modify-write per y
    rows[y // 2, x] += src[y, x] * b[x]
    rows.with_shape(3, 7)
    wr = Fun()
    wr[y, x] += src[y, wrap(x - 2, 7)] * b[x]
    wr.copy_shape(src)
    xs = iters("x")
    negidx = Fun()                                             # sdiv / srem on negative values: truncation toward zero
    negidx[xs] += b[(xs - 3) // 2 + 2] + 2.0 * b[(xs - 3) % 3 + 2]
    negidx.with_shape(7)
    tconv = Fun()
    tconv[xs + dx] += dsl.input("line")[xs] * flt[dx]
    tconv.with_shape(39)                                       # 37 + 3 - 1
    return [gather.target("gather"), scatter.target("scatter"), rows.target("scatter_rows"), wr.target("wrap"),
            negidx.target("negative_index"), tconv.target("conv_transposed")]


def reduce_program():
    y, x, r, it = iters("y x r it")
    a, b = dsl.input("a"), dsl.input("b")
    mv = Fun()
    mv[y] += a[y, x] * b[x]
    dot = Fun()
    dot[0] += a.raw[it] * b.raw[it]
    cols = Fun()
    cols[x] += split_body(a[r, x], b[r])
    s = dsl.iter_in("s", 1, 4)
    two = Fun()
    two[y] += a[y, r, s] * b[r, s]
    xb = dsl.iter_in("x", 0, 3)
    part = Fun()
    part[xb] += split_body(a[r, xb], b[r])
    part.with_shape(5)
    return [mv.target("matvec"), dot.target("dot"), cols.target("columns"), two.target("two_loops"), part.target("part_cover")]


def split_program():
    y, x, r = iters("y x r")
    a, b = dsl.input("a"), dsl.input("b")
    cols = Fun()
    cols[x] += split_body(a[r, x], b[r])
    s = dsl.iter_in("s", 1, 8)
    two = Fun()
    two[y, x] += split_body(a[r, s, y, x], b[r, s])
    twice = Fun()
    twice[x] += split_body(a[r, x], b[r])
    twice[x] += a[r, x] * b[r]
    ex = Fun()
    ex[x] += dsl.exp(a[r, x] * 0.5)
    return [cols.target("columns"), two.target("two_by_two"), twice.target("columns_twice"), ex.target("columns_exp")]


def index_program():
    it = iters("it")
    out = Fun()
    out.raw[it] += dsl.to_scalar(it * 100000)
    out.with_shape(21480)
    return [out.target("index_values")]


def f64_program():
    """One kernel of every family for compile[float64]."""
    y, x, r, it, n, c = iters("y x r it n c")
    a, b, img, src = dsl.input("a"), dsl.input("b"), dsl.input("img"), dsl.input("src")
    m = Fun()
    m[y, x] += a[y, x] * b[x] + a[y, x]
    m.copy_shape(a)
    p, q = dsl.input("p"), dsl.input("q")
    sh = Fun()
    sh[n, y, x, c] += p[n, y, x, c] * q[n, y, x, c]
    sh.copy_shape(p)
    ys, xs = dsl.iter_in("y", 0, 7), dsl.iter_in("x", 0, 9)
    st = Fun()
    st[ys, xs] += img[ys, xs] + img[ys + 1, xs + 2] - img[ys + 2, xs]
    st.with_shape(7, 9)
    sc = Fun()
    sc[y // 2, x % 3] += src[y, x] * b[x]
    sc.with_shape(3, 3)
    mv = Fun()
    mv[y] += a[y, x] * b[x]
    cols = Fun()
    cols[x] += split_body(a[r, x], b[r])
    iv = Fun()
    iv.raw[it] += dsl.to_scalar(it * 100000)
    iv.with_shape(21480)
    return [m.target("map"), sh.target("shared"), st.target("stencil"), sc.target("scatter"), mv.target("matvec"),
            cols.target("columns"), iv.target("index_values")]


PROGRAMS = {"maps": maps_program, "shared": shared_program, "displaced": displaced_program, "computed": computed_program,
            "reduce": reduce_program, "split": split_program, "index": index_program, "f64": f64_program}


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def uniform(rng, *shape):
    return (rng.random(shape, dtype=np.float32) - np.float32(0.5)).astype(np.float32)


def dyadic(rng, *shape):
    return (rng.integers(-16, 17, size=shape) / 8.0).astype(np.float32)


# ---- numpy references (float64, from the statements) ---------------------------------------------------------------------------------------
def f8(i):
    return {k: np.asarray(v, np.float64) for k, v in i.items()}


def ref_map(i):
    i = f8(i)
    return i["a"] * i["b"][None, :i["a"].shape[1]] + i["a"]


def ref_map_twice(i):
    i = f8(i)
    return i["a"] * i["b"][None, :] + (i["a"] - i["b"][None, :])


def ref_map_cols(lo, hi):
    def ref(i):
        i = f8(i)
        out = np.zeros_like(i["a"])
        out[:, lo:hi] = i["a"][:, lo:hi] * i["b"][None, lo:hi] + i["a"][:, lo:hi]
        return out
    return ref


def ref_map_raw(i):
    i = f8(i)
    return i["a"] * 2.0 - i["b"]


def ref_map_three(i):
    i = f8(i)
    return i["a"] * i["b"][None, :, :] + i["c"][None, None, :]


def ref_map_position(i):
    a = f8(i)["a"]
    return a * np.arange(a.shape[1])[None, :] + np.arange(a.shape[0])[:, None]


def ref_map_transposed(i):
    i = f8(i)
    return i["a"] + i["b"].T


def ref_shared(i):
    i = f8(i)
    a, b = (i["a"], i["b"]) if "a" in i else (i["p"], i["q"])
    out = np.zeros_like(a)
    w = min(a.shape[2], 5) if b.shape != a.shape else a.shape[2]
    out[:, :, :w] = a[:, :, :w] * b[:, :, :w]
    return out


def ref_stencil(i):
    g = f8(i)["img"]
    out = np.zeros((7, 9))
    for yy in range(7):
        for xx in range(9):
            out[yy, xx] = g[yy, xx] + g[yy + 1, xx + 2] - g[yy + 2, xx]
    return out


def ref_stencil_negative(i):
    g = f8(i)["img"]
    out = np.zeros_like(g)
    for yy in range(2, 9):
        for xx in range(2, 10):
            out[yy, xx] = g[yy, xx] - g[yy - 1, xx - 2] + g[yy - 2, xx + 1]
    return out


def ref_conv1(i):
    i = f8(i)
    line, flt = i["line"], i["flt"]
    n = line.size - flt.size + 1
    return sum(line[d:d + n] * flt[d] for d in range(flt.size))


def ref_gather(i):
    s = f8(i)["src"]
    out = np.zeros((10, 14))
    for yy in range(10):
        for xx in range(14):
            out[yy, xx] = s[yy // 2, xx // 2]
    return out


def ref_scatter(i):
    i = f8(i)
    out = np.zeros((3, 3))
    for yy in range(i["src"].shape[0]):
        for xx in range(i["src"].shape[1]):
            out[yy // 2, xx % 3] += i["src"][yy, xx] * i["b"][xx]
    return out


def ref_scatter_rows(i):
    i = f8(i)
    out = np.zeros((3, 7))
    for yy in range(5):
        out[yy // 2] += i["src"][yy] * i["b"]
    return out


def ref_wrap(i):
    i = f8(i)
    out = np.zeros_like(i["src"])
    for xx in range(7):
        out[:, xx] = i["src"][:, (xx - 2 + 7) % 7] * i["b"][xx]
    return out


def trunc_div(a, b):
    return int(np.trunc(a / b))


def ref_negative_index(i):
    b = f8(i)["b"]
    out = np.zeros(7)
    for xx in range(7):
        q = trunc_div(xx - 3, 2)
        rem = (xx - 3) - trunc_div(xx - 3, 3) * 3
        out[xx] = b[q + 2] + 2.0 * b[rem + 2]
    return out


def ref_conv_transposed(i):
    i = f8(i)
    out = np.zeros(39)
    for xx in range(37):
        for d in range(3):
            out[xx + d] += i["line"][xx] * i["flt"][d]
    return out


def ref_matvec(i):
    i = f8(i)
    return i["a"] @ i["b"]


def ref_dot(i):
    i = f8(i)
    return np.array([np.sum(i["a"].ravel() * i["b"].ravel())])


def ref_columns(i):
    i = f8(i)
    return np_split_body(i["a"], i["b"][:, None]).sum(axis=0)


def ref_two_loops(i):
    i = f8(i)
    return np.einsum("yrs,rs->y", i["a"][:, :, 1:4], i["b"][:, 1:4])


def ref_part_cover(i):
    out = np.zeros(5)
    out[:3] = ref_columns(i)[:3]
    return out


def ref_two_by_two(i):
    i = f8(i)
    return np_split_body(i["a"][:, 1:8], i["b"][:, 1:8, None, None]).sum(axis=(0, 1))


def ref_columns_twice(i):
    i = f8(i)
    return ref_columns(i) + (i["a"] * i["b"][:, None]).sum(axis=0)


def ref_columns_exp(i):
    return np.exp(f8(i)["a"] * 0.5).sum(axis=0)


def ref_index_values(i):
    return np.arange(21480, dtype=np.float64) * 100000.0


# ---- the table -------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, family, program, target, make_inputs, ref, route, exact=False, f64=False, total=None, rtotal=None,
                 tx=None, ragged=None, vec4=None):
        """route: words the case's launch lines must hold with fusion off (every generated line of the target);
        vec4: for maps, the conditions that keep the launch from four elements per thread (empty set: it takes them)."""
        self.name, self.family, self.program, self.target = name, family, program, target
        self.make_inputs, self.ref, self.route = make_inputs, ref, tuple(route)
        self.exact, self.f64, self.total, self.rtotal, self.tx, self.ragged, self.vec4 = exact, f64, total, rtotal, tx, ragged, vec4
        self.mode_b = "generated(split-reduce)" in self.route

    @property
    def dtype(self):
        return np.float64 if self.f64 else np.float32

    def inputs(self):
        rng = np.random.default_rng(sum(ord(ch) * (k + 1) for k, ch in enumerate(self.name)))
        return {k: np.ascontiguousarray(v, dtype=self.dtype) for k, v in self.make_inputs(rng).items()}

    def want(self):
        return np.asarray(self.ref(self.inputs()), np.float64)


def ab(shape_a, shape_b, draw=uniform, **more):
    def make(rng):
        out = {"a": draw(rng, *shape_a), "b": draw(rng, *shape_b)}
        for k, shp in more.items():
            out[k] = draw(rng, *shp)
        return out
    return make


def named(draw=uniform, **shapes):
    return lambda rng: {k: draw(rng, *shp) for k, shp in shapes.items()}


def expected_tx(total):
    tx = 1
    while tx < total and tx < 64:
        tx <<= 1
    return tx


def takes_mode_b(total, rtotal, full_cover=True):
    """The gate of plan.cpp for a kernel that is eligible for the split reduction."""
    return rtotal >= 2048 and total <= 8192 and total * 64 <= rtotal and full_cover


MAP, MAPV = ("generated(map)", "narrow"), ("generated(map)", "vec4", "narrow")
RED, SCAT = ("generated(map)", "reduce", "narrow"), ("generated(map)", "scatter", "narrow")


def split_case(name, target, total, rtotal, make, ref, ragged, exact=True, f64=False, program="split"):
    tx = expected_tx(total)
    assert takes_mode_b(total, rtotal)
    return Case(name, "split", program, target, make, ref, ("generated(split-reduce)", "reduce", "tx=%d " % tx), exact=exact, f64=f64,
                total=total, rtotal=rtotal, tx=tx, ragged=ragged)


# (total, rtotal, ragged): the issue's table, plus 9 -> tx = 16
SPLIT_TABLE = [(1, 2048, None), (2, 2051, "all"), (3, 2051, "all"), (5, 2051, "all"), (9, 2051, "all"), (17, 2051, "all"), (32, 2048, None),
               (33, 2112, None), (64, 4099, "last"), (65, 4160, None), (130, 8323, "last")]


def build_cases():
    c = []
    # ---- maps
    c.append(Case("MAP_5x8", "map", "maps", "map", ab((5, 8), (8,)), ref_map, MAPV, vec4=set()))
    c.append(Case("MAP_5x7", "map", "maps", "map", ab((5, 7), (7,)), ref_map, MAP, vec4={"extent", "total", "last_dim"}))
    c.append(Case("MAP_6x6", "map", "maps", "map", ab((6, 6), (6,)), ref_map, MAP, vec4={"extent", "last_dim"}))
    c.append(Case("MAP_LONG_B", "map", "maps", "map", ab((5, 8), (9,)), ref_map, MAP, vec4={"last_dim"}))
    c.append(Case("MAP_LOW", "map", "maps", "map_low", ab((5, 8), (8,)), ref_map_cols(0, 4), MAP, vec4={"bounds"}))
    c.append(Case("MAP_HIGH", "map", "maps", "map_high", ab((5, 8), (8,)), ref_map_cols(4, 8), MAP, vec4={"bounds"}))
    c.append(Case("MAP_TWICE_5x8", "map", "maps", "map_twice", ab((5, 8), (8,)), ref_map_twice, MAPV, vec4=set()))
    c.append(Case("MAP_TWICE_5x7", "map", "maps", "map_twice", ab((5, 7), (7,)), ref_map_twice, MAP, vec4={"extent", "total", "last_dim"}))
    c.append(Case("MAP_RAW_4100", "map", "maps", "map_raw", ab((4100,), (4100,)), ref_map_raw, MAPV, vec4=set()))
    c.append(Case("MAP_RAW_4099", "map", "maps", "map_raw", ab((4099,), (4099,)), ref_map_raw, MAP, vec4={"extent", "total", "last_dim"}))
    c.append(Case("MAP_3x5x8", "map", "maps", "map_three", ab((3, 5, 8), (5, 8), c=(8,)), ref_map_three, MAPV, vec4=set()))
    c.append(Case("MAP_3x5x7", "map", "maps", "map_three", ab((3, 5, 7), (5, 7), c=(7,)), ref_map_three, MAP, vec4={"extent", "total", "last_dim"}))
    c.append(Case("MAP_POSITION", "map", "maps", "map_position", named(a=(5, 8)), ref_map_position, MAP, vec4={"iterator_value"}))
    c.append(Case("MAP_TRANSPOSED", "map", "maps", "map_transposed", ab((4, 8), (8, 4)), ref_map_transposed, MAP, vec4={"operand_order"}))
    # ---- shared offsets
    c.append(Case("SHARED", "shared", "shared", "shared", ab((2, 3, 5, 4), (2, 3, 5, 4)), ref_shared, MAPV))
    # (x is bounded, but the fastest loop is c: unbounded, extent 4 = every last dimension, total 120 — four per thread, both branches)
    c.append(Case("SHARED_ELSE", "shared", "shared", "shared_else", ab((2, 3, 5, 4), (2, 3, 6, 4)), ref_shared, MAPV))
    c.append(Case("SHARED_ELSE_C3", "shared", "shared", "shared_else", ab((2, 3, 5, 3), (2, 3, 6, 3)), ref_shared, MAP))  # one per thread
    # ---- displaced reads
    c.append(Case("STENCIL", "displaced", "displaced", "stencil", named(img=(9, 11)), ref_stencil, MAP))
    c.append(Case("STENCIL_NEGATIVE", "displaced", "displaced", "stencil_negative", named(img=(9, 11)), ref_stencil_negative, MAP))
    c.append(Case("CONV1", "displaced", "displaced", "conv1", named(line=(41,), flt=(2,)), ref_conv1, RED))
    # ---- computed indices
    c.append(Case("GATHER", "computed", "computed", "gather", named(src=(5, 7)), ref_gather, MAP))
    c.append(Case("SCATTER", "computed", "computed", "scatter", named(src=(5, 7), b=(7,)), ref_scatter, SCAT))
    c.append(Case("SCATTER_ROWS", "computed", "computed", "scatter_rows", named(src=(5, 7), b=(7,)), ref_scatter_rows, SCAT))
    c.append(Case("WRAP", "computed", "computed", "wrap", named(src=(5, 7), b=(7,)), ref_wrap, MAP))
    c.append(Case("NEGATIVE_INDEX", "computed", "computed", "negative_index", named(b=(5,)), ref_negative_index, MAP))
    c.append(Case("CONV_TRANSPOSED", "computed", "computed", "conv_transposed", named(line=(37,), flt=(3,)), ref_conv_transposed, SCAT))
    # ---- serial reductions (mode A)
    c.append(Case("MATVEC_300x100", "reduce", "reduce", "matvec", ab((300, 100), (100,)), ref_matvec, RED, total=300, rtotal=100))
    c.append(Case("DOT_2047", "reduce", "reduce", "dot", ab((2047,), (2047,)), ref_dot, RED, total=1, rtotal=2047))
    c.append(Case("COLUMNS_32x2047", "reduce", "reduce", "columns", ab((2047, 32), (2047,)), ref_columns, RED, total=32, rtotal=2047))
    c.append(Case("COLUMNS_33x2111", "reduce", "reduce", "columns", ab((2111, 33), (2111,), dyadic), ref_columns, RED, exact=True, total=33,
                  rtotal=2111))
    c.append(Case("TWO_LOOPS", "reduce", "reduce", "two_loops", ab((7, 5, 4), (5, 4)), ref_two_loops, RED, total=7, rtotal=15))
    c.append(Case("PART_COVER", "reduce", "reduce", "part_cover", ab((2051, 5), (2051,), dyadic), ref_part_cover, RED, exact=True, total=3,
                  rtotal=2051))
    # ---- split reductions (mode B)
    for total, rtotal, ragged in SPLIT_TABLE:
        c.append(split_case("SPLIT_%dx%d" % (total, rtotal), "columns", total, rtotal, ab((rtotal, total), (rtotal,), dyadic), ref_columns, ragged))
    c.append(split_case("SPLIT_TWO_BY_TWO", "two_by_two", 15, 293 * 7, ab((293, 8, 3, 5), (293, 8), dyadic), ref_two_by_two, "all"))
    c.append(split_case("SPLIT_TWICE", "columns_twice", 5, 2051, ab((2051, 5), (2051,), dyadic), ref_columns_twice, "all"))
    c.append(split_case("SPLIT_EXP", "columns_exp", 3, 2051, named(a=(2051, 3)), ref_columns_exp, "all", exact=False))
    # ---- Index values: it * 100000 passes 2^31 at it = 21475; one correctly rounded conversion, so float32(reference) exactly
    c.append(Case("INDEX_VALUES", "index", "index", "index_values", lambda rng: {}, ref_index_values, ("generated(map)", "wide"), exact=True))
    # ---- float64: one case of every family, two split rows for the float64 fold
    W = ("generated(map)", "narrow")
    c.append(Case("F64_MAP", "map", "f64", "map", ab((5, 8), (8,)), ref_map, W, f64=True, vec4={"float64"}))
    c.append(Case("F64_SHARED", "shared", "f64", "shared", named(p=(2, 3, 5, 4), q=(2, 3, 5, 4)), ref_shared, W, f64=True))
    c.append(Case("F64_STENCIL", "displaced", "f64", "stencil", named(img=(9, 11)), ref_stencil, W, f64=True))
    c.append(Case("F64_SCATTER", "computed", "f64", "scatter", named(src=(5, 7), b=(7,)), ref_scatter, SCAT, f64=True))
    c.append(Case("F64_MATVEC", "reduce", "f64", "matvec", ab((300, 100), (100,)), ref_matvec, RED, f64=True, total=300, rtotal=100))
    c.append(split_case("F64_SPLIT_1x2051", "columns", 1, 2051, ab((2051, 1), (2051,), dyadic), ref_columns, "all", f64=True, program="f64"))
    c.append(split_case("F64_SPLIT_64x4099", "columns", 64, 4099, ab((4099, 64), (4099,), dyadic), ref_columns, "last", f64=True, program="f64"))
    c.append(Case("F64_INDEX_VALUES", "index", "f64", "index_values", lambda rng: {}, ref_index_values, ("generated(map)", "wide"), exact=True,
                  f64=True))
    names = [x.name for x in c]
    assert len(set(names)) == len(names)
    return c


CASES = build_cases()
BY_NAME = {c.name: c for c in CASES}


def program_text(program, f64=False):
    prog = dsl.to_program(*PROGRAMS[program]())
    prog.scalar = "f64" if f64 else "f32"
    return prog.to_text()


# ---- the comparisons both test modules use -----------------------------------------------------------------------------------------------------
TOL64 = 1e-12       # tests/test_gpu_f64.py: generated kernels over double against the oracle's float64 form


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def rel(got, want):
    want = np.asarray(want, np.float64)
    scale = max(float(np.max(np.abs(want))) if want.size else 0.0, 1e-300)
    with np.errstate(invalid="ignore"):
        d = np.abs(np.asarray(got, np.float64) - want)
    return float(np.max(d)) / scale if want.size else 0.0       # NaN if anything is NaN


def check_against_numpy(case, got, want, tol):
    """got: a result tensor of the case (whole tensor: what lies outside a bounded region must be zero); want: the float64
    numpy reference.  Exact cases: the reference rounded to the case's type, value for value (+0 and -0 alike: an
    accumulating store gives 0 + -0 = +0 where a plain one keeps -0).  Others: within tol of max|want|."""
    got = np.asarray(got)
    assert got.shape == want.shape, (case.name, got.shape, want.shape)
    assert np.all(np.isfinite(got)), (case.name, "not finite at", np.argwhere(~np.isfinite(got))[:4].tolist())
    if case.exact:
        wrong = np.argwhere(got.astype(np.float64) != want.astype(case.dtype).astype(np.float64))
        assert wrong.size == 0, (case.name, len(wrong), "values differ, first at", wrong[0].tolist(), got[tuple(wrong[0])], want[tuple(wrong[0])])
    else:
        e = rel(got, want)
        assert e <= tol, (case.name, "relative to max|reference|", e, "limit", tol)
