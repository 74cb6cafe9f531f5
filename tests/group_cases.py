"""The case table of the fusion groups (csrc/host/rowfuse_row.cpp, rowfuse_wide.cpp, rowfuse_sample.cpp and form_* of
plan_groups.cpp), member by member and route by route.

The cases of tests/generated_cases.py are one kernel per target and never reach a group; the planner prefers a group whenever
two or more kernels line up, and the group generators emit code of their own for the same statements.  Every case here is a
CHAIN of statements written so that a group forms: a program of the Python DSL mirror, a target, the input shapes, the words
the launch lines of the plan (Model.launch_plan) must hold, and a float64 numpy reference written from the statements
themselves — not through oracle/kd.py, which restates the rules of csrc/host/kd.cpp and could share a misreading.
tests/test_group_cases_cpu.py holds the oracle to these references and the per-member claims to the analyses (through
tests/group_route_driver.cpp); tests/test_gpu_group_routes.py the backend.

The words of a group's launch line (eg_model_launch_text; they come from the planner's and the generators' own records —
RowGroup, WideKernelInfo, SampleMemberRoute — not from the emitted text):

    row-fused <n> kernels, grid <g> x 256 | <ending> sums=<red_total>[ | unrolled trips=<t>]
        ending: `no sums` (nothing is summed over the batch), `direct` (one block adds its totals to their tensors itself),
        `partial rows folded by the last block to arrive` (at most 64 totals, 2 .. 4096 blocks) or `row_finalize` (a second
        launch folds the partial rows); `unrolled trips=` when the strided sample loop has a literal trip count.
    wide-row-fused <name> W=<w> <n> kernels (<tensor>:<kind>, ...), one wave per sample, grid <g> x 256
        kind: map | rowsum | colsum | total | seed, then `raw` for a {it} member and `nocol` for a member without a column
        loop (a [B]-only map is `rowsum nocol`: it writes a [B] tensor; a sum of [B] values is `total nocol`).
    sample-fused <n> kernels, one block per sample (<B> blocks) ... | threads=<t> narrow|wide lds=<n> zeroed=<n> staged=<n>
        barriers=<kept>/<members> | 0:<entry>; 1:<entry>; ...
        entry: seed | raw | items | scatter | split T=<n> | gather | conv-forward | conv-grad-filter | conv-grad-image, then
        `ragged=<n>` (a split whose outer reduction extent leaves n over T), `R=<n>` (register blocking), `trips=<whole>` and
        `+ragged` (the item loop: whole trips of the block, a last trip not every thread takes), `rolled` (no literal trip
        count), `slab` / `slab+` (first / later contribution to a batch sum), `lds` (the result lives in LDS).

Boundaries, read from plan_groups.cpp and the generators as they stand:
    thread per sample: every row of at most MAX_INNER = 64 floats; a group holds at most LOCAL_BUDGET = 192 floats of state
        per thread (row-local rows, totals).  CHAIN at W = 64 is 64 + 1 + 1 + 64 = 130 floats for u, s, m, v and 194 with cs:
        the run splits into u, s, m, v (no sums) and cs, rs, rq, rm (67 totals: above 64, so row_finalize above one block);
        at W = 60 it is 122 + 63 = 185 floats: one group, 63 totals, folded in the kernel; at W = 12 one group, 15 totals.
        B <= 256: direct.  65537 rows are 257 blocks and partial rows: the last block's fold loop (256 threads) takes a
        second trip.  B >= 4096 with at most 64 floats of state: launch bounds (256, 5) (`slim`: W = 12 has 41).
    wave per sample: 65 <= W <= 4096; state = ceil(W / 64) registers per [B, W] tensor written in the group and per [W] batch
        sum and one per single-element total, at most WIDE_STATE_MAX = 128 (chain_wide_groups below walks the members as
        form_wide_groups does).  CHAIN holds u, v, cs and three totals: 3 * 41 + 3 = 126 at W = 2624 (one group of eight);
        3 * 42 + 3 = 129 at W = 2688, where rm no longer fits (a group of seven; rm keeps a launch of its own); at W = 2752,
        3 * 43 = 129 with cs: u, s, m, v | cs, rs, rq, rm, as at 4096.
    block per sample: 2 <= B <= 1280, at least four members, 4096 .. 2^20 iterations per sample; a member that sums over the
        batch must write a parameter gradient.  The head of CHAIN (u, s, m, v: 3 W + 1 iterations) qualifies from W = 1365:
        those shapes run both ways, with EG_NO_SAMPLE_FUSE=1 and without.

Inputs: U[-0.5, 0.5) float32, except CHAIN.  Its totals rs, rq and rm would cancel on centred inputs (a sum near zero is held
to 1e-5 of ITSELF), so `a` is U[0, 1): u = 2 a - t has mean 1 and every total is a sum of mostly like-signed terms.  Above
CHAIN_UNIFORM_MAX = 4096 terms the oracle's own sequential float32 sums of such terms drift past the direct gate; there the
inputs are coarse dyadic values — a, t, c from {-1/2, 0, 1/2}, k = -1/2 — so that every term is a multiple of 1/32 and
the partial sums of the shapes here stay well inside float32's significand: oracle, backend and numpy then differ by a few
roundings at most, whatever the order of summation (tests/test_group_cases_cpu.py shows it for the oracle at every shape).
No case is marked exact: the worst-case partial sums of the large shapes exceed 2^24 units, only the typical ones do not.
"""
import numpy as np

from exprgrad_amd import dsl, layers
from exprgrad_amd.dsl import Fun, iters, param, select

f32 = np.float32


def body(a, b):
    """select, -, *: what a contraction's product is replaced by so that no library pattern matches."""
    return select(b < 0.0, a - b, a * b)


def np_body(a, b):
    return np.where(b < 0, a - b, a * b)


def f8(i):
    return {k: np.asarray(v, np.float64) for k, v in i.items()}


# ---- programs ------------------------------------------------------------------------------------------------------------------------------
def chain_program():
    y, x, it = iters("y x it")
    a, t, c, k = dsl.input("a"), dsl.input("t"), dsl.input("c"), dsl.input("k")
    u = Fun(name="u")
    u.raw[it] += a.raw[it] * 2.0 - t.raw[it]
    u.copy_shape(a)
    s = Fun(name="s")
    s[y] += body(u[y, x], c[x])
    m = Fun(name="m")
    m[y] += s[y] * k[0] + s[y]
    v = Fun(name="v")
    v[y, x] += u[y, x] * m[y] + c[x]
    cs = Fun(name="cs")
    cs[x] += body(v[y, x], t[y, x])
    rs = Fun(name="rs")
    rs[0] += v[y, x]
    rq = Fun(name="rq")
    rq[0] += u.raw[it] * t.raw[it]
    rm = Fun(name="rm")
    rm[0] += m[y]
    out = Fun(name="out")          # outside the group: it reads the group's batch totals
    out[x] += cs[x] + rs[0] + rq[0] + rm[0]
    return [out.target("out")]


def ref_chain(i):
    i = f8(i)
    a, t, c, k = i["a"], i["t"], i["c"], i["k"]
    u = a * 2.0 - t
    s = np_body(u, c[None, :]).sum(axis=1)
    m = s * k[0] + s
    v = u * m[:, None] + c[None, :]
    cs = np_body(v, t).sum(axis=0)
    rs, rq, rm = np.array([v.sum()]), np.array([(u * t).sum()]), np.array([m.sum()])
    return {"u": u, "s": s, "m": m, "v": v, "cs": cs, "rs": rs, "rq": rq, "rm": rm, "out": cs + rs[0] + rq[0] + rm[0]}


def wide_totals_program():
    y, i, j = iters("y i j")
    t, p, a = dsl.input("t"), dsl.input("p"), dsl.input("a")
    g = Fun(name="g")
    g[y, j] += t[y, j] - p[y, j]
    g.copy_shape(t)
    gw = Fun(name="gw")
    gw[i, j] += body(a[y, i], g[y, j])
    return [gw.target("out")]


def ref_wide_totals(i):
    i = f8(i)
    g = i["t"] - i["p"]
    return {"g": g, "out": np_body(i["a"][:, :, None], g[:, None, :]).sum(axis=0)}


def rows3d_program(inlined=False):
    """inlined: z is a pure unary map of o, which the model inlines into its reader when it is compiled (lower.cpp
    inline_producers): fin then reads o, z stays a member whose rows nobody stores, and no plan can hand z out."""
    y, it = iters("y it")
    p, q = dsl.iter_in("p", 0, 3), dsl.iter_in("q", 0, 5)
    a, f = dsl.input("a"), dsl.input("f")
    o = Fun(name="o")
    o[y, p, q] += a[y, p + 1, q] * f[p] - a[y, p, q + 1]
    o.with_shape(a.shape[0], 3, 5)
    r = Fun(name="r")
    r[y, p] += o[y, p, q]
    r.with_shape(a.shape[0], 3)
    z = Fun(name="z")
    z.raw[it] += o.raw[it] * 2.0 - (1.0 if inlined else dsl.input("zz").raw[it])
    z.copy_shape(o)
    tot = Fun(name="tot")
    tot[0] += r[y, p]
    fin = Fun(name="fin")          # outside the group: it reads the batch total
    fin.raw[it] += z.raw[it] + tot[0]
    fin.copy_shape(z)
    return [fin.target("out")]


def ref_rows3d(i):
    i = f8(i)
    a, f = i["a"], i["f"]
    o = a[:, 1:4, 0:5] * f[None, :, None] - a[:, 0:3, 1:6]
    r = o.sum(axis=2)
    z = o * 2.0 - (i["zz"] if "zz" in i else 1.0)
    tot = np.array([r.sum()])
    return {"o": o, "r": r, "z": z, "tot": tot, "out": z + tot[0]}


def earlier_writes_program():
    """A tensor's kernels are consecutive in a target, so a first writer that is no row kernel sits directly in front of
    the member that goes on from its values: two groups, e, h, hs (load_first, store) and cs (accumulate)."""
    y, j = iters("y j")
    x, b = dsl.input("x"), dsl.input("b")
    e = Fun(name="e")
    e[y, j] += x[y, j] * dsl.to_scalar(y)            # y as a value: no row kernel
    e[y, j] += x[y, j] * b[j]                        # member: starts from memory
    e.copy_shape(x)
    h = Fun(name="h")
    h[y, j] += e[y, j] - x[y, j]
    h.copy_shape(x)
    hs = Fun(name="hs")
    hs[0] += h[y, j]
    cs = Fun(name="cs")
    cs[j] += b[j] * 2.0                              # a small kernel: no row kernel
    cs[j] += x[y, j] * b[j]                          # member: adds to what is there
    cs[j] += body(x[y, j], b[j])                     # one more member, so that the group forms
    out = Fun(name="out")                            # outside both groups: it reads their batch totals
    out[y, j] += e[y, j] * h[y, j] + hs[0] + cs[j]
    out.copy_shape(x)
    return [out.target("out")]


def ref_earlier_writes(i):
    i = f8(i)
    x, b = i["x"], i["b"]
    cs = b * 2.0 + (x * b[None, :]).sum(axis=0) + np_body(x, b[None, :]).sum(axis=0)
    e = x * np.arange(x.shape[0])[:, None] + x * b[None, :]
    h = e - x
    hs = np.array([h.sum()])
    return {"cs": cs, "e": e, "h": h, "hs": hs, "out": e * h + hs[0] + cs[None, :]}


def tail_program():
    """A 2-wide regression step: bias add, leakyRelu, mse, gradientDescent — a row group whose last block goes on with the
    update."""
    y, j = iters("y j")
    x = dsl.input("x")
    w, bias = param([2], name="w"), param([2], name="bias")     # two parameters: two update kernels, a group the tail can take
    z = Fun(name="z")
    z[y, j] += x[y, j] * w[j] + bias[j]
    z.copy_shape(x)
    net = layers.leaky_relu(z).target("predict")
    loss = layers.mse(net, dsl.input("t")).target("loss")
    return [loss.backprop(layers.gradient_descent(0.05)).target("train")]


SF = {"P": 48, "Q": 32, "R": 8, "I": 70, "J": 24, "MP": (25, 30), "L": 7000, "RI": 1024, "RR": 130}


def sample_forward_program():
    y, p, q, r, i, j, it, x, dq = iters("y p q r i j it x dq")
    a, xs, big, lng, e, oo = dsl.input("a"), dsl.input("x"), dsl.input("big"), dsl.input("lng"), dsl.input("e"), dsl.input("oo")
    w, v, f = param([SF["R"], SF["Q"]], name="w"), param([SF["I"], SF["J"]], name="v"), param([3], name="f")
    o = Fun(name="o")
    o[y, p, q] += body(a[y, p, r], w[r, q])                   # blocked: two independent loops below the sample
    h = Fun(name="h")
    h[y, j] += body(xs[y, i], v[i, j])                        # few outputs, long reduction: split over lanes
    o2 = Fun(name="o2")
    o2.raw[it] += o.raw[it] * 2.0 - oo.raw[it]                # raw: 1536 items (two operands: no producer to inline)
    o2.copy_shape(o)
    mp = Fun(name="mp")
    mp[y, p, q] += big[y, p, q] * 0.5 + 1.0                   # 750 items: one whole trip and a ragged one
    mp.copy_shape(big)
    ml = Fun(name="ml")
    ml[y, x] += lng[y, x] * lng[y, x]                         # 7000 items: thirteen whole trips
    ml.copy_shape(lng)
    ib = dsl.iter_in("i", 0, SF["RI"])
    rr = Fun(name="rr")
    rr[y, ib] += body(lng[y, ib + r], e[r])                   # 1024 items of 130 terms: 2 x 130 > 256
    rr.with_shape(lng.shape[0], SF["RI"])
    sc = Fun(name="sc")
    sc[y, j + dq] += h[y, j] * f[dq]                          # a transposed convolution: scatter
    sc.with_shape(xs.shape[0], SF["J"] + 2)
    jb = dsl.iter_in("j", 0, 12)
    pz = Fun(name="pz")
    pz[y, jb] += h[y, jb] * 2.0                               # a bounded writer: the rest of pz must be zero
    pz.copy_shape(h)
    jo = dsl.iter_in("j", 0, SF["J"])
    out = Fun(name="out")
    out[y, jo] += o2[y, jo, 1] + mp[y, 0, jo] * ml[y, jo] + rr[y, jo] + sc[y, jo + 2] + pz[y, jo]
    out.with_shape(xs.shape[0], SF["J"])
    return [out.target("out")]


def ref_sample_forward(i, params):
    i, pr = f8(i), f8(params)
    a, xs, big, lng, e, w, v, f = i["a"], i["x"], i["big"], i["lng"], i["e"], pr["w"], pr["v"], pr["f"]
    J = SF["J"]
    o = np_body(a[:, :, :, None], w[None, None, :, :]).sum(axis=2)
    h = np_body(xs[:, :, None], v[None, :, :]).sum(axis=1)
    o2 = o * 2.0 - i["oo"]
    mp = big * 0.5 + 1.0
    ml = lng * lng
    rr = np.zeros((lng.shape[0], SF["RI"]))
    for r in range(SF["RR"]):
        rr += np_body(lng[:, r:r + SF["RI"]], e[r])
    sc = np.zeros((xs.shape[0], J + 2))
    for d in range(3):
        sc[:, d:d + J] += h * f[d]
    pz = np.zeros_like(h)
    pz[:, :12] = h[:, :12] * 2.0
    out = o2[:, :J, 1] + mp[:, 0, :J] * ml[:, :J] + rr[:, :J] + sc[:, 2:2 + J] + pz
    return {"o": o, "h": h, "o2": o2, "mp": mp, "ml": ml, "rr": rr, "sc": sc, "pz": pz, "out": out}


ST = {"I": 70, "H": 24, "O": 6, "RATE": 0.05, "LEAK": 0.01}


def sample_training_program():
    """dense 70 -> 24, leakyRelu, dense 24 -> 6 whose weight also takes the layer's input before the activation (two
    statements use it: two contributions to its gradient), mse, gradientDescent."""
    y, x, i = iters("y x i")
    xs = dsl.input("x")
    w1, b1 = param([ST["I"], ST["H"]], name="w1"), param([ST["H"]], name="b1")
    w2 = param([ST["H"], ST["O"]], name="w2")
    h = Fun(name="h")
    h[y, x] += xs[y, i] * w1[i, x]
    h[y, x] += b1[x]
    hl = layers.leaky_relu(h, ST["LEAK"])
    z = Fun(name="z")
    z[y, x] += hl[y, i] * w2[i, x]
    z[y, x] += h[y, i] * w2[i, x] * 0.5
    net = z.target("predict")
    loss = layers.mse(net, dsl.input("t")).target("loss")
    return [loss.backprop(layers.gradient_descent(ST["RATE"])).target("train")]


def ref_sample_training(i, params):
    """Forward values, the loss and the gradients of the three parameters, by hand."""
    i, pr = f8(i), f8(params)
    xs, t, w1, b1, w2 = i["x"], i["t"], pr["w1"], pr["b1"], pr["w2"]
    h = xs @ w1 + b1[None, :]
    slope = np.where(h >= 0, 1.0, float(f32(ST["LEAK"])))        # (the program's literals are float32)
    hl = slope * h
    z = hl @ w2 + 0.5 * (h @ w2)
    B = xs.shape[0]
    loss = ((z - t) ** 2).sum() / B
    gz = 2.0 * (z - t) / B
    gw2 = hl.T @ gz + 0.5 * (h.T @ gz)
    gh = (gz @ w2.T) * slope + 0.5 * (gz @ w2.T)
    return {"predict": z, "loss": np.array([loss]), "w1": xs.T @ gh, "b1": gh.sum(axis=0), "w2": gw2}


PROGRAMS = {"chain": chain_program, "wide_totals": wide_totals_program, "rows3d": rows3d_program,
            "rows3d_inlined": lambda: rows3d_program(True), "earlier": earlier_writes_program,
            "tail": tail_program, "sample_f": sample_forward_program, "sample_t": sample_training_program}


def program_text(program):
    return dsl.to_program(*PROGRAMS[program]()).to_text()


def tensor_ids(program):
    """name -> tensor id of the program's named tensors (the first of a name)."""
    ids = {}
    for tid, t in enumerate(dsl.to_program(*PROGRAMS[program]()).tensors, 1):
        if t.get("name"):
            ids.setdefault(t["name"], tid)
    return ids


# ---- the table -------------------------------------------------------------------------------------------------------------------------------
def uniform(rng, *shape):
    return (rng.random(shape, dtype=f32) - f32(0.5)).astype(f32)


CHAIN_UNIFORM_MAX = 4096


def chain_inputs(rng, B, W):
    if B * W <= CHAIN_UNIFORM_MAX:
        return {"a": rng.random((B, W), dtype=f32), "t": uniform(rng, B, W), "c": uniform(rng, W), "k": uniform(rng, 1)}
    half = lambda *shape: (rng.integers(-1, 2, size=shape) / 2.0).astype(f32)
    return {"a": half(B, W), "t": half(B, W), "c": half(W), "k": np.array([-0.5], f32)}


class Case:
    def __init__(self, name, program, target, shapes, ref, lines, env=None, stored=(), kept=(), members=None, rtotal=1, train=False,
                 absent=(), inlined=()):
        """shapes: input name -> shape; lines: one entry per group launch of the plan, in order, (kind, words) — the line of
        that kind must hold every word; absent: kinds no launch line may have; env: execution switches set while the plan
        is made; stored: tensors of `ref` that read_tensor must return as planned, kept: the ones a group never stores (refused
        as planned, equal to the reference under keep_values); members: tensor name -> what the analyses say of the kernel
        that writes it (tests/group_route_driver.cpp), checked without a GPU; rtotal: the longest sum, for the survey;
        inlined: tensors of producers the model inlined into their readers — refused by every plan."""
        self.name, self.program, self.target, self.shapes, self.ref = name, program, target, dict(shapes), ref
        self.lines, self.env, self.stored, self.kept = list(lines), dict(env or {}), tuple(stored), tuple(kept)
        self.members, self.rtotal, self.train, self.absent, self.inlined = members or {}, rtotal, train, tuple(absent), tuple(inlined)
        self.exact = False
        self.dtype = f32

    @property
    def model_key(self):
        return (self.program, tuple(sorted(self.shapes.items())), tuple(sorted(self.env.items())))

    def rng(self):
        return np.random.default_rng(sum(ord(ch) * (k + 1) for k, ch in enumerate(self.program + repr(sorted(self.shapes.items())))))

    def inputs(self):
        rng = self.rng()
        if self.program == "chain":
            return chain_inputs(rng, *self.shapes["a"])
        return {k: uniform(rng, *shp) for k, shp in sorted(self.shapes.items())}

    def params(self):
        """name -> value for the program's parameters (set on every model before the case runs)."""
        rng = np.random.default_rng(len(self.program))
        prog = dsl.to_program(*PROGRAMS[self.program]())
        return {t["name"]: (uniform(rng, *t["shape"]) * f32(0.6)).astype(f32) for t in prog.tensors if t["kind"] == "param"}

    def want(self):
        i = self.inputs()
        return self.ref(i, self.params()) if self.program.startswith("sample") else self.ref(i)


CHAIN_ORDER = ("u", "s", "m", "v", "cs", "rs", "rq", "rm")
CHAIN_READERS = {"u": ("s", "v", "rq"), "s": ("m",), "m": ("v", "rm"), "v": ("cs", "rs")}
CHAIN_WIDE_MEMBERS = {"u": "wide map raw", "s": "wide rowsum", "m": "wide rowsum nocol", "v": "wide map", "cs": "wide colsum", "rs": "wide total",
                      "rq": "wide total raw", "rm": "wide total nocol"}
CHAIN_ROW_MEMBERS = {n: "row raw" if n in ("u", "rq") else "row" for n in CHAIN_WIDE_MEMBERS}
NO_SAMPLE = {"EG_NO_SAMPLE_FUSE": "1"}
WIDE_STATE_MAX, LOCAL_BUDGET, SAMPLE_MIN_WORK, SAMPLE_MAX_BATCH = 128, 192, 4096, 1280


def chain_shapes(B, W):
    return {"a": (B, W), "t": (B, W), "c": (W,), "k": (1,)}


def wide_state(W, members=CHAIN_ORDER):
    """Floats of state per lane that a wide group of these members of CHAIN holds: ceil(W / 64) per [B, W] tensor it writes
    and per [W] sum, one per single total."""
    nj = -(-W // 64)
    return sum({"u": nj, "v": nj, "cs": nj, "rs": 1, "rq": 1, "rm": 1}.get(n, 0) for n in members)


def chain_wide_groups(W, members=CHAIN_ORDER):
    """The wide groups form_wide_groups makes of a run of CHAIN's members: each grows while its state fits; a run of one
    kernel is no group."""
    groups, run = [], []
    for n in members:
        if wide_state(W, run + [n]) > WIDE_STATE_MAX:
            groups.append(run)
            run = []
        run.append(n)
    groups.append(run)
    return [g for g in groups if len(g) >= 2]


def wide_words(group):
    return "(" + ", ".join("%s:%s" % (n, CHAIN_WIDE_MEMBERS[n][5:]) for n in group) + ")"


def stored_and_kept(groups):
    """Of the row tensors u, s, m, v: stored when a reader sits outside the writer's group, else kept in the group."""
    kept = tuple(n for n in CHAIN_READERS if any(n in g and all(r in g for r in CHAIN_READERS[n]) for g in groups))
    return tuple(n for n in CHAIN_ORDER if n not in kept), kept


def sample_takes_chain_head(B, W):
    return 2 <= B <= SAMPLE_MAX_BATCH and 3 * W + 1 >= SAMPLE_MIN_WORK


def grid(B):
    return "grid %d x 256" % -(-B // 256)


def chain_wide_case(B, W, sample):
    """sample: None — the shape forms no sample group; False — EG_NO_SAMPLE_FUSE=1; True — the sample group takes u, s, m, v."""
    w = "W=%d " % W

    def wide_line(g):
        sums = sum(1 for n in g if n in ("cs", "rs", "rq", "rm"))
        return ("wide-row-fused", (w, "%d kernels" % len(g), wide_words(g), grid(B)) + (("%d batch sums" % sums,) if sums else ()))
    if sample:
        head = ("0:raw trips=4;", "1:split T=64 rolled lds;", "2:items trips=0 +ragged;", "3:items trips=4") if W == 2048 else ()
        lines = [("sample-fused", ("sample-fused 4 kernels", "(%d blocks)" % B, "threads=512", "narrow", "lds=1 ", "zeroed=0", "staged=0") + head),
                 ] + [wide_line(g) for g in chain_wide_groups(W, CHAIN_ORDER[4:])]
        stored, kept = stored_and_kept([list(CHAIN_ORDER[:4])] + chain_wide_groups(W, CHAIN_ORDER[4:]))
    else:
        lines = [wide_line(g) for g in chain_wide_groups(W)]
        stored, kept = stored_and_kept(chain_wide_groups(W))
    name = "CHAIN_WIDE_%dx%d" % (B, W) + ("_SAMPLE" if sample else "_NOSAMPLE" if sample is False else "")
    return Case(name, "chain", "out", chain_shapes(B, W), ref_chain, lines, env=NO_SAMPLE if sample is False else None, stored=stored, kept=kept,
                members=CHAIN_WIDE_MEMBERS, rtotal=B * W, absent=("row-fused",) + (() if sample else ("sample-fused",)))


def chain_rows_case(B, W, env=None, tag=""):
    sums = W + 3
    ending = "direct" if B <= 256 and not (env or {}).get("EG_NO_ROW_DIRECT") else \
        "partial rows folded by the last block to arrive" if sums <= 64 and B > 256 and not (env or {}).get("EG_NO_ROW_TAIL") else "row_finalize"
    if 2 * W + 2 + sums <= LOCAL_BUDGET:
        lines = [("row-fused", ("row-fused 8 kernels", grid(B), "| " + ending, "sums=%d" % sums))]
        stored, kept = ("cs", "rs", "rq", "rm"), ("u", "s", "m", "v")
    else:
        lines = [("row-fused", ("row-fused 4 kernels", grid(B), "| no sums", "sums=0")),
                 ("row-fused", ("row-fused 4 kernels", grid(B), "| " + ending, "sums=%d" % sums))]
        stored, kept = ("u", "m", "v", "cs", "rs", "rq", "rm"), ("s",)
    return Case("CHAIN_ROWS_%dx%d%s" % (B, W, tag), "chain", "out", chain_shapes(B, W), ref_chain, lines, env=env, stored=stored, kept=kept,
                members=CHAIN_ROW_MEMBERS, rtotal=B * W, absent=("wide-row-fused", "sample-fused", "unrolled"))


def build_cases():
    c = []
    # ---- CHAIN, one wave per sample
    for W in (65, 127, 128, 129, 1000, 4096):
        for B in (1, 4, 5, 257):
            if sample_takes_chain_head(B, W):
                c += [chain_wide_case(B, W, False), chain_wide_case(B, W, True)]
            else:
                c.append(chain_wide_case(B, W, None))
    c.append(chain_wide_case(1025, 65, None))
    c += [chain_wide_case(65, 65, None), chain_wide_case(128, 128, None)]       # B == W: out[x] reads as a [B] member and must not join
    for W in (2624, 2688, 2752):                                                  # 126, 129 and (with cs) 129 floats of state against 128
        c += [chain_wide_case(1, W, None), chain_wide_case(4, W, False), chain_wide_case(4, W, True)]
    c += [chain_wide_case(5, 2048, False), chain_wide_case(5, 2048, True)]        # the mixed plan: a sample group of four, then a wide group
    # ---- CHAIN, one thread per sample
    for W in (64, 12):
        for B in (1, 255, 256, 257, 1000):
            c.append(chain_rows_case(B, W))
    c.append(chain_rows_case(257, 60))                                            # 63 totals: the most the in-kernel fold takes
    c.append(chain_rows_case(65537, 12))                                          # 257 partial rows: a second trip of the fold loop
    c.append(chain_rows_case(4096, 12))                                           # launch bounds (256, 5)
    c.append(chain_rows_case(255, 12, {"EG_NO_ROW_DIRECT": "1"}, "_NODIRECT"))    # same bits as direct
    c.append(chain_rows_case(1000, 12, {"EG_NO_ROW_TAIL": "1"}, "_NOTAIL"))       # same bits as the in-kernel fold (same grid)
    # ---- 80 totals: above 64, row_finalize
    for B in (257, 1000):
        c.append(Case("ROWS_WIDE_TOTALS_%d" % B, "wide_totals", "out", {"t": (B, 8), "p": (B, 8), "a": (B, 10)}, ref_wide_totals,
                      [("row-fused", ("row-fused 2 kernels", grid(B), "| row_finalize", "sums=80"))], kept=("g",),
                      members={"g": "row", "gw": "row"}, rtotal=B, absent=("wide-row-fused", "sample-fused")))
    # ---- [B, a, b] rows, bounded and displaced loops, a raw member of inner 15
    for B in (3, 300):
        c.append(Case("ROWS_3D_%d" % B, "rows3d", "out", {"a": (B, 4, 6), "f": (3,), "zz": (B, 3, 5)}, ref_rows3d,
                      [("row-fused", ("row-fused 4 kernels", grid(B), "| direct" if B <= 256 else "| partial rows folded", "sums=1"))],
                      stored=("z", "tot"), kept=("o", "r"), members={"o": "row", "r": "row", "z": "row raw", "tot": "row", "fin": "row raw"},
                      rtotal=B * 15,
                      absent=("wide-row-fused", "sample-fused")))
    c.append(Case("ROWS_3D_INLINED", "rows3d_inlined", "out", {"a": (300, 4, 6), "f": (3,)}, ref_rows3d,
                  [("row-fused", ("row-fused 4 kernels", grid(300), "| partial rows folded", "sums=1"))], stored=("o", "tot"), kept=("r",), inlined=("z",),
                  members={"o": "row", "r": "row", "z": "row raw", "tot": "row"}, rtotal=300 * 15, absent=("wide-row-fused", "sample-fused")))
    # ---- tensors written before their group: load_first + store, accumulate
    c.append(Case("ROWS_EARLIER_WRITES", "earlier", "out", {"x": (300, 8), "b": (8,)}, ref_earlier_writes,
                  [("row-fused", ("row-fused 3 kernels", grid(300), "| partial rows folded", "sums=1")),
                   ("row-fused", ("row-fused 2 kernels", grid(300), "| partial rows folded", "sums=8"))], stored=("cs", "e", "h", "hs"),
                  members={"e": "row", "h": "row", "hs": "row", "cs": "row"}, rtotal=300 * 8, absent=("wide-row-fused", "sample-fused")))
    # ---- block per sample, forward
    sf_members = {"o": "items R=3 trips=1", "o2": "raw trips=3", "mp": "items trips=1 +ragged", "ml": "items trips=13 +ragged rolled",
                  "rr": "items trips=2 rolled", "h": "split T=16 ragged=6", "sc": "scatter trips=0 +ragged rolled", "pz": "items trips=0 +ragged",
                  "out": "items trips=0 +ragged"}
    sf_entries = tuple("%d:%s%s" % (n, e, ";" if n < 8 else "") for n, e in enumerate(v + ("" if k == "out" else " lds") for k, v in sf_members.items()))
    for B in (2, 5, 64):
        shapes = {"a": (B, SF["P"], SF["R"]), "x": (B, SF["I"]), "big": (B,) + SF["MP"], "lng": (B, SF["L"]), "e": (SF["RR"],),
                  "oo": (B, SF["P"], SF["Q"])}
        inner = ("o", "h", "o2", "mp", "ml", "rr", "sc", "pz")
        c.append(Case("SAMPLE_F_%d" % B, "sample_f", "out", shapes, ref_sample_forward,
                      [("sample-fused", ("sample-fused 9 kernels", "(%d blocks)" % B, "threads=512", "narrow", "lds=8 ", "zeroed=2", "staged=3") + sf_entries)],
                      kept=inner, members={k: "sample " + v for k, v in sf_members.items()}, rtotal=SF["RR"], absent=("row-fused",)))
    names = [x.name for x in c]
    assert len(set(names)) == len(names)
    return c


CASES = build_cases()
BY_NAME = {c.name: c for c in CASES}

# the training cases run through Trio.step: (name, program, batch, words of the sample-fused line or None where no sample group may form)
TAIL_CASES = [("ROWS_TAIL_32768", 32768, ("grid 64 x 256", "partial rows folded", "unrolled trips=2")),
              ("ROWS_TAIL_33024", 32768 + 256, ("grid 64 x 256", "partial rows folded"))]
SAMPLE_T_BATCHES = (2, 3, 32, 1280, 1281)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
