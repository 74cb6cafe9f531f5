"""What sits between the two multi-head products (tests/multihead_programs.py): a scale and a softmax over the last axis of
the scores, written as the three statements anyone writes —

    e[b,h,i,j]  ++= s[b,h,i,j] * scale
    sums[b,h,i] ++= exp(e[b,h,i,j])
    p[b,h,i,j]  ++= exp(e[b,h,i,j]) / sums[b,h,i]

— at rank 4 and rank 3, the whole attention block as a training step, and the near misses of the collapsed wide row rule
(csrc/host/rowfuse.hpp, "Collapsed leading axes").  Shared by tests/test_wide_collapse_cpu.py,
tests/test_attention_oracle_cpu.py and tests/test_gpu_attention_rows.py."""
from exprgrad_amd import dsl, layers
from exprgrad_amd.dsl import Fun, iters

SCALE = 0.125


def _fun(name):
    f = Fun()
    f.name = name
    return f


def _softmax4(s, scale=SCALE):
    b, h, i, j = iters("b h i j")
    e, sums, p = _fun("scaled"), _fun("softmax.sums"), _fun("softmax")
    e[b, h, i, j] += s[b, h, i, j] * scale
    sums[b, h, i] += dsl.exp(e[b, h, i, j])
    p[b, h, i, j] += dsl.exp(e[b, h, i, j]) / sums[b, h, i]
    return p


def softmax_forward():
    """scale -> sums -> normalise over `s` [B, H, I, J]"""
    return [_softmax4(dsl.input("s")).target("out")]


def softmax_forward_rank3():
    """the same over `s` [G, I, J]"""
    g, i, j = iters("g i j")
    s = dsl.input("s")
    e, sums, p = _fun("scaled"), _fun("softmax.sums"), _fun("softmax")
    e[g, i, j] += s[g, i, j] * SCALE
    sums[g, i] += dsl.exp(e[g, i, j])
    p[g, i, j] += dsl.exp(e[g, i, j]) / sums[g, i]
    return [p.target("out")]


def attention_training(B, H, I, J, K, D, rate=0.05):
    """q, kk, v parameters -> scores -> scale -> softmax -> context -> mse -> gradient descent"""
    def graphs():
        b, h, i, j, k, d = iters("b h i j k d")
        q = dsl.param([B, I, H, K], name="q")
        kk = dsl.param([B, J, H, K], name="kk")
        v = dsl.param([B, J, H, D], name="v")
        s = _fun("scores")
        s[b, h, i, j] += q[b, i, h, k] * kk[b, j, h, k]
        p = _softmax4(s)
        o = _fun("context")
        o[b, i, h, d] += p[b, h, i, j] * v[b, j, h, d]
        loss = layers.mse(o, dsl.input("labels")).target("loss")
        return [o.target("out"), loss.backwards().optimize([q, kk, v], layers.gradient_descent(rate)).target("fit")]
    return graphs


# ---- near misses: every kernel that would sum over the row is refused, so no collapsed group forms -------------------------
def causal_mask():
    """a row register used as a value: the mask is `select` on i and j"""
    b, h, i, j = iters("b h i j")
    s = dsl.input("s")
    e, sums, p = _fun("scaled"), _fun("softmax.sums"), _fun("softmax")
    e[b, h, i, j] += s[b, h, i, j] * SCALE
    sums[b, h, i] += dsl.select(j <= i, dsl.exp(e[b, h, i, j]), 0.0)
    p[b, h, i, j] += dsl.select(j <= i, dsl.exp(e[b, h, i, j]) / sums[b, h, i], 0.0)
    return [p.target("out")]


def bounded_columns(width):
    """the row sum runs over `j in 0 ..< width` with explicit bounds"""
    def graphs():
        b, h, i, j = iters("b h i j")
        jb = dsl.iter_in("j", 0, width)
        s = dsl.input("s")
        e, sums, p = _fun("scaled"), _fun("softmax.sums"), _fun("softmax")
        e[b, h, i, j] += s[b, h, i, j] * SCALE
        sums[b, h, i] += dsl.exp(e[b, h, i, jb])
        p[b, h, i, j] += dsl.exp(e[b, h, i, j]) / sums[b, h, i]
        return [p.target("out")]
    return graphs


def transposed_operand():
    """a row operand indexed [b,i,h,j] next to [b,h,i,j]: h and i sit at different positions in two operands of one kernel
    (run with H == I, where the extents cannot tell)"""
    b, h, i, j = iters("b h i j")
    s, w = dsl.input("s"), dsl.input("w")
    e, sums, p = _fun("scaled"), _fun("softmax.sums"), _fun("softmax")
    e[b, h, i, j] += s[b, h, i, j] * SCALE
    sums[b, h, i] += dsl.exp(e[b, h, i, j]) * w[b, i, h, j]
    p[b, h, i, j] += dsl.exp(e[b, h, i, j]) * w[b, i, h, j] / sums[b, h, i]
    return [p.target("out")]


def softmax_forward_rank5():
    a, b, h, i, j = iters("a b h i j")
    s = dsl.input("s")
    e, sums, p = _fun("scaled"), _fun("softmax.sums"), _fun("softmax")
    e[a, b, h, i, j] += s[a, b, h, i, j] * SCALE
    sums[a, b, h, i] += dsl.exp(e[a, b, h, i, j])
    p[a, b, h, i, j] += dsl.exp(e[a, b, h, i, j]) / sums[a, b, h, i]
    return [p.target("out")]


def maps_only():
    """a chain of maps over [B, H, I, J] with a per-row operand but no row sum: map groups and epilogues keep it"""
    b, h, i, j = iters("b h i j")
    s, t = dsl.input("s"), dsl.input("t")
    e, f, g = _fun("scaled"), _fun("shifted"), _fun("squashed")
    e[b, h, i, j] += s[b, h, i, j] * SCALE
    f[b, h, i, j] += e[b, h, i, j] - t[b, h, i]
    g[b, h, i, j] += dsl.exp(f[b, h, i, j]) * e[b, h, i, j]
    return [g.target("out")]


# name -> (graphs, shapes of the inputs)
NEAR_MISSES = {
    "causal_mask": (causal_mask, {"s": (2, 3, 70, 70)}),
    "bounded_columns": (bounded_columns(70), {"s": (2, 3, 5, 70)}),
    "transposed_operand": (transposed_operand, {"s": (2, 3, 3, 70), "w": (2, 3, 3, 70)}),
    "rank5": (softmax_forward_rank5, {"s": (2, 2, 3, 5, 70)}),
    "width_64": (softmax_forward, {"s": (2, 3, 5, 64)}),
    "width_4097": (softmax_forward, {"s": (1, 2, 3, 4097)}),
    "maps_only": (maps_only, {"s": (2, 3, 5, 70), "t": (2, 3, 5)}),
}

# (B, H, I, J) of the rank-4 forward cases, and (G, I, J) of the rank-3 one
FORWARD_SHAPES = [(2, 3, 5, 70), (2, 3, 70, 70), (1, 1, 257, 65), (1, 1, 1, 128), (2, 70, 3, 70)]
RANK3_SHAPE = (3, 9, 257)
TRAINING_SHAPE = (2, 3, 33, 70, 16, 16)      # B, H, I, J, K, D
