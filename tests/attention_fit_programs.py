"""Attention training programs for the fused fit route (Model.fuse_attention_fit; csrc/host/match_attention_grad.cpp and
csrc/host/plan_attention.cpp, form_attention_fit_groups): the block of tests/attention_programs.py with the scale spelled all
three ways, the same block behind three projections —

    q[b,i,h,k]  ++= x[b,i,e] * wq[e,h,k]        kk[b,i,h,k] ++= x[b,i,e] * wk[e,h,k]        v[b,i,h,d] ++= x[b,i,e] * wv[e,h,d]

— where the gradients of q, kk and v are results that feed the projections' gradients, and one near miss per reason for
which match_attention_fit refuses a training step.  Shared by tests/test_attention_fit_match_cpu.py and
tests/test_gpu_attention_fit_model.py."""
import re

from exprgrad_amd import dsl, layers
from exprgrad_amd.dsl import Fun, iters

import refcases

SCALE = 0.125


def _fun(name):
    f = Fun()
    f.name = name
    return f


def _middle(s, scale=SCALE, scale_first=False):
    """scale (None: no scale map) -> sums -> softmax"""
    b, h, i, j = iters("b h i j")
    if scale is None:
        e = s
    else:
        e = _fun("scaled")
        if scale_first:
            e[b, h, i, j] += scale * s[b, h, i, j]
        else:
            e[b, h, i, j] += s[b, h, i, j] * scale
    sums, p = _fun("softmax.sums"), _fun("softmax")
    sums[b, h, i] += dsl.exp(e[b, h, i, j])
    p[b, h, i, j] += dsl.exp(e[b, h, i, j]) / sums[b, h, i]
    return p


def _block(q, kk, v, middle=_middle, before=None):
    b, h, i, j, k, d = iters("b h i j k d")
    s = _fun("scores")
    if before:
        before(s)
    s[b, h, i, j] += q[b, i, h, k] * kk[b, j, h, k]
    p = middle(s)
    o = _fun("context")
    o[b, i, h, d] += p[b, h, i, j] * v[b, j, h, d]
    return s, p, o


def _targets(o, params, rate, loss_of=None):
    loss = layers.mse(loss_of if loss_of is not None else o, dsl.input("labels")).target("loss")
    return [o.target("out"), loss.backwards().optimize(params, layers.gradient_descent(rate)).target("fit")]


def training(B, H, I, J, K, D, scale=SCALE, scale_first=False, rate=0.05):
    """tests/attention_programs.py::attention_training with the scale as `s * scale`, `scale * s` or, scale=None, absent"""
    def graphs():
        q = dsl.param([B, I, H, K], name="q")
        kk = dsl.param([B, J, H, K], name="kk")
        v = dsl.param([B, J, H, D], name="v")
        _, _, o = _block(q, kk, v, lambda s: _middle(s, scale, scale_first))
        return _targets(o, [q, kk, v], rate)
    return graphs


def projected(B, H, S, E, K, D, rate=0.05):
    """x [B,S,E] -> q, kk, v through wq, wk [E,H,K] and wv [E,H,D] -> the block -> mse -> gradient descent on the weights"""
    def graphs():
        b, i, h, k, d, e = iters("b i h k d e")
        x = dsl.input("x")
        wq = dsl.param([E, H, K], name="wq")
        wk = dsl.param([E, H, K], name="wk")
        wv = dsl.param([E, H, D], name="wv")
        q, kk, v = _fun("q"), _fun("kk"), _fun("v")
        q[b, i, h, k] += x[b, i, e] * wq[e, h, k]
        kk[b, i, h, k] += x[b, i, e] * wk[e, h, k]
        v[b, i, h, d] += x[b, i, e] * wv[e, h, d]
        _, _, o = _block(q, kk, v)
        return _targets(o, [wq, wk, wv], rate)
    return graphs


# ---- near misses: one per reason of match_attention_fit; the forward chain of each is the one match_attention takes -----------
def _params(B, H, I, J, K, D):
    return dsl.param([B, I, H, K], name="q"), dsl.param([B, J, H, K], name="kk"), dsl.param([B, J, H, D], name="v")


def v_is_an_input(B, H, I, J, K, D):
    """no gradient of v is asked for: derive makes no dv"""
    def graphs():
        q, kk, _ = _params(B, H, I, J, K, D)
        _, _, o = _block(q, kk, dsl.input("v"))
        return _targets(o, [q, kk], 0.05)
    return graphs


def scores_read_again(B, H, I, J, K, D):
    """the loss is taken of the context weighted by the scores' row sums: a kernel outside the thirteen reads the scores (and
    its gradient kernel writes their gradient)"""
    def graphs():
        b, h, i, j, d = iters("b h i j d")
        q, kk, v = _params(B, H, I, J, K, D)
        s, _, o = _block(q, kk, v)
        z, r = _fun("score.sums"), _fun("weighted")
        z[b, h, i] += s[b, h, i, j]
        r[b, i, h, d] += o[b, i, h, d] * z[b, h, i]
        return _targets(o, [q, kk, v], 0.05, loss_of=r)
    return graphs


def scores_written_twice(B, H, I, J, K, D):
    """an input is added into the scores in front of the product: the scores have another writer"""
    def graphs():
        def before(s):
            b, h, i, j = iters("b h i j")
            s[b, h, i, j] += dsl.input("bias")[b, h, i, j]
        q, kk, v = _params(B, H, I, J, K, D)
        _, _, o = _block(q, kk, v, before=before)
        return _targets(o, [q, kk, v], 0.05)
    return graphs


def q_is_kk(B, H, I, J, K, D):
    """self-similarity: q and kk are one tensor (I == J), so dq and dk are one tensor too"""
    def graphs():
        q, _, v = _params(B, H, I, J, K, D)
        _, _, o = _block(q, q, v)
        return _targets(o, [q, v], 0.05)
    return graphs


def custom_dv(B, H, I, J, K, D):
    """the context product carries hand-written gradients, and the one of v reads the context's gradient at [b,h,i,d]: h and i
    out of the positions the product fixes (run with H == I, where the extents cannot tell)"""
    def graphs():
        b, h, i, j, k, d = iters("b h i j k d")
        q, kk, v = _params(B, H, I, J, K, D)
        s = _fun("scores")
        s[b, h, i, j] += q[b, i, h, k] * kk[b, j, h, k]
        p = _middle(s)
        o = _fun("context")
        o[b, i, h, d] += p[b, h, i, j] * v[b, j, h, d]
        with o.custom_grad():
            dsl.grad_of(p)[b, h, i, j] += dsl.grad_of(o)[b, i, h, d] * v[b, j, h, d]
            dsl.grad_of(v)[b, j, h, d] += p[b, h, i, j] * dsl.grad_of(o)[b, h, i, d]
        return _targets(o, [q, kk, v], 0.05)
    return graphs


def custom_de(B, H, I, J, K, D):
    """the row sum carries a hand-written gradient with the factors the other way round inside another expression: in
    position, but not what derive emits (and not the same bits)"""
    def graphs():
        b, h, i, j, k, d = iters("b h i j k d")
        q, kk, v = _params(B, H, I, J, K, D)
        s = _fun("scores")
        s[b, h, i, j] += q[b, i, h, k] * kk[b, j, h, k]
        e, sums, p = _fun("scaled"), _fun("softmax.sums"), _fun("softmax")
        e[b, h, i, j] += s[b, h, i, j] * SCALE
        sums[b, h, i] += dsl.exp(e[b, h, i, j])
        with sums.custom_grad():
            dsl.grad_of(e)[b, h, i, j] += dsl.exp(e[b, h, i, j]) * dsl.grad_of(sums)[b, h, i] * 1.0
        p[b, h, i, j] += dsl.exp(e[b, h, i, j]) / sums[b, h, i]
        o = _fun("context")
        o[b, i, h, d] += p[b, h, i, j] * v[b, j, h, d]
        return _targets(o, [q, kk, v], 0.05)
    return graphs


def _forward_miss(middle):
    def make(B, H, I, J, K, D):
        def graphs():
            q, kk, v = _params(B, H, I, J, K, D)
            _, _, o = _block(q, kk, v, middle)
            return _targets(o, [q, kk, v], 0.05)
        return graphs
    return make


def _masked(s):
    b, h, i, j = iters("b h i j")
    e, sums, p = _fun("scaled"), _fun("softmax.sums"), _fun("softmax")
    e[b, h, i, j] += s[b, h, i, j] * SCALE
    sums[b, h, i] += dsl.select(j <= i, dsl.exp(e[b, h, i, j]), 0.0)
    p[b, h, i, j] += dsl.select(j <= i, dsl.exp(e[b, h, i, j]) / sums[b, h, i], 0.0)
    return p


def _scaled_by_division(s):
    b, h, i, j = iters("b h i j")
    e, sums, p = _fun("scaled"), _fun("softmax.sums"), _fun("softmax")
    e[b, h, i, j] += s[b, h, i, j] / 8.0
    sums[b, h, i] += dsl.exp(e[b, h, i, j])
    p[b, h, i, j] += dsl.exp(e[b, h, i, j]) / sums[b, h, i]
    return p


def _scaled_by_a_tensor(s):
    b, h, i, j = iters("b h i j")
    e, sums, p = _fun("scaled"), _fun("softmax.sums"), _fun("softmax")
    e[b, h, i, j] += s[b, h, i, j] * dsl.input("t")[b, h, i, j]
    sums[b, h, i] += dsl.exp(e[b, h, i, j])
    p[b, h, i, j] += dsl.exp(e[b, h, i, j]) / sums[b, h, i]
    return p


def _bounded(width):
    def middle(s):
        b, h, i, j = iters("b h i j")
        jb = dsl.iter_in("j", 0, width)
        e, sums, p = _fun("scaled"), _fun("softmax.sums"), _fun("softmax")
        e[b, h, i, j] += s[b, h, i, j] * SCALE
        sums[b, h, i] += dsl.exp(e[b, h, i, jb])
        p[b, h, i, j] += dsl.exp(e[b, h, i, j]) / sums[b, h, i]
        return p
    return middle


def _transposed(s):
    b, h, i, j = iters("b h i j")
    w = dsl.input("w")
    e, sums, p = _fun("scaled"), _fun("softmax.sums"), _fun("softmax")
    e[b, h, i, j] += s[b, h, i, j] * SCALE
    sums[b, h, i] += dsl.exp(e[b, h, i, j]) * w[b, i, h, j]
    p[b, h, i, j] += dsl.exp(e[b, h, i, j]) * w[b, i, h, j] / sums[b, h, i]
    return p


def rank3(G, I, J, K, D):
    def graphs():
        g, i, j, k, d = iters("g i j k d")
        q, kk, v = dsl.param([G, I, K], name="q"), dsl.param([G, J, K], name="kk"), dsl.param([G, J, D], name="v")
        s, e, sums, p, o = _fun("scores"), _fun("scaled"), _fun("softmax.sums"), _fun("softmax"), _fun("context")
        s[g, i, j] += q[g, i, k] * kk[g, j, k]
        e[g, i, j] += s[g, i, j] * SCALE
        sums[g, i] += dsl.exp(e[g, i, j])
        p[g, i, j] += dsl.exp(e[g, i, j]) / sums[g, i]
        o[g, i, d] += p[g, i, j] * v[g, j, d]
        return _targets(o, [q, kk, v], 0.05)
    return graphs


def rank5(A, B, H, I, J, K, D):
    def graphs():
        a, b, h, i, j, k, d = iters("a b h i j k d")
        q, kk, v = dsl.param([A, B, I, H, K], name="q"), dsl.param([A, B, J, H, K], name="kk"), dsl.param([A, B, J, H, D], name="v")
        s, e, sums, p, o = _fun("scores"), _fun("scaled"), _fun("softmax.sums"), _fun("softmax"), _fun("context")
        s[a, b, h, i, j] += q[a, b, i, h, k] * kk[a, b, j, h, k]
        e[a, b, h, i, j] += s[a, b, h, i, j] * SCALE
        sums[a, b, h, i] += dsl.exp(e[a, b, h, i, j])
        p[a, b, h, i, j] += dsl.exp(e[a, b, h, i, j]) / sums[a, b, h, i]
        o[a, b, i, h, d] += p[a, b, h, i, j] * v[a, b, j, h, d]
        return _targets(o, [q, kk, v], 0.05)
    return graphs


def _tensor_id(text, name):
    return int(re.search(r"^tensor (\d+) \w+ %s " % re.escape(name), text, re.M).group(1))


def softmax_is_the_fit_output(text):
    """the `fit` target of the training program's text, returning the softmax"""
    return text.replace("target fit 0\n", "target fit %d\n" % _tensor_id(text, "softmax"), 1)


def dv_is_the_context(text):
    """the training program's text with the gradient of v asked for in the context's own tensor: dv is an operand"""
    v, o = _tensor_id(text, "v"), _tensor_id(text, "context")
    dest = int(re.search(r"^gradient %d (\d+)$" % v, text, re.M).group(1))
    head, fit = text.split("backwards ", 1)
    fit, rest = fit.split("endtarget", 1)
    fit = re.sub(r"^gradient %d %d$" % (v, dest), "gradient %d %d" % (v, o), fit, flags=re.M)
    fit = re.sub(r"^read %d " % dest, "read %d " % o, fit, flags=re.M)
    return head + "backwards " + fit + "endtarget" + rest


def text_of(graphs):
    return refcases.program_text(graphs())


SHAPE = (2, 3, 33, 70, 16, 16)     # B, H, I, J, K, D of the near misses that need nothing else
SQUARE = (2, 3, 3, 33, 16, 16)     # H == I
SELF = (2, 3, 33, 33, 16, 16)      # I == J

# name -> (program text, reason of match_attention_fit at the chain's live position, that position,
#          inputs next to `labels` as name -> shape, or None where the program cannot run)
def near_misses():
    B, H, I, J, K, D = SHAPE
    base = text_of(training(*SHAPE))
    s4 = (B, H, I, J)
    return {
        "v_is_an_input": (text_of(v_is_an_input(*SHAPE)), "a gradient kernel of the chain is missing", 0, {"v": (B, J, H, D)}),
        "scores_read_again": (text_of(scores_read_again(*SHAPE)),
                              "an intermediate or its gradient is read outside the chain and its gradient kernels", 0, {}),
        "softmax_is_the_fit_output": (softmax_is_the_fit_output(base), "an intermediate is the target's output", 0, {}),
        "scores_written_twice": (text_of(scores_written_twice(*SHAPE)), "an intermediate has another writer", 1, {"bias": s4}),
        "q_is_kk": (text_of(q_is_kk(*SELF)), "two of the gradients of q, kk and v are one tensor", 0, {}),
        "dv_is_the_context": (dv_is_the_context(base), "a gradient tensor is an operand of the chain", 0, None),
        "custom_dv": (text_of(custom_dv(*SQUARE)),
                      "a gradient kernel does not read its operands in the positions the forward products fix", 0, {}),
        "custom_de": (text_of(custom_de(*SHAPE)), "a gradient kernel does not compute what derive makes of the chain", 0, {}),
        "causal_mask": (text_of(_forward_miss(_masked)(*SELF)), "the row sum is not a sum of exp alone", 0, {}),
        "bounded_columns": (text_of(_forward_miss(_bounded(70))(*SHAPE)), "the row sum has loop bounds, computed indices or another rank", 0, {}),
        "transposed_operand": (text_of(_forward_miss(_transposed)(*SQUARE)), "the row sum does not read the scaled scores alone", 0,
                               {"w": (2, 3, 3, 33)}),
        "rank3": (text_of(rank3(3, 9, 70, 16, 12)), "the first kernel is not an NT product with two batch indices", 0, {}),
        "rank5": (text_of(rank5(2, 2, 3, 5, 70, 8, 8)), "the first kernel is not an NT product with two batch indices", 0, {}),
        "scale_by_a_tensor": (text_of(_forward_miss(_scaled_by_a_tensor)(*SHAPE)),
                              "the kernel behind the scores is neither a scale map over them nor the row sum", 0, {"t": s4}),
        "scale_by_division": (text_of(_forward_miss(_scaled_by_division)(*SHAPE)), "the scale is not one multiplication by a literal", 0, {}),
    }


# shapes of `labels` per near miss (the context's), where it is not that of SHAPE
LABELS = {"q_is_kk": (2, 33, 3, 16), "custom_dv": (2, 3, 3, 16), "causal_mask": (2, 33, 3, 16), "transposed_operand": (2, 3, 3, 16),
          "rank3": (3, 9, 12), "rank5": (2, 2, 5, 3, 8)}
