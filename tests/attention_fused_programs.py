"""The attention block as a forward program over inputs — scores, scale, softmax (the three statements of
tests/attention_programs.py) and context —

    scores[b,h,i,j]  ++= q[b,i,h,k] * kk[b,j,h,k]
    scaled[b,h,i,j]  ++= scores[b,h,i,j] * scale
    sums[b,h,i]      ++= exp(scaled[b,h,i,j])
    softmax[b,h,i,j] ++= exp(scaled[b,h,i,j]) / sums[b,h,i]
    context[b,i,h,d] ++= softmax[b,h,i,j] * v[b,j,h,d]

with the scale written `s * scale`, `scale * s` or not at all.  What eg_attention (kernels/attention_f32.hip) computes in one
launch; the oracle runs the program as written.  Shared by tests/test_gpu_attention_fused.py,
tests/test_attention_fused_oracle_cpu.py, tests/test_attention_match_cpu.py and tests/test_gpu_attention_fused_model.py, the
last two with the near misses of the fused chain at the end of this file."""
from exprgrad_amd import dsl
from exprgrad_amd.dsl import Fun, iters

SCALE = 0.125


def _fun(name):
    f = Fun()
    f.name = name
    return f


def _block(scale, scale_first=False):
    b, h, i, j, k, d = iters("b h i j k d")
    q, kk, v = dsl.input("q"), dsl.input("kk"), dsl.input("v")
    s = _fun("scores")
    s[b, h, i, j] += q[b, i, h, k] * kk[b, j, h, k]
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
    o = _fun("context")
    o[b, i, h, d] += p[b, h, i, j] * v[b, j, h, d]
    return [o.target("out")]


def attention_forward(scale=SCALE):
    """q [B,I,H,K], kk [B,J,H,K], v [B,J,H,D] -> out [B,I,H,D]"""
    def graphs():
        return _block(scale)
    return graphs


def attention_forward_unscaled():
    return _block(None)


def attention_forward_scale_first():
    return _block(SCALE, scale_first=True)


# ---- near misses of the fused chain (csrc/host/match_attention.cpp): each is refused and keeps the unfused plan ------------
def _near_miss(middle, tail=None):
    """scores -> middle(s) -> context, with `middle` writing the three statements between the products"""
    def graphs():
        b, h, i, j, k, d = iters("b h i j k d")
        q, kk, v = dsl.input("q"), dsl.input("kk"), dsl.input("v")
        s = _fun("scores")
        s[b, h, i, j] += q[b, i, h, k] * kk[b, j, h, k]
        p = middle(s)
        o = _fun("context")
        o[b, i, h, d] += p[b, h, i, j] * v[b, j, h, d]
        return [(tail(s, p, o) if tail else o).target("out")]
    return graphs


def _masked(s):
    b, h, i, j = iters("b h i j")
    e, sums, p = _fun("scaled"), _fun("softmax.sums"), _fun("softmax")
    e[b, h, i, j] += s[b, h, i, j] * SCALE
    sums[b, h, i] += dsl.select(j <= i, dsl.exp(e[b, h, i, j]), 0.0)
    p[b, h, i, j] += dsl.select(j <= i, dsl.exp(e[b, h, i, j]) / sums[b, h, i], 0.0)
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


def _scaled_by(how):
    def middle(s):
        b, h, i, j = iters("b h i j")
        e, sums, p = _fun("scaled"), _fun("softmax.sums"), _fun("softmax")
        if how == "tensor":
            e[b, h, i, j] += s[b, h, i, j] * dsl.input("t")[b, h, i, j]
        else:
            e[b, h, i, j] += s[b, h, i, j] / 8.0
        sums[b, h, i] += dsl.exp(e[b, h, i, j])
        p[b, h, i, j] += dsl.exp(e[b, h, i, j]) / sums[b, h, i]
        return p
    return middle


def _sum_over_queries(s):
    """the sum runs over i and is written at [b,h,j]: not the row sum over the last axis (run with I == J)"""
    b, h, i, j = iters("b h i j")
    e, sums, p = _fun("scaled"), _fun("softmax.sums"), _fun("softmax")
    e[b, h, i, j] += s[b, h, i, j] * SCALE
    sums[b, h, j] += dsl.exp(e[b, h, i, j])
    p[b, h, i, j] += dsl.exp(e[b, h, i, j]) / sums[b, h, j]
    return p


def _softmax_of_the_transpose(s):
    """the softmax reads the scaled scores at [b,h,j,i] and writes [b,h,i,j]: a register out of position (run with I == J)"""
    b, h, i, j = iters("b h i j")
    e, sums, p = _fun("scaled"), _fun("softmax.sums"), _fun("softmax")
    e[b, h, i, j] += s[b, h, i, j] * SCALE
    sums[b, h, i] += dsl.exp(e[b, h, i, j])
    p[b, h, i, j] += dsl.exp(e[b, h, j, i]) / sums[b, h, i]
    return p


def _plain(s):
    b, h, i, j = iters("b h i j")
    e, sums, p = _fun("scaled"), _fun("softmax.sums"), _fun("softmax")
    e[b, h, i, j] += s[b, h, i, j] * SCALE
    sums[b, h, i] += dsl.exp(e[b, h, i, j])
    p[b, h, i, j] += dsl.exp(e[b, h, i, j]) / sums[b, h, i]
    return p


def _scores_read_again(s, p, o):
    """the scores feed a second consumer behind the chain"""
    b, h, i, j, d = iters("b h i j d")
    z, r = _fun("score.sums"), _fun("weighted")
    z[b, h, i] += s[b, h, i, j]
    r[b, i, h, d] += o[b, i, h, d] * z[b, h, i]
    return r


def _softmax_is_output(s, p, o):
    """the target's output is the softmax itself: the context product is dead, the chain ends at the softmax"""
    return p


def rank3():
    g, i, j, k, d = iters("g i j k d")
    q, kk, v = dsl.input("q"), dsl.input("kk"), dsl.input("v")
    s, e, sums, p, o = _fun("scores"), _fun("scaled"), _fun("softmax.sums"), _fun("softmax"), _fun("context")
    s[g, i, j] += q[g, i, k] * kk[g, j, k]
    e[g, i, j] += s[g, i, j] * SCALE
    sums[g, i] += dsl.exp(e[g, i, j])
    p[g, i, j] += dsl.exp(e[g, i, j]) / sums[g, i]
    o[g, i, d] += p[g, i, j] * v[g, j, d]
    return [o.target("out")]


def rank5():
    a, b, h, i, j, k, d = iters("a b h i j k d")
    q, kk, v = dsl.input("q"), dsl.input("kk"), dsl.input("v")
    s, e, sums, p, o = _fun("scores"), _fun("scaled"), _fun("softmax.sums"), _fun("softmax"), _fun("context")
    s[a, b, h, i, j] += q[a, b, i, h, k] * kk[a, b, j, h, k]
    e[a, b, h, i, j] += s[a, b, h, i, j] * SCALE
    sums[a, b, h, i] += dsl.exp(e[a, b, h, i, j])
    p[a, b, h, i, j] += dsl.exp(e[a, b, h, i, j]) / sums[a, b, h, i]
    o[a, b, i, h, d] += p[a, b, h, i, j] * v[a, b, j, h, d]
    return [o.target("out")]


def _qkv(B, H, I, J, K, D, **more):
    return dict({"q": (B, I, H, K), "kk": (B, J, H, K), "v": (B, J, H, D)}, **more)


# name -> (graphs, shapes of the inputs, width of the row sums)
NEAR_MISSES = {
    "causal_mask": (_near_miss(_masked), _qkv(2, 3, 33, 33, 16, 16), 33),
    "bounded_columns": (_near_miss(_bounded(70)), _qkv(2, 3, 5, 70, 16, 16), 70),
    "transposed_operand": (_near_miss(_transposed), _qkv(2, 3, 3, 70, 16, 16, w=(2, 3, 3, 70)), 70),
    "sum_over_queries": (_near_miss(_sum_over_queries), _qkv(2, 3, 33, 33, 16, 16), 33),
    "softmax_of_the_transpose": (_near_miss(_softmax_of_the_transpose), _qkv(2, 3, 33, 33, 16, 16), 33),
    "rank3": (rank3, {"q": (3, 9, 16), "kk": (3, 70, 16), "v": (3, 70, 12)}, 70),
    "rank5": (rank5, {"q": (2, 2, 5, 3, 8), "kk": (2, 2, 70, 3, 8), "v": (2, 2, 70, 3, 8)}, 70),
    "scale_by_a_tensor": (_near_miss(_scaled_by("tensor")), _qkv(2, 3, 5, 70, 16, 16, t=(2, 3, 5, 70)), 70),
    "scale_by_division": (_near_miss(_scaled_by("division")), _qkv(2, 3, 5, 70, 16, 16), 70),
    "scores_read_again": (_near_miss(_plain, tail=_scores_read_again), _qkv(2, 3, 5, 70, 16, 16), 70),
    "softmax_is_the_output": (_near_miss(_plain, tail=_softmax_is_output), {"q": (2, 5, 3, 16), "kk": (2, 70, 3, 16)}, 70),   # (v is dead)
}

# (B, H, I, J, K, D) of the cases that run against the oracle: those of the C ABI test, then those of the model test
ORACLE_SHAPES = [(2, 3, 33, 70, 16, 16), (1, 1, 1, 1, 1, 1), (1, 2, 65, 63, 20, 12), (2, 1, 64, 64, 64, 64), (1, 2, 130, 129, 128, 128),
                 (3, 2, 7, 200, 33, 1), (1, 2, 65, 64, 20, 12), (1, 2, 9, 70, 129, 16),
                 (1, 2, 65, 64, 40, 72)]     # K and D padded differently (64, 128): tests/test_gpu_attention_heads.py has the other pairs
