"""Programs with two batch indices (the multi-head products), shared by tests/test_batched2_cpu.py and
tests/test_gpu_multihead_model.py.  q, kk, v and the context are stored [batch, seq, head, feat]; the scores [batch, head, seq, seq]."""
from exprgrad_amd import dsl, layers
from exprgrad_amd.dsl import Fun, iters


def scores_forward():
    """s[b,h,i,j] ++= q[b,i,h,k] * kk[b,j,h,k]"""
    b, h, i, j, k = iters("b h i j k")
    s = Fun()
    s[b, h, i, j] += dsl.input("q")[b, i, h, k] * dsl.input("kk")[b, j, h, k]
    return [s.target("out")]


def context_forward():
    """o[b,i,h,d] ++= p[b,h,i,j] * v[b,j,h,d]: the items of the output interleave"""
    b, h, i, j, d = iters("b h i j d")
    o = Fun()
    o[b, i, h, d] += dsl.input("p")[b, h, i, j] * dsl.input("v")[b, j, h, d]
    return [o.target("out")]


def scores_training(B, H, I, J, K, rate=0.05):
    """Both operands of the scores product are parameters: the backward pass holds both derived gradients."""
    def graphs():
        b, h, i, j, k = iters("b h i j k")
        q = dsl.param([B, I, H, K], name="q")
        kk = dsl.param([B, J, H, K], name="kk")
        s = Fun()
        s[b, h, i, j] += q[b, i, h, k] * kk[b, j, h, k]
        loss = layers.mse(s, dsl.input("labels")).target("loss")
        return [s.target("out"), loss.backwards().optimize([q, kk], layers.gradient_descent(rate)).target("fit")]
    return graphs


def batch_register_last():
    """q stored [batch, seq, feat, head]: its last dimension is a batch register, no unit-stride matrix axis"""
    b, h, i, j, k = iters("b h i j k")
    s = Fun()
    s[b, h, i, j] += dsl.input("q")[b, i, k, h] * dsl.input("kk")[b, j, h, k]
    return [s.target("out")]


def bounded_loop():
    b, h, i, j = iters("b h i j")
    k = dsl.iter_in("k", 0, 3)
    s = Fun()
    s[b, h, i, j] += dsl.input("q")[b, i, h, k] * dsl.input("kk")[b, j, h, k]
    return [s.target("out")]


def third_factor():
    b, h, i, j, k = iters("b h i j k")
    s = Fun()
    s[b, h, i, j] += dsl.input("q")[b, i, h, k] * dsl.input("kk")[b, j, h, k] * 2.0
    return [s.target("out")]


def rank3_operand():
    """kk is shared by the batch: a rank-3 operand among rank-4 ones"""
    b, h, i, j, k = iters("b h i j k")
    s = Fun()
    s[b, h, i, j] += dsl.input("q")[b, i, h, k] * dsl.input("kk")[j, h, k]
    return [s.target("out")]


def register_twice():
    """q[b,i,h,h]: a register used twice in one operand (four loops: nothing is contracted over k)"""
    b, h, i, j, k = iters("b h i j k")
    s = Fun()
    s[b, h, i, j] += dsl.input("q")[b, i, h, h] * dsl.input("kk")[b, j, h, k]
    return [s.target("out")]


NEAR_MISSES = {"batch_last": batch_register_last, "bounded": bounded_loop, "third_factor": third_factor, "rank3": rank3_operand,
               "twice": register_twice}
