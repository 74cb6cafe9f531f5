"""Programs with a leading batch index, shared by tests/test_batched_match_cpu.py and tests/test_gpu_batched_model.py."""
from exprgrad_amd import dsl, layers
from exprgrad_amd.dsl import Fun, iters


def batched_forward():
    """out[g,i,j] ++= a[g,i,k] * b[g,k,j]"""
    g, i, j, k = iters("g i j k")
    out = Fun()
    out[g, i, j] += dsl.input("a")[g, i, k] * dsl.input("b")[g, k, j]
    return [out.target("out")]


def batched_training(G, I, J, K, rate=0.05):
    """Both operands are parameters: the backward pass holds both derived gradients of the batched form."""
    def graphs():
        g, i, j, k = iters("g i j k")
        a = dsl.param([G, I, K], name="a")
        b = dsl.param([G, K, J], name="b")
        out = Fun()
        out[g, i, j] += a[g, i, k] * b[g, k, j]
        loss = layers.mse(out, dsl.input("labels")).target("loss")
        return [out.target("out"), loss.backwards().optimize([a, b], layers.gradient_descent(rate)).target("fit")]
    return graphs


def shared_training(K, J, H, rate=0.05):
    """Two shared-weight layers over a [batch, seq, feat] activation: forward, input gradient and weight gradient."""
    def graphs():
        g, i, j, k, h = iters("g i j k h")
        x = dsl.input("x")
        w1 = dsl.param([K, J], name="w1")
        w2 = dsl.param([J, H], name="w2")
        hid = Fun()
        hid[g, i, j] += x[g, i, k] * w1[k, j]
        out = Fun()
        out[g, i, h] += hid[g, i, j] * w2[j, h]
        loss = layers.mse(out, dsl.input("labels")).target("loss")
        return [out.target("out"), loss.backwards().optimize([w1, w2], layers.gradient_descent(rate)).target("fit")]
    return graphs


def batch_in_the_middle():
    """out[i,g,j] ++= a[i,g,k] * b[g,k,j]: the batch index is not leading, the generated kernel stays."""
    g, i, j, k = iters("g i j k")
    out = Fun()
    out[i, g, j] += dsl.input("a")[i, g, k] * dsl.input("b")[g, k, j]
    return [out.target("out")]


def bounded_loop():
    g, i, j = iters("g i j")
    k = dsl.iter_in("k", 0, 3)
    out = Fun()
    out[g, i, j] += dsl.input("a")[g, i, k] * dsl.input("b")[g, k, j]
    return [out.target("out")]


def other_leading_register():
    """The second operand is rank 3 but led by i, not by the batch index."""
    g, i, j, k = iters("g i j k")
    out = Fun()
    out[g, i, j] += dsl.input("a")[g, i, k] * dsl.input("b")[i, k, j]
    return [out.target("out")]


def two_multiplications():
    g, i, j, k = iters("g i j k")
    out = Fun()
    out[g, i, j] += dsl.input("a")[g, i, k] * dsl.input("b")[g, k, j] * 2.0
    return [out.target("out")]


NEAR_MISSES = {"middle": batch_in_the_middle, "bounded": bounded_loop, "leading": other_leading_register, "two_muls": two_multiplications}
