"""A forward attention chain whose scale map adds a tensor,

    scaled[b,h,i,j] ++= scores[b,h,i,j] * scale + m[...]          (also scale * scores, m[...] first, or no scale)

with m an input indexed [i,j], [b,j] or [b,h,i,j], runs as ONE `eg_attn` launch with m as eg_attention_bias' operand
(csrc/host/match_attention.cpp, plan_attention.cpp).  The output is held to float64 numpy and to the unfused plan of the same
model (eg_model_keep_values) within TOL.  What the matcher refuses keeps the unfused plan and the right numbers."""
import numpy as np
import pytest

import attention_fused_programs as fp
from conftest import TOL, debug_toggles_active, rel_err
from exprgrad_amd import dsl
from exprgrad_amd import model as egm
from exprgrad_amd.dsl import iters
from test_gpu_attention_fused_model import inputs, launches

pytestmark = pytest.mark.gpu
SHAPES = [(2, 3, 33, 70, 16, 16), (1, 2, 65, 64, 20, 12)]
SPELLINGS = ["s*c+m", "c*s+m", "m+s*c", "s+m"]


def program(spelling, index, extra=None):
    """the five statements with the bias map; extra: "second" adds another tensor, "written" makes m a result of the target"""
    def graphs():
        b, h, i, j, k, d = iters("b h i j k d")
        q, kk, v, m = dsl.input("q"), dsl.input("kk"), dsl.input("v"), dsl.input("m")
        at = tuple({"b": b, "h": h, "i": i, "j": j}[c] for c in index)
        if extra == "written":
            m = fp._fun("mask")
            m[at] += dsl.input("m")[at] * 1.0
        s, e, sums, p, o = (fp._fun(n) for n in ("scores", "scaled", "softmax.sums", "softmax", "context"))
        s[b, h, i, j] += q[b, i, h, k] * kk[b, j, h, k]
        sc = s[b, h, i, j]
        value = {"s*c+m": lambda: sc * fp.SCALE + m[at], "c*s+m": lambda: fp.SCALE * sc + m[at], "m+s*c": lambda: m[at] + sc * fp.SCALE,
                 "s+m": lambda: sc + m[at]}[spelling]()
        if extra == "second":
            value = value + dsl.input("n")[i, j]
        e[b, h, i, j] += value
        sums[b, h, i] += dsl.exp(e[b, h, i, j])
        p[b, h, i, j] += dsl.exp(e[b, h, i, j]) / sums[b, h, i]
        o[b, i, h, d] += p[b, h, i, j] * v[b, j, h, d]
        return [o.target("out")]
    return graphs


def bias(rng, dims, index):
    """m over the extents of its indices: a causal table for [i,j] (key 0 stays), key lengths >= 1 for [b,j], else finite values"""
    B, H, I, J, _, _ = dims
    ext = {"b": B, "h": H, "i": I, "j": J}
    if index == "ij":
        return np.where(np.arange(J)[None, :] > np.arange(I)[:, None], -np.inf, 0.0).astype(np.float32)
    if index == "bj":
        return np.where(np.arange(J)[None, :] >= np.array([J - 9 - 20 * o for o in range(B)])[:, None], -np.inf, 0.0).astype(np.float32)
    return (rng.random(tuple(ext[c] for c in index), dtype=np.float32) - np.float32(0.5)).astype(np.float32)


def exact(x, index, scale, more=0.0):
    q, kk, v, m = (x[n].astype(np.float64) for n in ("q", "kk", "v", "m"))
    full = np.einsum(index + ",bhij->bhij", m, np.ones((q.shape[0], q.shape[2], q.shape[1], kk.shape[1])))   # m as indexed, over the scores
    e = np.exp(np.einsum("bihk,bjhk->bhij", q, kk) * np.float64(np.float32(scale)) + full + more)
    return np.einsum("bhij,bjhd->bihd", e / e.sum(-1, keepdims=True), v)


@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("spelling,index", [(s, "ij") for s in SPELLINGS] + [("s*c+m", "bj"), ("s*c+m", "bhij")])
def test_the_biased_chain_is_one_launch(gpu_ctx, spelling, index, dims):
    rng = np.random.default_rng(sum(dims))
    x = dict(inputs(rng, *dims), m=bias(rng, dims, index))
    want = exact(x, index, 1.0 if spelling == "s+m" else fp.SCALE)
    assert np.all(np.isfinite(want))
    m = egm.compile(*program(spelling, index)(), gpu=gpu_ctx)
    got = np.array(m.call("out", x))
    if not debug_toggles_active():
        lines = launches(m)
        assert len(lines) == 1 and "eg_attn " in lines[0] and "bias=m" in lines[0] and "eg_bgemm2" not in lines[0], lines
    m.keep_values(True)
    unfused = np.array(m.call("out", x))
    assert "eg_attn" not in m.launch_plan("out")
    errs = rel_err(got, want, "biased attention vs float64"), rel_err(got, unfused, "biased attention vs the unfused plan")
    print(spelling, index, dims, errs)
    assert np.all(np.isfinite(got)) and max(errs) <= TOL, errs
    m.close()


@pytest.mark.parametrize("name,index,extra,dtype", [
    ("written_by_the_target", "ij", "written", np.float32), ("out_of_order", "hbij", None, np.float32), ("no_key_index", "bhi", None, np.float32),
    ("second_tensor", "ij", "second", np.float32), ("float64_model", "ij", None, np.float64)])
def test_refusals_keep_the_unfused_plan(gpu_ctx, name, index, extra, dtype):
    dims = (2, 3, 33, 70, 16, 16)
    rng = np.random.default_rng(len(name))
    x = dict(inputs(rng, *dims), m=bias(rng, dims, index))
    if extra == "second":
        x["n"] = bias(rng, dims, "bhij")[0, 0]
    x = {k: v.astype(dtype) for k, v in x.items()}
    m = egm.compile(*program("m+s*c" if extra == "written" else "s*c+m", index, extra)(), gpu=gpu_ctx, dtype=dtype)   # (m's writer in front of the chain)
    got = m.call("out", x)
    assert "eg_attn" not in m.launch_plan("out"), m.launch_plan("out")
    want = exact(x, index, fp.SCALE, x["n"].astype(np.float64) if extra == "second" else 0.0)
    assert rel_err(got, want, "refused biased attention (%s) vs float64" % name) <= (TOL if dtype == np.float32 else 1e-12)
    m.close()


def test_replays_see_a_rebound_bias(gpu_ctx):
    """q, kk, v and two different biases are resident device tensors; the bias input is bound to one, then the other, in turn:
    the pointer a captured launch holds is the one bound for that run"""
    import torch
    dims = (2, 3, 33, 70, 16, 16)
    rng = np.random.default_rng(31)
    host = inputs(rng, *dims)
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    biases = [bias(rng, dims, "bhij") * np.float32(n + 1) for n in range(2)]
    resident = [torch.from_numpy(b).cuda() for b in biases]
    assert resident[0].data_ptr() != resident[1].data_ptr()
    m = egm.compile(*program("s*c+m", "bhij")(), gpu=gpu_ctx)
    for step in range(6):
        got = m.call("out", dict(dev, m=resident[step % 2]))
        assert rel_err(got, exact(dict(host, m=biases[step % 2]), "bhij", fp.SCALE), "replayed biased attention, call %d" % step) <= TOL
    if not debug_toggles_active():
        assert "bias=m" in m.launch_plan("out")
    m.close()
