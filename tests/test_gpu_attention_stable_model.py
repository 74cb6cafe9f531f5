"""Model.fuse_attention_stable: the forward attention chain of a float32 model, with and without a bias input, stays ONE eg_attn
launch and runs on eg_attention_stable's kernel.  On ordinary inputs the output is within TOL of float64; with q scaled so
that scores pass 89 it is finite where the same model with the switch off is NaN; and with the switch off the model gives the
bits of a model that never touched it."""
import numpy as np
import pytest

import attention_fused_programs as fp
from conftest import TOL, debug_toggles_active, rel_err
from exprgrad_amd import model as egm
from test_gpu_attention_bias_model import bias, program
from test_gpu_attention_fused_model import inputs, launches

pytestmark = pytest.mark.gpu


def exact(x):
    """float64 with the row maximum; (out [B,I,H,D], the largest score of each row [B,H,I])"""
    q, kk, v = (x[n].astype(np.float64) for n in ("q", "kk", "v"))
    s = np.einsum("bihk,bjhk->bhij", q, kk) * np.float64(np.float32(fp.SCALE)) + (x["m"].astype(np.float64) if "m" in x else 0.0)
    e = np.exp(s - s.max(-1, keepdims=True))
    return np.einsum("bhij,bjhd->bihd", e / e.sum(-1, keepdims=True), v), s.max(-1)


@pytest.mark.parametrize("biased", [False, True], ids=["plain", "bias_input"])
def test_the_switch(gpu_ctx, biased):
    dims = (2, 3, 33, 70, 16, 16)
    rng = np.random.default_rng(53 + biased)
    x = inputs(rng, *dims)
    if biased:
        x["m"] = bias(rng, dims, "bhij")
    graphs = program("s*c+m", "bhij") if biased else fp.attention_forward()
    untouched, m = egm.compile(*graphs(), gpu=gpu_ctx), egm.compile(*graphs(), gpu=gpu_ctx)
    base = np.array(untouched.call("out", x))
    m.fuse_attention_stable()
    got = np.array(m.call("out", x))
    if not debug_toggles_active():
        lines = launches(m)
        assert len(lines) == 1 and "eg_attn " in lines[0], lines
    err = rel_err(got, exact(x)[0], "stable attention model vs float64")
    print("biased" if biased else "plain", err)
    assert np.all(np.isfinite(got)) and err <= TOL, err

    far = dict(x, q=x["q"] * np.float32(2000.0))
    above = exact(far)[1].transpose(0, 2, 1) > 89   # [B,I,H]
    assert above.any()
    assert np.all(np.isfinite(np.array(m.call("out", far))))
    m.fuse_attention_stable(False)
    assert np.all(np.isnan(np.array(m.call("out", far))[above])), "as written, a row with a score above 89 is NaN"
    assert np.array_equal(np.array(m.call("out", x)).view(np.uint32), base.view(np.uint32)), "off: the bits of a model that never touched the switch"
    untouched.close()
    m.close()
