"""eg_attention_stable, eg_attention_stable_grad and eg_model_fuse_attention_stable at the drop-in boundary, without a device:
the built library exports them, include/exprgrad_hip.h declares them with the operands of their as-written neighbours (Stats,
lds and its strides in place of Sums and its strides), exprgrad_amd binds and wraps them, and the refusals that are decided
before any device work return their codes.  The refusals that need a context are in tests/test_gpu_attention_stable.py."""
import ctypes
import subprocess

from test_attention_cabi import EG_ERR_INVALID, declaration

STATS = ["float* Stats", "int64_t lds", "int64_t stride_s0", "int64_t stride_s1"]
BIAS = ["const float* Bias", "int64_t ldb", "int64_t stride_b0", "int64_t stride_b1"]


def test_declared_like_their_neighbours():
    forward, grad = declaration("eg_attention_stable"), declaration("eg_attention_stable_grad")
    assert forward == declaration("eg_attention") + STATS + BIAS
    neighbour = declaration("eg_attention_bias_grad")
    at = neighbour.index("const float* Sums")
    assert grad == neighbour[:at] + ["const " + STATS[0]] + STATS[1:] + neighbour[at + 3:]
    assert declaration("eg_model_fuse_attention_stable") == ["eg_model* model", "int on"]


def test_exported_bound_and_wrapped():
    from exprgrad_amd import _lib, ops
    from exprgrad_amd import model as egm
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name, count in (("eg_attention_stable", 33), ("eg_attention_stable_grad", 49), ("eg_model_fuse_attention_stable", 2)):
        assert name in exported and name in _lib.declared_symbols()
        assert len(getattr(_lib.lib(), name).argtypes) == count == len(declaration(name))
    assert callable(ops.attention_stable) and callable(ops.attention_stable_grad)
    assert egm.Model.fuse_attention_stable.__defaults__ == (True,)


def test_refused_without_a_device():
    from exprgrad_amd import _lib
    lib, null = _lib.lib(), ctypes.c_void_p(0)
    v = (null, 1, 2, 1)
    assert lib.eg_attention_stable(null, 2, 2, 1, 1, 1, 1, 0.125, *v, *v, *v, *v, 0, *v, *v) == EG_ERR_INVALID
    assert "eg_attention_stable:" in _lib.last_error()
    assert lib.eg_attention_stable_grad(null, 2, 2, 1, 1, 1, 1, 0.125, *v, *v, *v, *v, *v, *v, *v, *v, *v, 0, *v) == EG_ERR_INVALID
    assert "eg_attention_stable_grad:" in _lib.last_error()
    for on in (0, 1):
        assert lib.eg_model_fuse_attention_stable(None, on) == EG_ERR_INVALID
        assert "eg_model_fuse_attention_stable" in _lib.last_error()
