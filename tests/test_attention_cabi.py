"""eg_attention at the drop-in boundary, without a device: the built library exports it, include/exprgrad_hip.h declares it
with its 25 arguments, exprgrad_amd._lib binds it and exprgrad_amd.ops wraps it; a NULL context is refused with a message
before anything touches a device.  The refusals that need a context (a negative stride, an O that aliases itself, K = 129)
are in tests/test_gpu_attention_fused.py::test_error_returns."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "exprgrad_hip.h")
EG_ERR_INVALID = 1


def declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text)
    assert m, name + " is not declared in the header"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_declared_with_two_strides_per_operand():
    d = declaration("eg_attention")
    assert len(d) == 25
    assert d[:8] == ["eg_ctx* ctx", "int64_t batch0", "int64_t batch1", "int64_t I", "int64_t J", "int64_t K", "int64_t D", "float scale"]
    assert d[8:12] == ["const float* Q", "int64_t ldq", "int64_t stride_q0", "int64_t stride_q1"]
    assert d[12:16] == ["const float* Kk", "int64_t ldk", "int64_t stride_k0", "int64_t stride_k1"]
    assert d[16:20] == ["const float* V", "int64_t ldv", "int64_t stride_v0", "int64_t stride_v1"]
    assert d[20:] == ["float* O", "int64_t ldo", "int64_t stride_o0", "int64_t stride_o1", "int accumulate"]


def test_the_header_states_the_contract():
    text = open(HEADER).read()
    doc = text[text.index("Fused attention forward"):text.index("int eg_attention(")]
    for phrase in ("without the row maximum", "O is not read", "EG_ERR_UNSUPPORTED", "batched2_c_distinct", "mean of V's rows", "dnn.nim:90-94",
                   "The one departure", "two calls give the same bits"):
        assert phrase in doc, phrase


def test_exported_and_bound():
    from exprgrad_amd import _lib, ops
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert "eg_attention" in {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "eg_attention" in _lib.declared_symbols()
    argtypes = _lib.lib().eg_attention.argtypes
    assert len(argtypes) == 25 and argtypes[7] is ctypes.c_float
    assert callable(ops.attention)


def test_null_context_is_refused_without_a_device():
    from exprgrad_amd import _lib
    null = ctypes.c_void_p(0)
    rc = _lib.lib().eg_attention(null, 2, 2, 1, 1, 1, 1, 0.125, null, 1, 2, 1, null, 1, 2, 1, null, 1, 2, 1, null, 1, 2, 1, 0)
    assert rc == EG_ERR_INVALID
    assert "eg_attention" in _lib.last_error()
