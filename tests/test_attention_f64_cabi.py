"""eg_attention_f64, eg_attention_sums_f64 and eg_model_fuse_attention_f64 at the drop-in boundary, without a device: the
built library exports them, include/exprgrad_hip.h declares them (25 and 28 arguments, the scale a double),
exprgrad_amd._lib binds them and exprgrad_amd.ops wraps them; the refusals that come before anything touches a device — a
NULL context, a NULL model — return EG_ERR_INVALID with a message that names the entry.  The refusals that need a context
(a negative stride, an O that aliases itself, K = 129) are in tests/test_gpu_attention_f64.py::test_error_returns."""
import ctypes
import subprocess

from test_attention_cabi import EG_ERR_INVALID, HEADER, declaration

OPERAND = lambda t, x, ld, s: ["%s %s" % (t, x), "int64_t %s" % ld, "int64_t stride_%s0" % s, "int64_t stride_%s1" % s]
FIRST_25 = (["eg_ctx* ctx", "int64_t batch0", "int64_t batch1", "int64_t I", "int64_t J", "int64_t K", "int64_t D", "double scale"] +
            OPERAND("const double*", "Q", "ldq", "q") + OPERAND("const double*", "Kk", "ldk", "k") + OPERAND("const double*", "V", "ldv", "v") +
            OPERAND("double*", "O", "ldo", "o") + ["int accumulate"])


def test_declared_in_doubles_with_two_strides_per_operand():
    assert declaration("eg_attention_f64") == FIRST_25
    assert declaration("eg_attention_sums_f64") == FIRST_25 + ["double* Sums", "int64_t stride_s0", "int64_t stride_s1"]
    assert declaration("eg_model_fuse_attention_f64") == ["eg_model* model", "int on"]


def test_the_header_states_the_contract():
    text = open(HEADER).read()
    doc = text[text.index("eg_attention in float64"):text.index("int eg_attention_f64(")]
    for phrase in ("v_mfma_f64_16x16x4_f64", "without the row maximum", "EG_ERR_UNSUPPORTED", "batched2_c_distinct", "mean of V's rows",
                   "eg_dgemm_batched2", "The one departure", "two calls give the\n * same bits", "whatever batch it is part of"):
        assert phrase in doc, phrase
    doc = text[text.index("The forward attention chain of a compile[float64] model"):text.index("int eg_model_fuse_attention_f64(")]
    for phrase in ("eg_model_batched2_f64", "Turn both on", "a float32 model", "default is off"):
        assert phrase in doc, phrase


def test_exported_and_bound():
    from exprgrad_amd import _lib, ops
    from exprgrad_amd.model import Model
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name, n in (("eg_attention_f64", 25), ("eg_attention_sums_f64", 28), ("eg_model_fuse_attention_f64", 2)):
        assert name in exported and name in _lib.declared_symbols(), name
        assert len(getattr(_lib.lib(), name).argtypes) == n, name
    assert _lib.lib().eg_attention_f64.argtypes[7] is ctypes.c_double and _lib.lib().eg_attention_sums_f64.argtypes[7] is ctypes.c_double
    assert callable(ops.attention_f64) and callable(ops.attention_sums_f64) and callable(Model.fuse_attention_f64)


def test_null_context_is_refused_without_a_device():
    from exprgrad_amd import _lib
    null = ctypes.c_void_p(0)
    args = (null, 2, 2, 1, 1, 1, 1, 0.125, null, 1, 2, 1, null, 1, 2, 1, null, 1, 2, 1, null, 1, 2, 1, 0)
    assert _lib.lib().eg_attention_f64(*args) == EG_ERR_INVALID
    assert "eg_attention_f64" in _lib.last_error()
    sums = ctypes.c_void_p(4096)        # never dereferenced: the context is checked first
    assert _lib.lib().eg_attention_sums_f64(*(args + (sums, 2, 1))) == EG_ERR_INVALID
    assert "eg_attention_sums_f64" in _lib.last_error()
    # with Sums == NULL the entry is eg_attention_f64, and says so
    assert _lib.lib().eg_attention_sums_f64(*(args + (null, 2, 1))) == EG_ERR_INVALID
    assert "eg_attention_f64" in _lib.last_error() and "sums" not in _lib.last_error()


def test_a_null_model_is_refused():
    from exprgrad_amd import _lib
    assert _lib.lib().eg_model_fuse_attention_f64(ctypes.c_void_p(0), 1) == EG_ERR_INVALID
    assert "eg_model_fuse_attention_f64" in _lib.last_error()
