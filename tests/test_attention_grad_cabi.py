"""eg_attention_sums and eg_attention_grad at the drop-in boundary, without a device: the built library exports them,
include/exprgrad_hip.h declares them with their argument lists behind eg_attention, exprgrad_amd._lib binds them and
exprgrad_amd.ops wraps them; a NULL context is refused with a message that names the entry before anything touches a device.
The refusals that need a context are in tests/test_gpu_attention_grad.py::test_error_returns."""
import ctypes
import subprocess

from test_attention_cabi import EG_ERR_INVALID, HEADER, declaration


def operand(name, ld, s, const=True):
    return ["%sfloat* %s" % ("const " if const else "", name), "int64_t " + ld, "int64_t stride_%s0" % s, "int64_t stride_%s1" % s]


HEAD = ["eg_ctx* ctx", "int64_t batch0", "int64_t batch1", "int64_t I", "int64_t J", "int64_t K", "int64_t D", "float scale"]
INPUTS = operand("Q", "ldq", "q") + operand("Kk", "ldk", "k") + operand("V", "ldv", "v")


def test_sums_is_declared_with_attentions_arguments_and_the_sums_view():
    d = declaration("eg_attention_sums")
    assert d[:25] == declaration("eg_attention")
    assert d[25:] == ["float* Sums", "int64_t stride_s0", "int64_t stride_s1"]


def test_grad_is_declared_with_nine_operands():
    d = declaration("eg_attention_grad")
    assert len(d) == 8 + 4 * 4 + 3 + 4 * 4 + 1
    assert d[:8] == HEAD and d[8:20] == INPUTS
    assert d[20:24] == operand("O", "ldo", "o")
    assert d[24:27] == ["const float* Sums", "int64_t stride_s0", "int64_t stride_s1"]
    assert d[27:31] == operand("dO", "lddo", "do")
    assert d[31:43] == operand("dQ", "lddq", "dq", False) + operand("dK", "lddk", "dk", False) + operand("dV", "lddv", "dv", False)
    assert d[43:] == ["int accumulate"]


def test_the_header_states_both_contracts_behind_the_forward():
    text = open(HEADER).read()
    forward, sums, grad = text.index("int eg_attention("), text.index("int eg_attention_sums("), text.index("int eg_attention_grad(")
    assert forward < sums < grad
    doc = text[forward:sums]
    for phrase in ("Sums == NULL is eg_attention", "always overwritten", "batched2_c_distinct", "never written", "names eg_attention_sums"):
        assert phrase in doc, phrase
    doc = text[sums:grad]
    for phrase in ("delta_i = dO_i . o_i", "dS_ij = scale * p_ij * (dP_ij - delta_i)", "nothing of size", "bit 0 adds to dQ", "batched2_c_distinct",
                   "EG_ERR_UNSUPPORTED", "K > 128 or D > 128", "two calls give the same bits", "never the split-bf16 route", "not finite",
                   "unspecified", "contributes exactly 0"):
        assert phrase in doc, phrase


def test_exported_bound_and_wrapped():
    from exprgrad_amd import _lib, ops
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name, count in (("eg_attention_sums", 28), ("eg_attention_grad", 44)):
        assert name in exported and name in _lib.declared_symbols()
        argtypes = getattr(_lib.lib(), name).argtypes
        assert len(argtypes) == count and argtypes[7] is ctypes.c_float and argtypes[count - 1] is (ctypes.c_int64 if count == 28 else ctypes.c_int)
    assert _lib.lib().eg_attention_sums.argtypes[24] is ctypes.c_int
    assert callable(ops.attention_sums) and callable(ops.attention_grad)


def test_null_context_is_refused_without_a_device():
    from exprgrad_amd import _lib
    null = ctypes.c_void_p(0)
    view = [null, 1, 2, 1]
    some = ctypes.c_void_p(64)      # never dereferenced: the context is looked at first
    rc = _lib.lib().eg_attention_sums(null, 2, 2, 1, 1, 1, 1, 0.125, *(view * 4 + [0, some, 2, 1]))
    assert rc == EG_ERR_INVALID and "eg_attention_sums" in _lib.last_error(), _lib.last_error()
    rc = _lib.lib().eg_attention_sums(null, 2, 2, 1, 1, 1, 1, 0.125, *(view * 4 + [0, null, 0, 0]))
    assert rc == EG_ERR_INVALID and "eg_attention:" in _lib.last_error(), _lib.last_error()      # Sums == NULL is eg_attention
    rc = _lib.lib().eg_attention_grad(null, 2, 2, 1, 1, 1, 1, 0.125, *(view * 4 + [null, 2, 1] + view * 4 + [0]))
    assert rc == EG_ERR_INVALID and "eg_attention_grad" in _lib.last_error(), _lib.last_error()
