"""eg_attention_grad_f64 at the drop-in boundary, without a device: declared directly after eg_attention_grad with the same 44
arguments in doubles, exported, bound and wrapped; a NULL context is EG_ERR_INVALID with a message that names the entry.  The
refusals that need a context are in tests/test_gpu_attention_grad_f64.py."""
import ctypes
import subprocess

from exprgrad_amd import _lib, ops
from test_attention_cabi import EG_ERR_INVALID, HEADER, declaration


def test_declared_after_eg_attention_grad_with_its_arguments_in_doubles():
    got = declaration("eg_attention_grad_f64")
    assert len(got) == 44 and got == [x.replace("float", "double") for x in declaration("eg_attention_grad")] and "double scale" in got
    text = open(HEADER).read()
    between = text[text.index("int eg_attention_grad("):text.index("int eg_attention_grad_f64(")]
    assert "\nint " not in between      # no other declaration in between


def test_exported_bound_wrapped_and_a_null_context_refused():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert "eg_attention_grad_f64" in {line.split()[-1] for line in out.splitlines() if " T " in line} and "eg_attention_grad_f64" in _lib.declared_symbols()
    argtypes = _lib.lib().eg_attention_grad_f64.argtypes
    assert len(argtypes) == 44 and argtypes[7] is ctypes.c_double and callable(ops.attention_grad_f64)
    null = ctypes.c_void_p(0)
    args = (null, 2, 2, 1, 1, 1, 1, 0.125) + (null, 1, 2, 1) * 4 + (null, 2, 1) + (null, 1, 2, 1) * 4 + (0,)
    assert _lib.lib().eg_attention_grad_f64(*args) == EG_ERR_INVALID and "eg_attention_grad_f64" in _lib.last_error()
