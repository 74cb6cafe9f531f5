"""eg_dgemm_batched2 and eg_model_batched2_f64 at the drop-in boundary, without a device: the built library exports them,
include/exprgrad_hip.h declares them (eg_dgemm_batched2 with the argument list of eg_sgemm_batched2 over double),
exprgrad_amd._lib binds them, exprgrad_amd.ops and Model wrap them.  Every EG_ERR_INVALID case of the header is refused
with a message that names the entry, and empty calls return EG_OK, before anything touches a device: the context of these
calls is a zeroed block of host memory that no refused or empty call may look into, and C is a poisoned host buffer that
stays as it was."""
import ctypes
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "exprgrad_hip.h")
EG_OK, EG_ERR_INVALID = 0, 1
POISON = -777.25


def declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text)
    assert m, name + " is not declared in the header"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_declared_like_the_float32_form():
    d, s = declaration("eg_dgemm_batched2"), declaration("eg_sgemm_batched2")
    assert len(d) == 22 and d == [a.replace("float", "double") for a in s]
    assert d[3:8] == ["int64_t batch0", "int64_t batch1", "int64_t M", "int64_t N", "int64_t K"] and d[-1] == "const double* bias"
    assert declaration("eg_model_batched2_f64") == ["eg_model* model", "int on"]


def test_exported_and_bound():
    from exprgrad_amd import _lib, ops
    from exprgrad_amd.model import Model
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in ("eg_dgemm_batched2", "eg_model_batched2_f64"):
        assert name in exported and name in _lib.declared_symbols()
    assert len(_lib.lib().eg_dgemm_batched2.argtypes) == len(_lib.lib().eg_sgemm_batched2.argtypes) == 22
    assert callable(ops.dgemm_batched2) and callable(Model.batched2_f64)


def raw(ctx, b0=2, b1=3, M=8, N=8, K=8, A=None, lda=8, sa=(192, 64), B=None, ldb=8, sb=(192, 64), C=None, ldc=8, sc=(192, 64), ta=0, tb=0):
    from exprgrad_amd import _lib
    p = lambda x: ctypes.c_void_p(x)
    return _lib.lib().eg_dgemm_batched2(p(ctx), ta, tb, b0, b1, M, N, K, p(A), lda, sa[0], sa[1], p(B), ldb, sb[0], sb[1], p(C), ldc, sc[0],
                                        sc[1], 0, p(0))


def test_every_invalid_argument_is_refused_by_name():
    from exprgrad_amd import _lib
    ctx = ctypes.create_string_buffer(4096)
    c = np.full(2 * 3 * 8 * 8, POISON)
    ok = dict(ctx=ctypes.addressof(ctx), A=c.ctypes.data, B=c.ctypes.data, C=c.ctypes.data)
    bad = {
        "NULL ctx": dict(ctx=0),
        "negative batch0": dict(b0=-1), "negative batch1": dict(b1=-1), "negative M": dict(M=-1), "negative N": dict(N=-1), "negative K": dict(K=-1),
        "batch0 of 2^31": dict(b0=1 << 31), "batch1 of 2^31": dict(b1=1 << 31),
        "NULL C": dict(C=0), "NULL A": dict(A=0), "NULL B": dict(B=0),
        "lda below K": dict(lda=7), "ldb below N": dict(ldb=7), "lda below M, transposed": dict(ta=1, M=9, lda=8, sc=(216, 72)),
        "ldb below K, transposed": dict(tb=1, K=9, lda=9, sa=(216, 72), ldb=8),
        "negative stride_a0": dict(sa=(-192, 64)), "negative stride_a1": dict(sa=(192, -64)),
        "negative stride_b0": dict(sb=(-192, 64)), "negative stride_b1": dict(sb=(192, -64)),
        "ldc below N": dict(ldc=7), "items of C overlap": dict(sc=(192, 63)), "outer items of C overlap": dict(sc=(191, 64)),
        "stride_c0 == stride_c1": dict(sc=(64, 64)), "stride_c1 of 0": dict(sc=(192, 0)), "stride_c0 of 0": dict(sc=(0, 64)),
        "interleaved C one short": dict(ldc=24, sc=(192, 7)), "negative stride_c1": dict(sc=(192, -64)), "negative stride_c0": dict(sc=(-192, 64)),
    }
    for name, change in bad.items():
        assert raw(**dict(ok, **change)) == EG_ERR_INVALID, name
        assert "eg_dgemm_batched2" in _lib.last_error(), (name, _lib.last_error())
    assert np.all(c == POISON) and ctx.raw == bytes(4096)


def test_empty_calls_succeed():
    from exprgrad_amd import _lib
    ctx = ctypes.create_string_buffer(4096)
    c = np.full(2 * 3 * 8 * 8, POISON)
    ok = dict(ctx=ctypes.addressof(ctx), A=c.ctypes.data, B=c.ctypes.data, C=c.ctypes.data)
    for change in (dict(b0=0), dict(b1=0), dict(M=0), dict(N=0), dict(b0=0, A=0, B=0, C=0), dict(M=0, A=0, B=0, C=0),
                   dict(N=0, ldc=0, sc=(0, 0))):     # (an empty product's C is never addressed: its strides are not looked at)
        assert raw(**dict(ok, **change)) == EG_OK, (change, _lib.last_error())
    assert np.all(c == POISON) and ctx.raw == bytes(4096)


def test_the_model_setting_refuses_a_null_model():
    from exprgrad_amd import _lib
    assert _lib.lib().eg_model_batched2_f64(ctypes.c_void_p(0), 1) == EG_ERR_INVALID
    assert "eg_model_batched2_f64" in _lib.last_error()
