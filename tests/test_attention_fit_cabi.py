"""eg_model_fuse_attention_fit at the drop-in boundary, without a device: the built library exports it, include/exprgrad_hip.h
declares it behind eg_model_keep_values and says what forms, what is refused and that the default is off, exprgrad_amd._lib
binds it, and a NULL model is refused before anything touches a device."""
from exprgrad_amd import _lib
from exprgrad_amd import model as egm
from test_attention_cabi import EG_ERR_INVALID, HEADER, declaration


def test_it_is_declared_like_keep_values():
    assert declaration("eg_model_fuse_attention_fit") == ["eg_model* model", "int on"] == declaration("eg_model_keep_values")
    text = open(HEADER).read()
    assert text.index("int eg_model_keep_values(") < text.index("int eg_model_fuse_attention_fit(")
    doc = text[text.index("int eg_model_keep_values("):text.index("int eg_model_fuse_attention_fit(")]
    for words in ("eg_attention_sums", "eg_attention_grad", "refused", "default is off", "EG_ERR_INVALID", "plan key"):
        assert words in doc, words


def test_a_null_model_is_refused():
    lib = _lib.lib()
    for on in (0, 1):
        assert lib.eg_model_fuse_attention_fit(None, on) == EG_ERR_INVALID
        assert b"NULL model" in lib.eg_last_error()


def test_python_binds_it_next_to_keep_values():
    assert _lib._SIGS["eg_model_fuse_attention_fit"] == _lib._SIGS["eg_model_keep_values"]
    assert callable(egm.Model.fuse_attention_fit)
    assert egm.Model.fuse_attention_fit.__defaults__ == (True,)
