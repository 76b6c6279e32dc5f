"""Batch-invariant mode, what needs no GPU: the four C-ABI symbols (declared, exported, prototyped), the refusal of null
handles and bad values, and the parsing of the batch_invariant option / PEPPER_AMD_BATCH_INVARIANT."""
import ctypes
import os
import re

import pytest

from pepper_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pa_variant_set_batch_invariant", "pa_variant_get_batch_invariant",
       "pa_polish_set_batch_invariant", "pa_polish_get_batch_invariant")


def test_symbols_declared_exported_and_prototyped():
    header = open(os.path.join(REPO, "include", "pepper_amd.h")).read()
    protos = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(lib, name), name
        res, args = protos[name]
        assert res is ctypes.c_int and len(args) == 2, name
    assert protos["pa_variant_set_batch_invariant"][1][1] is ctypes.c_int32
    assert protos["pa_variant_get_batch_invariant"][1][1] is ctypes.POINTER(ctypes.c_int32)


def test_null_and_foreign_handles_are_refused():
    lib = _lib.load()
    v = ctypes.c_int32(7)
    junk = ctypes.create_string_buffer(256)          # no handle's magic word
    for setter, getter in (("pa_variant_set_batch_invariant", "pa_variant_get_batch_invariant"),
                           ("pa_polish_set_batch_invariant", "pa_polish_get_batch_invariant")):
        assert getattr(lib, setter)(None, 1) == _lib.PA_ERR_INVALID
        assert getattr(lib, getter)(None, ctypes.byref(v)) == _lib.PA_ERR_INVALID
        assert getattr(lib, setter)(ctypes.cast(junk, ctypes.c_void_p), 1) == _lib.PA_ERR_INVALID
        assert getattr(lib, getter)(ctypes.cast(junk, ctypes.c_void_p), ctypes.byref(v)) == _lib.PA_ERR_INVALID
        assert b"handle" in lib.pa_last_error()
    assert v.value == 7


@pytest.mark.parametrize("value, want", [(None, False), (False, False), (True, True), (0, False), (1, True),
                                         ("", False), ("0", False), ("1", True), ("true", True), ("FALSE", False),
                                         ("on", True), ("off", False), ("yes", True), (" no ", False)])
def test_option_parsing(value, want):
    assert _lib.parse_batch_invariant(value) is want


@pytest.mark.parametrize("value", ["2", "maybe", 2, -1])
def test_option_parsing_refuses_the_unknown(value):
    with pytest.raises(ValueError):
        _lib.parse_batch_invariant(value)


def test_environment_default(monkeypatch):
    monkeypatch.delenv(_lib.BATCH_INVARIANT_ENV, raising=False)
    assert _lib.batch_invariant_default() is False
    assert _lib.batch_invariant_default(True) is True
    monkeypatch.setenv(_lib.BATCH_INVARIANT_ENV, "1")
    assert _lib.batch_invariant_default() is True
    assert _lib.batch_invariant_default(False) is False     # an explicit option wins over the environment
    monkeypatch.setenv(_lib.BATCH_INVARIANT_ENV, "0")
    assert _lib.batch_invariant_default() is False
    monkeypatch.setenv(_lib.BATCH_INVARIANT_ENV, "bogus")
    with pytest.raises(ValueError):
        _lib.batch_invariant_default()


def test_wrappers_take_the_option_and_the_environment(monkeypatch):
    """The wrappers read the option (and the environment) at construction; no device is needed for that."""
    from pepper_amd.polish.models.simple_model import TransducerGRU as PolishModel
    from pepper_amd.variant.models.simple_model import TransducerGRU as VariantModel
    monkeypatch.delenv(_lib.BATCH_INVARIANT_ENV, raising=False)
    assert VariantModel(26, 1, 128, 28, 3, device=0).batch_invariant is False
    assert VariantModel(26, 1, 128, 28, 3, device=0, batch_invariant=True).batch_invariant is True
    assert PolishModel(1, 10, 1, 128, 5, device=0).batch_invariant is False
    assert PolishModel(1, 10, 1, 128, 5, device=0, batch_invariant=True).batch_invariant is True
    monkeypatch.setenv(_lib.BATCH_INVARIANT_ENV, "1")
    assert VariantModel(26, 1, 128, 28, 3, device=0).batch_invariant is True
    assert PolishModel(1, 10, 1, 128, 5, device=0).batch_invariant is True
    # an explicit False is not overridden by the environment
    assert VariantModel(26, 1, 128, 28, 3, device=0, batch_invariant=False).batch_invariant is False
    assert PolishModel(1, 10, 1, 128, 5, device=0, batch_invariant=False).batch_invariant is False
    from pepper_amd.polish.models.ModelHander import ModelHandler as PolishHandler
    from pepper_amd.variant.models.ModelHander import ModelHandler as VariantHandler
    assert VariantHandler.get_new_gru_model(26, 1, 128, 28, 3).batch_invariant is True
    assert VariantHandler.get_new_gru_model(26, 1, 128, 28, 3, batch_invariant=False).batch_invariant is False
    assert PolishHandler.get_new_gru_model(1, 10, 1, 128, 5).batch_invariant is True
    assert PolishHandler.get_new_gru_model(1, 10, 1, 128, 5, batch_invariant=False).batch_invariant is False
