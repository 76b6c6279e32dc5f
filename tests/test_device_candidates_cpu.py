"""The device-candidates switch without a GPU: the environment variable parses as its siblings do, and the entry points are
declared in the header, bound in _lib.py and named the same in both."""
import os
import re

from pepper_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pa_encoder_set_device_candidates", "pa_encoder_candidate_calls")


def test_environment_switch(monkeypatch):
    assert _lib.DEVICE_CANDIDATES_ENV == "PEPPER_AMD_DEVICE_CANDIDATES"
    monkeypatch.delenv(_lib.DEVICE_CANDIDATES_ENV, raising=False)
    assert _lib.device_candidates() is False                   # off unless asked for
    for value, want in (("1", True), ("0", False), ("", False)):
        monkeypatch.setenv(_lib.DEVICE_CANDIDATES_ENV, value)
        assert _lib.device_candidates() is want
    # its siblings read their variables the same way: "0" is off, "1" is on
    for env, fn in ((_lib.DEVICE_SAMPLING_ENV, _lib.device_sampling), (_lib.DEVICE_LONG_CIGARS_ENV, _lib.device_long_cigars)):
        for value, want in (("1", True), ("0", False)):
            monkeypatch.setenv(env, value)
            assert fn() is want


def test_entry_points_declared_and_bound():
    header = open(os.path.join(REPO, "include", "pepper_amd_encoder.h")).read()
    bound = {name: (restype, argtypes) for name, restype, argtypes in _lib.SYMBOLS}
    for name in ENTRY_POINTS:
        assert re.search(r"\bint " + name + r"\(pa_encoder\* e,", header), name
        assert name in bound and bound[name][1][0] is _lib.c_void_p
    assert bound["pa_encoder_set_device_candidates"][1] == [_lib.c_void_p, _lib.c_int32]
    assert len(bound["pa_encoder_candidate_calls"][1]) == 3
    assert "[12] the device enumeration" in header            # the timing slot is appended, the others keep their numbers


def test_python_surface():
    from pepper_amd.variant import PEPPER_VARIANT as pv
    assert callable(pv.set_device_candidates) and callable(pv.candidate_calls)
    for cls in (pv.PackedEncoder, pv.RegionalSummaryGenerator):
        assert callable(getattr(cls, "set_device_candidates"))
    assert callable(pv.PackedEncoder.candidate_calls)
