"""The K3 race entries of the C ABI: declared in include/mopa_hip.h, exported by the library, listed by the binding; the parameter
struct has the library's size and MopaPlanParams keeps its own; argument errors are status codes before anything touches a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RACE_SYMBOLS = ["mopa_plan_race_batch", "mopa_plan_race", "mopa_race_params_size"]


def test_race_symbols_are_declared_exported_and_bound():
    """fails on a library without the feature"""
    from mopa_rl_amd import _lib
    txt = open(os.path.join(ROOT, "include", "mopa_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(mopa_[a-z_0-9]+)\s*\(", txt))
    L = _lib.lib()
    for s in RACE_SYMBOLS:
        assert s in declared, f"{s} is not declared in include/mopa_hip.h"
        assert hasattr(L, s), f"{s} is not exported"
        assert s in _lib.EXPORTED_SYMBOLS
    assert "MopaRaceParams" in txt and "MopaPlanParams" in txt


def test_params_struct_layout_matches_the_library():
    from mopa_rl_amd import _lib
    assert _lib.lib().mopa_race_params_size() == C.sizeof(_lib.MopaRaceParams) == 56
    assert C.sizeof(_lib.MopaPlanParams) == 104           # the plain query's struct is not the race's


def test_argument_errors_are_status_codes():
    from mopa_rl_amd import _lib
    L = _lib.lib()
    prm = _lib.MopaRaceParams(10, 64, 8, 4, 0, 0, None, None, 0, 0)
    assert L.mopa_plan_race_batch(None, None, None, 0, C.byref(prm), None, None, None, None, None, None, None, None) == 1
    assert b"null" in L.mopa_last_error()
    assert L.mopa_plan_race(None, None, None, C.byref(prm), None, None, None, None, None, None, None) == 1
    assert L.mopa_plan_race_batch(None, None, None, 0, None, None, None, None, None, None, None, None, None) == 1
