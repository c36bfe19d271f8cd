"""CPU-side checks of the multi-time two-pass Exponentiator's surface: ll_expo_two_pass_multi and ll_recur_accum_multi are declared
in include/lanczos_hip.h, exported by the library and bound in the ctypes table; they are untyped additions within ABI minor 5 (no
struct changed size, ll_version() is what it was); an all-null call is refused before any device call; the Python methods have the
documented signatures.  No device compute here."""
import ctypes as C
import inspect
import re

import lambda_lanczos_amd as L
from lambda_lanczos_amd import _capi as capi

NAMES = ("ll_expo_two_pass_multi", "ll_recur_accum_multi")
TYPED_SUFFIXES = ("_d", "_z", "_s", "_c")


def _null(argtype):
    if issubclass(argtype, (C._Pointer, C.c_void_p, C.c_char_p)):
        return None
    return 0.0 if argtype is C.c_double else 0


def test_both_entry_points_are_declared_exported_and_bound():
    with open(capi.HEADER_PATH) as f:
        text = f.read()
    declared = set(re.findall(r"^\s*int\s+(ll_[a-z0-9_]+)\s*\(", text, flags=re.M))
    lib = capi.lib()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in capi.PROTOTYPES, name
        assert not name.endswith(TYPED_SUFFIXES), name   # untyped: the typed families keep their count
    preamble = text[:text.index("enum {")]
    assert "additive under minor 5" in preamble and all(name in preamble for name in NAMES)
    assert re.search(r"enum\s*\{\s*LL_EXPO_MULTI_MAX\s*=\s*16\s*\}", text) and capi.EXPO_MULTI_MAX == 16
    assert len(capi.PROTOTYPES["ll_expo_two_pass_multi"][1]) == 9 and len(capi.PROTOTYPES["ll_recur_accum_multi"][1]) == 11


def test_all_null_calls_are_refused_before_any_device_call():
    lib = capi.lib()
    for name, text in (("ll_expo_two_pass_multi", "invalid argument: null argument"),
                       ("ll_recur_accum_multi", "invalid argument: null context")):
        res, argtypes = capi.PROTOTYPES[name]
        assert res is C.c_int
        assert lib.ll_partition(-1, 0, 0, None, None) == capi.LL_ERR_INVALID   # another text: what is read below is this call's
        assert getattr(lib, name)(*[_null(t) for t in argtypes]) == capi.LL_ERR_INVALID
        assert lib.ll_last_error().decode() == text


def test_the_abi_is_still_minor_five_with_the_same_structs():
    lib = capi.lib()
    assert lib.ll_version() == 5 and capi.ABI_VERSION == (0, 5)
    assert C.sizeof(capi.RunStats) == 8 * 23
    assert C.sizeof(capi.ExpoParams) == 40
    assert lib.ll_abi_check(0, 5, C.sizeof(capi.RunStats), C.sizeof(capi.LanczosParams)) == capi.LL_OK


def test_the_python_methods_exist():
    assert list(inspect.signature(L.Exponentiator.run_two_pass_multi).parameters) == ["self", "a", "input", "out"]
    assert list(inspect.signature(L.Exponentiator.run_two_pass).parameters) == ["self", "a", "input", "out"]
    assert list(inspect.signature(L.recur_accum_multi).parameters) == ["ctx", "y_dev", "x_dev", "p_dev", "a", "b", "g_list", "psi_list", "n"]
