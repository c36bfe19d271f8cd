"""The typed entry points of the C ABI (every ll_*_d / _z / _s / _c of include/lanczos_hip.h) refuse a call whose arguments are
all null / zero with LL_ERR_INVALID before they touch a device, and the four storage types of one family refuse it with the same
words: the first argument check of a family is the same code whatever the type.  No device compute here."""
import ctypes as C

import pytest

from lambda_lanczos_amd import _capi as capi

SUFFIXES = ("_d", "_z", "_s", "_c")

# family -> what ll_last_error() says after the all-null call (the first check each family makes)
NULL_CONTEXT, NULL_ARGUMENT, NULL_CALLBACK, BAD_ARGUMENT = (
    "invalid argument: null context", "invalid argument: null argument", "invalid argument: null callback",
    "invalid argument: bad argument")
MESSAGES = {
    "ll_op_create_csr": NULL_CONTEXT,
    "ll_op_create_csr_dev": NULL_CONTEXT,
    "ll_op_create_csr_opt": NULL_CONTEXT,
    "ll_op_create_csr_sym": NULL_CONTEXT,
    "ll_op_create_coo": BAD_ARGUMENT,
    "ll_op_create_dense": NULL_CONTEXT,
    "ll_op_create_stencil": NULL_CONTEXT,
    "ll_op_create_pauli": NULL_CONTEXT,
    "ll_op_create_pauli_sector": NULL_CONTEXT,
    "ll_op_create_pauli_momentum": NULL_CONTEXT,
    "ll_op_create_pauli_momentum_full": NULL_CONTEXT,
    "ll_op_create_pauli_symmetric": NULL_CONTEXT,
    "ll_op_create_host": NULL_CALLBACK,
    "ll_op_create_device": NULL_CALLBACK,
    "ll_spmv": NULL_CONTEXT,
    "ll_dot": NULL_CONTEXT,
    "ll_nrm2": NULL_CONTEXT,
    "ll_scal": NULL_CONTEXT,
    "ll_normalize": NULL_CONTEXT,
    "ll_three_term": NULL_CONTEXT,
    "ll_recur_accum": NULL_CONTEXT,
    "ll_orth_block": NULL_CONTEXT,
    "ll_gemv_basis": NULL_CONTEXT,
    "ll_lanczos_run": NULL_ARGUMENT,
    "ll_lanczos_run_iteration": NULL_ARGUMENT,
    "ll_lanczos_two_pass": NULL_ARGUMENT,
    "ll_expo_run": NULL_ARGUMENT,
    "ll_expo_taylor_run": NULL_ARGUMENT,
}


def _typed_names():
    return sorted(n for n in capi.PROTOTYPES if n.endswith(SUFFIXES) and n != "ll_memcpy_h2d")


def _null(argtype):
    if issubclass(argtype, C._CFuncPtr):
        return argtype()  # a null callback
    if issubclass(argtype, (C._Pointer, C.c_void_p, C.c_char_p)):
        return None
    return 0.0 if argtype is C.c_double else 0


def test_every_typed_family_exists_in_all_four_storage_types():
    names = _typed_names()
    assert len(names) == 112
    families = {}
    for n in names:
        families.setdefault(n[:-2], set()).add(n[-2:])
    assert len(families) == 28 and set(families) == set(MESSAGES), set(families) ^ set(MESSAGES)
    for fam, sfx in families.items():
        assert sfx == set(SUFFIXES), (fam, sfx)


@pytest.mark.parametrize("family", sorted(MESSAGES))
def test_all_null_call_is_refused_alike_by_the_four_types(family):
    lib = capi.lib()
    texts = {}
    for sfx in SUFFIXES:
        res, argtypes = capi.PROTOTYPES[family + sfx]
        assert res is C.c_int
        assert lib.ll_partition(-1, 0, 0, None, None) == capi.LL_ERR_INVALID  # another text: what is read below is this call's
        status = getattr(lib, family + sfx)(*[_null(t) for t in argtypes])
        texts[sfx] = lib.ll_last_error().decode()
        assert status == capi.LL_ERR_INVALID, (family + sfx, status, texts[sfx])
    assert len(set(texts.values())) == 1, texts
    assert texts["_d"] == MESSAGES[family], texts
