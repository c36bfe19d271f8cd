"""CPU-side checks of the two-pass eigen-solver's interface (ll_lanczos_two_pass_*, ll_recur_accum_*): the symbols are declared
and exported, the two statistics came out of ll_run_stats' reserved tail without moving anything, and the ABI minor is unchanged.
No device compute here."""
import ctypes as C
import re

import numpy as np

import lambda_lanczos_amd as L
from lambda_lanczos_amd import _capi as capi

SYMBOLS = ["ll_lanczos_two_pass_" + s for s in "dzsc"] + ["ll_recur_accum_" + s for s in "dzsc"]


def test_symbols_are_declared_exported_and_bound():
    with open(capi.HEADER_PATH) as f:
        text = f.read()
    declared = set(re.findall(r"^\s*int\s+(ll_[a-z0-9_]+)\s*\(", text, flags=re.M))
    lib = capi.lib()
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in capi.PROTOTYPES, name
    # one prototype per family: the float forms mirror the double ones
    assert capi.PROTOTYPES["ll_lanczos_two_pass_s"] == capi.PROTOTYPES["ll_lanczos_two_pass_d"]
    assert capi.PROTOTYPES["ll_recur_accum_c"] == capi.PROTOTYPES["ll_recur_accum_z"]
    assert len(capi.PROTOTYPES["ll_lanczos_two_pass_d"][1]) == 10 and len(capi.PROTOTYPES["ll_recur_accum_d"][1]) == 9
    assert callable(L.recur_accum) and callable(L.LambdaLanczos.run_two_pass)


def test_run_stats_keeps_its_size_and_the_abi_minor():
    assert C.sizeof(capi.RunStats) == 23 * 8          # 17 statistics + reserved[6] before; 19 + reserved[4] now
    names = [k for k, _ in capi.RunStats._fields_]
    assert names[-3:] == ["workspace_vectors", "replay_mismatches", "reserved"]
    assert capi.RunStats.workspace_vectors.offset == 17 * 8 and capi.RunStats.replay_mismatches.offset == 18 * 8
    assert capi.RunStats.pair_gate_trips.offset == 16 * 8          # nothing in front of them moved
    st = capi.RunStats()
    assert set(["workspace_vectors", "replay_mismatches"]) <= set(st.as_dict()) and "reserved" not in st.as_dict()
    lib = capi.lib()
    assert lib.ll_version() == 5 and capi.ABI_VERSION == (0, 5)
    assert lib.ll_abi_check(0, 5, C.sizeof(capi.RunStats), C.sizeof(capi.LanczosParams)) == capi.LL_OK
    with open(capi.HEADER_PATH) as f:
        text = f.read()
    body = text[text.index("typedef struct ll_run_stats {"):text.index("} ll_run_stats;")]
    fields = re.findall(r"^\s*(?:int64_t|double)\s+([a-z_0-9]+)(\[\d+\])?;", body, flags=re.M)
    assert [f[0] for f in fields] == names and fields[-1][1] == "[4]"
    assert "#define LL_VERSION_MINOR 5" in text


def test_null_arguments_are_refused_without_a_device():
    lib = capi.lib()
    val = C.c_double()
    assert lib.ll_lanczos_two_pass_d(None, None, None, C.byref(val), None, None, None, None, None, None) == capi.LL_ERR_INVALID
    assert lib.ll_recur_accum_d(None, 4, None, None, None, 0.0, 0.0, 0.0, None) == capi.LL_ERR_INVALID
    assert np.isfinite(val.value)
