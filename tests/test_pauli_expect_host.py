"""CPU-side checks of the expectation-value feature (ll_pauli_expect): the host reference generators.pauli_string_apply_np — P psi
by permutation and sign — against the matrix of the one-term operator (generators.pauli_csr / pauli_sector_csr), and the
all-null call, which the library refuses before it touches a device."""
import ctypes as C

import numpy as np
import pytest

import contract_cases as K
from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G
from util import csr_matvec


def _strings(n_sites, rng, count):
    m = (1 << n_sites) - 1
    out = [(0, 0, 1.0), (m, 0, 1.0), (0, m, 1.0), (m, m, 1.0)]
    out += [(int(rng.integers(0, m + 1)), int(rng.integers(0, m + 1)), 1.0) for _ in range(count)]
    return out


@pytest.mark.parametrize("n_sites", [1, 2, 5, 8])
@pytest.mark.parametrize("dtype", [np.float64, np.complex128, np.float32, np.complex64], ids=["d", "z", "s", "c"])
def test_string_apply_is_the_one_term_matrix(n_sites, dtype):
    rng = np.random.default_rng(n_sites)
    psi = K.start_x(1 << n_sites, dtype)
    wide = np.complex128
    for term in _strings(n_sites, rng, 12):
        q = G.pauli_string_apply_np(n_sites, term, psi)
        ny = bin(term[0] & term[1]).count("1")
        assert q.dtype == (psi.dtype if ny % 2 == 0 else np.result_type(psi.dtype, np.complex64))
        want = csr_matvec(G.pauli_csr(n_sites, [term], wide, merge=False), psi.astype(wide))
        assert np.array_equal(q.astype(wide), want), term   # a permutation, a sign and i^nY: exact
        # the coefficient plays no part
        assert np.array_equal(G.pauli_string_apply_np(n_sites, (term[0], term[1], -3.5), psi), q)


@pytest.mark.parametrize("n_sites,n_down", [(1, 0), (4, 2), (6, 0), (6, 6), (7, 3), (9, 4)])
def test_string_apply_on_a_sector_is_the_sector_block(n_sites, n_down):
    rng = np.random.default_rng(n_sites * 31 + n_down)
    states = G.sector_states(n_sites, n_down)
    psi = K.start_x(states.shape[0], np.complex128)
    for term in _strings(n_sites, rng, 12):
        q = G.pauli_string_apply_np(n_sites, term, psi, states=states)
        rp, ci, va = G.pauli_sector_csr(n_sites, n_down, [term], np.complex128, merge=False)
        want = csr_matvec((rp, ci, va), psi) if ci.size else np.zeros_like(psi)
        assert np.array_equal(q, want), term
        if bin(term[0]).count("1") % 2:
            assert not np.any(q)   # an odd number of flips leaves the sector


def test_string_apply_refuses_bad_input():
    with pytest.raises(ValueError):
        G.pauli_string_apply_np(3, (8, 0, 1.0), np.zeros(8))
    with pytest.raises(ValueError):
        G.pauli_string_apply_np(3, (1, 0, 1.0), np.zeros(7))


def test_all_null_call_is_refused_before_a_device_is_touched():
    """No context, no operator: LL_ERR_INVALID with the wording of the other entry points — on a machine without a GPU too,
    where anything that touched the device would answer LL_ERR_HIP."""
    lib = capi.lib()
    sweeps = C.c_int64(-7)
    st = lib.ll_pauli_expect(None, None, 0, None, None, None, C.byref(sweeps))
    assert st == capi.LL_ERR_INVALID and b"null argument" in lib.ll_last_error()
    assert sweeps.value == -7
    st = lib.ll_pauli_expect(None, None, 3, None, None, None, None)
    assert st == capi.LL_ERR_INVALID and b"null argument" in lib.ll_last_error()
