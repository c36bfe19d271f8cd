"""CPU-side checks of the reduced-density-matrix feature (ll_pauli_rdm): the host reference generators.reduced_density_matrix_np
against the DEFINITION by tomography — rho = 2^-m sum_P <P> P over the 4^m Pauli strings on the sites, <P> = <psi, P psi> with
P psi from generators.pauli_string_apply_np — the entropy helper, and the all-null call, which the library refuses before it
touches a device."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import contract_cases as K
import exact_ref as E
import lambda_lanczos_amd as L
from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G

PAULI = {"I": np.eye(2, dtype=np.complex128), "X": np.array([[0, 1], [1, 0]], np.complex128),
         "Y": np.array([[0, -1j], [1j, 0]], np.complex128), "Z": np.array([[1, 0], [0, -1]], np.complex128)}


def tomography(n_sites, sites, psi, states=None):
    """(rho, bound): rho = 2^-m sum_P <P> P and the sum over the strings of dot_bound(psi, P psi).  Bit k of a is sites[k]: the
    matrix of the string is kron over k descending."""
    m = len(sites)
    rho = np.zeros((1 << m, 1 << m), np.complex128)
    bound = 0.0
    for letters in itertools.product("IXYZ", repeat=m):
        x = sum(1 << s for s, c in zip(sites, letters) if c in "XY")
        z = sum(1 << s for s, c in zip(sites, letters) if c in "YZ")
        q = G.pauli_string_apply_np(n_sites, (x, z, 1.0), psi, states=states)
        mat = np.eye(1, dtype=np.complex128)
        for c in reversed(letters):
            mat = np.kron(mat, PAULI[c])
        rho += complex(E.dot_exact(psi, q)) * mat
        bound += E.dot_bound(psi, q)
    return rho / (1 << m), bound


def _site_lists(n_sites, rng):
    out = []
    for m in range(1, min(3, n_sites) + 1):
        out.append(list(range(m)))
        out.append([int(s) for s in rng.permutation(n_sites)[:m]])
    return out


@pytest.mark.parametrize("n_sites", [1, 2, 5, 8])
@pytest.mark.parametrize("dtype", [np.float64, np.complex128, np.float32, np.complex64], ids=["d", "z", "s", "c"])
def test_reference_is_the_definition_by_tomography(n_sites, dtype):
    rng = np.random.default_rng(n_sites)
    psi = K.start_x(1 << n_sites, dtype)
    for sites in _site_lists(n_sites, rng):
        m = len(sites)
        rho, fibres = G.reduced_density_matrix_np(n_sites, sites, psi)
        assert rho.dtype == np.complex128 and rho.shape == (1 << m, 1 << m)
        assert fibres.dtype == psi.dtype and fibres.shape == (1 << m, 1 << (n_sites - m))
        want, bound = tomography(n_sites, sites, psi)
        err = max(np.max(np.abs(rho.real - want.real)), np.max(np.abs(rho.imag - want.imag)))
        assert err <= (4 ** m) * E.dot_bound(psi, psi), (sites, err, bound)
        assert np.array_equal(rho, rho.conj().T)
        # the fibres are psi, rearranged: every amplitude once
        assert np.array_equal(np.sort(np.abs(fibres).ravel()), np.sort(np.abs(psi)))


@pytest.mark.parametrize("n_sites,n_down", [(4, 2), (7, 3), (9, 4)])
def test_reference_on_a_sector_is_the_definition_by_tomography(n_sites, n_down):
    rng = np.random.default_rng(n_sites * 31 + n_down)
    states = G.sector_states(n_sites, n_down)
    psi = K.start_x(states.shape[0], np.complex128)
    for sites in _site_lists(n_sites, rng):
        m = len(sites)
        rho, fibres = G.reduced_density_matrix_np(n_sites, sites, psi, states=states)
        want, _ = tomography(n_sites, sites, psi, states=states)
        err = max(np.max(np.abs(rho.real - want.real)), np.max(np.abs(rho.imag - want.imag)))
        assert err <= (4 ** m) * E.dot_bound(psi, psi), (sites, err)
        pc = np.array([bin(a).count("1") for a in range(1 << m)])
        assert not np.any(rho[pc[:, None] != pc[None, :]])   # S_z is conserved: popcount-off-diagonal entries vanish
        assert np.count_nonzero(fibres) <= states.shape[0]


def test_reference_refuses_bad_input():
    with pytest.raises(ValueError):
        G.reduced_density_matrix_np(3, [0, 0], np.zeros(8))
    with pytest.raises(ValueError):
        G.reduced_density_matrix_np(3, [3], np.zeros(8))
    with pytest.raises(ValueError):
        G.reduced_density_matrix_np(3, [1], np.zeros(7))


def test_all_null_call_is_refused_before_a_device_is_touched():
    """No context, no operator: LL_ERR_INVALID with the wording of the other entry points — on a machine without a GPU too,
    where anything that touched the device would answer LL_ERR_HIP."""
    lib = capi.lib()
    sweeps = C.c_int64(-7)
    st = lib.ll_pauli_rdm(None, None, 0, None, None, None, C.byref(sweeps))
    assert st == capi.LL_ERR_INVALID and b"null argument" in lib.ll_last_error()
    assert sweeps.value == -7
    st = lib.ll_pauli_rdm(None, None, 3, None, None, None, None)
    assert st == capi.LL_ERR_INVALID and b"null argument" in lib.ll_last_error()


def test_entanglement_entropy():
    assert L.entanglement_entropy(np.diag([1.0, 0.0])) == 0.0
    assert abs(L.entanglement_entropy(np.eye(4) / 4) - math.log(4)) <= 4 * E.EPS_D * math.log(4)
    # not normalised: rho / tr rho is what counts; a tiny negative eigenvalue contributes nothing
    assert abs(L.entanglement_entropy(3.0 * np.eye(2)) - math.log(2)) <= 4 * E.EPS_D
    assert L.entanglement_entropy(np.diag([1.0, -1e-18])) == 0.0
