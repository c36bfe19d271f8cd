"""The host reference of the momentum blocks of the FULL 2^n_sites space (generators.full_momentum_basis,
full_momentum_embedding, pauli_momentum_full_csr; ll_op_create_pauli_momentum_full_*) against dense algebra: B is an isometry,
B^H H B is the block the gather form builds, the blocks' sizes and spectra add up to the full matrix's, real models give real
blocks at 2 m = 0 (mod L), and for an H that conserves S_z the block is the direct sum over n_down of the sector blocks of
generators.pauli_momentum_csr.  No GPU."""
import numpy as np
import pytest

from lambda_lanczos_amd import generators as G

EPS_D = 2.0 ** -53
SIZES = [2, 3, 4, 6, 8, 9]


def dm_ring(n_sites, D):
    """One Dzyaloshinskii-Moriya bond j -> (j + 1) mod L per site; generators.dm_terms keeps ONE bond at L = 2 (an open chain)."""
    if n_sites != 2:
        return G.dm_terms(n_sites, D, periodic=True)
    return [(3, 2, float(D)), (3, 1, -float(D)), (3, 1, float(D)), (3, 2, -float(D))]


def model_terms(model, n_sites):
    if model == "tfim":
        return G.tfim_terms(n_sites, 1.0, 0.7, periodic=True)
    if model == "tfim_z":   # the z field breaks the spin-flip parity
        return G.tfim_terms(n_sites, 1.0, 0.7, periodic=True) + G.zfield_terms(n_sites, 0.3)
    if model == "xyz":
        return G.xyz_terms(n_sites, 1.0, 0.6, 0.8)
    if model == "xyz_dm_x":  # complex H (one Y per Dzyaloshinskii-Moriya term)
        return G.xyz_terms(n_sites, 1.0, 0.6, 0.8) + dm_ring(n_sites, 0.35) + [(1 << j, 0, -0.45) for j in range(n_sites)]
    if model == "heisenberg":
        return G.heisenberg_terms(n_sites, 1.0, 1.0, periodic=True)
    raise KeyError(model)


def _dense(csr, n_cols=None):
    rp, ci, va = csr
    n = rp.shape[0] - 1
    A = np.zeros((n, n if n_cols is None else n_cols), va.dtype)
    np.add.at(A, (np.repeat(np.arange(n), np.diff(rp)), ci), va)
    return A


def test_xyz_terms_are_the_three_bonds_per_site():
    assert G.xyz_terms(3, 1.0, 2.0, 3.0) == [(3, 0, 1.0), (3, 3, 2.0), (0, 3, 3.0), (6, 0, 1.0), (6, 6, 2.0), (0, 6, 3.0),
                                              (5, 0, 1.0), (5, 5, 2.0), (0, 5, 3.0)]
    assert len(G.xyz_terms(4, 1.0, 1.0, 1.0, periodic=False)) == 9 and len(G.xyz_terms(2, 1.0, 1.0, 1.0)) == 3
    assert G.translation_fault(2, G.xyz_terms(2, 1.0, 0.6, 0.8)) is None
    # J_x = J_y is the Heisenberg bond in Pauli units
    H = _dense(G.pauli_csr(4, G.xyz_terms(4, 0.25, 0.25, 0.25)))
    assert np.array_equal(H, _dense(G.pauli_csr(4, G.heisenberg_terms(4))))


@pytest.mark.parametrize("model", ["tfim_z", "xyz_dm_x"])
@pytest.mark.parametrize("n_sites", SIZES)
def test_blocks_against_dense_algebra(n_sites, model):
    """Tolerance 64 L eps_d sum |coef| (entries: a few roundings each; a product B^H H B row sums at most 2^L / L products of
    entries below sum |coef| / sqrt(R) with |B| <= 1; spectra: Weyl, the same bound on the 2-norm of the difference)."""
    terms = model_terms(model, n_sites)
    tol = 64 * n_sites * EPS_D * sum(abs(c) for _, _, c in terms)
    H = _dense(G.pauli_csr(n_sites, terms, np.complex128))
    assert np.array_equal(H, H.conj().T)
    total, spectrum = 0, []
    for m in range(n_sites):
        reps, period = G.full_momentum_basis(n_sites, m)
        assert reps.dtype == np.uint32 and np.all(np.diff(reps.astype(np.int64)) > 0)
        assert np.all(n_sites % period == 0) and np.all((m * period) % n_sites == 0)
        B = G.full_momentum_embedding(n_sites, m)
        D = reps.shape[0]
        assert B.shape == (1 << n_sites, D) and D >= 1
        assert np.max(np.abs(B.conj().T @ B - np.eye(D))) <= tol
        col, val = G.full_momentum_embedding(n_sites, m, dense=False)
        assert np.array_equal(np.flatnonzero(col >= 0), np.flatnonzero(np.any(B != 0, axis=1)))
        assert np.array_equal(B[col >= 0, col[col >= 0]], val[col >= 0])
        block = B.conj().T @ H @ B
        for merge in (True, False):
            got = _dense(G.pauli_momentum_full_csr(n_sites, m, terms, np.complex128, merge=merge))
            assert got.shape == (D, D)
            assert np.max(np.abs(got - block)) <= tol, (n_sites, m, merge, np.max(np.abs(got - block)))
        total += D
        spectrum.append(np.linalg.eigvalsh(block))
    assert total == 1 << n_sites
    assert np.max(np.abs(np.sort(np.concatenate(spectrum)) - np.linalg.eigvalsh(H))) <= tol


@pytest.mark.parametrize("model", ["tfim", "tfim_z", "xyz", "heisenberg"])
@pytest.mark.parametrize("n_sites", SIZES)
def test_real_models_give_real_blocks_at_momentum_zero_and_half(n_sites, model):
    terms = model_terms(model, n_sites)
    for m in range(n_sites):
        if (2 * m) % n_sites:
            with pytest.raises(ValueError):
                G.pauli_momentum_full_csr(n_sites, m, terms, np.float64)
            continue
        rp, ci, va = G.pauli_momentum_full_csr(n_sites, m, terms, np.float64)
        rz, cz, vz = G.pauli_momentum_full_csr(n_sites, m, terms, np.complex128)
        assert va.dtype == np.float64 and np.array_equal(rp, rz) and np.array_equal(ci, cz)
        assert np.all(vz.imag == 0) and np.array_equal(va, vz.real)
        A = _dense((rp, ci, va))
        assert np.max(np.abs(A - A.T)) <= 64 * n_sites * EPS_D * sum(abs(c) for _, _, c in terms)


def test_refusals_of_the_host_reference():
    with pytest.raises(ValueError):
        G.full_momentum_basis(4, 4)
    with pytest.raises(ValueError):
        G.full_momentum_basis(31, 0)
    with pytest.raises(ValueError, match="does not commute with the one-site translation"):
        G.pauli_momentum_full_csr(6, 0, G.tfim_terms(6, 1.0, 0.7, periodic=False))
    with pytest.raises(ValueError):    # an odd number of Y in a real dtype
        G.pauli_momentum_full_csr(6, 0, model_terms("xyz_dm_x", 6), np.float64)


def test_an_sz_conserving_ring_gives_the_direct_sum_of_the_sector_blocks():
    """Heisenberg ring, L = 8: the representatives of the full block are the union over n_down of momentum_basis; sorted, the full
    block equals the block-diagonal matrix of the pauli_momentum_csr blocks, entry for entry."""
    n_sites = 8
    terms = model_terms("heisenberg", n_sites)
    for m in range(n_sites):
        reps, period = G.full_momentum_basis(n_sites, m)
        parts = [(nd,) + G.momentum_basis(n_sites, nd, m) for nd in range(n_sites + 1)]
        union = np.concatenate([p[1] for p in parts])
        order = np.argsort(union, kind="stable")
        assert np.array_equal(union[order], reps) and np.array_equal(np.concatenate([p[2] for p in parts])[order], period)
        direct = np.zeros((reps.shape[0], reps.shape[0]), np.complex128)
        at = 0
        for nd, r, _ in parts:
            if r.shape[0]:
                direct[at:at + r.shape[0], at:at + r.shape[0]] = _dense(G.pauli_momentum_csr(n_sites, nd, m, terms, np.complex128))
            at += r.shape[0]
        full = _dense(G.pauli_momentum_full_csr(n_sites, m, terms, np.complex128))
        assert np.array_equal(full, direct[np.ix_(order, order)]), m
