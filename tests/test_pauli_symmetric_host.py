"""The host reference of the momentum / reflection / spin-inversion blocks of a ring (generators.symmetric_basis,
symmetric_embedding, pauli_symmetric_csr, reflection_fault, inversion_fault; ll_op_create_pauli_symmetric_*) against dense
algebra: B is an isometry, H B = B (B^H H B), the gather form builds B^H H B, the block is real wherever the reflection is in
use, the pinned dimensions and their sum rules.  No GPU."""
import numpy as np
import pytest

from lambda_lanczos_amd import generators as G

SIGNS = [(1, 1), (1, -1), (-1, 1), (-1, -1)]


def dm_ring(n_sites, D):
    return G.dm_terms(n_sites, D, periodic=True)


def model_terms(model, n_sites):
    if model == "tfim":
        return G.tfim_terms(n_sites, 1.0, 0.7, periodic=True)
    if model == "xyz":
        return G.xyz_terms(n_sites, 1.0, 0.6, 0.8)
    if model == "heisenberg":
        return G.heisenberg_terms(n_sites, 1.0, 1.0, periodic=True)
    raise KeyError(model)


def _dense(csr, n_cols=None):
    rp, ci, va = csr
    n = rp.shape[0] - 1
    A = np.zeros((n, n if n_cols is None else n_cols), va.dtype)
    np.add.at(A, (np.repeat(np.arange(n), np.diff(rp)), ci), va)
    return A


def _times(csr_unmerged, B):
    """H B for H given with one entry per term and state (the same number of entries in every row)."""
    rp, ci, va = csr_unmerged
    n = rp.shape[0] - 1
    T = ci.shape[0] // n
    out = np.zeros(B.shape, np.complex128)
    for t in range(T):
        out += va.reshape(n, T)[:, t, None] * B[ci.reshape(n, T)[:, t]]
    return out


def _blocks(n_sites):
    """Every (m, parity, inversion) the operator takes at n_sites."""
    for m in range(n_sites):
        for p in (0, 1, -1):
            if p and (2 * m) % n_sites:
                continue
            for z in (0, 1, -1):
                yield m, p, z


def _dim(n_sites, m, p, z, n_down=None):
    return G.symmetric_basis(n_sites, m, p, z, n_down)[0].shape[0]


def _check_block(n_sites, m, p, z, terms, n_down=None):
    """The four dense checks on one block; H by rows (never as a dense 2^L x 2^L matrix)."""
    reps, R = G.symmetric_basis(n_sites, m, p, z, n_down)
    D = reps.shape[0]
    if D == 0:
        with pytest.raises(ValueError, match="empty"):
            G.pauli_symmetric_csr(n_sites, m, p, z, terms, np.complex128, n_down=n_down)
        return 0
    group = n_sites * (2 if p else 1) * (2 if z else 1)
    assert reps.dtype == np.uint32 and np.all(np.diff(reps.astype(np.int64)) > 0)
    assert np.all(group % R == 0) and np.all(R >= 1) and R.max() <= 120
    B = G.symmetric_embedding(n_sites, m, p, z, n_down)
    if n_down is None:
        H = G.pauli_csr(n_sites, terms, np.complex128, merge=False)
        HB = _times(H, B)
        fro = np.linalg.norm(H[2])
    else:
        Hd = _dense(G.pauli_sector_csr(n_sites, n_down, terms, np.complex128))
        HB = Hd @ B
        fro = np.linalg.norm(Hd)
    norm_h = fro / np.sqrt(B.shape[0])          # Frobenius / sqrt(n): a lower bound of the 2-norm of H
    assert B.shape[1] == D
    assert np.max(np.abs(B.conj().T @ B - np.eye(D))) <= 1e-13
    col, val = G.symmetric_embedding(n_sites, m, p, z, n_down, dense=False)
    assert np.array_equal(np.flatnonzero(col >= 0), np.flatnonzero(np.any(B != 0, axis=1)))
    assert np.array_equal(B[col >= 0, col[col >= 0]], val[col >= 0])
    block = B.conj().T @ HB
    assert np.linalg.norm(HB - B @ block) <= 1e-12 * norm_h, (n_sites, m, p, z, n_down)
    for merge in (True, False):
        got = _dense(G.pauli_symmetric_csr(n_sites, m, p, z, terms, np.complex128, n_down=n_down, merge=merge))
        assert got.shape == (D, D)
        assert np.max(np.abs(got - block)) <= 1e-12 * norm_h, (n_sites, m, p, z, n_down, merge)
    if (2 * m) % n_sites == 0:                  # real H, real characters: a real symmetric block
        rp, ci, va = G.pauli_symmetric_csr(n_sites, m, p, z, terms, np.float64, n_down=n_down)
        rz, cz, vz = G.pauli_symmetric_csr(n_sites, m, p, z, terms, np.complex128, n_down=n_down)
        assert va.dtype == np.float64 and np.array_equal(rp, rz) and np.array_equal(ci, cz)
        assert np.all(vz.imag == 0) and np.array_equal(va, vz.real)
        if p:
            assert np.max(np.abs(block.imag)) <= 1e-12 * norm_h
    return D


@pytest.mark.parametrize("model", ["tfim", "xyz", "heisenberg"])
@pytest.mark.parametrize("n_sites", [4, 6, 8, 9, 10])
def test_blocks_against_dense_algebra(n_sites, model):
    terms = model_terms(model, n_sites)
    for m in range(n_sites):
        plain = _check_block(n_sites, m, 0, 0, terms)
        assert plain == G.full_momentum_basis(n_sites, m)[0].shape[0]
        by_z = [_check_block(n_sites, m, 0, z, terms) for z in (1, -1)]
        assert sum(by_z) == plain
        if (2 * m) % n_sites == 0:
            by_p = [_check_block(n_sites, m, p, 0, terms) for p in (1, -1)]
            assert sum(by_p) == plain
            assert sum(_check_block(n_sites, m, p, z, terms) for p, z in SIGNS) == plain


@pytest.mark.parametrize("n_sites", [4, 6, 8, 9, 10])
def test_sector_blocks_against_dense_algebra(n_sites):
    """Heisenberg ring with n_down: the blocks of the sector; spin inversion only at half filling."""
    terms = model_terms("heisenberg", n_sites)
    for n_down in sorted({1, n_sites // 2, n_sites - 2}):
        for m, p, z in _blocks(n_sites):
            if z and 2 * n_down != n_sites:
                with pytest.raises(ValueError):
                    G.symmetric_basis(n_sites, m, p, z, n_down)
                continue
            _check_block(n_sites, m, p, z, terms, n_down)
        for m in range(n_sites):
            assert np.array_equal(G.symmetric_basis(n_sites, m, 0, 0, n_down)[0], G.momentum_basis(n_sites, n_down, m)[0])


@pytest.mark.parametrize("case", [("tfim", 0, 1, 1, None), ("xyz", 6, -1, -1, None), ("xyz", 0, 1, 0, None),
                                  ("heisenberg", 0, 1, 1, 6), ("heisenberg", 6, -1, -1, 6), ("heisenberg", 0, 1, 0, 6),
                                  ("xyz", 5, 0, -1, None)], ids=str)
def test_a_few_blocks_of_twelve_sites(case):
    model, m, p, z, n_down = case
    want = {(0, 1, 1, None): 122, (6, -1, -1, None): 102, (0, 1, 0, None): 224, (0, 1, 1, 6): 35, (6, -1, -1, 6): 27,
            (0, 1, 0, 6): 50}
    D = _check_block(12, m, p, z, model_terms(model, 12), n_down)
    assert D == want.get((m, p, z, n_down), D) and D > 0


def test_pinned_dimensions():
    assert [_dim(8, 0, p, z) for p, z in SIGNS] == [18, 12, 2, 4]
    assert [_dim(8, 4, p, z) for p, z in SIGNS] == [9, 4, 9, 12]
    assert [_dim(8, m, p, 0) for m, p in [(0, 1), (0, -1), (4, 1), (4, -1)]] == [30, 6, 13, 21]
    assert [_dim(10, *c) for c in [(0, 1, 1), (0, 1, -1), (0, -1, 1), (0, -1, -1), (5, 1, 1), (5, -1, -1)]] == [44, 34, 12, 18, 24, 34]
    assert [_dim(12, *c) for c in [(0, 1, 1), (6, -1, -1), (0, 1, 0)]] == [122, 102, 224]
    assert [_dim(12, *c, 6) for c in [(0, 1, 1), (6, -1, -1), (0, 1, 0)]] == [35, 27, 50]
    reps, R = G.symmetric_basis(8, 0, 1, 1, 4)
    assert reps.shape[0] == 7 and R.tolist() == [8, 16, 16, 16, 8, 4, 2]
    for z in (0, 1, -1):                              # empty blocks
        assert _dim(4, 0, -1, z) == 0
    assert _dim(6, 0, -1, 1) == 0


@pytest.mark.parametrize("n_sites", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16])
def test_sum_rules(n_sites):
    for m in range(n_sites):
        reps, R = G.symmetric_basis(n_sites, m, 0, 0)
        full = G.full_momentum_basis(n_sites, m)
        assert np.array_equal(reps, full[0]) and np.array_equal(R, full[1])
        for p in (0, 1, -1):
            if p and (2 * m) % n_sites:
                with pytest.raises(ValueError):
                    G.symmetric_basis(n_sites, m, p, 0)
                continue
            assert _dim(n_sites, m, p, 1) + _dim(n_sites, m, p, -1) == _dim(n_sites, m, p, 0)
        if (2 * m) % n_sites == 0:
            for z in (0, 1, -1):
                assert _dim(n_sites, m, 1, z) + _dim(n_sites, m, -1, z) == _dim(n_sites, m, 0, z)


def test_the_ring_ground_energy_of_the_tfim_is_the_lowest_eigenvalue():
    """generators.tfim_ground_energy is the OPEN chain's; the ring's closed form against a dense diagonalisation."""
    for n_sites in (4, 8):
        H = _dense(G.pauli_csr(n_sites, model_terms("tfim", n_sites)))
        e0 = np.linalg.eigvalsh(H)[0]
        assert abs(e0 - G.tfim_ring_ground_energy(n_sites, 1.0, 0.7)) <= 1e-12 * abs(e0)
        assert abs(e0 - G.tfim_ground_energy(n_sites, 1.0, 0.7)) > 0.1


def test_the_fault_functions():
    for n_sites in (4, 6, 9):
        for model in ("tfim", "xyz", "heisenberg"):
            terms = model_terms(model, n_sites)
            assert G.reflection_fault(n_sites, terms) is None and G.inversion_fault(n_sites, terms) is None
        heis = model_terms("heisenberg", n_sites)
        dm = heis + dm_ring(n_sites, 0.35)
        assert G.reflection_fault(n_sites, dm) == len(heis)           # the first Dzyaloshinskii-Moriya term
        assert G.translation_fault(n_sites, dm) is None
        zf = heis + G.zfield_terms(n_sites, 0.3)
        assert G.inversion_fault(n_sites, zf) == len(heis) and G.reflection_fault(n_sites, zf) is None
        assert G.inversion_fault(n_sites, zf + G.zfield_terms(n_sites, -0.3)) is None      # merged to 0
        with pytest.raises(ValueError, match="does not commute with the reflection"):
            G.pauli_symmetric_csr(n_sites, 0, 1, 0, dm, np.complex128)
        with pytest.raises(ValueError, match="does not commute with the global spin flip"):
            G.pauli_symmetric_csr(n_sites, 0, 0, 1, zf)


def test_refusals_of_the_host_reference():
    ring = model_terms("xyz", 6)
    for bad in [(6, 6, 0, 0), (31, 0, 0, 0), (6, 0, 2, 0), (6, 0, 0, -2), (6, 1, 1, 0)]:
        with pytest.raises(ValueError):
            G.symmetric_basis(*bad)
    with pytest.raises(ValueError):
        G.symmetric_basis(6, 0, 0, 0, 7)
    with pytest.raises(ValueError):
        G.symmetric_basis(6, 0, 0, 1, 2)
    with pytest.raises(ValueError):           # a real dtype at a complex momentum
        G.pauli_symmetric_csr(6, 1, 0, 1, ring, np.float64)
    with pytest.raises(ValueError, match="empty"):
        G.pauli_symmetric_csr(6, 0, -1, 1, ring)
