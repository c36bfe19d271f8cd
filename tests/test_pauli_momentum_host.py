"""Host side of the momentum-block operator (ll_op_create_pauli_momentum_*): the generators that define a block's basis
(momentum_basis), its embedding B into the S_z sector (momentum_embedding) and the block itself from the gather form
(pauli_momentum_csr), checked against the normative definition B^H H_sector B.  No GPU."""
import math

import numpy as np
import pytest

from lambda_lanczos_amd import generators as G

EPS = float(np.finfo(np.float64).eps)


def dm_ring(L, D):
    """The Dzyaloshinskii-Moriya RING: one bond j -> (j + 1) mod L per site.  generators.dm_terms(L, D, periodic=True) is this for
    L >= 3; at L = 2 it keeps one bond only (an open chain, which does not commute with the translation), while the ring's two
    bonds cancel."""
    if L >= 3:
        return G.dm_terms(L, D, periodic=True)
    terms = []
    for j in range(L if L == 2 else 0):
        a, b = 1 << j, 1 << ((j + 1) % L)
        terms += [(a | b, b, float(D)), (a | b, a, -float(D))]
    return terms


MODELS = {
    "heisenberg": (True, lambda L: G.heisenberg_terms(L, 1.0, 1.0, periodic=True)),
    "xxz_zfield": (True, lambda L: G.heisenberg_terms(L, 1.0, 0.8, periodic=True) + G.zfield_terms(L, 0.37)),
    "xxz_dm": (False, lambda L: G.heisenberg_terms(L, 1.0, 0.8, periodic=True) + dm_ring(L, 0.35)),
}


def dense_of(csr, nrows, ncols):
    rp, ci, va = csr
    A = np.zeros((nrows, ncols), np.complex128)
    np.add.at(A, (np.repeat(np.arange(nrows), np.diff(rp)), ci), va)
    return A


@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("L", range(1, 13))
def test_blocks_are_the_compression_of_the_sector_by_the_embedding(L, model):
    real_h, make = MODELS[model]
    terms = make(L)
    assert G.translation_fault(L, terms) is None
    for n_down in range(L + 1):
        D = math.comb(L, n_down)
        H = dense_of(G.pauli_sector_csr(L, n_down, terms, np.complex128), D, D)
        norm = float(np.abs(H).sum(1).max())
        tol = 64 * EPS * norm
        dims, spectrum = [], []
        for m in range(L):
            reps, periods = G.momentum_basis(L, n_down, m)
            Dm = reps.shape[0]
            dims.append(Dm)
            assert reps.dtype == np.uint32 and np.all(np.diff(reps.astype(np.int64)) > 0)
            assert np.all(L % periods == 0) and np.all((m * periods) % L == 0)
            B = G.momentum_embedding(L, n_down, m)
            assert B.shape == (D, Dm)
            assert np.max(np.abs(B.conj().T @ B - np.eye(Dm)), initial=0.0) <= 8 * EPS          # B^H B = I
            col, val = G.momentum_embedding(L, n_down, m, dense=False)
            assert np.array_equal(B[np.flatnonzero(col >= 0), col[col >= 0]], val[col >= 0]) and np.count_nonzero(B) == np.sum(col >= 0)
            M = dense_of(G.pauli_momentum_csr(L, n_down, m, terms, np.complex128), Dm, Dm)
            P = B.conj().T @ H @ B
            assert np.max(np.abs(M - P), initial=0.0) <= tol, (L, n_down, m, np.max(np.abs(M - P)), tol)
            assert np.max(np.abs(M - M.conj().T), initial=0.0) <= tol                             # Hermitian
            split = dense_of(G.pauli_momentum_csr(L, n_down, m, terms, np.complex128, merge=False), Dm, Dm)
            assert np.max(np.abs(split - M), initial=0.0) <= tol                                  # one entry per term and state
            if real_h and (2 * m) % L == 0:                                                       # a real block
                assert np.all(M.imag == 0)
                R = dense_of(G.pauli_momentum_csr(L, n_down, m, terms, np.float64), Dm, Dm)
                assert np.array_equal(R.real, M.real)
            elif (2 * m) % L:                                                                     # complex phases
                with pytest.raises(ValueError):
                    G.pauli_momentum_csr(L, n_down, m, terms, np.float64)
            if L <= 10 and Dm:
                spectrum += list(np.linalg.eigvalsh(M))
        assert sum(dims) == D, (L, n_down, dims)
        if L <= 10:
            # eigvalsh is backward stable to a modest multiple of D eps |H| (D <= 252): 1e-11 |H| leaves two orders of margin
            assert np.max(np.abs(np.sort(spectrum) - np.linalg.eigvalsh(H))) <= 1e-11 * max(norm, 1.0)


def test_hand_checkable_blocks():
    assert [G.momentum_basis(4, 2, m)[0].shape[0] for m in range(4)] == [2, 1, 2, 1]
    assert [G.momentum_basis(6, 3, m)[0].shape[0] for m in range(6)] == [4, 3, 3, 4, 3, 3]
    for m in range(4):                       # 0101 has R = 2: in the block only when 2 m = 0 (mod 4)
        reps, periods = G.momentum_basis(4, 2, m)
        assert (0b0101 in reps) == (m % 2 == 0)
        assert reps[0] == 0b0011 and periods[0] == 4
        if m % 2 == 0:
            assert list(reps) == [0b0011, 0b0101] and list(periods) == [4, 2]
    reps, periods = G.momentum_basis(1, 0, 0)
    assert list(reps) == [0] and list(periods) == [1]
    reps, periods = G.momentum_basis(6, 0, 0)
    assert list(reps) == [0] and list(periods) == [1]
    assert G.momentum_basis(6, 0, 1)[0].shape == (0,)          # the all-up state has momentum 0 only
    for bad in [(4, 2, 4), (4, 2, -1), (4, 5, 0), (0, 0, 0)]:
        with pytest.raises(ValueError):
            G.momentum_basis(*bad)


def test_the_generators_take_18_sites_in_seconds():
    reps, periods = G.momentum_basis(18, 9, 9)
    assert reps.shape[0] == sum(1 for _ in reps) and abs(reps.shape[0] - math.comb(18, 9) / 18) < 60
    rp, ci, va = G.pauli_momentum_csr(18, 9, 9, G.heisenberg_terms(18), np.float64)
    assert rp.shape[0] == reps.shape[0] + 1 and ci.max() < reps.shape[0] and va.dtype == np.float64


def test_an_h_that_does_not_commute_with_the_translation_is_refused():
    ring = G.heisenberg_terms(6, 1.0, 1.0, periodic=True)
    assert G.translation_fault(6, ring) is None
    chain = G.heisenberg_terms(6, 1.0, 1.0, periodic=False)
    assert G.translation_fault(6, chain) is not None
    with pytest.raises(ValueError, match="does not commute"):
        G.pauli_momentum_csr(6, 3, 0, chain)
    bent = list(ring)
    bent[3] = (bent[3][0], bent[3][1], np.nextafter(bent[3][2], 1.0))     # one coefficient changed in its last bit
    assert G.translation_fault(6, bent) in (0, 3)
    assert G.translation_fault(2, G.dm_terms(2, 0.35)) is not None       # one DM bond on two sites changes sign under the swap
    assert G.translation_fault(6, ring[:9] + [(0, 0, 0.5)] + ring[9:]) is None   # the identity commutes
