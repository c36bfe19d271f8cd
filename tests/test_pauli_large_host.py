"""What tests/test_gpu_pauli_large.py rests on, without a GPU: the pinned dimensions of tests/pauli_large_cases.py tied by sum
rules that the host generator does not use, the symmetric block's matrix at 30 and 20 sites against the momentum block it
refines, generators.pauli_csr(states=...) against the whole matrix, and the row magnitudes of the embedding bound."""
import math

import numpy as np
import pytest

import exact_ref as E
import pauli_large_cases as C
from lambda_lanczos_amd import generators as G

SIGNS = (1, -1)


def _dense(csr):
    rp, ci, va = csr
    n = rp.shape[0] - 1
    A = np.zeros((n, n), va.dtype)
    np.add.at(A, (np.repeat(np.arange(n), np.diff(rp)), ci), va)
    return A


# ------------------------------------------------------------------ the pinned dimensions
def _mobius(k):
    out, q = 1, 2
    while k > 1:
        if k % q == 0:
            k //= q
            if k % q == 0:
                return 0
            out = -out
        q += 1
    return out


def _sector_necklaces_with_character(L, k, m):
    """The number of orbits of the rotation on the states of L sites with k set bits that carry the character m, by the divisor
    formula: an orbit of length R (a divisor of L) repeats L / R times an aperiodic necklace of R beads with j = k R / L set ones
    (an integer), of which there are (1 / R) sum_{d | gcd(R, j)} mu(d) C(R / d, j / d); it carries the character iff m R = 0 mod L."""
    total = 0
    for R in range(1, L + 1):
        if L % R or (m * R) % L or (k * R) % L:
            continue
        j = k * R // L
        total += sum(_mobius(d) * math.comb(R // d, j // d) for d in range(1, R + 1) if R % d == 0 and j % d == 0) // R
    return total


def _check_symmetric_sums(n_sites, n_down, m, d_m, seen):
    """At an m with 2 m mod L = 0 the parity blocks add up to D_m, and where 2 n_down = L the four (parity, inversion) blocks do."""
    parts = {p: G.symmetric_basis(n_sites, m, p, 0, n_down)[0].shape[0] for p in SIGNS}
    assert sum(parts.values()) == d_m
    seen.update({(n_sites, m, p, 0, n_down): d for p, d in parts.items()})
    if 2 * n_down == n_sites:
        four = {(p, z): G.symmetric_basis(n_sites, m, p, z, n_down)[0].shape[0] for p in SIGNS for z in SIGNS}
        assert sum(four.values()) == d_m
        for p in SIGNS:
            assert four[(p, 1)] + four[(p, -1)] == parts[p]
        seen.update({(n_sites, m, p, z, n_down): d for (p, z), d in four.items()})


def _check_pinned(n_sites, n_down, seen):
    for shape, (_, D) in C.SYMMETRIC.items():
        if (shape[0], shape[4]) == (n_sites, n_down):
            assert seen[shape] == D, shape


@pytest.mark.parametrize("n_sites,n_down", [(30, 4), (30, 5), (28, 5), (20, 10), (27, 4)])
def test_momentum_and_symmetric_dimensions_obey_the_sum_rules(n_sites, n_down):
    """sum_m D_m = C(L, n_down) and every D_m is the divisor formula's count; at every m with 2 m mod L = 0 the parity blocks add
    up to D_m, and where 2 n_down = L the four (parity, inversion) blocks do.  The pinned D of the cases are among the terms."""
    dm = [G.momentum_basis(n_sites, n_down, m)[0].shape[0] for m in range(n_sites)]
    assert sum(dm) == math.comb(n_sites, n_down)
    assert dm == [_sector_necklaces_with_character(n_sites, n_down, m) for m in range(n_sites)]
    for (L, nd, m), D in C.MOMENTUM.items():
        if (L, nd) == (n_sites, n_down):
            assert dm[m] == D
    seen = {}
    for m in sorted({0, n_sites // 2} if n_sites % 2 == 0 else {0}):
        _check_symmetric_sums(n_sites, n_down, m, dm[m], seen)
    for m in range(n_sites):      # with every flag 0 the symmetric basis is the momentum block
        if (n_sites, m, 0, 0, n_down) in C.SYMMETRIC:
            seen[(n_sites, m, 0, 0, n_down)] = G.symmetric_basis(n_sites, m, 0, 0, n_down)[0].shape[0]
            assert seen[(n_sites, m, 0, 0, n_down)] == dm[m]
    _check_pinned(n_sites, n_down, seen)


def test_dimensions_of_22_sites_at_half_filling_obey_the_sum_rules_at_momentum_zero():
    """C(22, 11) = 705 432 states: block 0 alone (the 22 momentum bases would take half a minute), its D_0 by the divisor formula."""
    d0 = G.momentum_basis(22, 11, 0)[0].shape[0]
    assert d0 == _sector_necklaces_with_character(22, 11, 0)
    assert sum(_sector_necklaces_with_character(22, 11, m) for m in range(22)) == math.comb(22, 11)
    seen = {}
    _check_symmetric_sums(22, 11, 0, d0, seen)
    _check_pinned(22, 11, seen)


def _necklaces_with_character(L, m):
    """The number of orbits of the rotation on the 2^L states that carry the character m, by the divisor formula: an orbit of
    length R (a divisor of L) is an aperiodic necklace of R beads, of which there are (1 / R) sum_{d | R} mu(R / d) 2^d, and it
    carries the character iff m R = 0 (mod L)."""
    total = 0
    for R in range(1, L + 1):
        if L % R == 0 and (m * R) % L == 0:
            total += sum(_mobius(R // d) * (1 << d) for d in range(1, R + 1) if R % d == 0) // R
    return total


@pytest.mark.parametrize("n_sites,ms", [(20, (0, 3, 4, 5, 10)), (21, (7,))])
def test_full_space_dimensions_equal_the_necklace_counts(n_sites, ms):
    assert sum(_necklaces_with_character(n_sites, m) for m in range(n_sites)) == 1 << n_sites
    for m in ms:
        D = G.full_momentum_basis(n_sites, m)[0].shape[0]
        assert D == _necklaces_with_character(n_sites, m)
        if (n_sites, m) in C.MOMENTUM_FULL:
            assert D == C.MOMENTUM_FULL[(n_sites, m)][1]


@pytest.mark.parametrize("m", [0, 10])
def test_full_space_symmetric_dimensions_add_up_to_the_necklace_count(m):
    four = {(p, z): G.symmetric_basis(20, m, p, z)[0].shape[0] for p in SIGNS for z in SIGNS}
    assert sum(four.values()) == _necklaces_with_character(20, m)
    for (p, z), D in four.items():
        if (20, m, p, z, None) in C.SYMMETRIC:
            assert D == C.SYMMETRIC[(20, m, p, z, None)][1]


def test_every_pinned_dimension_is_covered_by_a_sum_rule():
    assert {(s[0], s[4]) for s in C.SYMMETRIC if s[4] is not None} | {s[:2] for s in C.MOMENTUM} <= {
        (30, 4), (30, 5), (28, 5), (20, 10), (27, 4), (22, 11)}
    assert {s[:2] for s in C.SYMMETRIC if s[4] is None} <= {(20, 0), (20, 10)}
    assert set(C.MOMENTUM_FULL) <= {(20, 10), (20, 3), (21, 7)}
    assert C.small_bits(184756) == 4 and C.small_bits(6145) == 0 and C.small_bits(6144) == 0 and C.small_bits(2 * 6144) == 0
    assert C.small_bits(2 * 6144 + 1) == 1      # 6145 blocks of two indices, the last one ragged
    for kind, table in (("momentum", C.MOMENTUM), ("symmetric", {s: d for s, (_, d) in C.SYMMETRIC.items()}),
                        ("sector", {s: math.comb(*s) for s, _ in C.SECTOR})):
        for shape, D in table.items():
            assert ((kind, shape) in C.BELOW_WRAP) == (D < C.WRAPS), (kind, shape)
    assert all(D >= C.WRAPS for _, D in C.MOMENTUM_FULL.values())


# ------------------------------------------------------------------ the symmetric block's matrix against the momentum block
def _match_subset(small, big, tol):
    """Every value of `small` (ascending) meets a value of `big` (ascending) of its own within tol: the earliest free one."""
    j = 0
    for v in small:
        while j < big.shape[0] and big[j] < v - tol:
            j += 1
        if j == big.shape[0] or abs(big[j] - v) > tol:
            return False
        j += 1
    return True


@pytest.mark.parametrize("shape", [(30, 15, -1, 0, 5), (20, 10, -1, -1, 10)], ids=["30-15", "20-10"])
def test_symmetric_block_is_hermitian_and_its_spectrum_lies_in_the_momentum_blocks(shape):
    n_sites, m, p, z, nd = shape
    terms = C.model_terms("heisenberg", n_sites)
    norm = sum(abs(c) for _, _, c in terms)
    csr = G.pauli_symmetric_csr(n_sites, m, p, z, terms, np.complex128, n_down=nd)
    A = _dense(csr)
    assert A.shape[0] == C.SYMMETRIC[shape][1]
    assert np.max(np.abs(A - A.conj().T)) <= 1e-14 * np.max(np.abs(A))
    assert np.max(np.abs(A.imag)) == 0.0                 # 2 m = 0 mod L with the reflection in use: a real block
    sym = np.linalg.eigvalsh(A.real)
    M = _dense(G.pauli_momentum_csr(n_sites, nd, m, terms, np.float64))
    assert np.max(np.abs(M - M.T)) <= 1e-14 * np.max(np.abs(M))
    mom = np.linalg.eigvalsh(M)
    assert _match_subset(sym, mom, 1e-10 * norm)
    assert not _match_subset(sym + 1e-6 * norm, mom, 1e-10 * norm)      # the comparison can fail
    assert sym.shape[0] < mom.shape[0] and abs(sym[0]) > 1.0


# ------------------------------------------------------------------ rows of chosen states
@pytest.mark.parametrize("merge", [True, False])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_pauli_csr_of_chosen_states_is_the_rows_of_the_full_matrix(cplx, merge):
    n_sites = 12
    dtype = np.complex128 if cplx else np.float64
    terms = G.tfim_terms(n_sites, 1.0, 0.7, periodic=True) + [(0b11 << 9, 0b111 << 9, 0.3), (0, 0, 0.5), (1 << 11, 1, 0.2)]
    if cplx:
        terms += G.dm_terms(n_sites, 0.35, periodic=True)
    rp, ci, va = G.pauli_csr(n_sites, terms, dtype, merge=merge)
    rng = np.random.default_rng(3)
    states = np.concatenate([[0, 4095, 4095, 1], rng.permutation(4096)[:300]])      # unsorted, one state twice
    srp, sci, sva = G.pauli_csr(n_sites, terms, dtype, merge=merge, states=states)
    assert srp.shape[0] == states.shape[0] + 1 and srp[0] == 0 and sva.dtype == va.dtype and sci.dtype == ci.dtype
    for k, s in enumerate(states):
        assert np.array_equal(sci[srp[k]:srp[k + 1]], ci[rp[s]:rp[s + 1]])
        assert np.array_equal(sva[srp[k]:srp[k + 1]], va[rp[s]:rp[s + 1]])
    full = G.pauli_csr(n_sites, terms, dtype, merge=merge, states=np.arange(4096))
    assert all(np.array_equal(a, b) for a, b in zip(full, (rp, ci, va)))
    with pytest.raises(ValueError):
        G.pauli_csr(n_sites, terms, dtype, merge=merge, states=[4096])


def test_the_sample_of_the_20_site_operator():
    s = C.pauli_sample()
    assert s.shape[0] == C.PAULI_SAMPLE and s[0] == 0 and s[-1] == (1 << 20) - 1
    have = set(s.tolist())
    assert set(range(64)) <= have and set(range((1 << 20) - 64, 1 << 20)) <= have
    assert all({k - 2, k - 1, k, k + 1} <= have for k in range(1 << 12, 1 << 20, 1 << 12))
    assert np.array_equal(s, C.pauli_sample())
    for cplx in (False, True):
        terms = C.pauli_terms(cplx)
        high = [t for t in terms[40:]]
        assert len(high) == (6 if cplx else 4) and all((x | z) >> 14 and not (x | z) & ((1 << 14) - 1) for x, z, _ in high)
        assert sum(bin(x & z).count("1") & 1 for x, z, _ in terms) == (2 if cplx else 0)
        assert {"X", "Y", "Z"} <= {"XZY"[(x >> j & 1) + 2 * (z >> j & 1) - 1] for x, z, _ in high for j in range(14, 20) if (x | z) >> j & 1}


# ------------------------------------------------------------------ the row magnitudes of the embedding bound
@pytest.mark.parametrize("model", ["heisenberg", "dm"])
def test_sector_abs_rows_are_those_of_the_exact_rows(model):
    n_sites, n_down = 12, 5
    terms = C.model_terms(model, n_sites)
    rng = np.random.default_rng(4)
    X = rng.standard_normal(math.comb(n_sites, n_down)) + 1j * rng.standard_normal(math.comb(n_sites, n_down))
    ex = E.rows_exact(G.pauli_sector_csr(n_sites, n_down, terms, np.complex128, merge=False), X)
    got = C.sector_abs_rows(n_sites, n_down, terms, X)
    assert np.array_equal(got.nnz, ex.nnz)
    assert np.allclose(got.absrow, ex.absrow, rtol=1e-13, atol=0) and np.allclose(got.rowsum, ex.rowsum, rtol=1e-13, atol=0)
