"""The numpy expansion of a sum of Pauli strings (generators.pauli_csr) against explicit Kronecker products of the 2 x 2 Pauli
matrices, and the two closed forms the GPU tests lean on.  No GPU."""
import functools

import numpy as np

from lambda_lanczos_amd import generators as G

I2 = np.eye(2, dtype=np.complex128)
SX = np.array([[0, 1], [1, 0]], dtype=np.complex128)
SY = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
SZ = np.array([[1, 0], [0, -1]], dtype=np.complex128)


def kron_term(n_sites, x, z, c):
    """c times the Kronecker product with site 0 as the LAST factor."""
    mats = []
    for j in range(n_sites - 1, -1, -1):
        xb, zb = (x >> j) & 1, (z >> j) & 1
        mats.append(SY if xb and zb else SX if xb else SZ if zb else I2)
    return c * functools.reduce(np.kron, mats)


def dense(csr):
    rp, ci, va = csr
    n = rp.shape[0] - 1
    a = np.zeros((n, n), dtype=va.dtype)
    np.add.at(a, (np.repeat(np.arange(n), np.diff(rp)), ci), va)
    return a


def test_pauli_csr_equals_kronecker_products():
    cases = [
        (4, [(0b0101, 0b1100, 0.7)]),                                   # X0 Y2 Z3
        (3, [(0b011, 0, 0.25), (0b011, 0b011, 0.25)]),                  # XX + YY: the weights cancel on aligned spins
        (5, [(0, 0, 1.5), (0b00110, 0b00110, -0.3), (0b10000, 0b10001, 0.2), (0, 0b01010, 2.0), (0, 0, 0.25)]),
        (6, G.heisenberg_terms(6, 1.3, 0.4) + G.tfim_terms(6, 0.5, 0.8, periodic=True) + [(0b100001, 0b100000, -0.9)]),
        (1, [(1, 1, 2.0), (1, 0, 1.0), (0, 1, -1.0)]),
    ]
    for n_sites, terms in cases:
        want = sum(kron_term(n_sites, *t) for t in terms)
        for merge in (True, False):
            got = dense(G.pauli_csr(n_sites, terms, np.complex128, merge=merge))
            assert np.max(np.abs(got - want)) == 0.0, (n_sites, merge)
    rp, ci, va = G.pauli_csr(3, cases[1][1], np.float64, merge=False)
    assert np.array_equal(np.diff(rp), np.full(8, 2)) and va.dtype == np.float64     # one entry per term and state
    rp, ci, va = G.pauli_csr(3, cases[1][1], np.float64, merge=True)
    assert np.all(va != 0) and rp[-1] == 4                                            # cancelled weights are dropped


def test_real_dtype_refuses_an_odd_number_of_y():
    try:
        G.pauli_csr(2, [(1, 1, 1.0)], np.float64)
    except ValueError:
        return
    raise AssertionError("an odd number of Y is complex")


def test_heisenberg_ring_and_tfim_closed_forms():
    for J in (1.0, 2.5):
        a = dense(G.pauli_csr(4, G.heisenberg_terms(4, J), np.float64))
        assert np.array_equal(a, a.T)
        assert abs(np.linalg.eigvalsh(a)[0] + 2.0 * J) <= 1e-13 * J
        c = dense(G.pauli_csr(4, G.heisenberg_terms(4, J), np.complex128))
        assert np.max(np.abs(c.imag)) == 0.0
    e0 = G.tfim_ground_energy(8, 1.0, 1.5)
    assert abs(e0 + 13.1914049521889) <= 1e-12
    a = dense(G.pauli_csr(8, G.tfim_terms(8, 1.0, 1.5), np.float64))
    assert abs(np.linalg.eigvalsh(a)[0] - e0) <= 1e-12 * abs(e0)
