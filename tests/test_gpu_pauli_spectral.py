"""The dynamical structure factor of a Heisenberg ring of 8 sites through the whole chain of calls: the ground state psi of the block
(n_down = 4, m = 0) from run_two_pass; phi = transfer(Z_0) into every momentum m_t; (alpha, beta) from lanczos_coefficients on
the target block with more steps than the block has dimensions; G(omega + E_0 + i eta) = norm2 continued_fraction at eta = 0.1 on
64 frequencies.  Reference: the dense resolvent phi_ref^H (z - H_t)^-1 phi_ref with H_t from generators.pauli_momentum_csr and
phi_ref from generators.pauli_block_transfer_np of the same stored psi.

The margin is not a fixed number: the same plain three-term recurrence run in numpy on the dense block from phi_ref deviates
from the dense resolvent by d_ref (its largest deviation over the frequencies), and the GPU value must stay within
10 d_ref + 1e-12 max |G| — the two recurrences round differently but lose orthogonality alike.
Measured on an MI355X: d_ref and the GPU deviation are printed per target block.

The sum rule: norm2 = <psi| Pbar_q^dagger Pbar_q |psi> = (1 / L) sum_d cos(2 pi q d / L) <psi| Z_0 Z_d |psi> for a state of one
momentum, with the correlators from `expectation` on the source block."""
import numpy as np
import pytest

import contract_cases as K
import exact_ref as E
import lambda_lanczos_amd as L
from lambda_lanczos_amd import generators as G
from test_gpu_pauli_block_transfer import transfer_bound

pytestmark = pytest.mark.gpu

N_SITES, N_DOWN, ETA = 8, 4, 0.1
Z0 = [(0, 1, 1.0)]
BREAKDOWN = 10 * E.EPS_D     # the library's test on beta (ritz_tracker.hpp)


def _lanczos_np(H, start, steps):
    """The plain three-term recurrence of the library in numpy: (alpha, beta), beta[k] = ||r_(k+1)||, ended by beta < BREAKDOWN."""
    u_prev, u = np.zeros_like(start), start / np.linalg.norm(start)
    alpha, beta = [], []
    for k in range(steps):
        w = H @ u
        alpha.append(float(np.vdot(u, w).real))
        w = w - alpha[-1] * u - (beta[-1] if beta else 0.0) * u_prev
        beta.append(float(np.linalg.norm(w)))
        if beta[-1] < BREAKDOWN:
            break
        u_prev, u = u, w / beta[-1]
    return np.array(alpha), np.array(beta)


def test_structure_factor_of_the_heisenberg_ring(ctx):
    dtype = np.complex128
    terms = G.heisenberg_terms(N_SITES, 1.0, 1.0, periodic=True)
    src = L.PauliMomentumOperator(ctx, N_SITES, N_DOWN, 0, terms, dtype)
    ops = [src]
    try:
        eng = L.LambdaLanczos(src, src.n, False, 1)
        e0, psi, info = eng.run_two_pass()
        H0 = K.dense_of(G.pauli_momentum_csr(N_SITES, N_DOWN, 0, terms, np.complex128), src.n)
        assert abs(e0 - np.linalg.eigvalsh(H0)[0]) <= 1e-10   # (the solver's own tests hold it to its bound: a sanity check here)
        nn = float(np.sum(np.abs(psi) ** 2))
        corr = src.expectation(psi, [(0, 1 | (1 << d), 1.0) for d in range(1, N_SITES)])
        corr_bound = (2 * (src.n * N_SITES + 8) + 32) * E.EPS_D * nn      # pauli_expect_block_cases.reference: scale <= ||psi||^2
        omega = np.linspace(0.0, 6.0, 64)
        z = omega + e0 + 1j * ETA
        ran = 0
        for m_t in range(N_SITES):
            tgt = L.PauliMomentumOperator(ctx, N_SITES, N_DOWN, m_t, terms, dtype)
            ops.append(tgt)
            phi_ref, mag = G.pauli_block_transfer_np("momentum", (N_SITES, N_DOWN, 0), (N_SITES, N_DOWN, m_t), Z0, psi, return_magnitude=True)
            phi = ctx.empty(tgt.n, dtype)
            _, norm2 = src.transfer(Z0, psi, tgt, out=phi, return_norm2=True)
            e = transfer_bound(N_SITES, 1, mag, phi_ref, dtype)
            # the sum rule
            s_q = (nn + float(np.sum(np.cos(2 * np.pi * m_t * np.arange(1, N_SITES) / N_SITES) * corr))) / N_SITES
            slack = corr_bound + 2 * (tgt.n + 8) * E.EPS_D * norm2 + float(np.sum(2 * np.abs(phi_ref) * e + e * e))
            assert abs(norm2 - s_q) <= slack, (m_t, norm2, s_q, slack)
            if m_t == 0:   # q = 0: Z_0 stands for the total magnetisation / L, which is 0 in this sector — nothing to start from
                assert np.all(np.abs(phi.get()) <= e) and norm2 <= float(np.sum(e * e))
                phi.free()
                continue
            steps = tgt.n + 5
            alpha, beta, iterations = L.lanczos_coefficients(tgt, phi, steps)
            phi.free()
            assert 1 <= iterations <= steps and alpha.shape == beta.shape == (iterations,)
            g_gpu = L.continued_fraction(alpha, beta, z, norm2)
            Ht = K.dense_of(G.pauli_momentum_csr(N_SITES, N_DOWN, m_t, terms, np.complex128), tgt.n)
            g_ref = np.array([np.vdot(phi_ref, np.linalg.solve(zz * np.eye(tgt.n) - Ht, phi_ref)) for zz in z])
            a_np, b_np = _lanczos_np(Ht, phi_ref, steps)
            g_np = L.continued_fraction(a_np, b_np, z, float(np.vdot(phi_ref, phi_ref).real))
            d_ref = float(np.max(np.abs(g_np - g_ref)))
            d_gpu = float(np.max(np.abs(g_gpu - g_ref)))
            print("m_t %d: D_t %d, iterations %d (numpy %d), norm2 %.6e, max|G| %.4e, d_ref %.3e, GPU deviation %.3e" % (
                m_t, tgt.n, iterations, a_np.shape[0], norm2, float(np.max(np.abs(g_ref))), d_ref, d_gpu))
            assert d_gpu <= 10 * d_ref + 1e-12 * float(np.max(np.abs(g_ref))), (m_t, d_gpu, d_ref)
            spec = L.spectral_function(alpha, beta, omega, ETA, e0=e0, norm2=norm2)
            assert np.array_equal(spec, -g_gpu.imag / np.pi) and np.all(spec > 0)
            ran += 1
        assert ran == N_SITES - 1
    finally:
        for o in ops:
            o.close()
