"""Expectation values of Pauli strings on a state of a ring's symmetry block (ll_pauli_expect_block, csrc/pauli_expect_block.hip,
planned by csrc/pauli_expect_block_plan.hpp): c is a seeded random vector on the block's representatives (complex for the complex
types, no eigenvector), every value against coef * Re <Psi, P Psi> with Psi = B c formed in double through the embeddings of
generators.py, P Psi by permutation and sign (generators.pauli_string_apply_np) and the dot product correctly rounded
(exact_ref.dot_exact).  Bound per observable, S_k its distinct symmetrised strings, D = n_local, scale_k = |coef_k| sum |Psi||P Psi|:
    (2 (D S_k + 8) + 32) eps_d scale_k + eps_d |want_k|
— exact_ref.dot_bound's count over the D S_k summands (sum |block summands| <= scale_k: each is a sum of full-space summands) plus
32 for the roundings that do not grow with the count (the weight, sqrt(R_a / R_b), the phase, the complex products, the
reference's own B c); all arithmetic is in double, so the float types get the same bound and a float accumulation fails it.
c in guarded, NaN-padded device buffers at two alignments and on the host (the same bits), the sweep count from
generators.symmetrised_strings, the exact zeros, bit-equal answers inside a G-orbit and for every order of the observables, a
cross-check against the operator's own apply, and the refusals.

Worst error / bound measured on an MI355X (printed per case): DESIGN.md 3.5."""
import ctypes as C
import math

import numpy as np
import pytest

import contract_cases as K
import exact_ref as E
import lambda_lanczos_amd as L
from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G
from pauli_cases import TYPES, TYPE_IDS, _cplx, _set_block_bits
from pauli_expect_block_cases import BATCH, Block, is_zero, reference, strings_of, sweeps_of
from test_gpu_accuracy_contracts import _guarded, _unguard
from test_gpu_pauli_expect import _refused, measure_everywhere   # guarded NaN-padded buffers at two alignments, the host, the same bits

pytestmark = pytest.mark.gpu

BLOCKS = [
    Block("momentum_full", 10, 0), Block("momentum_full", 10, 5), Block("momentum_full", 10, 3),
    Block("momentum_full", 14, 0),                      # D = 1182: several blocks of 2^8 indices, the last one ragged
    Block("momentum", 12, 0, n_down=6), Block("momentum", 12, 6, n_down=6), Block("momentum", 12, 4, n_down=6),   # orbits of 12, 6, 4, 3, 2
    Block("symmetric", 12, 0, 1, 1), Block("symmetric", 12, 6, -1, -1), Block("symmetric", 12, 0, -1, 0), Block("symmetric", 12, 3, 0, 1),
    Block("symmetric", 12, 0, 1, 1, n_down=6),
    Block("symmetric", 16, 0, 1, 1),                    # several blocks; run again at one index per workgroup
]
CASES = [(b, t) for b in BLOCKS for t in TYPES if _cplx(t) or b.real_ok()]
CASE_IDS = ["%s-%s" % (b.id, TYPE_IDS[TYPES.index(t)]) for b, t in CASES]
SMALLEST_BITS = 0        # the smallest value the block-bits keys admit: one index per workgroup


# ------------------------------------------------------------------ 1. every block against the exact reference
@pytest.mark.parametrize("block,dtype", CASES, ids=CASE_IDS)
def test_block_against_the_exact_reference(ctx, block, dtype):
    op = block.create(L, ctx, dtype, block.hamiltonian())   # the Hamiltonian's terms play no part
    worst = 0.0
    try:
        c, obs, want, bound, (i02, i35, ixz) = reference(block, dtype, op.n_local)
        sweeps = sweeps_of(block, obs, dtype)
        live = sum(not is_zero(block, t, dtype) for t in obs)
        assert len(obs) >= 40 and sweeps == -(-live // BATCH)
        if block.kind == "momentum_full" and _cplx(dtype):
            assert live == len(obs) > BATCH           # nothing is dropped: two sweeps
        for bits in ([None, SMALLEST_BITS] if block.n_sites == 16 else [None]):
            _set_block_bits(ctx, block.kind, bits)
            worst = max(worst, measure_everywhere(ctx, op, c, obs, want, bound, sweeps, (block.id, bits)))
            got = op.expectation(c, obs)               # (the bits of every placement: measure_everywhere asserts it)
            for k, t in enumerate(obs):                # the zero rules: exactly +0.0
                if is_zero(block, t, dtype):
                    assert got[k] == 0.0 and not np.signbit(got[k]), (block.id, t)
            # Z_3 Z_5 lies in the orbit of Z_0 Z_2: the same tables, the same sum — the coefficients are 1 and -1/2
            assert (obs[i02][2], obs[i35][2]) == (1.0, -0.5) and got[i02] == got[i35] / -0.5, (got[i02], got[i35])
            if ixz is not None:                        # X_0 Z_1 and Z_0 X_1 are mirror images
                assert got[ixz] == got[ixz + 1] and (got[ixz] != 0.0 or is_zero(block, obs[ixz], dtype))
            assert got[0] != 0.0                       # the identity: ||c||^2
        # the operator still applies
        _set_block_bits(ctx, block.kind, None)
        n = op.n_local
        xb, xv = _guarded(ctx, np.asarray(c), 0)
        yb, yv = _guarded(ctx, np.zeros(n, c.dtype), 0)
        L.spmv(op, xv, yv)
        assert np.all(np.isfinite(_unguard(yb, n, 0)))
        xb.free()
        yb.free()
    finally:
        _set_block_bits(ctx, block.kind, None)
        op.close()
    print("worst error / bound", block.id, np.dtype(dtype).char, worst)


# ------------------------------------------------------------------ 2. the order of the observables plays no part
@pytest.mark.parametrize("dtype", [np.float64, np.complex64], ids=["d", "c"])
def test_an_observable_gets_the_same_bits_in_every_slot(ctx, dtype):
    block = Block("symmetric", 12, 0, 1, 1)
    op = block.create(L, ctx, dtype, block.hamiltonian())
    try:
        c, obs, _, _, _ = reference(block, dtype, op.n_local)
        base = op.expectation(c, obs)
        perm = np.random.default_rng(3).permutation(len(obs))
        moved, nsw = op.expectation(c, [obs[j] for j in perm], return_sweeps=True)
        assert nsw == sweeps_of(block, obs, dtype)
        assert np.array_equal(moved.view(np.uint64), base[perm].view(np.uint64))
        alone = np.array([op.expectation(c, [t])[0] for t in obs[:8]])
        assert np.array_equal(alone.view(np.uint64), base[:8].view(np.uint64))
    finally:
        op.close()


# ------------------------------------------------------------------ 3. exact zeros, nothing to do
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_zero_rules_cost_no_sweep(ctx, dtype):
    sym = Block("symmetric", 12, 0, 1, -1)
    mom = Block("momentum", 12, 0, n_down=6)
    ops = sym.create(L, ctx, dtype, sym.hamiltonian())
    opm = mom.create(L, ctx, dtype, mom.hamiltonian())
    try:
        cs, cm = K.start_x(ops.n_local, dtype), K.start_x(opm.n_local, dtype)
        odd_z = [(0, 1, 1.0), (3, 4, -2.0), (1, 1, 0.5), (0, 7, 1.0)]          # popcount(z) odd under the flip: every image cancels
        got, nsw = ops.expectation(cs, odd_z, return_sweeps=True)
        assert nsw == 0 and np.array_equal(got.view(np.uint64), np.zeros(4, np.uint64))
        odd_x = [(1, 0, 1.0), (7, 2, 3.0), (0x1f, 0, -1.0)]                     # an odd number of flips leaves the sector
        got, nsw = opm.expectation(cm, odd_x, return_sweeps=True)
        assert nsw == 0 and np.array_equal(got.view(np.uint64), np.zeros(3, np.uint64))
        odd_y = [(3, 1, 1.0), (0x33, 0x10, -2.0)]                                # nY = 1 (two and four flips: a partner can stay in the sector)
        got, nsw = opm.expectation(cm, odd_y, return_sweeps=True)
        if _cplx(dtype):
            assert nsw == 1 and np.any(got != 0.0)
        else:
            assert nsw == 0 and np.array_equal(got.view(np.uint64), np.zeros(2, np.uint64))
        # mixed with observables that need the sweep: the zeros stay +0.0, the identity returns ||c||^2 (nothing is divided)
        mixed = [(1, 0, 1.0), (0, 0, 1.0), (3, 0, 0.5), (7, 2, 3.0)]
        got, nsw = opm.expectation(cm, mixed, return_sweeps=True)
        nn = E.dot_exact(cm, cm).real
        assert nsw == 1 and got[0] == 0.0 and got[3] == 0.0 and abs(got[1] - nn) <= E.dot_bound(cm, cm) + E.EPS_D * nn
        # n_obs = 0 is valid and touches nothing (no c either)
        sweeps = C.c_int64(-1)
        capi.check(capi.lib().ll_pauli_expect_block(ctx.handle, ops.handle, 0, None, None, None, C.byref(sweeps)))
        assert sweeps.value == 0
        got, nsw = ops.expectation(cs, [], return_sweeps=True)
        assert got.shape == (0,) and nsw == 0
    finally:
        ops.close()
        opm.close()


# ------------------------------------------------------------------ 4. the Hamiltonian's own terms against its apply
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_sum_over_the_hamiltonian_terms_is_the_rayleigh_quotient(ctx, dtype):
    """Without the CPU state: on the L = 16 block (0, +1, +1), sum_t <P_t> over the Hamiltonian's terms = Re <c| H c> from the
    operator's apply and ll_dot.  Tolerance: the summed bounds of the measurement (the scale of a term bounded by |coef| ||c||^2,
    since |<Psi| P |Psi>| summands are bounded through Cauchy-Schwarz by sum |Psi|^2 <= 2 ||c||^2 in the |re| + |im| measure) plus
    the apply's class bound, eps_T per term on sum_t |coef_t| ||c||^2, and the dot product's."""
    block = Block("symmetric", 16, 0, 1, 1)
    terms = block.hamiltonian()
    op = block.create(L, ctx, dtype, terms)
    try:
        n = op.n_local
        c = K.start_x(n, dtype, seed=11)
        got = op.expectation(c, terms)
        xb, xv = _guarded(ctx, c, 0)
        yb, yv = _guarded(ctx, np.zeros(n, c.dtype), 0)
        L.spmv(op, xv, yv)
        rq = L.dot(ctx, xv, yv, n)
        rq = rq.real if isinstance(rq, complex) else rq
        xb.free()
        yb.free()
    finally:
        op.close()
    nn = 2.0 * E.dot_abs(c, c)
    bound = 0.0
    for t in terms:
        s_k = len(strings_of(block, t))
        bound += (2 * (n * s_k + 8) + 32) * E.EPS_D * abs(t[2]) * nn + E.EPS_D * abs(t[2]) * nn
    eps_t = E.EPS_F if np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.complex64)) else E.EPS_D
    norm = sum(abs(t[2]) for t in terms)
    bound += 8.0 * eps_t * (len(terms) + 2) * norm * nn + 2.0 * (n + 8) * E.EPS_D * norm * nn
    total = math.fsum(got)
    print("sum of the terms", total, "Re <c|Hc>", rq, "bound", bound, "error / bound", abs(total - rq) / bound)
    assert abs(total - rq) <= bound


# ------------------------------------------------------------------ 5. refusals, each with its message
def test_refusals(ctx):
    n_sites = 6
    one = [(0, 3, 1.0)]
    ring = G.tfim_terms(n_sites, 1.0, 0.7, periodic=True)
    csr = L.CsrOperator(ctx, *G.laplace2d_np(4))
    full = L.PauliOperator(ctx, n_sites, one, np.float64)
    sect = L.PauliSectorOperator(ctx, n_sites, 3, one, np.float64)
    mom = L.PauliMomentumFullOperator(ctx, n_sites, 0, ring, np.float64)
    ctx2 = L.Context(0)
    ctx2.init_comm(L.Context.unique_id(), 0, 1)
    shard = L.PauliMomentumFullOperator(ctx2, n_sites, 0, ring, np.float64)
    c = K.start_x(mom.n_local, np.float64)
    try:
        _refused(lambda: L.pauli_expect_block(csr, K.start_x(16, np.float64), one), "a CSR operator")
        _refused(lambda: L.pauli_expect_block(full, K.start_x(64, np.float64), one), "a full-space sum of Pauli strings", "ll_pauli_expect")
        _refused(lambda: L.pauli_expect_block(sect, K.start_x(20, np.float64), one), "on an S_z sector", "ll_pauli_expect")
        _refused(lambda: shard.expectation(c, one), "a context with a communicator")
        _refused(lambda: L.pauli_expect_block(shard, c, one), "a context with a communicator")
        _refused(lambda: mom.expectation(c, [(0, 1, 1.0), (64, 0, 1.0)]), "observable 1", "a mask bit at or above n_sites")
        _refused(lambda: mom.expectation(c, [(0, 64, 1.0)]), "observable 0", "a mask bit at or above n_sites")
        _refused(lambda: mom.expectation(c, [(1, 0, float("nan"))]), "observable 0", "the coefficient is not finite")
        _refused(lambda: mom.expectation(c, [(1, 0, float("inf"))]), "the coefficient is not finite")
        arr = (capi.PauliTerm * 1)()
        arr[0].x_mask, arr[0].z_mask, arr[0].coef = 0, 3, 1.0
        out = np.zeros(1)
        st = capi.lib().ll_pauli_expect_block(ctx.handle, mom.handle, 1, arr, None, out.ctypes.data_as(C.POINTER(C.c_double)), None)
        assert st == capi.LL_ERR_INVALID and b"null argument" in capi.lib().ll_last_error()
        st = capi.lib().ll_pauli_expect_block(ctx.handle, mom.handle, 1, arr, capi.ptr(c), None, None)
        assert st == capi.LL_ERR_INVALID and b"null argument" in capi.lib().ll_last_error()
        st = capi.lib().ll_pauli_expect_block(ctx2.handle, mom.handle, 1, arr, capi.ptr(c), out.ctypes.data_as(C.POINTER(C.c_double)), None)
        assert st == capi.LL_ERR_INVALID and b"another context" in capi.lib().ll_last_error()
        # the operator still measures after the refusals
        nn = E.dot_exact(c, c).real
        assert abs(mom.expectation(c, [(0, 0, 1.0)])[0] - nn) <= E.dot_bound(c, c) + E.EPS_D * nn
    finally:
        for o in (csr, full, sect, mom, shard):
            o.close()
        ctx2.close()
