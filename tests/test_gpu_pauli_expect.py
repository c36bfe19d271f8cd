"""Expectation values of Pauli strings in one sweep over a state (ll_pauli_expect, csrc/pauli_expect.hip, planned by
csrc/pauli_expect_plan.hpp): every value against the EXACT host reference — coef * Re <psi, P psi> with P psi formed by permutation
and sign (generators.pauli_string_apply_np) and the dot product correctly rounded (exact_ref.dot_exact) — at the project's bound for
a double-accumulated dot (exact_ref.dot_bound, which a float accumulation fails) plus one double rounding of the result; in all four
storage types, on the full space for tiles shorter than the vector, equal to it and with remote groups, on S_z sectors with one and
with many blocks; psi in guarded, NaN-padded device buffers at two alignments and on the host (the same bits), the exact zeros, the
sweep count, two physical identities on ground states, and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import contract_cases as K
import exact_ref as E
import lambda_lanczos_amd as L
from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G
from pauli_cases import TYPES, TYPE_IDS, _cplx, _run_lanczos, _set_block_bits
from test_gpu_accuracy_contracts import _guarded, _unguard

pytestmark = pytest.mark.gpu

NAN_FILL = 0xFF          # every byte 0xFF: a NaN in all four storage types
BATCH = 32               # accumulators per sweep (csrc/pauli_expect.hip kPauliExpectBatch)
FULL_SITES = [1, 2, 3, 5, 6, 9, 11, 14]
TILE_BITS = [None, 6, 9]   # default (at 14 sites: a tile shorter than the vector for d, z, c); 64 and 512 states per tile
SECTORS = [(6, 0), (6, 6), (9, 4), (12, 6), (13, 4), (14, 7)]
BLOCK_BITS = [None, 4, 7]  # default (1024 indices per block); 16 and 128


def observable_set(n_sites, seed):
    """The identity, every single-site X, Y, Z, every pair X_i X_j, Y_i Y_j, Z_i Z_j, the full-length X...X and Z...Z, 40 random
    strings, three duplicates and one zero coefficient.  More than 300 observables at 14 sites."""
    rng = np.random.default_rng(seed)
    full = (1 << n_sites) - 1
    obs = [(0, 0, 1.0)]
    for j in range(n_sites):
        b = 1 << j
        obs += [(b, 0, 0.5 + 0.01 * j), (b, b, -1.25), (0, b, 2.0)]
    for i in range(n_sites):
        for j in range(i + 1, n_sites):
            m = (1 << i) | (1 << j)
            obs += [(m, 0, 0.25), (m, m, -0.25), (0, m, 1.0 + 0.125 * i)]
    obs += [(full, 0, 1.0), (0, full, -1.0)]
    obs += [(int(rng.integers(0, full + 1)), int(rng.integers(0, full + 1)), float(rng.uniform(-2, 2))) for _ in range(40)]
    obs += [obs[1], obs[len(obs) // 2], obs[-1]]
    obs += [(full & 5, full & 3, 0.0)]
    return obs


def is_zero(term, dtype, sector):
    """The two rules that answer +0.0 without a sweep."""
    x, z, _ = term
    return (not _cplx(dtype) and bin(x & z).count("1") % 2 == 1) or (sector and bin(x).count("1") % 2 == 1)


def sweeps_of(obs, dtype, sector):
    return -(-sum(not is_zero(t, dtype, sector) for t in obs) // BATCH)


_REF = {}


def reference(n_sites, n_down, dtype):
    """(psi, observables, expected values, bounds), computed once per basis and storage type and left unchanged."""
    key = (n_sites, n_down, np.dtype(dtype).char)
    if key not in _REF:
        states = None if n_down is None else G.sector_states(n_sites, n_down)
        n = (1 << n_sites) if states is None else states.shape[0]
        psi = K.start_x(n, dtype)
        obs = observable_set(n_sites, 100 * n_sites + (0 if n_down is None else n_down + 1))
        want, bound = np.zeros(len(obs)), np.zeros(len(obs))
        for j, t in enumerate(obs):
            q = G.pauli_string_apply_np(n_sites, t, psi, states=states)
            want[j] = t[2] * E.dot_exact(psi, q).real
            bound[j] = abs(t[2]) * E.dot_bound(psi, q) + E.EPS_D * abs(want[j])   # + one double rounding of the result
        psi.setflags(write=False)
        _REF[key] = (psi, obs, want, bound)
    return _REF[key]


def check_values(got, want, bound, what):
    assert np.all(np.isfinite(got)), (what, "a value is not finite: the kernel read past psi")
    err = np.abs(got - want)
    j = int(np.argmax(err - bound))
    assert np.all(err <= bound), (what, j, got[j], want[j], bound[j])
    return float(np.max(err / np.maximum(bound, 1e-300)))


def measure_everywhere(ctx, op, psi, obs, want, bound, sweeps, what):
    """psi in guarded, NaN-padded device buffers at shift 0 and 1 and on the host: every value within its bound, psi unchanged,
    the sweeps counted, the same bits for every placement and from call to call.  Returns the worst error / bound."""
    n = psi.shape[0]
    first, worst = None, 0.0
    for shift in (0, 1):
        buf, view = _guarded(ctx, psi, shift, NAN_FILL)
        for rep in range(2):
            got, nsw = op.expectation(view, obs, return_sweeps=True)
            assert got.dtype == np.float64 and got.shape == (len(obs),) and nsw == sweeps, (what, shift, nsw, sweeps)
            worst = max(worst, check_values(got, want, bound, (what, "device", shift)))
            if first is None:
                first = got
            assert np.array_equal(first.view(np.uint8), got.view(np.uint8)), (what, "device", shift, rep)
        assert np.array_equal(_unguard(buf, n, shift, NAN_FILL), psi), "the measurement changed psi"
        buf.free()
    got, nsw = op.expectation(psi, obs, return_sweeps=True)
    assert nsw == sweeps and np.array_equal(first.view(np.uint8), got.view(np.uint8)), (what, "host psi")
    return worst


# ------------------------------------------------------------------ 1. the full space
@pytest.mark.parametrize("n_sites", FULL_SITES)
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_full_space_against_the_exact_reference(ctx, dtype, n_sites):
    psi, obs, want, bound = reference(n_sites, None, dtype)
    if n_sites == 14:
        assert len(obs) > 300 and sum(not is_zero(t, dtype, False) for t in obs) % BATCH != 0
    op = L.PauliOperator(ctx, n_sites, G.tfim_terms(n_sites, 1.0, 0.7), dtype)   # the Hamiltonian's terms play no part
    worst = 0.0
    try:
        for bits in TILE_BITS:
            _set_block_bits(ctx, "pauli", bits)
            worst = max(worst, measure_everywhere(ctx, op, psi, obs, want, bound, sweeps_of(obs, dtype, False), (n_sites, bits)))
    finally:
        _set_block_bits(ctx, "pauli", None)
        op.close()
    print("worst error / bound", np.dtype(dtype).char, n_sites, worst)


# ------------------------------------------------------------------ 2. S_z sectors
@pytest.mark.parametrize("n_sites,n_down", SECTORS)
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_sector_against_the_exact_reference(ctx, dtype, n_sites, n_down):
    psi, obs, want, bound = reference(n_sites, n_down, dtype)
    op = L.PauliSectorOperator(ctx, n_sites, n_down, G.heisenberg_terms(n_sites, 1.0, 0.8, periodic=False), dtype)
    assert op.n_local == psi.shape[0] == math.comb(n_sites, n_down)
    worst = 0.0
    try:
        for bits in BLOCK_BITS:
            _set_block_bits(ctx, "sector", bits)
            worst = max(worst, measure_everywhere(ctx, op, psi, obs, want, bound, sweeps_of(obs, dtype, True), (n_sites, n_down, bits)))
    finally:
        _set_block_bits(ctx, "sector", None)
        op.close()
    print("worst error / bound", np.dtype(dtype).char, (n_sites, n_down), worst)


# ------------------------------------------------------------------ 3. exact zeros, the identity, nothing to do
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_zero_rules_cost_no_sweep(ctx, dtype):
    n_sites, n_down = 9, 4
    psi_f = K.start_x(1 << n_sites, dtype)
    psi_s = K.start_x(math.comb(n_sites, n_down), dtype)
    full = L.PauliOperator(ctx, n_sites, [(0, 1, 1.0)], dtype)
    sect = L.PauliSectorOperator(ctx, n_sites, n_down, [(0, 1, 1.0)], dtype)
    try:
        odd_y = [(1, 1, 1.0), (7, 7, -2.0), (0x1f, 0x10, 0.5)]           # nY = 1, 3, 1
        got, nsw = full.expectation(psi_f, odd_y, return_sweeps=True)
        if _cplx(dtype):
            assert nsw == 1 and np.any(got != 0.0)
        else:   # imaginary and antisymmetric: not refused, exactly +0.0
            assert nsw == 0 and np.array_equal(got.view(np.uint64), np.zeros(3, np.uint64))
        odd_x = [(1, 0, 1.0), (7, 2, 3.0), (0x1f, 0, -1.0)]              # 1, 3, 5 flips leave the sector
        got, nsw = sect.expectation(psi_s, odd_x, return_sweeps=True)
        assert nsw == 0 and np.array_equal(got.view(np.uint64), np.zeros(3, np.uint64))
        # mixed with observables that need the sweep: the zeros stay +0.0, the others are answered
        mixed = [(1, 0, 1.0), (0, 0, 1.0), (3, 0, 0.5), (7, 2, 3.0)]
        got, nsw = sect.expectation(psi_s, mixed, return_sweeps=True)
        nn = E.dot_exact(psi_s, psi_s).real
        assert nsw == 1 and got[0] == 0.0 and got[3] == 0.0 and abs(got[1] - nn) <= E.dot_bound(psi_s, psi_s) + E.EPS_D * nn
        # nothing is divided by <psi|psi>: the identity returns ||psi||^2
        got = full.expectation(psi_f, [(0, 0, 1.0)])
        nn = E.dot_exact(psi_f, psi_f).real
        assert abs(got[0] - nn) <= E.dot_bound(psi_f, psi_f) + E.EPS_D * nn
        # n_obs = 0 is valid and touches nothing (no psi either)
        sweeps = C.c_int64(-1)
        capi.check(capi.lib().ll_pauli_expect(ctx.handle, full.handle, 0, None, None, None, C.byref(sweeps)))
        assert sweeps.value == 0
        got, nsw = full.expectation(psi_f, [], return_sweeps=True)
        assert got.shape == (0,) and nsw == 0
    finally:
        full.close()
        sect.close()


# ------------------------------------------------------------------ 4. physics
@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=["d", "z"])
def test_energy_of_the_open_transverse_field_chain(ctx, dtype):
    """Sum_t coef_t <P_t> over the Hamiltonian's own terms on its ground state from run(): the host's exact value within the summed
    bounds, and eigenvalue * <psi|psi> within the project's eigenvalue tolerance."""
    n_sites = 10
    terms = G.tfim_terms(n_sites, 1.0, 0.7)
    n = 1 << n_sites
    op = L.PauliOperator(ctx, n_sites, terms, dtype)
    try:
        _, vals, vecs = _run_lanczos(op, n, K.start_x(n, dtype, 3), False, -op.inf_norm())
        lam, psi = float(vals[0]), np.ascontiguousarray(vecs[0])
        got = op.expectation(psi, terms)
    finally:
        op.close()
    exact, bound = [], 0.0
    for t in terms:
        q = G.pauli_string_apply_np(n_sites, t, psi)
        exact.append(t[2] * E.dot_exact(psi, q).real)
        bound += abs(t[2]) * E.dot_bound(psi, q) + E.EPS_D * abs(exact[-1])
    energy, want = math.fsum(got), math.fsum(exact)   # (the sums over the terms: correctly rounded on both sides)
    print("energy", energy, "exact", want, "eigenvalue", lam, "summed bounds", bound)
    assert abs(energy - want) <= bound
    nn = E.dot_exact(psi, psi).real
    assert abs(energy - lam * nn) <= 1e-10 * max(1.0, abs(lam))
    assert abs(lam - G.tfim_ground_energy(n_sites, 1.0, 0.7)) <= 1e-10 * max(1.0, abs(lam))


def test_total_spin_of_the_heisenberg_singlet(ctx):
    """Sum_{i,j} <S_i . S_j> = <S_tot^2> = 0 on the ground state of the Heisenberg ring of 12 sites in the sector of 6 flipped
    spins (a singlet): S_i . S_j = (X X + Y Y + Z Z) / 4 for i != j and 3 / 4 for i = j."""
    n_sites, n_down = 12, 6
    terms = G.heisenberg_terms(n_sites, 1.0, 1.0, periodic=True)
    states = G.sector_states(n_sites, n_down)
    n = states.shape[0]
    op = L.PauliSectorOperator(ctx, n_sites, n_down, terms, np.float64)
    obs = [(0, 0, 0.75 * n_sites)]
    for i in range(n_sites):
        for j in range(i + 1, n_sites):
            m = (1 << i) | (1 << j)
            obs += [(m, 0, 0.5), (m, m, 0.5), (0, m, 0.5)]   # (i, j) and (j, i)
    try:
        _, vals, vecs = _run_lanczos(op, n, K.start_x(n, np.float64, 5), False, -op.inf_norm())
        lam, psi = float(vals[0]), np.ascontiguousarray(vecs[0])
        got, nsw = op.expectation(psi, obs, return_sweeps=True)
    finally:
        op.close()
    assert nsw == -(-len(obs) // BATCH)
    bound = 0.0
    for t, g in zip(obs, got):
        q = G.pauli_string_apply_np(n_sites, t, psi, states=states)
        w = t[2] * E.dot_exact(psi, q).real
        b = abs(t[2]) * E.dot_bound(psi, q) + E.EPS_D * abs(w)
        assert abs(g - w) <= b, t
        bound += b
    total = math.fsum(got)
    print("S_tot^2", total, "eigenvalue", lam, "summed bounds", bound)
    assert abs(total) <= bound + 1e-10 * max(1.0, abs(lam)) * n_sites ** 2


# ------------------------------------------------------------------ 5. refusals, each with its message
def _refused(fn, *needles):
    with pytest.raises(L.LanczosHipError) as e:
        fn()
    assert e.value.code == capi.LL_ERR_INVALID, str(e.value)
    for needle in needles:
        assert needle in str(e.value), (needle, str(e.value))


def test_refusals(ctx):
    n_sites = 4
    psi = K.start_x(16, np.float64)
    one = [(0, 1, 1.0)]
    csr = L.CsrOperator(ctx, *G.laplace2d_np(4))
    mom = L.PauliMomentumFullOperator(ctx, n_sites, 0, G.tfim_terms(n_sites, 1.0, 0.7, periodic=True), np.float64)
    full = L.PauliOperator(ctx, n_sites, one, np.float64)
    try:
        _refused(lambda: L.pauli_expect(csr, psi, one), "a CSR operator")
        _refused(lambda: L.pauli_expect(mom, K.start_x(mom.n_local, np.float64), one), "a momentum block of the full space",
                 "symmetrised observables are not built")
        _refused(lambda: full.expectation(psi, [(0, 1, 1.0), (16, 0, 1.0)]), "observable 1", "a mask bit at or above n_sites")
        _refused(lambda: full.expectation(psi, [(0, 16, 1.0)]), "observable 0", "a mask bit at or above n_sites")
        _refused(lambda: full.expectation(psi, [(1, 0, float("nan"))]), "observable 0", "the coefficient is not finite")
        _refused(lambda: full.expectation(psi, [(1, 0, float("inf"))]), "the coefficient is not finite")
        arr = (capi.PauliTerm * 1)()
        arr[0].x_mask, arr[0].z_mask, arr[0].coef = 0, 1, 1.0
        out = np.zeros(1)
        st = capi.lib().ll_pauli_expect(ctx.handle, full.handle, 1, arr, None, out.ctypes.data_as(C.POINTER(C.c_double)), None)   # a null psi with n_obs > 0
        assert st == capi.LL_ERR_INVALID and b"null argument" in capi.lib().ll_last_error()
        st = capi.lib().ll_pauli_expect(ctx.handle, full.handle, 1, arr, capi.ptr(psi), None, None)
        assert st == capi.LL_ERR_INVALID and b"null argument" in capi.lib().ll_last_error()
        # the operator still measures after the refusals
        assert abs(full.expectation(psi, [(0, 0, 1.0)])[0] - E.dot_exact(psi, psi)) <= E.dot_bound(psi, psi) + E.EPS_D * 16
    finally:
        for o in (csr, mom, full):
            o.close()
