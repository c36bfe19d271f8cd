"""The four measuring kernels (csrc/pauli_expect.hip: pauli_expect_kernel, pauli_expect_sector_kernel; csrc/pauli_rdm.hip:
pauli_rdm_kernel, pauli_rdm_sector_kernel) on 20 to 30 sites — the sizes they exist for.  What the 14-site files
(tests/test_gpu_pauli_expect.py, tests/test_gpu_pauli_rdm.py) never reach: the second and later trips of the persistent
workgroups' grid-stride loops (the barrier that guards the LDS tile, the accumulators carried from trip to trip, workgroups with
one trip more than their neighbours), the grids of 240, 481, 910 and 1820 workgroups that the partial-buffer cap gives at
m = 5, 6, state and mask bits 14 to 29, partner tiles and tile parities with more than 8 tile bits, rank tables of 2^15 entries,
2^29 environment configurations, super-tile numbers above 2^8.  The cases and their trip counts: tests/pauli_measure_large_cases.py
and tests/test_pauli_measure_large_host.py.

The instrument is an integer state (parts from +-{1 .. 7}): every product and every partial sum is an integer below 2^53, exact
in double in any order, so the kernels must return the host's integers — `==`, tolerance zero, by derivation
(pauli_measure_large_cases.exact_condition); a missed, repeated or misaddressed tile changes the integer, and so does an
accumulator reset between trips or a float accumulation (the sums pass 2^24).  Rounding is the 14-site files' subject; one
random-amplitude case per kernel at 20 sites ties the two together at THEIR bound (exact_ref.dot_exact, dot_bound plus one double
rounding) — no new tolerance.

Measured on one MI355X: the 77 cases take 12 s together; the slowest are the expectation values at 23 (z) and 24 (d) sites, 2.1 and
1.8 s, of which 1.8 and 1.5 s are the host reference (40 observables on 2^24 numbers), then the sector (24, 12) at 1.5 and 1.0 s;
every other case is below 0.2 s.  (30, 4) at m = 6 — 240 workgroups walking 2^30 pairs in z — takes 0.02 s for its three
placements, so it runs in all four types.  Every test prints its units, grid, GPU and host-reference time."""
import math
import time

import numpy as np
import pytest

import contract_cases as K
import exact_ref as E
import lambda_lanczos_amd as L
import pauli_large_cases as PL
import pauli_measure_large_cases as C
from guarded import guarded, unguard
from lambda_lanczos_amd import generators as G
from test_gpu_pauli_expect import check_values
from test_gpu_pauli_rdm import check_rho, reference as rdm_reference

pytestmark = pytest.mark.gpu

NAN_FILL = 0xFF          # every byte 0xFF: a NaN in all four storage types
SEED = 2024


def _full_operator(ctx, n_sites, dtype):
    return L.PauliOperator(ctx, n_sites, [(0, 1, 1.0)], dtype)                  # the Hamiltonian's terms play no part


def _sector_operator(ctx, n_sites, n_down, dtype):
    return L.PauliSectorOperator(ctx, n_sites, n_down, G.heisenberg_terms(n_sites, 1.0, 0.8, periodic=True), dtype)


def everywhere(ctx, psi, measure, sweeps, what):
    """measure(psi) -> (result, sweeps) with psi in guarded, NaN-padded device buffers at shift 0 and 1 (for every type but
    complex double shift 1 is off the 16-byte grid: the element-wise loads) and on the host: the same bits every time, psi
    unchanged, the guards intact, the sweeps as planned.  Returns the result."""
    n = psi.shape[0]
    first = None
    for shift in (0, 1):
        buf, view = guarded(ctx, psi, shift, NAN_FILL)
        try:
            got, nsw = measure(view)
            assert nsw == sweeps, (what, shift, nsw, sweeps)
            if first is None:
                first = got
            assert np.array_equal(first.view(np.uint8), got.view(np.uint8)), (what, "device, shift", shift)
            assert np.array_equal(unguard(buf, n, shift, NAN_FILL), psi), (what, "the measurement changed psi")
        finally:
            buf.free()
    got, nsw = measure(psi)
    assert nsw == sweeps and np.array_equal(first.view(np.uint8), got.view(np.uint8)), (what, "host psi")
    return first


def assert_exact_values(got, want, obs, cplx, sector, what):
    assert got.dtype == np.float64 and got.shape == want.shape
    bad = np.flatnonzero(~(got == want))
    assert bad.size == 0, (what, "%d of %d values differ" % (bad.size, got.size), [(int(j), obs[j], got[j], want[j]) for j in bad[:4]])
    for j, t in enumerate(obs):
        if C.is_zero(t, cplx, sector):
            assert got[j] == 0.0 and not np.signbit(got[j]), (what, j, "a zero by rule is not +0.0")
    check_values(got, want, np.zeros(len(obs)), what)                           # the 14-site file's check at bound 0


def assert_exact_rho(got, want, dtype, n_down, what):
    bad = np.argwhere(~(got == want))
    assert bad.shape[0] == 0, (what, "%d of %d entries differ" % (bad.shape[0], got.size),
                               [(tuple(j), got[tuple(j)], want[tuple(j)]) for j in bad[:4]])
    # the 14-site file's checks at bound 0: Hermitian bit for bit, every zero +0.0, a real rho for real storage, the exact
    # zeros at the popcount-off-diagonal entries of a sector
    check_rho(got, want, np.zeros(want.shape), dtype, n_down, what)


# ------------------------------------------------------------------ the integer references, once per module
_STATE, _EXPECT, _RHO = {}, {}, {}
HOST_SECONDS = {}       # reference -> seconds on the host (printed by the tests)


def _state(tid, n_sites, n_down):
    key = (tid, n_sites, n_down)
    if key not in _STATE:
        n = (1 << n_sites) if n_down is None else math.comb(n_sites, n_down)
        assert C.exact_condition(n)
        psi = C.integer_state(n, C.TYPES[tid], SEED + n_sites)
        psi.setflags(write=False)
        _STATE[key] = psi
    return _STATE[key]


def expect_reference(tid, n_sites, n_down, k):
    """(psi, observables, coef * float(S)) around the boundary k, computed once and left unchanged."""
    key = (tid, n_sites, n_down, k)
    if key not in _EXPECT:
        cplx, sector = tid in "zc", n_down is not None
        psi = _state(tid, n_sites, n_down)
        obs = C.observables(n_sites, k, cplx, sector)
        t0 = time.perf_counter()
        sums = C.expect_sums_sector(n_sites, n_down, psi, obs) if sector else C.expect_sums_full(n_sites, psi, obs)
        HOST_SECONDS[("expect",) + key] = time.perf_counter() - t0
        want = C.expect_values(sums, obs, cplx, sector)
        assert np.count_nonzero(want) > len(obs) // 2
        want.setflags(write=False)
        _EXPECT[key] = (psi, obs, want)
    return _EXPECT[key]


def rho_reference(tid, n_sites, n_down, sites):
    key = (tid, n_sites, n_down, tuple(sites))
    if key not in _RHO:
        psi = _state(tid, n_sites, n_down)
        t0 = time.perf_counter()
        fib = C.full_fibres(n_sites, sites, psi) if n_down is None else C.sector_fibres(n_sites, n_down, sites, psi)
        want = C.gram(fib)
        HOST_SECONDS[("rho",) + key] = time.perf_counter() - t0
        assert np.array_equal(want.real, np.rint(want.real)) and np.array_equal(want.imag, np.rint(want.imag))
        wide = psi.astype(np.complex128)
        assert want.real.diagonal().sum() == float(np.sum(wide.real ** 2 + wide.imag ** 2))     # tr rho = ||psi||^2, an integer
        want.setflags(write=False)
        _RHO[key] = (psi, want)
    return _RHO[key]


# ------------------------------------------------------------------ 1. expectation values, the full space
@pytest.mark.parametrize("case", C.EXPECT_FULL, ids=[C.case_id(c) for c in C.EXPECT_FULL])
def test_expectation_on_the_full_space_equals_the_integer_reference(ctx, case):
    tid, n_sites, bits = case
    dtype = C.TYPES[tid]
    k = C.expect_tile_bits(n_sites, np.dtype(dtype).itemsize, bits)
    units, grid = C.launch_of("expect_full", case)
    psi, obs, want = expect_reference(tid, n_sites, None, k)
    sweeps = -(-C.slots_of(obs, tid in "zc", False) // C.EXPECT_BATCH)
    assert sweeps == 2
    op = _full_operator(ctx, n_sites, dtype)
    t0 = time.perf_counter()
    try:
        ctx.set_tuning("pauli_tile_bits", None if bits is None else str(bits))
        got = everywhere(ctx, psi, lambda p: op.expectation(p, obs, return_sweeps=True), sweeps, case)
    finally:
        ctx.set_tuning("pauli_tile_bits", None)
        op.close()
    print("expectation, full space", case, "tiles", units, "grid", grid, "three placements %.2f s" % (time.perf_counter() - t0),
          "host reference %.2f s" % HOST_SECONDS[("expect", tid, n_sites, None, k)])
    assert_exact_values(got, want, obs, tid in "zc", False, case)


# ------------------------------------------------------------------ 2. expectation values, S_z sectors
@pytest.mark.parametrize("case", C.EXPECT_SECTOR, ids=[C.case_id(c) for c in C.EXPECT_SECTOR])
def test_expectation_on_a_sector_equals_the_integer_reference(ctx, case):
    tid, (n_sites, n_down), which = case
    dtype = C.TYPES[tid]
    h = (n_sites + 1) // 2                                                       # the split of the rank tables
    units, grid = C.launch_of("expect_sector", case)
    psi, obs, want = expect_reference(tid, n_sites, n_down, h)
    bits = C.sector_block_bits(psi.shape[0], which)
    sweeps = -(-C.slots_of(obs, tid in "zc", True) // C.EXPECT_BATCH)
    assert sweeps == 2
    op = _sector_operator(ctx, n_sites, n_down, dtype)
    t0 = time.perf_counter()
    try:
        assert op.n_local == psi.shape[0]
        ctx.set_tuning("pauli_sector_block_bits", None if bits is None else str(bits))
        got = everywhere(ctx, psi, lambda p: op.expectation(p, obs, return_sweeps=True), sweeps, case)
    finally:
        ctx.set_tuning("pauli_sector_block_bits", None)
        op.close()
    print("expectation, sector", case, "blocks", units, "grid", grid, "three placements %.2f s" % (time.perf_counter() - t0),
          "host reference %.2f s" % HOST_SECONDS[("expect", tid, n_sites, n_down, h)])
    assert_exact_values(got, want, obs, tid in "zc", True, case)


# ------------------------------------------------------------------ 3. reduced density matrices, the full space
@pytest.mark.parametrize("case", C.RDM_FULL, ids=[C.case_id(c[:4]) for c in C.RDM_FULL])
def test_rdm_on_the_full_space_equals_the_integer_reference(ctx, case):
    tid, n_sites, sites, bits, units, grid = case
    dtype = C.TYPES[tid]
    assert C.launch_of("rdm_full", case) == (units, grid)
    psi, want = rho_reference(tid, n_sites, None, sites)
    op = _full_operator(ctx, n_sites, dtype)
    t0 = time.perf_counter()
    try:
        ctx.set_tuning("pauli_rdm_tile_bits", None if bits is None else str(bits))
        got = everywhere(ctx, psi, lambda p: op.reduced_density_matrix(p, sites, return_sweeps=True), 1, case)
    finally:
        ctx.set_tuning("pauli_rdm_tile_bits", None)
        op.close()
    print("rdm, full space", case[:4], "super-tiles", units, "grid", grid, "three placements %.2f s" % (time.perf_counter() - t0),
          "host reference %.2f s" % HOST_SECONDS[("rho", tid, n_sites, None, tuple(sites))])
    assert_exact_rho(got, want, dtype, None, case)


# ------------------------------------------------------------------ 4. reduced density matrices, S_z sectors
@pytest.mark.parametrize("case", C.RDM_SECTOR, ids=[C.case_id(c) for c in C.RDM_SECTOR])
def test_rdm_on_a_sector_equals_the_integer_reference(ctx, case):
    tid, (n_sites, n_down), sites, bits = case
    dtype = C.TYPES[tid]
    units, grid = C.launch_of("rdm_sector", case)
    psi, want = rho_reference(tid, n_sites, n_down, sites)
    op = _sector_operator(ctx, n_sites, n_down, dtype)
    t0 = time.perf_counter()
    try:
        assert op.n_local == psi.shape[0]
        ctx.set_tuning("pauli_rdm_block_bits", None if bits is None else str(bits))
        got = everywhere(ctx, psi, lambda p: op.reduced_density_matrix(p, sites, return_sweeps=True), 1, case)
    finally:
        ctx.set_tuning("pauli_rdm_block_bits", None)
        op.close()
    print("rdm, sector", case, "batches", units, "grid", grid, "three placements %.2f s" % (time.perf_counter() - t0),
          "host reference %.2f s" % HOST_SECONDS[("rho", tid, n_sites, n_down, tuple(sites))])
    assert_exact_rho(got, want, dtype, n_down, case)


# ------------------------------------------------------------------ 5. random amplitudes at the bound of the 14-site files
def _expect_bound_reference(n_sites, n_down, dtype, obs):
    """(psi, want, bound) as tests/test_gpu_pauli_expect.py's reference() forms them."""
    states = None if n_down is None else G.sector_states(n_sites, n_down)
    psi = K.start_x((1 << n_sites) if states is None else states.shape[0], dtype)
    want, bound = np.zeros(len(obs)), np.zeros(len(obs))
    for j, t in enumerate(obs):
        q = G.pauli_string_apply_np(n_sites, t, psi, states=states)
        want[j] = t[2] * E.dot_exact(psi, q).real
        bound[j] = abs(t[2]) * E.dot_bound(psi, q) + E.EPS_D * abs(want[j])      # + one double rounding of the result
    return psi, want, bound


def test_random_amplitudes_expectation_on_the_full_space(ctx):
    """s, 20 sites, 12 observables, tiles of 64 states (8 trips)."""
    n_sites, dtype, bits = 20, np.float32, 6
    obs = C.observables(n_sites, bits, False, False)[:12]
    assert sum(1 for x, _, _ in obs if x >> bits) >= 4 and C.slots_of(obs, False, False) == 11
    psi, want, bound = _expect_bound_reference(n_sites, None, dtype, obs)
    op = _full_operator(ctx, n_sites, dtype)
    try:
        ctx.set_tuning("pauli_tile_bits", str(bits))
        got = everywhere(ctx, psi, lambda p: op.expectation(p, obs, return_sweeps=True), 1, "random, expectation, full")
    finally:
        ctx.set_tuning("pauli_tile_bits", None)
        op.close()
    print("worst error / bound", "s", n_sites, check_values(got, want, bound, "random, expectation, full"))


def test_random_amplitudes_expectation_on_a_sector(ctx):
    """d, (20, 10), 12 observables, blocks of 16 indices (11548 blocks)."""
    n_sites, n_down, dtype = 20, 10, np.float64
    obs = C.observables(n_sites, 10, False, True)[:12]
    psi, want, bound = _expect_bound_reference(n_sites, n_down, dtype, obs)
    op = _sector_operator(ctx, n_sites, n_down, dtype)
    try:
        ctx.set_tuning("pauli_sector_block_bits", str(PL.small_bits(psi.shape[0])))
        got = everywhere(ctx, psi, lambda p: op.expectation(p, obs, return_sweeps=True), 1, "random, expectation, sector")
    finally:
        ctx.set_tuning("pauli_sector_block_bits", None)
        op.close()
    print("worst error / bound", "d", (n_sites, n_down), check_values(got, want, bound, "random, expectation, sector"))


def test_random_amplitudes_rdm_on_the_full_space(ctx):
    """z, 20 sites, sites [3, 19], tiles of 64 states (four trips) and the default tile."""
    n_sites, sites, dtype = 20, [3, 19], np.complex128
    assert C.rdm_full_launch(n_sites, sites, dtype, 6) == (8192, 2048)
    psi, want, bound = rdm_reference(n_sites, None, sites, dtype)
    op = _full_operator(ctx, n_sites, dtype)
    worst = 0.0
    try:
        for bits in (6, None):
            ctx.set_tuning("pauli_rdm_tile_bits", None if bits is None else str(bits))
            got = everywhere(ctx, psi, lambda p: op.reduced_density_matrix(p, sites, return_sweeps=True), 1, ("random, rdm, full", bits))
            worst = max(worst, check_rho(got, want, bound, dtype, None, ("random, rdm, full", bits)))
    finally:
        ctx.set_tuning("pauli_rdm_tile_bits", None)
        op.close()
    print("worst error / bound", "z", n_sites, sites, worst)


def test_random_amplitudes_rdm_on_a_sector(ctx):
    """d, (20, 10), m = 3 across the rank split, 16 configurations per batch (8192 batches, four trips)."""
    n_sites, n_down, sites, dtype, bits = 20, 10, [19, 9, 10], np.float64, 4
    assert C.rdm_sector_launch(n_sites, len(sites), dtype, bits) == (8192, 2048)
    psi, want, bound = rdm_reference(n_sites, n_down, sites, dtype)
    op = _sector_operator(ctx, n_sites, n_down, dtype)
    try:
        ctx.set_tuning("pauli_rdm_block_bits", str(bits))
        got = everywhere(ctx, psi, lambda p: op.reduced_density_matrix(p, sites, return_sweeps=True), 1, "random, rdm, sector")
    finally:
        ctx.set_tuning("pauli_rdm_block_bits", None)
        op.close()
    print("worst error / bound", "d", (n_sites, n_down), sites, check_rho(got, want, bound, dtype, n_down, "random, rdm, sector"))
