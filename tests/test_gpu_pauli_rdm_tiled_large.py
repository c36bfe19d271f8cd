"""ll_pauli_rdm_tiled (csrc/pauli_rdm_tiled.hip) at the sizes it exists for, on INTEGER states built as
tests/pauli_measure_large_cases.py builds them: every product is an integer of magnitude at most 98 and every partial sum an integer
below 2^53 — exact in double in ANY summation order, whatever the matrix core does inside an instruction — so rho must equal the
host's integer product F F^H entry by entry, tolerance zero.  The full space of 20 sites at m = 10 (136 macro-tiles, split-K by
the default rule) in d and z; 22 sites at m = 8 with the default KC and ksplit (several K-steps and slices per workgroup); the
sector (20, 10) at m = 8.  A wrong lane map of v_mfma_f64_16x16x4_f64 puts exact integers into wrong entries: this is also the
check of the hardware's map against the plan's functions that exact integer data give."""
import numpy as np
import pytest

import lambda_lanczos_amd as L
import pauli_measure_large_cases as C
from lambda_lanczos_amd import generators as G
from test_gpu_pauli_rdm import check_rho

pytestmark = pytest.mark.gpu

TEN_20 = [19, 0, 3, 5, 6, 9, 11, 14, 16, 17]
EIGHT_22 = [21, 1, 2, 7, 8, 12, 15, 20]
EIGHT_20 = [0, 19, 4, 5, 9, 10, 13, 18]


def _measure(ctx, op, psi, sites, n_down, what):
    """psi on the device and on the host: the same bits, every entry the host's integer, the Hermitian contract."""
    fib = C.full_fibres(op.n_sites, sites, psi) if n_down is None else C.sector_fibres(op.n_sites, n_down, sites, psi)
    assert C.exact_condition(fib.shape[1])
    want = C.gram(fib)
    dpsi = ctx.to_device(psi)
    try:
        got = op.reduced_density_matrix_tiled(dpsi, sites)
    finally:
        dpsi.free()
    wrong = np.argwhere(got != want)
    assert wrong.shape[0] == 0, (what, "entries that differ", wrong.shape[0], "the first", wrong[0], got[tuple(wrong[0])], want[tuple(wrong[0])])
    check_rho(got, want, np.zeros(want.shape), psi.dtype, n_down, what)
    host = op.reduced_density_matrix_tiled(psi, sites)
    assert np.array_equal(host.view(np.uint8), got.view(np.uint8)), (what, "psi on the host")


@pytest.mark.parametrize("tid", ["d", "z"])
def test_twenty_sites_half_chain_equals_the_integer_reference(ctx, tid):
    dtype = C.TYPES[tid]
    psi = C.integer_state(1 << 20, dtype, seed=20)
    op = L.PauliOperator(ctx, 20, [(0, 1, 1.0)], dtype)
    try:
        _measure(ctx, op, psi, TEN_20, None, ("20 sites, m = 10", tid))
    finally:
        op.close()


@pytest.mark.parametrize("tid", ["d", "c"])
def test_many_k_steps_and_slices_per_workgroup(ctx, tid):
    """22 sites at m = 8, default KC = 16 and ksplit = 64: 1024 K-steps, 16 per workgroup, ten macro-tiles."""
    dtype = C.TYPES[tid]
    psi = C.integer_state(1 << 22, dtype, seed=22)
    op = L.PauliOperator(ctx, 22, [(0, 1, 1.0)], dtype)
    try:
        _measure(ctx, op, psi, EIGHT_22, None, ("22 sites, m = 8", tid))
    finally:
        op.close()


@pytest.mark.parametrize("tid", ["d", "z"])
def test_sector_of_twenty_sites_equals_the_integer_reference(ctx, tid):
    dtype = C.TYPES[tid]
    n_sites, n_down = 20, 10
    psi = C.integer_state(G.sector_states(n_sites, n_down).shape[0], dtype, seed=2010)
    op = L.PauliSectorOperator(ctx, n_sites, n_down, G.heisenberg_terms(n_sites, 1.0, 0.8, periodic=False), dtype)
    try:
        assert op.n_local == psi.shape[0]
        _measure(ctx, op, psi, EIGHT_20, n_down, ("sector (20, 10), m = 8", tid))
    finally:
        op.close()
