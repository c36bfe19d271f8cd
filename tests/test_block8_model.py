"""Blocks of EIGHT Lanczos iterations per sweep behind the measured guard (kBlock8Tau / kBlock8Quiet in
csrc/ll_internal.hpp, LoopState::collect and enqueue_block_f64), in the numpy model the device code was written from
(tools/block_gs_model.py: run_guarded; its numbers: profiles/block8_model.txt).  The device kernels are checked against the oracle
in tests/test_gpu_block8.py.

The reference is full re-orthogonalisation (model.reference), run ONCE per problem to 1 024 iterations: its first K alpha / beta
are its run of K.  Tolerance for alpha and beta: 1e-10 ||A||_inf, the device suite's."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = (100, 300, 1024)


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location("block_gs_model", os.path.join(ROOT, "tools", "block_gs_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


_cache = {}


def problem(model, name, complex_):
    """(A, v0, reference alpha, reference beta) of 'model' (the model's own problem) or 'config3' (the flagship's type), n = 2 000."""
    if (name, complex_) not in _cache:
        A, v0 = model.make_problem(2000, complex_) if name == "model" else model.config3_problem(2000, complex_)
        ra, rb, _ = model.reference(A, v0, max(WINDOWS))
        _cache[(name, complex_)] = (A, v0, ra, rb)
    return _cache[(name, complex_)]


def guarded(model, A, v0, K, **kw):
    with np.errstate(all="ignore"):
        return model.run_guarded(A, v0, K, **kw)


@pytest.mark.parametrize("K", WINDOWS)
@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("name", ["model", "config3"])
def test_eights_behind_the_guard_reproduce_full_reorthogonalisation(model, name, complex_, K):
    A, v0, ra, rb = problem(model, name, complex_)
    L = guarded(model, A, v0, K)
    al, be = np.array(L.al), np.array(L.be)
    da, db, tol = np.abs(al - ra[:K]).max(), np.abs(be - rb[:K]).max(), 1e-10 * model.norm_inf(A)
    print("%s %s K = %d: dalpha %.2e dbeta %.2e (tolerance %.2e) largest relative coefficient %.2e, in eights %d, blocks %s" % (
        name, "complex" if complex_ else "real", K, da, db, tol, L.maxcoef, L.n8, L.sizes[:8]))
    assert len(al) == K and sum(L.sizes) == K - 2      # never past K: two entry iterations, then the blocks
    assert da <= tol and db <= tol and L.gate_trips == 0
    assert L.n8 >= K // 2                              # most of the window runs in eights
    assert L.sizes[:5] == [4, 4, 4, 4, 8]              # kBlock8Quiet = 12 collected iterations, seen one block late


@pytest.mark.parametrize("K,tail", [(100, [2]), (101, [2, 1]), (102, [4]), (107, [8, 1]), (109, [8, 2, 1]), (113, [8, 4, 2, 1])])
def test_the_block_order_before_max_iteration(model, K, tail):
    """8, then 4, 2, 1 where fewer iterations remain: 2 + 16 + 8 j iterations are behind the blocks of eight."""
    A, v0, ra, rb = problem(model, "config3", False)
    L = guarded(model, A, v0, K)
    full = (K - 18) // 8
    assert L.sizes == [4, 4, 4, 4] + [8] * (full - (1 if tail[0] == 8 else 0)) + tail and len(L.al) == K
    assert np.abs(np.array(L.al) - ra[:K]).max() <= 1e-10 * model.norm_inf(A)


@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("seed", [0, 2, 4, 7])
def test_the_outlier_matrix_stays_at_four(model, seed, complex_):
    """A Ritz value converged to a dominant outlier: rounding along it grows by r ~ 13 per application.  The guard admits no block
    of eight and the run IS the run in blocks of four.  A guard on ONE quiet block at 1.6e-13 (ten times under the gate by g (g / eps)^(4/3)) admits one in
    the second or third block, before the growth shows (seeds 2 and 4 are those a shorter run of quiet iterations lets through)."""
    A, v0 = model.outlier_problem(4000, complex_, seed)
    L = guarded(model, A, v0, 100)
    with np.errstate(all="ignore"):
        L4 = model.run_loop(A, v0, 100, 4)
    assert L.n8 == 0 and 8 not in L.sizes and L.gate_trips == 0
    assert np.array_equal(L.al, L4.al) and np.array_equal(L.be, L4.be) and L.maxcoef == L4.maxcoef
    one_block = guarded(model, A, v0, 100, tau=1.6e-13, quiet_need=1)
    assert one_block.n8 > 0 and one_block.maxcoef > 10 * L.maxcoef


@pytest.mark.parametrize("pos", range(8))
def test_a_planted_component_is_caught_in_every_position_of_a_block_of_eight(model, pos):
    """1e-6 along stored vectors in vector pos + 1 of the block of eight that starts at vector 27: the fold measures it, the gate
    trips, the vector stands and single iterations finish the pass within the tolerance."""
    A, v0, ra, rb = problem(model, "config3", False)
    L = guarded(model, A, v0, 120, plant=(1e-6, 27, pos))
    assert L.sizes[:6] == [4, 4, 4, 4, 8, 8]           # (vectors 19 .. 26, then 27 .. 34)
    assert L.gate_trips == 1 and 0.5e-6 <= L.maxcoef <= 5e-6
    tol = 1e-10 * model.norm_inf(A)
    assert len(L.al) == 120 and np.abs(np.array(L.al) - ra[:120]).max() <= tol and np.abs(np.array(L.be) - rb[:120]).max() <= tol


def _drop_the_compensations(p, M):
    if len(p) == 8:
        p[4:] = 0


def _zero_the_measured_columns_of_the_last_four(p, M):
    if M.shape[1] == 8:
        M[:, 4:] = 0


def _compensate_last_vector_only(p, M):
    if len(p) == 8:
        p[-2] = 0


def _double_the_last_prediction(p, M):
    if len(p) == 8:
        p[-1] *= 2


@pytest.mark.parametrize("mutate", [_drop_the_compensations, _zero_the_measured_columns_of_the_last_four, _compensate_last_vector_only,
                                    _double_the_last_prediction], ids=lambda f: f.__name__.strip("_"))
def test_a_mutated_prediction_or_column_is_detected(model, mutate):
    """Stand-ins for a device kernel that gets the part of a block of eight wrong that a block of four does not have (they touch
    blocks of eight only), 300 iterations.  Two lines of defence.  With the guard switched off (tau = inf) the coefficients grow
    from block to block until the gate trips.  With the guard as shipped they never get that far: the first wrong block publishes
    a coefficient more than a hundred times above the guard's threshold, the guard falls back to blocks of four — which the mutant does not
    touch — and alpha / beta stay within the tolerance."""
    A, v0, ra, rb = problem(model, "config3", False)
    tol = 1e-10 * model.norm_inf(A)
    clean = guarded(model, A, v0, 300)
    assert clean.maxcoef <= 1e-13 and clean.n8 == 280
    off = guarded(model, A, v0, 300, mutate=mutate, tau=np.inf)
    L = guarded(model, A, v0, 300, mutate=mutate)
    da, db = np.abs(np.array(L.al) - ra[:300]).max(), np.abs(np.array(L.be) - rb[:300]).max()
    print("%s: guard off: largest relative coefficient %.2e gate trips %d; guard on: dalpha %.2e dbeta %.2e coefficient %.2e in eights %d" % (
        mutate.__name__, off.maxcoef, off.gate_trips, da, db, L.maxcoef, L.n8))
    assert off.gate_trips == 1 and off.maxcoef > 1e-8
    assert L.gate_trips == 0 and 100 * model.TAU <= L.maxcoef <= 1e-8 and L.n8 < clean.n8
    assert da <= tol and db <= tol
