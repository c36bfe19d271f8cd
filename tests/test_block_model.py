"""The algebra of the block form of the Gram-Schmidt step — up to four Lanczos iterations per sweep over a basis of raw vectors
that is never rewritten (gs_block.hip, LoopState::enqueue_block) — in numpy, at a size the CPU suite runs in
seconds.  tools/block_gs_model.py is the executable specification the device kernels were written from (same launches, same
formulas, real and complex); the GPU kernels themselves are checked against the oracle in tests/test_gpu_block.py."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location("block_gs_model", os.path.join(ROOT, "tools", "block_gs_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("m", [2, 4])
@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
def test_block_form_reproduces_the_recurrence_of_full_reorthogonalisation(model, complex_, m):
    r = model.measure(complex_, m, n=1500, K=120)
    assert r["iterations"] == 120 and r["gate_trips"] == 0
    assert r["dalpha"] <= 1e-12 and r["dbeta"] <= 1e-12
    assert r["orth"] <= 1e-14                          # the basis the record defines
    assert r["maxcoef"] <= 1e-12                       # every coefficient of a raw vector stays eps-sized
    assert abs(r["ritz"]) <= 1e-14                     # the Ritz vector through transformed coefficients
    assert r["orth_flushed"] <= 1e-14 and r["dvec_flushed"] <= 1e-11   # the flush completes the raw vectors in place


def test_both_seeds_must_be_compensated(model):
    """With only the last vector of a block compensated the stored-basis components of the other operand of the next three-term
    update survive and are amplified from block to block."""
    r = model.measure(False, 4, n=1500, K=100, both_seeds=False, gate=np.inf)
    assert r["maxcoef"] >= 1e-8


@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
def test_entry_from_the_pair_state_and_an_odd_last_iteration(model, complex_):
    r = model.pair_entry(complex_, n=1200, K=61, at=21)
    assert r["iterations"] == 61 and r["dalpha"] <= 1e-12 and r["dbeta"] <= 1e-12 and r["orth_flushed"] <= 1e-14


@pytest.mark.parametrize("stop", [41, 42, 43, 44])
def test_a_stop_inside_a_block_reads_nothing_behind_it(model, stop):
    r = model.stop_in_block(stop % 2 == 0, stop, n=1200)
    assert r["dropped"] == (2 - stop) % 4
    assert r["dlambda"] <= 1e-12 and abs(r["ritz"]) <= 1e-14 and r["dnorm"] <= 1e-14


@pytest.mark.parametrize("size,pos,trips", [(1e-9, 3, 0), (1e-6, 0, 1), (1e-6, 3, 1), (1e-3, 2, 1)])
def test_planted_components_and_the_gate(model, size, pos, trips):
    """Below the gate planted components are measured and leave no trace; above it the vector stands, the rest of its block is
    dropped, the basis is flushed and single iterations finish the pass — within the recurrence's tolerance either way."""
    r = model.measure(False, 4, n=1500, K=120, plant=(size, 23, pos))
    assert r["gate_trips"] == trips and 0.5 * size <= r["maxcoef"] <= 5 * size
    assert r["dalpha"] <= 1e-12 and r["dbeta"] <= 1e-12 and r["orth_flushed"] <= 1e-14


# ---------------------------------------------------------------------------------------------------------------------------
# Why tests/test_gpu_block_long.py runs windows of 700 and 1 024 iterations: a fault in anything indexed past 255 (the second trip
# of every strided loop of block_predict_kernel / block_fold_kernel, waves 2 and 3 of their reductions) is invisible in a window of
# 41 stored vectors and an O(1) error by 700.  Mutants of the model through BlockLoop's mutate hook, m = 4, gate off.
def _drop_predictions_from_256(p, M):
    p[:, 256:] = 0


def _zero_measured_from_256(p, M):
    M[256:] = 0


def _compensate_last_vector_only(p, M):
    if len(p) >= 2:
        p[-2] = 0


MUTANTS = {"prediction columns >= 256 dropped": _drop_predictions_from_256, "measured columns M[256:] zeroed": _zero_measured_from_256,
           "only the last vector of a block compensated": _compensate_last_vector_only}


def _long_problem(n, complex_):
    import block_long_cases as B
    from lambda_lanczos_amd import generators as G

    A = B.as_sparse(B.long_chain(n, complex_))
    v0 = G.start_vector(n, 5, np.complex128 if complex_ else np.float64)
    return A, v0 / np.linalg.norm(v0)


def _full_reorthogonalisation(A, v0, K):
    """The recurrence with every new vector orthogonalised twice against all its predecessors (classical Gram-Schmidt, twice: the
    same vectors as model.reference's sequential sweep to a few ulp, as matrix products)."""
    U = np.zeros((K + 1, v0.shape[0]), dtype=v0.dtype)
    U[0] = v0
    al, be = np.zeros(K), np.zeros(K)
    for k in range(1, K + 1):
        w = A @ U[k - 1]
        al[k - 1] = np.vdot(U[k - 1], w).real
        w = w - al[k - 1] * U[k - 1] - (be[k - 2] * U[k - 2] if k > 1 else 0)
        for _ in range(2):
            w = w - np.conj(U[:k] @ np.conj(w)) @ U[:k]
        be[k - 1] = np.linalg.norm(w)
        U[k] = w / be[k - 1]
    return al, be


def _run_model(model, A, v0, K, mutate=None):
    with np.errstate(all="ignore"):
        L = model.run_loop(A, v0, K, 4, gate=np.inf, mutate=mutate)
    return np.array(L.al[:K]), np.array(L.be[:K]), L.maxcoef


@pytest.fixture(scope="module")
def short_long_problem(model):
    A, v0 = _long_problem(1500, False)
    ra, rb = _full_reorthogonalisation(A, v0, 700)
    return A, v0, ra, rb


def test_a_window_of_41_cannot_see_a_fault_past_column_255(model, short_long_problem):
    A, v0, ra, rb = short_long_problem
    al, be, coef = _run_model(model, A, v0, 41)
    assert np.abs(al - ra[:41]).max() <= 1e-12 and np.abs(be - rb[:41]).max() <= 1e-12
    for name in ("prediction columns >= 256 dropped", "measured columns M[256:] zeroed"):
        mal, mbe, mcoef = _run_model(model, A, v0, 41, MUTANTS[name])
        assert np.array_equal(mal, al) and np.array_equal(mbe, be) and mcoef == coef, name


@pytest.mark.parametrize("name", list(MUTANTS))
def test_a_window_of_700_sees_every_mutant(model, short_long_problem, name):
    """At 700 iterations every mutant misses the device tests' tolerance for alpha or beta (1e-10 ||A||_inf) or shows a
    coefficient above the gate (1e-8), which the device tests refuse through pair_gate_trips == 0.  (A diverged run is NaN:
    `not <=`.)"""
    import block_long_cases as B

    A, v0, ra, rb = short_long_problem
    al, be, coef = _run_model(model, A, v0, 700)
    assert np.abs(al - ra).max() <= 1e-12 and np.abs(be - rb).max() <= 1e-12 and coef <= 1e-8   # the unmutated model passes
    mal, mbe, mcoef = _run_model(model, A, v0, 700, MUTANTS[name])
    with np.errstate(all="ignore"):
        da, db = np.abs(mal - ra).max(), np.abs(mbe - rb).max()
    print("%s: dalpha %.2e dbeta %.2e largest relative coefficient %.2e" % (name, da, db, mcoef))
    tol = 1e-10 * B.NORM_INF
    assert not (da <= tol and db <= tol) or not mcoef <= 1e-8


@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
def test_the_model_at_the_device_tests_long_window(model, complex_):
    """The exact matrix, start vector and longest window of tests/test_gpu_block_long.py (n = 6 149, 1 024 iterations, blocks of
    four): the form reproduces full re-orthogonalisation to 1e-12 and its largest relative coefficient stays ten times under the gate
    of 1e-8 — the condition that lets the device tests demand pair_gate_trips == 0 over the whole window."""
    import block_long_cases as B

    A, v0 = _long_problem(B.N_LONG, complex_)
    ra, rb = _full_reorthogonalisation(A, v0, 1024)
    al, be, coef = _run_model(model, A, v0, 1024)
    da, db = np.abs(al - ra).max(), np.abs(be - rb).max()
    print("dalpha %.2e dbeta %.2e largest relative coefficient %.2e" % (da, db, coef))
    assert len(al) == 1024 and da <= 1e-12 and db <= 1e-12
    assert coef <= 1e-9
