"""The host reference of the float / complex-float whole-run tests (tests/float_run_model.py) against itself, in the manner
of tests/test_exact_ref.py: the correct models stay inside the bounds of the table, plausibly wrong implementations do not.

The table.  For every case of tests/test_gpu_float_runs.py both correct models (sequential Gram-Schmidt done twice, and the
one-sweep scheme) are run in the case's storage types and every invariant is measured; the bound of an invariant in a
storage type is max(floor, 4 x that type's worst ratio over the cases) — per type, so that a double model's ratio (a whole
number of roundings) does not loosen the float bound.  The floors are derived, not measured:
    relation, ritz, hermitian, interlace   1 u_A   one rounding of v to storage moves A v - theta v by (eps/2) ||A - theta|| <= u_A
    unit                                   1 eps   the last multiplication of the normalisation
    cross                                  1       in units of (sqrt(m)/2 + 2) eps: each u_k is orthogonal to a locked vector to
                                                   one storage rounding, v = sum s_k u_k with |s| = 1
    expo_error, expo_norm, taylor_error    1 eps ||v||   the rounding of the output
and the factor 4 covers what the models do not replay (the order of the sums, the pair form's fold, one rounding of the sum
of all projections instead of one per vector in the small-vector kernels).  This file recomputes the ratios (minutes of numpy:
the models are sequential, rounding after every subtracted vector) and fails when the committed table is stale; it also
derives the two numbers the device test takes from the model: the post-convergence window and the Exponentiator's
iteration count.

The Laplacian 173 x 173 has no post-convergence window: its float model does not reach beta_m |s_m| <= 1e3 u_A within
the 130 iterations searched (asserted below).  A 61 x 61 Laplacian, whose model gets there at m = 103, runs both windows in
its place, on the host and on the device; the large one keeps the early window.

The mutants, and what rejects them by a factor of ten or more (asserted below):
    no compensation in the one-sweep scheme          relation, randsym float, window 30 (|c| = 0.38 there; at k = 35 the derived
                                                     norm of the model is no longer positive — a window of 41 does not exist)
    re-orthogonalisation against the last two only   interlace, randsym float, post-convergence window (a ghost of lambda_1)
    alpha without its second-order term, |c| = 1e-3  relation, randsym double, window 41 (|c|^2 ||A|| = 3e-5 is 0.25 u_A in
                                                     float: out of reach there)
    Exponentiator with the coefficients of T_{m-1}   expo_error, double and complex double (in float the truncation at m - 1 is
                                                     still far below eps: out of reach, like every error below eps_f)
Out of reach of basis-free checks: the output vector formed from the raw (not late-updated) last basis vector — the late
coefficients of a healthy run are ~3e-7, the vector moves by half an eps_f times |s_m|, no invariant sees it; and Gram-Schmidt
coefficients accumulated in float, which test_orth_and_gemv_single_precision_exact owns."""
import numpy as np
import pytest

import float_run_model as M


@pytest.fixture(scope="module")
def measured():
    return M.measure()


def test_the_windows_and_iteration_counts_of_the_table_come_from_the_models(measured):
    _, windows, expo_m = measured
    print("post-convergence windows:", windows, " Exponentiator m:", expo_m)
    assert windows == M.WINDOW_LATE
    assert expo_m == M.EXPO_M
    assert all(2 * M.WINDOW_EARLY < w <= 325 for w in windows.values())
    assert M.late_window("laplace", 173) is None


def test_the_bounds_of_the_table_are_four_times_the_models_worst_ratios_or_the_floor(measured):
    ratios, _, _ = measured
    bounds = M.bounds_of(ratios)
    assert set(bounds) == set(M.BOUNDS) == set(M.FLOORS) == set(M.MODEL_RATIOS)
    for inv in sorted(bounds):
        print("%-13s model %s  -> bound %s (table %s, floor %g)" % (
            inv, {t: float("%.3g" % v) for t, v in ratios[inv].items()}, {t: float("%.3g" % v) for t, v in bounds[inv].items()},
            M.BOUNDS[inv], M.FLOORS[inv]))
    for inv, per_type in bounds.items():
        assert set(per_type) == set(M.BOUNDS[inv]) == set(M.MODEL_RATIOS[inv])
        for t, b in per_type.items():
            table, worst = M.BOUNDS[inv][t], ratios[inv][t]
            # the sums of A x and of the dot products are numpy's / the BLAS': a ratio may move a little from machine to machine,
            # and a double model's ratio is a whole number of roundings (0, 1/2, 1, 2 eps_d) that differs between BLAS builds
            slack = 4.0 if t in "dz" else 0.0
            assert b / 1.25 - slack <= table <= 1.25 * b + slack, (inv, t, b, table)
            assert table >= M.FLOORS[inv] and worst <= table                     # the correct models stay inside
            # the noted ratio, where it is large enough to decide the bound (below floor / 4 it is one rounding's luck)
            low = M.FLOORS[inv] / 4
            noted = max(M.MODEL_RATIOS[inv][t], low)
            assert abs(max(worst, low) - noted) <= 0.25 * noted + slack / 4, (inv, t, worst)


def _rejects(ratio, inv, t, case):
    print("%s on %s: %.3g against the bound %.3g" % (inv, case, ratio, M.BOUNDS[inv][t]))
    assert ratio >= 10 * M.BOUNDS[inv][t], (inv, case, ratio)


def test_mutant_without_compensation():
    op, v0, find_max = M.case_setup("randsym", 30011, "s")
    run = M.lagged_model(op, v0, 30, compensate=False)
    assert run["maxc"][9] < 1e-5 and run["maxc"][-1] > 0.1          # the late coefficients double every iteration
    _rejects(M.relation(op, M.model_returns(op, run, find_max), find_max), "relation", "s", "randsym float, window 30")
    assert M.lagged_model(op, v0, M.WINDOW_EARLY, compensate=False).get("failed_at", 99) <= M.WINDOW_EARLY


def test_mutant_that_reorthogonalises_against_the_last_two_vectors_only():
    op, v0, find_max = M.case_setup("randsym", 30011, "s")
    run = M.lanczos_model(op, v0, M.WINDOW_LATE["randsym30011"], last_two_from=30)
    ret = M.model_returns(op, run, find_max)
    _rejects(M.interlace(op, ret, find_max, M.exact_eigenvalues("randsym", 30011, op.storage.name)), "interlace", "s",
             "randsym float, post-convergence window")


def test_mutant_without_the_second_order_term_of_alpha():
    op, v0, find_max = M.case_setup("randsym", 30011, "d")
    run = M.lagged_model(op, v0, M.WINDOW_EARLY, second_order=False, inject=1e-3)
    assert abs(run["maxc"].max() - 1e-3) <= 1e-5
    _rejects(M.relation(op, M.model_returns(op, run, find_max), find_max), "relation", "d", "randsym double, window 41")
    full = M.lagged_model(op, v0, M.WINDOW_EARLY, inject=1e-3)      # the full scheme is exact for a |c| of any size
    assert M.relation(op, M.model_returns(op, full, find_max), find_max) <= M.BOUNDS["relation"]["d"]


def test_mutant_with_the_raw_last_vector_is_out_of_reach():
    """Recorded, not tuned for: U[m-1] of the Ritz sum taken without its late update."""
    op, v0, find_max = M.case_setup("randsym", 30011, "s")
    run = M.lagged_model(op, v0, M.WINDOW_EARLY)
    raw = M.lagged_model(op, v0, M.WINDOW_EARLY - 1)["raw_last"].astype(op.wide)
    moved = np.linalg.norm(raw - run["U"][M.WINDOW_EARLY - 1].astype(op.wide))
    assert 0 < moved <= 2 * op.eps
    ret = M.model_returns(op, run, find_max, last_vector=raw)
    got = dict(relation=M.relation(op, ret, find_max), unit=M.unit(op, ret["vecs"][0]), ritz=M.ritz(op, ret, find_max))
    print("raw last vector:", got)
    assert all(v <= M.BOUNDS[k]["s"] for k, v in got.items())


@pytest.mark.parametrize("name,size,a,t", [("laplace", 41, -0.3, "d"), ("torus", 40, -0.5j, "z"), ("torus", 40, -2.0j, "z")])
def test_mutant_exponentiator_with_the_coefficients_of_one_iteration_less(name, size, a, t):
    op, v = M.expo_setup(name, size, t)
    m = M.EXPO_M[M.expo_key(name, size, a)]
    exact = M.expo_exact(name, size, op.storage, a, v)
    assert M.expo_error(op, M.expo_model(op, a, v, m, True), exact, v) <= M.BOUNDS["expo_error"][t]
    _rejects(M.expo_error(op, M.expo_model(op, a, v, m, True, coeff_of=m - 1), exact, v), "expo_error", t,
             "%s %d, a = %s, %s" % (name, size, a, t))
