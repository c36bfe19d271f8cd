"""Whole solver runs in all four storage types, in every form of the Gram-Schmidt step and both strip geometries, held to
float-level (storage-level) bounds against exact references.

The traces of two correct float runs drift apart, so the existing float tests compare a dozen alphas to 6e-3 and an
eigenvalue to 0.06.  What does not drift are the invariants of tests/float_run_model.py, which need only what a run returns:
the Lanczos relation in norm form, the returned eigenvalue against the returned T, Cauchy interlacing against exact
eigenvalues (a ghost breaks it by a spectral gap), the norm of the returned vector, the residual bound of a Rayleigh pair,
orthogonality between returned vectors, and the Exponentiator's output against a dense exponential.  Bounds: BOUNDS of
float_run_model.py — max(derived floor, 4 x what the host models of the same scheme give), in units of the storage epsilon;
the windows and the Exponentiator's iteration counts come from the host model too (tests/test_float_run_model_host.py).

Which assertion guards the float instantiations of the one-sweep kernels: without the compensation term of lagged_trip
(fnma_acc(wp[e], dj, ur[b][e])) the late coefficients double every iteration; the float model of that build has
`relation` = 1.3e3 at window 30 and no positive derived norm at k = 35, so case A fails at window 41 in the one-sweep forms
for s and c through `relation`: the DGKS test fires only at |c| ~ 1, so T is contaminated at first order long before any
repair of the basis."""
import numpy as np
import pytest

import float_run_model as M
import lambda_lanczos_amd as L

pytestmark = pytest.mark.gpu

# id: (switches, what last_stats must show)
FORMS = {
    "two_sweep": ({"LL_FUSE_LAUNCHES": "1"}, "none"),
    "one_sweep_stream": ({"LL_BLAS_SMALL_BYTES": "0", "LL_PAIR_GS": "0"}, "lagged"),
    "pair_stream": ({"LL_BLAS_SMALL_BYTES": "0"}, "pair"),
    "pair_stream_split": ({"LL_BLAS_SMALL_BYTES": "0", "LL_TEST_PAIR_SPLIT": "37"}, "pair"),
    "one_sweep_small": ({"LL_TEST_LAGGED_MIN_BYTES": "0", "LL_PAIR_GS": "0"}, "lagged"),
    "pair_small": ({"LL_TEST_LAGGED_MIN_BYTES": "0"}, "pair"),
    "mgs": ({}, "mgs"),
}


def set_form(llenv, form):
    for k, v in FORMS[form][0].items():
        llenv.setenv(k, v)
    return L.ORTH_MGS if form == "mgs" else L.ORTH_CGS_DGKS


def check_form(form, st, iterations, half=True, handover=False, repairs=True):
    """The named form took `iterations` less the set-up iterations and what the repairs cost (the formula of test_gpu_pair.py;
    repairs = False: less the set-up and the gate trips only) AND (half) at least half of them.  handover: the pair form may
    hand over to the one-sweep form of its geometry at its column limit — then the one-sweep forms together meet the
    formula and the pair form the half.  Returns the form's share."""
    kind = FORMS[form][1]
    spent = 3 + (4 * st["second_passes"] if repairs else 0) + 2 * st["pair_gate_trips"]
    if handover and st["pair_iterations"] < iterations - spent:
        assert kind == "pair" and st["lagged_iterations"] >= iterations - spent, (form, iterations, st)
        assert 2 * st["pair_iterations"] >= iterations, (form, iterations, st)
        return st["pair_iterations"] / iterations
    if kind == "none":
        assert st["lagged_iterations"] == 0 and st["pair_iterations"] == 0, st
        return None
    if kind == "mgs":
        assert st["lagged_iterations"] == 0, st
        return None
    if kind == "lagged":
        assert st["pair_iterations"] == 0, st
    took = st["pair_iterations"] if kind == "pair" else st["lagged_iterations"]
    assert took >= iterations - spent, (form, iterations, st)
    assert not half or 2 * took >= iterations, (form, iterations, st)
    return took / iterations


def solve(op_dev, op, v0, find_max, form_mode, num_eigs=1, window=None):
    eng = L.LambdaLanczos(op_dev, op.n, find_max, num_eigs)
    eng.eigenvalue_offset = op.offset
    eng.init_vector = lambda out, *_: np.copyto(out, v0)
    eng.orth_mode = form_mode
    if window:
        eng.eps = 0.0
        eng.max_iteration = window
    vals, vecs = eng.run()
    assert vecs.dtype == op.storage
    return dict(vals=vals, vecs=vecs, last_alpha=eng.last_alpha, last_beta=eng.last_beta, iters=eng.getIterationCounts(),
                stats=dict(eng.last_stats), eps=eng.eps)


def assert_bounds(got, t, what):
    print(what, {k: float("%.3g" % v) for k, v in got.items()})
    for k, v in got.items():
        assert v <= M.BOUNDS[k][t], (what, k, v, M.BOUNDS[k][t])


# ------------------------------------------------------------------ A: fixed windows, every form, every type
CASES_A = [(name, size, t, form) for name, size, types in M.CASES_A[:2] for t in types for form in FORMS]
CASES_A += [("laplace", size, t, form) for size in (61, 173) for t in "ds" for form in ("one_sweep_stream", "pair_stream")]


@pytest.mark.parametrize("name,size,t,form", CASES_A, ids=["%s%d-%s-%s" % c for c in CASES_A])
def test_fixed_window_runs_keep_the_invariants(ctx, llenv, name, size, t, form):
    """eps = 0, max_iteration = m: m = 41 (before convergence, an odd last iteration: `relation` is sharpest) and the
    post-convergence window of the host model (only re-orthogonalisation keeps ghosts out: `interlace`).  d and z run the same
    code at eps_d.  (The 173 x 173 Laplacian has the early window only and a 61 x 61 one runs both, see float_run_model.CASES_LATE.)
    The small-geometry pair sweep keeps its partial columns in one workgroup's LDS and hands over to the one-sweep form of the same
    geometry when they no longer fit (pair_small_fits; complex float first, inside the torus' late window): `handover`."""
    op, v0, find_max = M.case_setup(name, size, t)
    exact = M.exact_eigenvalues(name, size, op.storage.name)
    mode = set_form(llenv, form)
    op_dev = L.CsrOperator(ctx, *op.csr)
    try:
        for window in (M.WINDOW_EARLY, M.WINDOW_LATE.get(M.case_key(name, size))):
            if window is None:
                continue
            r = solve(op_dev, op, v0, find_max, mode, window=window)
            assert r["iters"] == [window] and len(r["last_alpha"]) == window
            share = check_form(form, r["stats"], window, handover=form == "pair_small" and window > M.WINDOW_EARLY)
            print("%s %s %s window %d: share %s, second passes %d" % (name, t, form, window, share, r["stats"]["second_passes"]))
            assert_bounds(M.run_invariants(op, r, find_max, exact), t, "%s%d %s %s window %d" % (name, size, t, form, window))
    finally:
        op_dev.close()


# ------------------------------------------------------------------ B: several eigenpairs to convergence
@pytest.mark.parametrize("form", ["two_sweep", "one_sweep_stream", "pair_stream", "pair_small"])
@pytest.mark.parametrize("name,size,t", M.CASES_B, ids=["randsym-s", "torus-c"])
def test_three_eigenpairs_in_single_precision(ctx, llenv, name, size, t, form):
    """Default eps, three pairs, restart passes behind locked eigenvectors: eigenvalues against the exact ones at the project's
    float tolerance (test_engines_single_precision), and for every pair the residual bound, the norm and the orthogonality
    to the others.  (No `relation`: the last pass's T does not see the locked vectors' residuals.)
    The named form is asserted for the FIRST pass: a float eigenvector locked at the default eps has a residual far above the
    one-sweep forms' gate for locked columns (3e-8 of the operator's size, LoopState::begin_pass), which refuses it by design,
    and the restart passes of a float run take the two-sweep form — half of ALL iterations is out of the named form's reach.
    last_stats counts over all passes, so the first pass's requirement takes off no second passes (they may be the restart
    passes'): the form took the first pass less its set-up and gate trips, and at least half of it."""
    op, v0, find_max = M.case_setup(name, size, t)
    exact = M.exact_eigenvalues(name, size, op.storage.name)
    mode = set_form(llenv, form)
    op_dev = L.CsrOperator(ctx, *op.csr)
    try:
        r = solve(op_dev, op, v0, find_max, mode, num_eigs=3)
    finally:
        op_dev.close()
    assert len(r["iters"]) > 1 and len(r["vals"]) == 3, r["iters"]
    share = check_form(form, r["stats"], r["iters"][0], repairs=False)
    print("%s %s %s: passes %s, stats %s, first-pass form %s" % (name, t, form, r["iters"], r["stats"], share))
    m = max(r["iters"])
    got = {}
    for i in range(3):
        assert abs(r["vals"][i] - exact[i]) <= 20 * r["eps"] * max(1.0, abs(exact[i] + op.offset)), (i, r["vals"], exact[:3])
        got["hermitian"] = max(got.get("hermitian", -np.inf), M.hermitian(op, r["vals"][i], r["vecs"][i], exact))
        got["unit"] = max(got.get("unit", 0.0), M.unit(op, r["vecs"][i]))
        for j in range(i):
            got["cross"] = max(got.get("cross", 0.0), M.cross(op, r["vecs"][i], r["vecs"][j], m))
    assert_bounds(got, t, "%s %s %s" % (name, t, form))


# ------------------------------------------------------------------ C: default switches at the sizes where the forms switch on
@pytest.mark.parametrize("name,size,t", M.CASES_C, ids=["randsym150001-s", "laplace520-s", "torus300-c"])
def test_default_switches_take_the_pair_form_and_keep_the_invariants(ctx, name, size, t):
    """No hook: float n = 150 001 (600 KB, the pair form in the small-vector geometry), the float Laplacian 520 x 520
    (1.08 MB, the streaming pair form), the complex-float torus 300 x 300 (720 KB) — the code a user gets.  Window 41, the
    invariants of case A (the exact eigenvalues of the two eigsh cases take half a minute each, once per process)."""
    op, v0, find_max = M.case_setup(name, size, t)
    op_dev = L.CsrOperator(ctx, *op.csr)
    try:
        r = solve(op_dev, op, v0, find_max, L.ORTH_CGS_DGKS, window=M.WINDOW_EARLY)
    finally:
        op_dev.close()
    assert r["iters"] == [M.WINDOW_EARLY]
    share = check_form("pair_stream", r["stats"], M.WINDOW_EARLY)
    print("%s %d %s: pair share %s" % (name, size, t, share))
    got = M.run_invariants(op, r, find_max, M.exact_eigenvalues(name, size, op.storage.name))
    assert_bounds(got, t, "%s %d %s" % (name, size, t))


# ------------------------------------------------------------------ D: the Exponentiator
CASES_D = [(name, size, a, t) for name, size, a, types in M.CASES_D for t in types]


@pytest.mark.parametrize("form", ["two_sweep", "one_sweep_small", "pair_stream"])
@pytest.mark.parametrize("full", [False, True], ids=["three_term", "full_orthogonalize"])
@pytest.mark.parametrize("name,size,a,t", CASES_D, ids=["%s-%s-%s" % (c[0], c[2], c[3]) for c in CASES_D])
def test_exponentiator_output_against_the_dense_exponential(ctx, llenv, name, size, a, t, full, form):
    """eps = 0, max_iteration = m with m from the host model (the double model within 1e-12 of the dense exponential: what
    remains in float is rounding); exp(a A) v against dense diagonalisation, and the norm for imaginary a."""
    op, v = M.expo_setup(name, size, t)
    m = M.EXPO_M[M.expo_key(name, size, a)]
    exact = M.expo_exact(name, size, op.storage, a, v)
    set_form(llenv, form)
    op_dev = L.CsrOperator(ctx, *op.csr)
    try:
        ex = L.Exponentiator(op_dev, op.n)
        ex.eps, ex.max_iteration, ex.full_orthogonalize = 0.0, m, full
        out, itern = ex.run(a, v)
        st = dict(ex.last_stats)
    finally:
        op_dev.close()
    assert out.dtype == op.storage and itern == m
    if full:
        print("form share", check_form(form, st, m))
    else:
        assert st["lagged_iterations"] == 0 and st["pair_iterations"] == 0
    got = dict(expo_error=M.expo_error(op, out, exact, v))
    if np.iscomplexobj(a):
        got["expo_norm"] = M.expo_norm(op, out, v)
    assert_bounds(got, t, "%s a = %s %s %s full = %s" % (name, a, t, form, full))


@pytest.mark.parametrize("name,size,a,t", CASES_D, ids=["%s-%s-%s" % (c[0], c[2], c[3]) for c in CASES_D])
def test_taylor_run_against_the_dense_exponential(ctx, name, size, a, t):
    """taylor_run at its default eps (with eps = 0 its term test never ends the series): bound from the host model of the same
    series, whose powers A^k v are rounded to storage like the device's."""
    op, v = M.expo_setup(name, size, t)
    op_dev = L.CsrOperator(ctx, *op.csr)
    try:
        out, terms = L.Exponentiator(op_dev, op.n).taylor_run(a, v)
    finally:
        op_dev.close()
    _, model_terms = M.taylor_model(op, a, v, 1e2 * op.eps)
    assert abs(terms - model_terms) <= 1, (terms, model_terms)
    assert_bounds(dict(taylor_error=M.expo_error(op, out, M.expo_exact(name, size, op.storage, a, v), v)), t,
                  "%s a = %s %s taylor, %d terms" % (name, a, t, terms))
