"""Long runs of the HIP path against the REAL reference (tests/golden/long_runs.json, written by tests/golden/make_golden.py
from oracle/_ref/libref.so): several hundred iterations to convergence or to an exhausted Krylov space, default kernel
geometry, no environment overrides.  The reference orthogonalises sequentially (modified Gram-Schmidt, LL:260 -> LA:132-144);
the HIP path uses the block forms (two-sweep CGS + DGKS below 320 KiB per vector, the one-sweep "lagged" form above) — these
tests compare them DIRECTLY with the reference's numbers, iteration by iteration:

  alpha_k, beta_k    |d| <= 1e-10 * ||A||_inf over the first 200 iterations
  iteration counts   within +-2 of the reference's, every pass
  eigenvalues        |l_gpu - l_ref| <= 1e-10 * max(1, |l + offset|)
  eigenvectors       sampled entries (512 fixed positions) agree to 3e-4 of the sample's norm (1 - overlap <= 1e-8 corresponds
                     to 1.4e-4) and the residual ||A v - l v|| <= 1e-6 * ||A||_inf is measured on the full GPU vector
"""
import os
import sys

import numpy as np
import pytest

import lambda_lanczos_amd as L
from lambda_lanczos_amd import generators as G
from util import inf_norm, list2c, load_golden, residual

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden as MG  # noqa: E402  (only the matrix recipes and sample positions; the reference is not needed here)

pytestmark = pytest.mark.gpu
GOLD = load_golden("long_runs.json")


def fixed_init(vec):
    return lambda v, *_: v.__setitem__(slice(None), vec)


def check_trace(eng, gold, csr, upto=200):
    norm = inf_norm(csr) + abs(gold["offset"])
    a, b = np.asarray(gold["alpha_pass1"]), np.asarray(gold["beta_pass1"])
    m = min(upto, len(a), len(eng.last_alpha))
    assert m >= min(upto, len(a)) - 3
    da = np.max(np.abs(eng.last_alpha[:m] - a[:m]))
    mb = min(m, len(b), len(eng.last_beta))
    db = np.max(np.abs(eng.last_beta[:mb] - b[:mb]))
    assert da <= 1e-10 * norm and db <= 1e-10 * norm, (da, db, norm)
    return da, db


def check_values(vals, gold):
    want = np.asarray(gold["eigenvalues"])
    assert len(vals) == len(want)
    for got, ref in zip(vals, want):
        assert abs(got - ref) <= 1e-10 * max(1.0, abs(ref + gold["offset"])), (got, ref)


def check_counts(counts, gold):
    assert len(counts) == len(gold["iter_counts"]), (counts, gold["iter_counts"])
    for got, ref in zip(counts, gold["iter_counts"]):
        assert abs(got - ref) <= 2, (counts, gold["iter_counts"])


def check_vectors(vecs, vals, gold, csr):
    idx = MG.sample_indices(gold["n"])
    norm = inf_norm(csr)
    for v, lam, ref in zip(vecs, vals, gold["eigenvector_samples"]):
        ref = list2c(ref)
        got = v[idx]
        ip = np.vdot(got, ref)           # eigenvectors are fixed up to a sign (real) / a phase (complex)
        phase = ip / abs(ip) if abs(ip) > 0 else 1.0
        assert np.linalg.norm(phase * got - ref) <= 3e-4 * np.linalg.norm(ref)
        assert residual(csr, lam, v) <= 1e-6 * norm


# ------------------------------------------------------------------ exhausted Krylov space: the ring of examples/drop_in.cpp
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("path", ["host_callback", "device_csr"])
def test_exhausted_krylov_space_both_operator_paths(ctx, path, seed):
    """n = 2000 alternating ring, two lowest pairs, offset -3: 1002 distinct eigenvalues, the reference stops pass 1 at 1003
    (Krylov space exhausted at 1002, beta_1002 ~ 5e-14 is above the breakdown threshold, LL:279-283) and pass 2 at ~985.
    The unmodified-user-lambda path (host callback, LL:126,200-208) and the device-resident CSR path must both reproduce
    values and counts, and the callback must be called exactly once per executed iteration (LL:243)."""
    gold = GOLD["ring2000_two_lowest_s%d" % seed]
    csr = MG.long_run_matrix(gold)
    n = gold["n"]
    init = G.start_vector(n, seed)
    calls = [0]
    if path == "host_callback":
        import scipy.sparse as sp

        A = sp.csr_matrix((csr[2], csr[1], csr[0]), shape=(n, n))

        def mv_mul(x, out):
            assert not out.any()  # zero-filled on entry (LL:242)
            calls[0] += 1
            out += A @ x

        op = L.HostOperator(ctx, mv_mul, n)
    else:
        op = L.CsrOperator(ctx, *csr)
    eng = L.LambdaLanczos(op, n, False, 2)
    eng.eigenvalue_offset = gold["offset"]
    eng.init_vector = fixed_init(init)
    vals, vecs = eng.run()
    counts = eng.getIterationCounts()
    check_values(vals, gold)
    check_counts(counts, gold)
    check_vectors(vecs, vals, gold, csr)
    if path == "host_callback":
        assert calls[0] == sum(counts), (calls[0], counts)
    # pass 1 alone (num_eigs = 1 runs the same first pass): the recurrence coefficients up to the exhaustion
    eng1 = L.LambdaLanczos(op, n, False, 1)
    eng1.eigenvalue_offset = gold["offset"]
    eng1.init_vector = fixed_init(init)
    eng1.run()
    check_trace(eng1, gold, csr, upto=1000)
    assert abs(eng1.getIterationCounts()[0] - gold["iter_counts"][0]) <= 2
    if "fresh_pass" in gold:
        # What run() does by default in a restart pass: a FRESH random start vector (LL:70-104), orthogonalised against the
        # locked pairs.  Every eigenvalue of this ring but two is doubly degenerate, so the fresh vector brings the partner of
        # the locked E1 back as the lowest Ritz value; the pass exhausts its Krylov space at m = 1001 and either breaks down
        # there (the reference: beta_1001 < 10 eps) or continues on rounding noise (1002 or ~1850 iterations: the reference
        # itself ends anywhere in that set for other vectors) — the converged Ritz VALUES are the invariant that is checked.
        fresh = gold["fresh_pass"]
        engf = L.LambdaLanczos(op, n, False, 1)
        engf.eigenvalue_offset = gold["offset"]
        engf.init_vector = fixed_init(G.start_vector(n, gold["fresh_seed"]))
        fv, _, fit = engf.run_iteration(5, orthogonalize_to=vecs)
        assert fit >= 1001, fit
        # robust to where the noise-driven tail ends: the lowest value is the partner of the locked E1, and every returned
        # value is one of the reference's converged levels (a run that continues past the exhaustion finds second copies)
        tol = [1e-10 * max(1.0, abs(ref + gold["offset"])) for ref in fresh["eigenvalues"]]
        assert abs(fv[0] - fresh["eigenvalues"][0]) <= tol[0], (fv, fresh["eigenvalues"])
        for got in fv:
            assert any(abs(got - ref) <= t for ref, t in zip(fresh["eigenvalues"], tol)), (fv, fresh["eigenvalues"])
    op.close()


@pytest.mark.parametrize("path", ["host_callback", "device_csr"])
def test_misconvergence_of_the_reference_is_reproduced(ctx, path):
    """The same ring from the reference's own initialiser with seed 1967 (std::mt19937, LL:70-104): the start vector has an
    overlap of 2.4e-5 with the ground state, the five tracked Ritz values stand still at m = 1000 before that component has
    grown, and the reference's stopping rule (LL:290-309) ends the pass there with E1 as the "lowest" eigenvalue — one of three
    such vectors among 6000 (profiles/r04_ring_start_vector_sweep.txt; 0.18 % expected for a random vector), and what round 3's
    randomly seeded example ran into on the driver's box.  A drop-in must stop where the reference stops and return what it
    returns, here too."""
    gold = GOLD["ring2000_misconverged_mt1967"]
    csr = MG.long_run_matrix(gold)
    n = gold["n"]
    init = np.asarray(gold["start_vector"])
    if path == "host_callback":
        import scipy.sparse as sp

        A = sp.csr_matrix((csr[2], csr[1], csr[0]), shape=(n, n))
        op = L.HostOperator(ctx, lambda x, out: out.__iadd__(A @ x), n)
    else:
        op = L.CsrOperator(ctx, *csr)
    eng = L.LambdaLanczos(op, n, False, 1)
    eng.eigenvalue_offset = gold["offset"]
    eng.init_vector = fixed_init(init)
    vals, vecs = eng.run()
    assert gold["iter_counts"] == [1000]
    check_counts(eng.getIterationCounts(), gold)
    check_values(vals, gold)
    assert abs(vals[0] - (-2.022365081214)) < 1e-9 and abs(vals[0] - (-2.022374841616)) > 5e-6   # E1's value, not E0
    check_trace(eng, gold, csr, upto=990)
    op.close()


# ------------------------------------------------------------------ one-sweep form, run to convergence
@pytest.mark.parametrize("name,pair", [("randsym1e5_converge", "1"), ("randsym1e5_converge", "0"), ("laplace200_converge", "1")])
def test_one_sweep_form_to_convergence_matches_the_reference(ctx, llenv, name, pair):
    """randsym n = 1e5 (352 reference iterations) and the 200 x 200 Laplacian with offset -8 (729), default geometry.  The 800 KB
    vectors of the first take the SMALL-VECTOR geometry of the one-sweep forms: two iterations per sweep (pair_small_kernel, round 6;
    the default) or one (lagged_small_kernel, LL_PAIR_GS=0) in every iteration but the first ones; the 320 000-byte vectors of the
    second sit just below the 320 KiB switch and keep the two-sweep small-vector kernels (block CGS + DGKS) for all 729 iterations —
    all three forms against the reference's sequential MGS."""
    gold = GOLD[name]
    csr = MG.long_run_matrix(gold)
    n = gold["n"]
    llenv.setenv("LL_PAIR_GS", pair)
    op = L.CsrOperator(ctx, *csr)
    eng = L.LambdaLanczos(op, n, gold["find_max"], 1)
    eng.eigenvalue_offset = gold["offset"]
    eng.init_vector = fixed_init(G.start_vector(n, gold["seed"]))
    vals, vecs = eng.run()
    itern = eng.getIterationCounts()[0]
    if n * 8 >= 320 << 10 or os.environ.get("LL_BLAS_SMALL_BYTES") == "0":   # (the suite is also run with the streaming geometry forced)
        assert eng.last_stats["lagged_iterations"] >= itern - 3, eng.last_stats
        if pair == "1":
            assert eng.last_stats["pair_iterations"] >= itern - 3 - 4 * eng.last_stats["second_passes"], eng.last_stats
        else:
            assert eng.last_stats["pair_iterations"] == 0
    else:
        assert eng.last_stats["lagged_iterations"] == 0, eng.last_stats
    check_counts(eng.getIterationCounts(), gold)
    check_trace(eng, gold, csr)
    check_values(vals, gold)
    check_vectors(vecs, vals, gold, csr)
    op.close()


def test_one_sweep_streaming_geometry_fixed_window_matches_the_reference(ctx):
    """randsym n = 1e6, max_iteration = 120: 8 MB vectors, lagged_kernel in the streaming geometry; every alpha / beta of the
    window against the reference's."""
    gold = GOLD["randsym1e6_fixed120"]
    csr = G.randsym(gold["n"])
    n = gold["n"]
    op = L.CsrOperator(ctx, *csr)
    eng = L.LambdaLanczos(op, n, True, 1)
    eng.max_iteration = gold["max_iteration"]
    eng.init_vector = fixed_init(G.start_vector(n, gold["seed"]))
    vals, vecs = eng.run()
    assert eng.getIterationCounts() == gold["iter_counts"] == [120]
    assert eng.last_stats["lagged_iterations"] >= 117, eng.last_stats
    check_trace(eng, gold, csr, upto=120)
    check_values(vals, gold)
    check_vectors(vecs, vals, gold, csr)
    op.close()


def test_one_sweep_form_in_restart_passes_matches_the_reference(ctx):
    """randsym n = 1e5, three largest pairs: the restart passes deflate against the locked eigenvectors (LL:233,259) and keep
    the one-sweep form (LoopState::begin_pass measures the locked residuals); values and per-pass counts against the reference."""
    gold = GOLD["randsym1e5_three_roots"]
    csr = MG.long_run_matrix(gold)
    n = gold["n"]
    op = L.CsrOperator(ctx, *csr)
    eng = L.LambdaLanczos(op, n, True, 3)
    eng.init_vector = fixed_init(G.start_vector(n, gold["seed"]))
    vals, vecs = eng.run()
    counts = eng.getIterationCounts()
    check_values(vals, gold)
    check_counts(counts, gold)
    check_vectors(vecs, vals, gold, csr)
    # every pass but the breakdown / gate exceptions runs one sweep per iteration: at most 3 two-sweep iterations per pass
    assert eng.last_stats["lagged_iterations"] >= sum(counts) - 3 * len(counts), (eng.last_stats, counts)
    op.close()


# ------------------------------------------------------------------ the STREAMING one-sweep kernel over whole runs (round 5)
@pytest.mark.parametrize("form", ["pair", "pair_split", "one_sweep"])
@pytest.mark.parametrize("name", ["laplace400_converge", "torus300_converge"])
def test_streaming_one_sweep_kernel_over_a_whole_run_matches_the_reference(ctx, llenv, name, form):
    """The streaming geometry of the Gram-Schmidt step (vectors >= 1 MiB — what configs 2 and 3 run for thousands / hundreds of
    iterations) against the reference's sequential MGS (LL:260 -> LA:132-144) over WHOLE runs to convergence, default geometry:
    the 400 x 400 Laplacian (smallest pair, offset -8, 1.28 MB vectors, 1448 reference iterations) and the complex torus 300 x 300
    (config 5's matrix in small, smallest pair, offset -10, 1.44 MB vectors, 524 iterations), in both forms these vectors can take:
    `pair` — the default: two iterations per sweep (pair_sweep_kernel) — and `one_sweep` — LL_PAIR_GS=0: one sweep per iteration
    (lagged_kernel), the form the pair form falls back to; `pair_split` — the pair form with its sweep split into launches of at most
    300 stored vectors each (LL_TEST_PAIR_SPLIT: what happens by itself beyond 2 497 real / 1 247 complex stored vectors, where one
    workgroup's LDS no longer holds a column per coefficient).  EVERY alpha / beta of the run to 1e-10 ||A||_inf (an error of a
    compensation that grew slowly with k would show here), iteration count +-2, eigenvalue, sampled eigenvector entries, residual,
    and the run really took that kernel."""
    if form == "one_sweep":
        llenv.setenv("LL_PAIR_GS", "0")
    if form == "pair_split":
        llenv.setenv("LL_TEST_PAIR_SPLIT", "300")
    gold = GOLD[name]
    csr = MG.long_run_matrix(gold)
    n = gold["n"]
    dtype = np.complex128 if gold.get("complex") else np.float64
    assert n * np.dtype(dtype).itemsize >= 1 << 20      # streaming geometry of the one-sweep form
    op = L.CsrOperator(ctx, *csr)
    eng = L.LambdaLanczos(op, n, gold["find_max"], 1)
    eng.eigenvalue_offset = gold["offset"]
    eng.init_vector = fixed_init(G.start_vector(n, gold["seed"], dtype))
    vals, vecs = eng.run()
    itern = eng.getIterationCounts()[0]
    assert eng.last_stats["lagged_iterations"] >= itern - 3, eng.last_stats
    if form in ("pair", "pair_split"):
        assert eng.last_stats["pair_iterations"] >= itern - 3 - 4 * eng.last_stats["second_passes"], eng.last_stats
    else:
        assert eng.last_stats["pair_iterations"] == 0
    check_counts(eng.getIterationCounts(), gold)
    da, db = check_trace(eng, gold, csr, upto=10 ** 9)    # the whole run
    check_values(vals, gold)
    check_vectors(vecs, vals, gold, csr)
    op.close()


@pytest.mark.parametrize("form", ["pair", "one_sweep"])
def test_run_beyond_the_column_capacity_of_one_sweep_launch_matches_the_reference(ctx, llenv, form):
    """800 x 800 Laplacian, smallest pair, offset -8 (5.12 MB vectors): the REAL reference needs 2 557 iterations (85 minutes on one core) — more
    stored vectors than one workgroup of the pair sweep holds coefficient columns for (2 497), so from there on every sweep of the
    default form is two launches (gs_pair.hip pair_sweep_kernel; bit-identical to an unsplit sweep by construction,
    test_split_sweeps_change_no_bit) — nothing forced, nothing hooked.  Every alpha / beta of the run, count, eigenvalue, sampled
    eigenvector entries and the residual against the fixture; `one_sweep` (LL_PAIR_GS=0) runs the same length in the form the
    pair form hands over to at 4 992 stored vectors."""
    name = "laplace800_converge"
    if name not in GOLD:
        pytest.skip("fixture not generated (tests/golden/make_golden.py long_runs laplace800_converge)")
    if form == "one_sweep":
        llenv.setenv("LL_PAIR_GS", "0")
    gold = GOLD[name]
    csr = MG.long_run_matrix(gold)
    n = gold["n"]
    op = L.CsrOperator(ctx, *csr)
    eng = L.LambdaLanczos(op, n, gold["find_max"], 1)
    eng.eigenvalue_offset = gold["offset"]
    eng.init_vector = fixed_init(G.start_vector(n, gold["seed"]))
    vals, vecs = eng.run()
    itern = eng.getIterationCounts()[0]
    assert itern > 2497 + 40        # the last ~30 sweeps of the pair form are two launches each
    assert eng.last_stats["lagged_iterations"] >= itern - 3, eng.last_stats
    if form == "pair":
        assert eng.last_stats["pair_iterations"] >= itern - 3 - 4 * eng.last_stats["second_passes"], eng.last_stats
    else:
        assert eng.last_stats["pair_iterations"] == 0
    check_counts(eng.getIterationCounts(), gold)
    check_trace(eng, gold, csr, upto=10 ** 9)
    check_values(vals, gold)
    check_vectors(vecs, vals, gold, csr)
    op.close()
