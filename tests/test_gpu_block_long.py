"""The block form of the Gram-Schmidt step (gs_block.hip, LoopState::enqueue_block; tests/test_gpu_block.py has the short windows)
over LONG passes, up to the form's bound of 1 024 iterations: the second and later trips of every strided loop of the predict,
fold and enter kernels (reals (k + 1) > 256), data in waves 2 and 3 of their reductions, the natural split of a complex sweep past
623 stored vectors at the real LDS size, the far end of the packed triangle and of the records, block_flush and the transformed
Ritz / Exponentiator coefficients over hundreds of raw vectors, the form as pass 1 of a several-eigenpair run and its re-entry after
a DGKS repair.  tests/test_block_model.py shows on the CPU that windows of 41 cannot see a fault in anything indexed past 255,
that a window of 700 sees it, and that this matrix keeps every relative coefficient ten times under the gate over 1 024 iterations.

Matrix (block_long_cases.long_chain): n = 3 x 2 048 + 5, diag(linspace(0, 1, n)) with six separated eigenvalues (-1.0, -0.6 in
front; 1.3, 1.5, 1.8, 2.2 behind), coupling 0.1 (complex: +-0.1 i), ||A||_inf = 2.4, start vector G.start_vector(n, 5).  The
separated eigenvalues converge within a few dozen iterations; every later iteration depends on the re-orthogonalisation.

References.  ONE oracle run per type (1 024 iterations, eps = 0: the reference's stopping rule `|d theta| < min|theta| eps` cannot
fire and its breakdown test does not, so the oracle runs all W iterations of every window W <= 1 024, and its first W alpha / beta
ARE its run of window W) supplies alpha and beta of every window; the eigenvalue of a window is that of the oracle's own W x W
tridiagonal (scipy).  The eigenvector of the longest window is the oracle's; for the shorter windows and for find_maximum = False the
oracle returned none, and the reference is the eigenvector of A itself (A is tridiagonal, the complex one similar to the real one by
diag(i^k): scipy.linalg.eigh_tridiagonal, error ~ eps ||A|| / gap = 1e-15) — the extreme eigenvalues are separated by 0.4 and the
Ritz pairs have converged to rounding long before iteration 300, so the oracle's Ritz vector of that window is this vector to 1e-15.

Tolerances as everywhere: alpha / beta 1e-10 ||A||_inf, eigenvalue 1e-10 max(1, |lambda|), 1 - overlap <= 1e-8,
residual <= 1e-6 ||A||_inf, iteration counts equal.  The streaming geometry is forced as in test_gpu_block.py."""
import numpy as np
import pytest
import scipy.linalg

import lambda_lanczos_amd as L
from block_long_cases import N_LONG, NORM_INF, T_LONG, long_chain, long_diagonal
from lambda_lanczos_amd import generators as G
from test_gpu_block import check_against, fixed_init, took_the_form
from util import overlap, residual

pytestmark = pytest.mark.gpu

KEYS = ("blas_small_bytes", "sweep_pipeline", "block_gs", "pair_split", "pair_max_stored", "ritz_tail", "dgks_threshold")
BOUND = 1024

_problems, _oracle_runs, _plain_runs, _exact = {}, {}, {}, {}


def dtype_of(cplx):
    return np.complex128 if cplx else np.float64


def problem(cplx):
    if cplx not in _problems:
        _problems[cplx] = (long_chain(N_LONG, cplx), G.start_vector(N_LONG, 5, dtype_of(cplx)))
    return _problems[cplx]


def exact_vector(cplx, find_max):
    """The eigenvector of A for its largest / smallest eigenvalue."""
    if (cplx, find_max) not in _exact:
        at = N_LONG - 1 if find_max else 0
        _, v = scipy.linalg.eigh_tridiagonal(long_diagonal(N_LONG), np.full(N_LONG - 1, T_LONG), select="i", select_range=(at, at))
        v = v[:, 0]
        _exact[(cplx, find_max)] = v * 1j ** (np.arange(N_LONG) % 4) if cplx else v
    return _exact[(cplx, find_max)]


def oracle_window(oracle, cplx, window, find_max=True):
    """What the oracle's run of `window` iterations returns, from its one run of 1 024 (module docstring)."""
    if cplx not in _oracle_runs:
        csr, init = problem(cplx)
        full = oracle.lanczos(csr, init, True, max_iteration=BOUND, eps=0.0)
        assert full["iter_counts"] == [BOUND] and len(full["alpha"]) == BOUND
        _oracle_runs[cplx] = full
    full = _oracle_runs[cplx]
    at = window - 1 if find_max else 0
    lam = scipy.linalg.eigh_tridiagonal(full["alpha"][:window], full["beta"][:window - 1], eigvals_only=True, select="i",
                                        select_range=(at, at))[0]
    vec = full["eigenvectors"][0] if window == BOUND and find_max else exact_vector(cplx, find_max)
    return dict(iter_counts=[window], alpha=full["alpha"][:window], beta=full["beta"][:window], eigenvalues=[lam], eigenvectors=[vec])


def run(ctx, cplx, window, *, find_max=True, num_eigs=1, eps=0.0, block=True, split=None, ivs=None, tail=True, max_stored=None,
        dgks=None):
    csr, init = problem(cplx)
    settings = {"blas_small_bytes": "0", "sweep_pipeline": "2", "block_gs": "1" if block else "0"}
    if split:
        settings["pair_split"] = str(split)
    if max_stored:
        settings["pair_max_stored"] = str(max_stored)
    if not tail:
        settings["ritz_tail"] = "0"
    if dgks is not None:
        settings["dgks_threshold"] = str(dgks)
    try:
        for k, v in settings.items():
            ctx.set_tuning(k, v)
        op = L.CsrOperator(ctx, *csr)
        eng = L.LambdaLanczos(op, N_LONG, find_max, num_eigs)
        eng.init_vector = fixed_init(init)
        eng.max_iteration = window
        if eps is not None:
            eng.eps = eps
        if ivs:
            eng.initial_vector_size = ivs
        vals, vecs = eng.run()
        out = dict(vals=vals, vecs=vecs, iters=eng.getIterationCounts(), alpha=eng.last_alpha.copy(), beta=eng.last_beta.copy(),
                   stats=dict(eng.last_stats))
        op.close()
        return out
    finally:
        for k in KEYS:
            ctx.set_tuning(k, None)


def plain(ctx, cplx, window):
    """The run of a window with nothing but the streaming geometry forced (shared: the cases below compare against its bits)."""
    if (cplx, window) not in _plain_runs:
        _plain_runs[(cplx, window)] = run(ctx, cplx, window)
    return _plain_runs[(cplx, window)]


def check(r, ora, cplx, what):
    """check_against (counts, alpha, beta, eigenvalue, overlap; prints the maxima) and the residual of the returned pair"""
    what = "long %s %s" % ("complex" if cplx else "real", what)
    check_against(r, ora, NORM_INF, what)
    res = residual(problem(cplx)[0], r["vals"][0], r["vecs"][0])
    print("%s residual %.2e" % (what, res))
    assert res <= 1e-6 * NORM_INF


def same_bits(r, ref, what):
    assert r["iters"] == ref["iters"], what
    assert np.array_equal(r["alpha"], ref["alpha"]) and np.array_equal(r["beta"], ref["beta"]), what
    assert np.array_equal(r["vals"], ref["vals"]) and np.array_equal(r["vecs"][0], ref["vecs"][0]), what


def took_the_whole_window(st, window):
    took_the_form(st, window)
    assert st["second_passes"] == 0, st


@pytest.mark.parametrize("window", [300, 700, BOUND])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_long_windows_up_to_the_bound(ctx, oracle, cplx, window):
    """300: reals (k + 1) crosses 256 (complex: at 128 stored vectors), the strided loops take a second trip.  700: third and later
    trips; the complex sweep splits into two launches from 624 stored vectors on.  1 024: the bound of the form, the last rows
    of the packed triangle and the end of the records; both ends of the spectrum."""
    ora = oracle_window(oracle, cplx, window)
    r = plain(ctx, cplx, window)
    assert r["iters"] == [window]
    check(r, ora, cplx, "window %d" % window)
    took_the_whole_window(r["stats"], window)
    if window == BOUND:
        low = run(ctx, cplx, window, find_max=False)
        check(low, oracle_window(oracle, cplx, window, find_max=False), cplx, "window %d, smallest eigenvalue" % window)
        took_the_whole_window(low["stats"], window)
        assert np.array_equal(low["alpha"], r["alpha"]) and np.array_equal(low["beta"], r["beta"])


@pytest.mark.parametrize("cplx,window,split", [(True, 700, 300), (False, BOUND, 500)], ids=["complex-700-by-300", "real-1024-by-500"])
def test_the_natural_split_changes_no_bit(ctx, cplx, window, split):
    """Complex, 700: the plain run makes two launches from 624 stored vectors on (block_sweep_max_vecs = 623 at 160 kB of LDS);
    launches of at most 300 are three there.  Real, 1 024: one launch in the plain run (up to 1 247), three of at most 500."""
    r = run(ctx, cplx, window, split=split)
    took_the_whole_window(r["stats"], window)
    same_bits(r, plain(ctx, cplx, window), "launches of %d" % split)


def test_a_hundred_slabs_change_no_bit(ctx):
    """initial_vector_size = 7, complex, 700: the pointer table is filled slab by slab up to k = 700."""
    r = run(ctx, True, 700, ivs=7)
    took_the_whole_window(r["stats"], 700)
    same_bits(r, plain(ctx, True, 700), "slabs of 7")


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_hand_over_at_depth(ctx, oracle, cplx):
    """pair_max_stored = 600 in a window of 700: block_flush completes about 600 raw vectors in place (one multi-axpy over the
    basis each, coefficients from the far rows of the triangle) and the one-sweep form finishes the pass on them."""
    r = run(ctx, cplx, 700, max_stored=600)
    check(r, oracle_window(oracle, cplx, 700), cplx, "hand-over at 600 of 700")
    st = r["stats"]
    assert st["block_flushed_vectors"] >= 590 and 590 <= st["block_iterations"] <= 600 and st["pair_gate_trips"] == 0, st


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_the_whole_raw_basis_completed_at_the_end_of_the_pass(ctx, oracle, cplx):
    """ritz_tail = 0 at the bound: the loop is the default run's (same bits of alpha, beta, eigenvalue), then end_pass flushes
    more than 1 000 raw vectors and the Ritz GEMV reads them with the plain coefficients, where the default run transforms the
    coefficients over 1 024 raw vectors (block_coeff_over_raw)."""
    default = plain(ctx, cplx, BOUND)
    r = run(ctx, cplx, BOUND, tail=False)
    assert r["iters"] == default["iters"] == [BOUND]
    assert np.array_equal(r["alpha"], default["alpha"]) and np.array_equal(r["beta"], default["beta"])
    assert np.array_equal(r["vals"], default["vals"])
    ov_default = 1 - overlap(r["vecs"][0], default["vecs"][0])
    ov_oracle = 1 - overlap(r["vecs"][0], oracle_window(oracle, cplx, BOUND)["eigenvectors"][0])
    print("long %s ritz_tail = 0 at %d: 1-overlap against the default run %.2e, against the oracle %.2e  stats %s" % (
        "complex" if cplx else "real", BOUND, ov_default, ov_oracle, {k: r["stats"][k] for k in ("block_iterations", "block_flushed_vectors")}))
    assert ov_default <= 1e-8 and ov_oracle <= 1e-8
    assert r["stats"]["block_flushed_vectors"] >= 1000 and default["stats"]["block_flushed_vectors"] == 0


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_three_eigenpairs_with_the_block_form_in_pass_one(ctx, oracle, cplx):
    """num_eigs = 3, the default eps: pass 1 is the block form and ends inside a block, its five Ritz vectors come through the
    transformed coefficients; the later passes deflate against them."""
    csr, init = problem(cplx)
    ora = oracle.lanczos(csr, init, True, num_eigs=3, max_iteration=BOUND)
    r = run(ctx, cplx, BOUND, num_eigs=3, eps=None)
    assert len(r["vals"]) == len(ora["eigenvalues"]) == 3
    dl = max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(r["vals"], ora["eigenvalues"]))
    ov = max(1 - overlap(a, b) for a, b in zip(r["vecs"], ora["eigenvectors"]))
    gram = np.conj(r["vecs"]) @ r["vecs"].T
    orth = np.max(np.abs(gram - np.eye(3)))
    res = max(residual(csr, lam, v) for lam, v in zip(r["vals"], r["vecs"]))
    print("long %s three eigenpairs: counts %s (oracle %s)  dlambda %.2e  1-overlap %.2e  max|V^H V - I| %.2e  residual %.2e  stats %s" % (
        "complex" if cplx else "real", r["iters"], ora["iter_counts"], dl, ov, orth, res,
        {k: r["stats"][k] for k in ("block_iterations", "block_flushed_vectors", "pair_gate_trips", "second_passes")}))
    assert r["iters"] == ora["iter_counts"]
    assert dl <= 1e-10 and ov <= 1e-8 and orth <= 1e-9 and res <= 1e-6 * NORM_INF
    assert r["stats"]["block_iterations"] >= r["iters"][0] - 2 and r["stats"]["pair_gate_trips"] == 0, r["stats"]


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_a_repair_in_every_iteration(ctx, oracle, cplx):
    """dgks_threshold = 2: every iteration is followed by a second Gram-Schmidt pass on its vector, which completes the raw
    basis in place (block_flush) and cuts the block short; the form re-enters with blk_k0 > 2 and unit rho in front of it."""
    r = run(ctx, cplx, 60, dgks=2.0)
    check(r, oracle_window(oracle, cplx, 60), cplx, "a repair in every iteration, window 60")
    st = r["stats"]
    assert st["second_passes"] >= 50 and st["block_flushed_vectors"] >= 1 and st["block_iterations"] >= 1, st


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_exponentiator_over_a_long_raw_basis(ctx, oracle, cplx):
    """exp(-1.5 i A) / exp(-1.5 A) with full_orthogonalize over 700 iterations (eps = 0: neither side's overlap test fires): the
    output GEMV reads 700 raw vectors through transformed coefficients.  Against the oracle and against the pair form.  (The slowest
    case of the file, about 40 s: the oracle and both runs of the library diagonalise T_j in every iteration, EX:124, O(j^3) on the
    host each.)"""
    csr = problem(cplx)[0]
    inp = G.start_vector(N_LONG, 7, dtype_of(cplx))
    a = -1.5j if cplx else -1.5
    window = 700
    o_out, o_it, _ = oracle.expo(csr, a, inp, max_iteration=window, eps=0.0, full_orthogonalize=True)
    got = {}
    try:
        for k, v in (("blas_small_bytes", "0"), ("sweep_pipeline", "2")):
            ctx.set_tuning(k, v)
        for block in (True, False):
            ctx.set_tuning("block_gs", "1" if block else "0")
            op = L.CsrOperator(ctx, *csr)
            ex = L.Exponentiator(op, N_LONG)
            ex.full_orthogonalize = True
            ex.max_iteration = window
            ex.eps = 0.0
            out, it = ex.run(a, inp)
            got[block] = (out, it, dict(ex.last_stats))
            op.close()
    finally:
        for k in KEYS:
            ctx.set_tuning(k, None)
    (out, it, st), (out0, it0, st0) = got[True], got[False]
    scale = np.linalg.norm(inp)
    err, err0 = np.max(np.abs(out - o_out)) / scale, np.max(np.abs(out - out0)) / scale
    print("long %s exponentiator: iterations %d (oracle %d, pair form %d)  max error %.2e  against the pair form %.2e  stats %s" % (
        "complex" if cplx else "real", it, o_it, it0, err, err0,
        {k: st[k] for k in ("block_iterations", "block_flushed_vectors", "pair_gate_trips", "second_passes")}))
    assert it == it0 == o_it == window
    assert err <= 1e-10 and err0 <= 1e-10
    assert st["block_iterations"] >= it - 2 and st["pair_gate_trips"] == 0 and st0["block_iterations"] == 0
