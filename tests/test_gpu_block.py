"""The block form of the Gram-Schmidt step — UP TO FOUR Lanczos iterations per sweep over a basis of RAW vectors that is never
rewritten (gs_block.hip, LoopState::enqueue_block in lanczos_loop.hpp; tools/block_gs_model.py is the executable specification) —
against the oracle's sequential modified Gram-Schmidt and against the pair form it replaces (block_gs = 0), at the smallest shapes
where the new code can go wrong.  By itself the form runs where the software-pipelined pair sweep runs (vectors of more than
~9 MiB) in passes of at most 1 024 iterations; here the streaming geometry is forced onto short vectors with the pair tests' hooks
(blas_small_bytes = 0, sweep_pipeline = 2).  Tolerances as everywhere: alpha / beta 1e-10 ||A||_inf, eigenvalue
1e-10 max(1, |lambda|), eigenvector 1 - overlap <= 1e-8, iteration counts equal."""
import numpy as np
import pytest

import lambda_lanczos_amd as L
from lambda_lanczos_amd import generators as G
from util import overlap

pytestmark = pytest.mark.gpu

KEYS = ("blas_small_bytes", "sweep_pipeline", "block_gs", "pair_split", "lagged_pieces", "test_workspace_fill", "ritz_tail")


def chain(n, t, cplx):
    """diag(0 .. 1, one separated eigenvalue 1.5) with nearest-neighbour coupling t (complex: i t above, -i t below the diagonal)."""
    d = np.linspace(0.0, 1.0, n)
    d[-1] = 1.5
    i = np.arange(n)
    cols = np.stack([i - 1, i, i + 1], 1)
    lo, up = (1j * t, -1j * t) if cplx else (t, t)
    vals = np.stack([np.full(n, lo), d.astype(complex if cplx else float), np.full(n, up)], 1)
    ok = (cols >= 0) & (cols < n)
    rp = np.concatenate([[0], np.cumsum(ok.sum(1))]).astype(np.int64)
    return rp, cols[ok].astype(np.int32), np.ascontiguousarray(vals[ok])


def norm_inf(t):
    return 1.5 + 2 * t


def fixed_init(v):
    return lambda out, *_: np.copyto(out, v)


def run(ctx, csr, init, window, *, block=True, split=None, pieces=None, ivs=None, fill=None, tail=True):
    n = len(init)
    settings = {"blas_small_bytes": "0", "sweep_pipeline": "2", "block_gs": "1" if block else "0"}
    if split:
        settings["pair_split"] = str(split)
    if pieces:
        settings["lagged_pieces"] = str(pieces)
    if fill is not None:
        settings["test_workspace_fill"] = str(fill)
    if not tail:
        settings["ritz_tail"] = "0"
    try:
        for k, v in settings.items():
            ctx.set_tuning(k, v)
        op = L.CsrOperator(ctx, *csr)
        eng = L.LambdaLanczos(op, n, True, 1)
        eng.init_vector = fixed_init(init)
        eng.max_iteration = window
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


def check_against(r, ora, scale, what=""):
    m = r["iters"][0]
    assert r["iters"] == ora["iter_counts"], what
    da = np.max(np.abs(r["alpha"][:m] - ora["alpha"][:m]))
    db = np.max(np.abs(r["beta"][:m - 1] - ora["beta"][:m - 1])) if m > 1 else 0.0
    dl = abs(r["vals"][0] - ora["eigenvalues"][0])
    ov = 1 - overlap(r["vecs"][0], ora["eigenvectors"][0])
    print("%s m %d  dalpha %.2e  dbeta %.2e  dlambda %.2e  1-overlap %.2e  stats %s" % (what, m, da, db, dl, ov, {
        k: r["stats"][k] for k in ("pair_iterations", "block_iterations", "block_flushed_vectors", "pair_gate_trips", "second_passes")}))
    assert da <= 1e-10 * scale and db <= 1e-10 * scale
    assert dl <= 1e-10 * max(1.0, abs(ora["eigenvalues"][0]))
    assert ov <= 1e-8


def took_the_form(st, window):
    """iterations 1 and 2 set the pipeline up; blocks of four, then of two, an odd last iteration as a block of one"""
    assert st["block_iterations"] == max(0, window - 2), st
    assert st["pair_iterations"] == (0 if window < 3 else 2 * ((window - 2) // 2)), st
    assert st["block_flushed_vectors"] == 0 and st["pair_gate_trips"] == 0, st


@pytest.mark.parametrize("window", [3, 4, 5, 6, 7, 41])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("n", [1500, 2048 * 3 + 5])
def test_short_and_ragged_vectors_with_every_block_remainder(ctx, oracle, n, cplx, window):
    """n = 1 500 (shorter than one 16 KiB strip of doubles) and 3 x 2 048 + 5 (ragged last strip), windows that end on every position
    of a block (remainders 0 - 3 of window - 2), real and complex."""
    csr, init = chain(n, 0.1, cplx), G.start_vector(n, 5, np.complex128 if cplx else np.float64)
    ora = oracle.lanczos(csr, init, True, max_iteration=window)
    r = run(ctx, csr, init, window)
    check_against(r, ora, norm_inf(0.1), "n %d window %d" % (n, window))
    took_the_form(r["stats"], window)
    if window in (7, 41):  # the same in 16 KiB strips (4 pieces per lane; by itself on vectors of 200 strips and more)
        r4 = run(ctx, csr, init, window, pieces=4)
        check_against(r4, ora, norm_inf(0.1), "n %d window %d, 16 KiB strips" % (n, window))
        took_the_form(r4["stats"], window)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_basis_across_slab_boundaries_and_split_sweeps_change_no_bit(ctx, oracle, cplx):
    """Slabs of 7 vectors (initial_vector_size): the trips of the sweep and the new vectors of a block cross slab boundaries.  Sweeps
    split into launches of at most 5 stored vectors, and of one (pair_split): every launch measures against the raw vectors, the two
    compensated vectors travel through memory, every column is summed in one launch.  Same bits as the plain run, which agrees
    with the oracle."""
    n = 2048 * 3 + 5
    csr, init = chain(n, 0.1, cplx), G.start_vector(n, 5, np.complex128 if cplx else np.float64)
    ora = oracle.lanczos(csr, init, True, max_iteration=41)
    plain = run(ctx, csr, init, 41)
    check_against(plain, ora, norm_inf(0.1), "plain")
    for what, kw in (("slabs of 7", dict(ivs=7)), ("launches of 5", dict(split=5)), ("launches of 1", dict(split=1))):
        r = run(ctx, csr, init, 41, **kw)
        took_the_form(r["stats"], 41)
        assert np.array_equal(r["alpha"], plain["alpha"]) and np.array_equal(r["beta"], plain["beta"]), what
        assert np.array_equal(r["vals"], plain["vals"]) and np.array_equal(r["vecs"][0], plain["vecs"][0]), what


@pytest.mark.parametrize("cplx,t,residue", [(False, 0.02, 1), (False, 0.03, 2), (False, 0.35, 3), (False, 0.06, 0),
                                            (True, 0.02, 1), (True, 0.15, 2), (True, 0.04, 3)])
def test_stop_inside_a_block(ctx, oracle, cplx, t, residue):
    """Runs that converge at an iteration = 1, 2, 3 (and 0) mod 4: blocks start at iterations 3, 7, 11, ..., so the stop falls on
    every position of a block.  The reported count, the eigenpair and the traces equal the oracle's and those of the pair form
    (block_gs = 0); the later vectors of the last block are slots nothing reads."""
    n = 1500
    csr, init = chain(n, t, cplx), G.start_vector(n, 5, np.complex128 if cplx else np.float64)
    ora = oracle.lanczos(csr, init, True, max_iteration=200)
    count = ora["iter_counts"][0]
    assert count < 200 and count % 4 == residue, count
    blk = run(ctx, csr, init, 200)
    pair = run(ctx, csr, init, 200, block=False)
    check_against(blk, ora, norm_inf(t), "block")
    check_against(pair, ora, norm_inf(t), "pair")
    assert blk["iters"] == pair["iters"] == [count]
    assert blk["stats"]["block_iterations"] >= count - 2 and pair["stats"]["block_iterations"] == 0
    assert blk["stats"]["block_flushed_vectors"] == 0
    assert abs(blk["vals"][0] - pair["vals"][0]) <= 1e-10 * max(1.0, abs(pair["vals"][0]))
    assert 1 - overlap(blk["vecs"][0], pair["vecs"][0]) <= 1e-8
    assert np.max(np.abs(blk["alpha"] - pair["alpha"])) <= 1e-10 * norm_inf(t)


def test_block_form_leaves_through_its_gate_when_the_krylov_space_is_exhausted(ctx, oracle):
    """No plant hook reaches the block sweep, so a near-breakdown matrix: an operator with 5 distinct eigenvalues exhausts its
    Krylov space after 5 iterations, inside the block of iterations 3 - 6.  Vector 5 is rounding noise whose components along the
    stored vectors are not small against its norm: the fold's gate catches it, the vector stands, the basis is flushed (the raw
    vectors completed in place) and the pass finishes in the one-sweep form."""
    rng = np.random.default_rng(4)
    n = 300
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.repeat([1.0, 2.0, 3.5, 5.0, 9.0], n // 5)
    a = (q * lam) @ q.T
    a = (a + a.T) / 2
    init = G.start_vector(n, 1)
    ora = oracle.lanczos(G.dense_to_csr(a), init, True, max_iteration=60)
    try:
        for k, v in (("blas_small_bytes", "0"), ("sweep_pipeline", "2")):
            ctx.set_tuning(k, v)
        op = L.DenseOperator(ctx, a)
        eng = L.LambdaLanczos(op, n, True, 1)
        eng.init_vector = fixed_init(init)
        eng.max_iteration = 60
        vals, vecs = eng.run()
        st = dict(eng.last_stats)
        count = eng.getIterationCounts()[0]
        alpha, beta = eng.last_alpha.copy(), eng.last_beta.copy()
        op.close()
    finally:
        for k in KEYS:
            ctx.set_tuning(k, None)
    print("count %d (oracle %d) stats %s" % (count, ora["iter_counts"][0], st))
    assert abs(vals[0] - 9.0) <= 1e-10 and abs(count - ora["iter_counts"][0]) <= 1
    assert np.linalg.norm(a @ vecs[0] - vals[0] * vecs[0]) <= 1e-9
    assert st["block_iterations"] >= 2 and st["pair_gate_trips"] == 1 and st["block_flushed_vectors"] >= 1, st
    m = 4   # the recurrence up to the exhaustion
    assert np.max(np.abs(alpha[:m] - ora["alpha"][:m])) <= 1e-10 * 9 and np.max(np.abs(beta[:m] - ora["beta"][:m])) <= 1e-10 * 9


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_off_switch_and_poisoned_workspace(ctx, oracle, cplx):
    """block_gs = 0 takes the pair form in every iteration the block form would have taken (the two settings' statistics say
    which form ran; bits of the parent commit are not stored in the repository), within the oracle's tolerances.  And the
    form reads nothing it has not written: with the workspace filled with NaN bytes a run returns the bits of a clean one."""
    n, window = 2048 * 3 + 5, 41
    csr, init = chain(n, 0.1, cplx), G.start_vector(n, 5, np.complex128 if cplx else np.float64)
    ora = oracle.lanczos(csr, init, True, max_iteration=window)
    on = run(ctx, csr, init, window)
    off = run(ctx, csr, init, window, block=False)
    check_against(off, ora, norm_inf(0.1), "off")
    took_the_form(on["stats"], window)
    assert off["stats"]["block_iterations"] == 0 and off["stats"]["pair_iterations"] == 2 * ((window - 2) // 2), off["stats"]
    poisoned = run(ctx, csr, init, window, fill=255)
    took_the_form(poisoned["stats"], window)
    assert np.array_equal(poisoned["alpha"], on["alpha"]) and np.array_equal(poisoned["beta"], on["beta"])
    assert np.array_equal(poisoned["vals"], on["vals"]) and np.array_equal(poisoned["vecs"][0], on["vecs"][0])


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_block_pending_at_the_end_of_a_pass_is_completed_in_place_without_the_ritz_tail(ctx, oracle, cplx):
    """ritz_tail = 0 while a block is pending at the end of the pass: the raw vectors are completed in place (block_flush, one
    multi-axpy each) and the Ritz GEMV reads them with the plain coefficients, where the default run transforms the coefficients and
    leaves the basis raw.  The loop is the same up to there — alpha, beta and the eigenvalue are the default run's bits — and the
    eigenvector agrees with the default run's and the oracle's to the file's tolerance."""
    n, window = 2048 * 3 + 5, 41
    csr, init = chain(n, 0.1, cplx), G.start_vector(n, 5, np.complex128 if cplx else np.float64)
    ora = oracle.lanczos(csr, init, True, max_iteration=window)
    default = run(ctx, csr, init, window)
    flushed = run(ctx, csr, init, window, tail=False)
    check_against(default, ora, norm_inf(0.1), "default")
    check_against(flushed, ora, norm_inf(0.1), "ritz_tail = 0")
    assert np.array_equal(flushed["alpha"], default["alpha"]) and np.array_equal(flushed["beta"], default["beta"])
    assert np.array_equal(flushed["vals"], default["vals"]) and flushed["iters"] == default["iters"]
    ov = 1 - overlap(flushed["vecs"][0], default["vecs"][0])
    print("1-overlap against the default run %.2e" % ov)
    assert ov <= 1e-8
    assert flushed["stats"]["block_flushed_vectors"] >= 1 and default["stats"]["block_flushed_vectors"] == 0


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_exponentiator_over_a_raw_basis(ctx, oracle, cplx):
    """The Exponentiator with full_orthogonalize takes the form too: its output GEMV reads the raw basis through transformed
    coefficients.  Complex, exp(-1.5 i A): the run converges inside a block.  Real, exp(-1.5 A): the reference's overlap test never
    fires for a real exponent, so the window (29 iterations: blocks of four, a block of two, a block of one) ends the run.  Against
    the oracle, and against the pair form (block_gs = 0)."""
    n = 2048 * 3 + 5
    csr, inp = chain(n, 0.3, cplx), G.start_vector(n, 7, np.complex128 if cplx else np.float64)
    a = -1.5j if cplx else -1.5
    window = 200 if cplx else 29
    o_out, o_it, _ = oracle.expo(csr, a, inp, max_iteration=window, full_orthogonalize=True)
    got = {}
    try:
        for k, v in (("blas_small_bytes", "0"), ("sweep_pipeline", "2")):
            ctx.set_tuning(k, v)
        for block in (True, False):
            ctx.set_tuning("block_gs", "1" if block else "0")
            op = L.CsrOperator(ctx, *csr)
            ex = L.Exponentiator(op, n)
            ex.full_orthogonalize = True
            ex.max_iteration = window
            out, it = ex.run(a, inp)
            got[block] = (out, it, dict(ex.last_stats))
            op.close()
    finally:
        for k in KEYS:
            ctx.set_tuning(k, None)
    (out, it, st), (out0, it0, st0) = got[True], got[False]
    err = np.max(np.abs(out - o_out)) / np.linalg.norm(inp)
    print("iterations %d (oracle %d, pair form %d)  max error %.2e  stats %s" % (it, o_it, it0, err, st))
    assert it == it0 and abs(it - o_it) <= 1
    assert err <= 1e-10 and np.max(np.abs(out - out0)) <= 1e-10 * np.linalg.norm(inp)
    assert st["block_iterations"] >= it - 2 and st["block_flushed_vectors"] == 0 and st0["block_iterations"] == 0
