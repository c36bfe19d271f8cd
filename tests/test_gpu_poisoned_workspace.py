"""The whole loops on POISONED workspace: the Krylov slabs, the run-scoped work vectors and every floating-point buffer the context
hands out are filled, before anyone uses them, with one byte (the test hook test_workspace_fill / LL_TEST_WORKSPACE_FILL,
util.HOOK_KEYS).  In production that memory holds old matrix values or old vectors of another type and shape: the pads [n, ld) of
a slab row, the vectors beyond the current count and recycled work buffers are never cleared.  In the rest of the suite it holds
zeros.

Each case creates its operator and runs four times on one context: fill 0x00, 0x00 again (the form is bit-reproducible at all), 0xFF
(NaN in every floating-point type) and 0x7F (huge and finite: a max|x| scan drops NaN but takes this).  The operator is created
anew under each fill, so its value images come out of filled memory too.  Fixed windows (eps = 0, max_iteration = 41) involve no
stop decision.  Asserted: alpha, beta, eigenvalues, eigenvectors, iteration counts agree bit for bit over the four runs, and
last_stats shows the named form (test_gpu_float_runs.check_form).  The operators take the PB kernel with fixed-point sums: its
choice involves no timing, and its bits do not depend on the placement of its image."""
import numpy as np
import pytest

import float_run_model as M
import lambda_lanczos_amd as L
from guarded import pattern
from lambda_lanczos_amd import _capi as capi
from test_gpu_float_runs import CASES_D, FORMS, check_form, set_form, solve

pytestmark = pytest.mark.gpu

RUN_FILLS = (0x00, 0x00, 0xFF, 0x7F)
WINDOW = 41
# lengths that are no multiple of a strip or of 256: n = 3721 (d, s) and n = 1369 (z, c)
PROBLEM = {"d": ("laplace", 61), "s": ("laplace", 61), "z": ("torus", 37), "c": ("torus", 37)}
# the run forms of test_gpu_float_runs.FORMS and the software-pipelined pair sweep (by itself only on vectors of more than ~9 MiB;
# forced as in test_gpu_pair.test_software_pipelined_sweep_changes_no_bit), whole and in split sweeps
PIPELINED = {"pair_pipelined": "pair_stream", "pair_pipelined_split": "pair_stream_split"}
COUNTS = {}


def _bytes(v):
    return np.atleast_1d(np.asarray(v)).view(np.uint8)


def _four_runs(llenv, family, what, run):
    """run() under each fill of RUN_FILLS; every entry of its result dict must agree bit for bit.  Returns the first result."""
    outs = []
    for fill in RUN_FILLS:
        llenv.setenv("LL_TEST_WORKSPACE_FILL", str(fill))
        outs.append(run(fill))
    llenv.delenv("LL_TEST_WORKSPACE_FILL")
    for i, (fill, r) in enumerate(zip(RUN_FILLS, outs)):
        if i == 0:
            continue
        for k, v in outs[0].items():
            assert np.array_equal(_bytes(v), _bytes(r[k])), (
                "%s: %s differs between the first run (fill 0x00) and run %d (fill 0x%02X)" % (what, k, i + 1, fill))
    COUNTS[family] = COUNTS.get(family, 0) + 1
    print("poisoned workspace, %s: %d cases compared bit for bit, 0 by bound" % (family, COUNTS[family]))
    return outs[0]


def _operator(ctx, op):
    op_dev = L.CsrOperator(ctx, *op.csr, accuracy=capi.ACCURACY_NORMWISE, kernel=capi.SPMV_PB)
    assert op_dev.selected_spmv() == capi.SPMV_PB
    return op_dev


def _run_bits(r):
    return dict(alpha=r["last_alpha"], beta=r["last_beta"], vals=np.asarray(r["vals"]), vecs=np.asarray(r["vecs"]),
                iters=np.asarray(r["iters"], dtype=np.int64))


# ------------------------------------------------------------------ the run forms
@pytest.mark.parametrize("form", list(FORMS) + list(PIPELINED))
@pytest.mark.parametrize("t", list(PROBLEM))
def test_run_forms_give_the_same_bits_on_poisoned_workspace(ctx, llenv, t, form):
    name, size = PROBLEM[t]
    op, v0, find_max = M.case_setup(name, size, t)
    named = PIPELINED.get(form, form)
    mode = set_form(llenv, named)
    stats = []

    def run(fill):
        op_dev = _operator(ctx, op)
        try:
            r = solve(op_dev, op, v0, find_max, mode, window=WINDOW)
        finally:
            op_dev.close()
        assert r["iters"] == [WINDOW] and len(r["last_alpha"]) == WINDOW
        stats.append(r["stats"])
        return _run_bits(r)

    if form in PIPELINED:
        ctx.set_tuning("sweep_pipeline", "2")
    try:
        _four_runs(llenv, "run forms", "%s%d %s %s" % (name, size, t, form), run)
    finally:
        ctx.set_tuning("sweep_pipeline", None)
    for st in stats:
        check_form(named, st, WINDOW)


# ------------------------------------------------------------------ restart passes behind locked vectors
@pytest.mark.parametrize("t", ["d", "c"])
def test_restart_passes_give_the_same_bits_on_poisoned_workspace(ctx, llenv, t):
    """Three eigenpairs to convergence at the default eps: the locked vectors' buffer, the Ritz vectors and the slabs of every pass."""
    name, size = PROBLEM[t]
    op, v0, find_max = M.case_setup(name, size, t)

    def run(fill):
        op_dev = _operator(ctx, op)
        try:
            r = solve(op_dev, op, v0, find_max, L.ORTH_CGS_DGKS, num_eigs=3)
        finally:
            op_dev.close()
        assert len(r["iters"]) > 1 and len(r["vals"]) == 3, r["iters"]
        return _run_bits(r)

    _four_runs(llenv, "restart passes", "%s%d %s three eigenpairs" % (name, size, t), run)


# ------------------------------------------------------------------ the Exponentiator
CASE_D_IDS = ["%s-%s-%s" % (c[0], c[2], c[3]) for c in CASES_D]


@pytest.mark.parametrize("full", [False, True], ids=["three_term", "full_orthogonalize"])
@pytest.mark.parametrize("name,size,a,t", CASES_D, ids=CASE_D_IDS)
def test_exponentiator_gives_the_same_bits_on_poisoned_workspace(ctx, llenv, name, size, a, t, full):
    op, v = M.expo_setup(name, size, t)
    m = M.EXPO_M[M.expo_key(name, size, a)]

    def run(fill):
        op_dev = _operator(ctx, op)
        try:
            ex = L.Exponentiator(op_dev, op.n)
            ex.eps, ex.max_iteration, ex.full_orthogonalize = 0.0, m, full
            out, itern = ex.run(a, v)
        finally:
            op_dev.close()
        assert out.dtype == op.storage and itern == m
        return dict(out=out, iterations=np.int64(itern))

    _four_runs(llenv, "exponentiator", "expo %s%d a = %s %s full = %s" % (name, size, a, t, full), run)


@pytest.mark.parametrize("name,size,a,t", CASES_D, ids=CASE_D_IDS)
def test_taylor_run_gives_the_same_bits_on_poisoned_workspace(ctx, llenv, name, size, a, t):
    """The series at its default eps, and a = 0 from one device buffer into another (whose previous contents are the fill): the
    output is the input."""
    op, v = M.expo_setup(name, size, t)

    def run(fill):
        op_dev = _operator(ctx, op)
        inp, outd = ctx.to_device(v), ctx.empty(op.n, op.storage)
        outd.set(pattern(op.n, op.storage, fill))
        try:
            out, terms = L.Exponentiator(op_dev, op.n).taylor_run(a, v)
            _, terms0 = L.Exponentiator(op_dev, op.n).taylor_run(0.0, inp, out=outd)
            out0 = outd.get()
            assert np.array_equal(inp.get(), v)
        finally:
            op_dev.close()
            inp.free()
            outd.free()
        return dict(out=out, terms=np.int64(terms), out_zero=out0, terms_zero=np.int64(terms0))

    r = _four_runs(llenv, "taylor", "taylor %s%d a = %s %s" % (name, size, a, t), run)
    assert np.array_equal(r["out_zero"].view(np.uint8), v.view(np.uint8)), "exp(0 A) v is not v"


# ------------------------------------------------------------------ two-pass Lanczos
@pytest.mark.parametrize("t", list(PROBLEM))
def test_two_pass_gives_the_same_bits_on_poisoned_workspace(ctx, llenv, t):
    """Its four-vector workspace (the Ritz vector accumulated in a work vector, returned to the host) and its three-vector one (the
    Ritz vector accumulated in the caller's device buffer, whose previous contents are the fill)."""
    name, size = PROBLEM[t]
    op, v0, find_max = M.case_setup(name, size, t)

    def run(fill):
        op_dev = _operator(ctx, op)
        outd = ctx.empty(op.n, op.storage)
        outd.set(pattern(op.n, op.storage, fill))
        try:
            res = {}
            for key, dev in (("four", None), ("three", outd)):
                eng = L.LambdaLanczos(op_dev, op.n, find_max, 1)
                eng.eigenvalue_offset = op.offset
                eng.init_vector = lambda out, *_: np.copyto(out, v0)
                eng.eps, eng.max_iteration = 0.0, WINDOW
                eng.eigenvectors_out = dev
                val, vec, info = eng.run_two_pass()
                assert info["iterations"] == WINDOW and info["stats"]["workspace_vectors"] == (3 if dev is not None else 4)
                assert info["stats"]["replay_mismatches"] == 0
                res.update({key + "_val": np.float64(val), key + "_vec": vec if dev is None else outd.get(),
                            key + "_residual": np.float64(info["residual"]), key + "_alpha": eng.last_alpha, key + "_beta": eng.last_beta})
        finally:
            op_dev.close()
            outd.free()
        return res

    r = _four_runs(llenv, "two-pass", "two-pass %s%d %s" % (name, size, t), run)
    assert np.array_equal(r["four_vec"].view(np.uint8), r["three_vec"].view(np.uint8))


# ------------------------------------------------------------------ a cached slab crosses scalar types and shapes (no hook)
def test_a_float_run_on_a_slab_cached_by_a_complex_double_run(ctx):
    """The slab cache matches on byte count only.  A complex-double run on the 37 x 37 torus leaves slabs of 25 vectors x 1536
    elements x 16 bytes; the float run on the 61 x 61 Laplacian asks for 40 vectors x 3840 elements x 4 bytes, the same 614 400
    bytes, and takes them — full of complex doubles, at another leading dimension.  Its bits must be those of the same run on
    fresh memory (after release_cache)."""
    def ld(n):
        return -(-n // 256) * 256

    zop, zv0, zmax = M.case_setup("torus", 37, "z")
    sop, sv0, smax = M.case_setup("laplace", 61, "s")
    ivs_z, ivs_s = 25, 40          # both below max_iteration + 2 (pick_chunk_vecs): the slab holds exactly that many vectors
    assert ivs_z * ld(zop.n) * 16 == ivs_s * ld(sop.n) * 4 and max(ivs_z, ivs_s) <= WINDOW + 2

    def run(op, v0, find_max, ivs):
        op_dev = _operator(ctx, op)
        try:
            eng = L.LambdaLanczos(op_dev, op.n, find_max, 1)
            eng.eigenvalue_offset = op.offset
            eng.init_vector = lambda out, *_: np.copyto(out, v0)
            eng.eps, eng.max_iteration, eng.initial_vector_size = 0.0, WINDOW, ivs
            vals, vecs = eng.run()
        finally:
            op_dev.close()
        assert eng.getIterationCounts() == [WINDOW]
        return dict(alpha=eng.last_alpha, beta=eng.last_beta, vals=np.asarray(vals), vecs=np.asarray(vecs))

    ctx.release_cache()
    run(zop, zv0, zmax, ivs_z)
    reused = run(sop, sv0, smax, ivs_s)
    ctx.release_cache()
    fresh = run(sop, sv0, smax, ivs_s)
    for k, v in fresh.items():
        assert np.array_equal(_bytes(v), _bytes(reused[k])), "%s differs between the run on a recycled slab and on fresh memory" % k
    print("poisoned workspace, cross-run reuse: 1 case compared bit for bit, 0 by bound")
