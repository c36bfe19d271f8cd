"""The two-pass eigen-solver without a stored Krylov basis (ll_lanczos_two_pass_*, csrc/two_pass_run.cpp, csrc/recur.hip):
the replayed-step kernel against exact arithmetic in all four types, the solver against numpy.linalg.eigh of the dense matrix on
every operator family, the replay invariant and the constant work-space, the edges, and the refusal of a sharded context."""
import ctypes as C
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import contract_cases as K
import exact_ref as E
import lambda_lanczos_amd as L
from guarded import GUARD, guarded as _guarded, unguard as _unguard  # noqa: F401 (fill 0xA5)
from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G
from util import csr_matvec, inf_norm

pytestmark = pytest.mark.gpu

TYPES = {"d": np.float64, "z": np.complex128, "s": np.float32, "c": np.complex64}


def _single(dtype):
    return np.dtype(dtype) in (np.float32, np.complex64)


def _cplx(dtype):
    return np.dtype(dtype).kind == "c"


def _eps(dtype):
    return E.EPS_F if _single(dtype) else E.EPS_D


# ------------------------------------------------------------------ 1. the replayed step against exact arithmetic
@pytest.mark.parametrize("with_p", [True, False], ids=["p", "nop"])
@pytest.mark.parametrize("tid", list(TYPES))
def test_recur_accum_against_exact_arithmetic(ctx, tid, with_p):
    """y' = y - a x - b p and psi' = psi + g y' in one sweep.  With S = |y| + |a||x| + |b||p| (element-wise moduli) and first-order
    chains of individually rounded operations in T, each scaled by 1.01 for second order:
      |y' - y'_exact|     <= 3 eps_T S                    two products and two subtractions (the bound of the three_term check)
      |psi' - psi'_exact| <= eps_T (|psi| + 5 |g| S)      the product g y', the final sum, the error inherited from y'
    The exact values are formed in extended precision from the stored inputs.  x, p and everything outside [0, n) stay as they were."""
    dtype = TYPES[tid]
    ept = 64 // np.dtype(dtype).itemsize
    elems = 256 * ept
    wide = np.clongdouble if _cplx(dtype) else np.longdouble
    a, b, g = -1.7, 0.3, 0.625
    eps = _eps(dtype)
    worst = [0.0, 0.0]
    for n in [1, 7, ept - 1, 2047, 2048, 2049, 3 * elems + 5]:
        y, x, p, psi = (K.start_x(n, dtype, s) for s in (41, 42, 43, 44))
        for shift in (0, 1):
            yb, yv = _guarded(ctx, y, shift)
            xb, xv = _guarded(ctx, x, shift)
            pb, pv = _guarded(ctx, p, shift)
            qb, qv = _guarded(ctx, psi, shift)
            L.recur_accum(ctx, yv, xv, pv if with_p else None, a, b, g, qv, n)
            gy, gq = _unguard(yb, n, shift).astype(wide), _unguard(qb, n, shift).astype(wide)
            assert np.array_equal(_unguard(xb, n, shift), x) and np.array_equal(_unguard(pb, n, shift), p)
            bp = b if with_p else 0.0
            y_exact = y.astype(wide) - wide(a) * x.astype(wide) - wide(bp) * p.astype(wide)
            q_exact = psi.astype(wide) + wide(g) * y_exact
            S = (np.abs(y) + abs(a) * np.abs(x) + abs(bp) * np.abs(p)).astype(np.float64)
            by = 3 * eps * S * 1.01
            bq = eps * (np.abs(psi).astype(np.float64) + 5 * abs(g) * S) * 1.01
            ey, eq = np.abs(gy - y_exact).astype(np.float64), np.abs(gq - q_exact).astype(np.float64)
            worst = [max(worst[0], float(np.max(ey / by))), max(worst[1], float(np.max(eq / bq)))]
            assert np.all(ey <= by), (n, shift, float(np.max(ey / by)))
            assert np.all(eq <= bq), (n, shift, float(np.max(eq / bq)))
            for buf in (yb, xb, pb, qb):
                buf.free()
    print("recur_accum", tid, "p" if with_p else "no p", "largest error / bound (y, psi):", worst)


# ------------------------------------------------------------------ 2. the solver against exact diagonalisation
def _laplace_case():
    return G.laplace2d(40)


def _terms(name):
    if name == "tfim":
        return 10, G.tfim_terms(10, 1.0, 1.5, periodic=True)
    if name == "xyz":
        return 10, G.xyz_terms(10, 1.0, 0.8, 0.6)
    if name == "sector":
        return 12, G.heisenberg_terms(12)
    return 12, G.tfim_terms(12, 1.0, 1.5, periodic=True)   # symmetric


def _matrix(name):
    """CSR (float64) of the operator `name` from the generator that matches its operator class."""
    if name in ("laplace", "host"):
        return _laplace_case()
    sites, terms = _terms(name)
    if name == "sector":
        return G.pauli_sector_csr(sites, 6, terms)
    if name == "symmetric":
        return G.pauli_symmetric_csr(sites, 0, 1, 1, terms)
    return G.pauli_csr(sites, terms)


def _operator(ctx, name, dtype):
    if name == "laplace":
        rp, ci, va = _laplace_case()
        return L.CsrOperator(ctx, rp, ci, va.astype(dtype))
    if name == "host":
        csr = _laplace_case()

        def mv_mul(vin, vout):
            vout[:] = csr_matvec(csr, vin)

        return L.HostOperator(ctx, mv_mul, csr[0].shape[0] - 1, dtype)
    sites, terms = _terms(name)
    if name == "sector":
        return L.PauliSectorOperator(ctx, sites, 6, terms, dtype)
    if name == "symmetric":
        return L.PauliSymmetricOperator(ctx, sites, 0, terms, dtype, parity=1, inversion=1)
    return L.PauliOperator(ctx, sites, terms, dtype)


_EXACT, _RUNS = {}, {}


def _exact(name):
    """(csr, dense A, eigenvalues ascending, eigenvectors, ||A||_inf) — numpy.linalg.eigh, once per operator."""
    key = "laplace" if name == "host" else name
    if key not in _EXACT:
        csr = _matrix(key)
        n = csr[0].shape[0] - 1
        A = np.asarray(K.dense_of(csr, n), dtype=np.float64)
        w, V = np.linalg.eigh(A)
        _EXACT[key] = (csr, A, w, V, float(inf_norm(csr)))
    return _EXACT[key]


def _start(n, dtype, seed=1):
    return G.start_vector(n, seed, np.complex128 if _cplx(dtype) else np.float64).astype(dtype)


def _engine(op, n, find_max, init, offset=0.0):
    eng = L.LambdaLanczos(op, n, find_max, 1)
    eng.eigenvalue_offset = offset
    eng.init_vector = lambda v, *_: np.copyto(v, init)
    return eng


def _offset(name, find_max):
    """The eigenvalue_offset of every eigen-solver test of this suite (tests/test_gpu_pauli.py): -||A||_inf for the lowest
    eigenvalue, +||A||_inf for the highest."""
    norm = _exact(name)[4]
    return norm if find_max else -norm


def _runs(ctx, name, find_max, tid):
    """One two-pass run and one stored-basis run (one tracked root, like the two-pass solver) on the same operator and start
    vector, shared by the tests below."""
    key = (name, find_max, tid)
    if key not in _RUNS:
        dtype = TYPES[tid]
        n = _exact(name)[1].shape[0]
        op = _operator(ctx, name, dtype)
        try:
            init = _start(n, dtype)
            eng = _engine(op, n, find_max, init, _offset(name, find_max))
            val, vec, info = eng.run_two_pass()
            alpha, beta = eng.last_alpha, eng.last_beta
            ref = _engine(op, n, find_max, init, _offset(name, find_max))
            ref.num_eigs_per_iteration = 1   # one tracked root: the stop rule of the two-pass solver
            rvals, rvecs = ref.run()
            _RUNS[key] = dict(val=val, vec=vec, info=info, alpha=alpha, beta=beta, eps=eng.eps, ref_val=rvals[0],
                              ref_vec=rvecs[0], ref_iterations=ref.getIterationCounts()[0])
        finally:
            op.close()
    return _RUNS[key]


DOUBLE_CASES = [("tfim", False), ("tfim", True), ("xyz", False), ("sector", False), ("symmetric", False), ("laplace", False),
                ("laplace", True), ("host", False)]
FLOAT_CASES = [("tfim", False), ("tfim", True), ("laplace", False), ("laplace", True)]
SOLVER_CASES = [(n, f, t) for t in "dz" for n, f in DOUBLE_CASES] + [(n, f, t) for t in "sc" for n, f in FLOAT_CASES]


def _case_id(c):
    return "%s-%s-%s" % (c[0], "max" if c[1] else "min", c[2])


@pytest.mark.parametrize("case", SOLVER_CASES, ids=_case_id)
def test_two_pass_against_exact_diagonalisation(ctx, case):
    """Eigenvalue, residual (recomputed on the host), overlap with the exact eigenvector, the reported residual, ||psi|| and the
    iteration count, by the rules of tests/test_gpu_pauli.py and DESIGN.md section 4:
      eigenvalue error        double <= 1e-10 max(1, |lambda|)    float <= 20 eps max(1, |lambda + offset|) (eps: the run's
                                                                  tolerance 1e3 FLT_EPSILON; the rule of tests/test_gpu_float.py)
      ||A psi - lambda psi||  double <= 1e-5 ||A||_inf
      1 - |<psi, psi_exact>|  double <= 1e-8                      float <= 1e-3
      iterations              within 3 of LambdaLanczos.run() with one tracked root on the same operator and start vector
    The start vector is generators.start_vector(n, 1); eigenvalue_offset is -/+ ||A||_inf as in every eigen-solver test of
    tests/test_gpu_pauli.py.  Why not 0: the stop rule compares the change of the Ritz value with eps |theta|, theta the Ritz value
    of A + offset.  For the Laplacian's lowest eigenvalue 0.0117 and offset 0 that threshold is 2.6e-15, one rounding of
    ||A|| = 8, so rounding noise decides the iteration at which ANY implementation stops: a numpy model of the plain and of the
    re-orthogonalised recurrence stops after 127 and 126 iterations, the stored-basis solver here after 123 (CSR kernel) and 126
    (host callback), the two-pass solver after 130 and 125 — no two of them are "the same recurrence until orthogonality is
    lost" to within 3.  With the offset the threshold is 1.8e-12, a thousand roundings, and all of them stop at iteration 109.
    Measured on an MI355X: every one of the 24 cases stops at exactly the stored-basis solver's iteration; double: eigenvalue
    error <= 3e-12 scale, residual <= 2.6e-7 ||A||_inf, 1 - overlap <= 1.2e-11.
    Float overlap: a float run stops at a change of 1e3 FLT_EPSILON |theta|, i.e. 1e-3 to 3e-3 here, before the eigenvector has
    converged to 1e-3 wherever that is not small against the gap (1 - overlap: TFIM 4e-4 .. 1.9e-3, Laplacian 0.05 .. 0.6; the
    stored-basis solver's float result is as far from the exact vector, to three digits).  Where 1e-3 against the exact vector is
    exceeded the check is settled against the stored-basis solver's float result on the same operator and start vector:
    1 - |<psi, psi_stored>| <= 1e-3; measured <= 6e-8, a margin of four orders of magnitude."""
    name, find_max, tid = case
    dtype = TYPES[tid]
    csr, A, w, V, norm = _exact(name)
    r = _runs(ctx, name, find_max, tid)
    lam, xv = (w[-1], V[:, -1]) if find_max else (w[0], V[:, 0])
    psi = r["vec"].astype(np.complex128)
    scale = max(1.0, abs(lam))
    scale_float = max(1.0, abs(lam + _offset(name, find_max)))   # the float rule's scale (tests/test_gpu_float.py)
    err = abs(r["val"] - lam)
    res = float(np.linalg.norm(A @ psi - r["val"] * psi))
    miss = 1.0 - abs(np.vdot(xv, psi))
    miss_stored = 1.0 - abs(np.vdot(r["ref_vec"].astype(np.complex128), psi))
    norm_err = abs(float(np.linalg.norm(psi)) - 1.0)
    its, ref_its = r["info"]["iterations"], r["ref_iterations"]
    print("two-pass %s: m = %d (stored basis %d), eigenvalue error / scale %.3e, residual / |A|_inf %.3e (reported %.3e), "
          "1 - overlap %.3e (against the stored-basis vector %.3e), | |psi| - 1 | %.3e, stored-basis 1 - overlap %.3e"
          % (_case_id(case), its, ref_its, err / scale, res / norm, r["info"]["residual"] / norm, miss, miss_stored, norm_err,
             1.0 - abs(np.vdot(xv, r["ref_vec"].astype(np.complex128)))))
    assert r["vec"].dtype == np.dtype(dtype) and r["vec"].shape == (A.shape[0],)
    if _single(dtype):
        assert err <= 20 * r["eps"] * scale_float
        assert miss <= 1e-3 or miss_stored <= 1e-3
    else:
        assert err <= 1e-10 * scale
        assert res <= 1e-5 * norm
        assert miss <= 1e-8
        assert abs(r["info"]["residual"] - res) <= 1e-3 * res + 1e-12 * norm
    assert norm_err <= 4 * _eps(dtype)
    assert its == len(r["alpha"]) == len(r["beta"]) == r["info"]["stats"]["total_iterations"]
    assert abs(its - ref_its) <= 3


# ------------------------------------------------------------------ 3. replay invariant and memory
@pytest.mark.parametrize("case", [c for c in SOLVER_CASES if c[2] in "dz" and c[0] != "host"], ids=_case_id)
def test_replay_reproduces_every_alpha_bit_for_bit(ctx, case):
    """Pass 2 makes the same operator calls on the same buffers with the same element update: the alpha every operator kernel
    produces again equals the recorded one as bits, in every iteration."""
    r = _runs(ctx, *case)
    assert r["info"]["stats"]["replay_mismatches"] == 0
    assert r["info"]["stats"]["workspace_vectors"] == 4   # host eigenvector: three rotating vectors and psi


def test_workspace_is_three_or_four_vectors_and_device_buffers_change_nothing(ctx):
    dtype = np.float64
    n = _exact("tfim")[1].shape[0]
    host = _runs(ctx, "tfim", False, "d")
    op = _operator(ctx, "tfim", dtype)
    init = _start(n, dtype)
    eng = _engine(op, n, False, init, _offset("tfim", False))
    val, vec, info = eng.run_two_pass(want_vector=False)
    assert vec is None and info["residual"] is None and info["stats"]["workspace_vectors"] == 3
    assert val == host["val"] and info["iterations"] == host["info"]["iterations"]
    # the Ritz vector accumulated in the caller's device buffer; then the start vector read from the caller's device buffer too
    start_dev, out_dev = ctx.to_device(init), ctx.empty(n, dtype)
    eng.eigenvectors_out = out_dev
    val2, vec2, info2 = eng.run_two_pass()
    assert vec2 is out_dev and info2["stats"]["workspace_vectors"] == 3
    assert val2 == host["val"] and np.array_equal(out_dev.get().view(np.uint8), host["vec"].view(np.uint8))
    eng.init_vector = start_dev
    out_dev.set(np.zeros(n, dtype))
    val3, _, info3 = eng.run_two_pass()
    assert info3["stats"]["workspace_vectors"] == 3 and info3["stats"]["replay_mismatches"] == 0
    assert val3 == host["val"] and info3["residual"] == host["info"]["residual"]
    assert np.array_equal(out_dev.get().view(np.uint8), host["vec"].view(np.uint8))   # bit for bit the host-buffer run
    assert np.array_equal(start_dev.get(), init)                                      # the start buffer is unchanged
    assert np.array_equal(eng.last_alpha, host["alpha"]) and np.array_equal(eng.last_beta, host["beta"])
    op.close()
    start_dev.free()
    out_dev.free()


# ------------------------------------------------------------------ 4. edges
def _diag_csr(d):
    n = len(d)
    return np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), np.asarray(d, dtype=np.float64)


def test_start_vector_that_is_an_eigenvector_stops_after_one_iteration(ctx):
    n = 50
    op = L.CsrOperator(ctx, *_diag_csr(np.arange(1.0, n + 1.0)))
    init = np.zeros(n)
    init[7] = -2.5
    val, vec, info = _engine(op, n, False, init).run_two_pass()
    assert info["iterations"] == 1 and val == 8.0
    assert np.array_equal(np.abs(vec), np.abs(init) / 2.5)
    assert info["residual"] == 0.0 and info["stats"]["replay_mismatches"] == 0
    op.close()


def test_max_iteration_ends_the_pass_with_the_ritz_pair_of_that_tridiagonal(ctx):
    csr, A, w, V, norm = _exact("laplace")
    n = A.shape[0]
    op = _operator(ctx, "laplace", np.float64)
    for find_max in (False, True):
        eng = _engine(op, n, find_max, _start(n, np.float64))
        eng.max_iteration = 5
        val, vec, info = eng.run_two_pass()
        assert info["iterations"] == 5 and len(eng.last_alpha) == 5
        T = np.diag(eng.last_alpha) + np.diag(eng.last_beta[:4], 1) + np.diag(eng.last_beta[:4], -1)
        ext = np.linalg.eigvalsh(T)[-1 if find_max else 0]
        assert abs(val - ext) <= 1e-14 * abs(ext)
        # the Ritz vector of a 5-dimensional Krylov space: its Rayleigh quotient is the Ritz value
        assert abs(np.vdot(vec, A @ vec) - val) <= 1e-12 * norm and abs(np.linalg.norm(vec) - 1) <= 4 * E.EPS_D
        assert info["stats"]["replay_mismatches"] == 0
    op.close()


def test_more_than_one_eigenpair_is_refused(ctx):
    n = 50
    op = L.CsrOperator(ctx, *_diag_csr(np.arange(1.0, n + 1.0)))
    eng = L.LambdaLanczos(op, n, False, 2)
    p = eng._params(2)
    val, itern, stats = C.c_double(), C.c_int64(), capi.RunStats()
    rc = capi.lib().ll_lanczos_two_pass_d(ctx.handle, op.handle, C.byref(p), C.byref(val), None, C.byref(itern), None, None, None,
                                          C.byref(stats))
    assert rc == capi.LL_ERR_INVALID and b"num_eigs" in capi.lib().ll_last_error()
    p.num_eigs = 1
    rc = capi.lib().ll_lanczos_two_pass_d(ctx.handle, op.handle, C.byref(p), C.byref(val), None, C.byref(itern), None, None, None,
                                          C.byref(stats))
    assert rc == capi.LL_OK and abs(val.value - 1.0) <= 1e-10 and stats.workspace_vectors == 3
    op.close()


@pytest.mark.parametrize("tid", list(TYPES))
def test_one_by_one_matrix(ctx, tid):
    dtype = TYPES[tid]
    op = L.CsrOperator(ctx, np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32), np.array([3.0], dtype=dtype))
    val, vec, info = _engine(op, 1, False, np.array([-0.5], dtype=dtype)).run_two_pass()
    assert info["iterations"] == 1 and val == 3.0 and vec.shape == (1,) and abs(abs(vec[0]) - 1.0) <= 4 * _eps(dtype)
    op.close()


# ------------------------------------------------------------------ 5. sharded contexts are refused
def test_refused_on_a_sharded_context(tmp_path):
    """Two ranks on the box's GPU over the host-staged test transport, each with its shard of a Laplacian."""
    from conftest import SHM_TRANSPORT

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name = "/ll_shm_tp_" + uuid.uuid4().hex[:12]
    env = dict(os.environ, LL_COMM_PLUGIN=SHM_TRANSPORT, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen(["timeout", "-k", "10", "120", sys.executable, os.path.join(root, "tests", "shm_two_pass_refused_worker.py"),
                               str(r), "2", name, str(tmp_path)], env=env, cwd=root, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-4000:]
    for r in range(2):
        res = json.load(open(os.path.join(tmp_path, "rank%d.json" % r)))
        assert res["code"] == capi.LL_ERR_INVALID and "sharded" in res["msg"], res
