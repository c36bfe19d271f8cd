"""The Exponentiator without a stored Krylov basis (ll_expo_two_pass, csrc/expo_two_pass_multi_run.cpp, csrc/recur.hip): the replayed step
with a complex coefficient against exact arithmetic, the solver against the oracle's plain recurrence (EX:87-173 with
full_orthogonalize = false) and against this library's stored-basis run, the buffer conventions and the constant work-space, the
edges, and the refusals."""
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import cases
import contract_cases as K
import exact_ref as E
import lambda_lanczos_amd as L
from guarded import guarded as _guarded, unguard as _unguard
from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G
from util import csr_matvec, overlap

pytestmark = pytest.mark.gpu

TYPES = {"d": np.float64, "z": np.complex128, "s": np.float32, "c": np.complex64}
EPS = np.finfo(np.float64).eps


def _single(dtype):
    return np.dtype(dtype) in (np.float32, np.complex64)


def _eps(dtype):
    return E.EPS_F if _single(dtype) else E.EPS_D


def _bits(v):
    return np.ascontiguousarray(v).view(np.uint8)


# ------------------------------------------------------------------ 1. the replayed step with a complex g against exact arithmetic
@pytest.mark.parametrize("with_p", [True, False], ids=["p", "nop"])
@pytest.mark.parametrize("tid", ["z", "c"])
def test_recur_accum_with_a_complex_coefficient_against_exact_arithmetic(ctx, tid, with_p):
    """y' = y - a x - b p and psi' = psi + g y' in one sweep, g complex.  With S = |y| + |a||x| + |b||p| (element-wise moduli, as in
    test_gpu_two_pass.test_recur_accum_against_exact_arithmetic) and first-order chains of individually rounded operations in T,
    each scaled by 1.01 for second order:
      |y' - y'_exact|     <= 3 eps_T S
      |psi' - psi'_exact| <= eps_T (|psi| + 8 |g| S)    8 = 3 inherited from y' + 2 sqrt(2) for a complex product of individually
                                                        rounded operations + 1 for rounding g to T + 1 for the final sum
    x, p and everything outside [0, n) stay as they were."""
    dtype = TYPES[tid]
    ept = 64 // np.dtype(dtype).itemsize
    elems = 256 * ept
    wide = np.clongdouble
    a, b, g = -1.7, 0.3, 0.625 - 0.4j
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
            bq = eps * (np.abs(psi).astype(np.float64) + 8 * abs(g) * S) * 1.01
            ey, eq = np.abs(gy - y_exact).astype(np.float64), np.abs(gq - q_exact).astype(np.float64)
            worst = [max(worst[0], float(np.max(ey / by))), max(worst[1], float(np.max(eq / bq)))]
            assert np.all(ey <= by), (n, shift, float(np.max(ey / by)))
            assert np.all(eq <= bq), (n, shift, float(np.max(eq / bq)))
            for buf in (yb, xb, pb, qb):
                buf.free()
    print("recur_accum, complex g,", tid, "p" if with_p else "no p", "largest error / bound (y, psi):", worst)


@pytest.mark.parametrize("tid", list(TYPES))
def test_a_real_coefficient_still_takes_the_typed_entry_point(ctx, tid):
    """recur_accum(g real) through the Python function and ll_recur_accum_<type> called directly: the same bits in y and psi."""
    dtype = TYPES[tid]
    n = 2049
    a, b, g = -1.7, 0.3, 0.625
    y, x, p, psi = (K.start_x(n, dtype, s) for s in (41, 42, 43, 44))
    got = []
    for direct in (False, True):
        yd, xd, pd, qd = (ctx.to_device(v) for v in (y, x, p, psi))
        if direct:
            capi.check(getattr(capi.lib(), "ll_recur_accum_" + tid)(ctx.handle, n, yd.ptr, xd.ptr, pd.ptr, a, b, g, qd.ptr))
        else:
            L.recur_accum(ctx, yd, xd, pd, a, b, np.float64(g), qd, n)
        got.append((yd.get(), qd.get()))
        for v in (yd, xd, pd, qd):
            v.free()
    assert np.array_equal(_bits(got[0][0]), _bits(got[1][0])) and np.array_equal(_bits(got[0][1]), _bits(got[1][1]))
    assert not np.array_equal(got[0][1], psi)


# ------------------------------------------------------------------ 2. the solver against the oracle's plain recurrence
TFIM = (10, G.tfim_terms(10, 1.0, 1.5, periodic=True))
SECTOR = (12, 6, G.heisenberg_terms(12))


def _laplace_host_operator(ctx, dtype):
    csr = G.laplace2d(40)

    def mv_mul(vin, vout):
        vout[:] = csr_matvec(csr, vin)

    return L.HostOperator(ctx, mv_mul, 1600, dtype)


def _problem(name):
    """name -> (csr in the oracle's type, make_operator(ctx, dtype), input in double / complex double, device operator?)"""
    if name in cases.expo_cases():
        c = cases.expo_cases()[name]
        return c["csr"], (lambda ctx, dtype: L.CsrOperator(ctx, c["csr"][0], c["csr"][1], c["csr"][2].astype(dtype))), c["input"], True
    if name == "tfim":
        csr = G.pauli_csr(TFIM[0], TFIM[1], np.complex128)
        return csr, (lambda ctx, dtype: L.PauliOperator(ctx, TFIM[0], TFIM[1], dtype)), G.start_vector(1024, 1, np.complex128), True
    if name == "sector":
        rp, ci, va = G.pauli_sector_csr(*SECTOR)
        n = rp.shape[0] - 1
        return (rp, ci, va.astype(np.complex128)), (lambda ctx, dtype: L.PauliSectorOperator(ctx, SECTOR[0], SECTOR[1], SECTOR[2], dtype)), \
            G.start_vector(n, 1, np.complex128), True
    rp, ci, va = G.laplace2d(40)
    if name == "laplace_real":
        return (rp, ci, va), (lambda ctx, dtype: L.CsrOperator(ctx, rp, ci, va.astype(dtype))), G.start_vector(1600, 1), True
    csr = (rp, ci, va.astype(np.complex128))
    if name == "laplace_host":
        return csr, _laplace_host_operator, G.start_vector(1600, 1, np.complex128), False
    return csr, (lambda ctx, dtype: L.CsrOperator(ctx, rp, ci, va.astype(dtype))), G.start_vector(1600, 1, np.complex128), True


# (problem, storage type, a or None = the case's, max_iteration or None)
SOLVER_CASES = [(name, "d" if name == "exponentiate_real" else "z", None, None) for name in sorted(cases.expo_cases())] + [
    ("tfim", "z", -0.5j, None), ("tfim", "c", -0.5j, None), ("sector", "z", -0.2j, None), ("laplace", "z", -1j, None),
    ("laplace_host", "z", -1j, None), ("laplace_real", "d", -0.5, 40), ("laplace_real", "s", -0.5, 40)]


def _solver_id(c):
    return "%s-%s" % (c[0], c[1])


@pytest.mark.parametrize("case", SOLVER_CASES, ids=_solver_id)
def test_two_pass_against_the_oracle_and_the_stored_basis_run(ctx, oracle, case):
    """oracle.expo(csr, a, input, eps = the run's) is EX:87-173 with full_orthogonalize = false: the same recurrence, normalised.
    Rules of the stored-basis tests (tests/test_gpu_engines.py, tests/test_gpu_pauli.py):
      double  |iterations - oracle's| <= 1; max|out - o_out| <= 1e-10 ||o_out||; for imaginary a: | ||out|| / ||in|| - 1 | <= 1e-12
              and 1 - overlap <= 10 eps; against Exponentiator.run on the same operator: max|delta| <= 1e-10 ||in||
      float   iterations within 2; ||out - o_out|| <= 1e-3 ||o_out||
    With real a the reference's overlap test never fires (exp(a T) e_1 is no unit vector): those runs end at max_iteration, or on
    breakdown (the 3 x 3 case)."""
    name, tid, a, max_it = case
    dtype = TYPES[tid]
    csr, make_op, inp, device_op = _problem(name)
    a = cases.expo_cases()[name]["a"] if a is None else a
    n = csr[0].shape[0] - 1
    inp_t = inp.astype(dtype)
    op = make_op(ctx, dtype)
    try:
        ex = L.Exponentiator(op, n)
        ex.full_orthogonalize = False
        if max_it is not None:
            ex.max_iteration = max_it
        out, it = ex.run_two_pass(a, inp_t)
        stats = ex.last_stats
        ref_out, ref_it = ex.run(a, inp_t)
    finally:
        op.close()
    o_in = inp_t.astype(csr[2].dtype)
    o_out, o_it, _ = oracle.expo(csr, a, o_in, max_iteration=max_it, eps=ex.eps)
    in_norm, o_norm = float(np.linalg.norm(o_in)), float(np.linalg.norm(o_out))
    err_max = float(np.max(np.abs(out - o_out)))
    err_2 = float(np.linalg.norm(out - o_out))
    err_run = float(np.max(np.abs(out.astype(o_out.dtype) - ref_out.astype(o_out.dtype))))
    norm_err = abs(float(np.linalg.norm(out.astype(o_out.dtype))) / in_norm - 1)
    miss = 1 - overlap(out.astype(o_out.dtype), o_out)
    print("expo two-pass %s a = %s: m = %d (oracle %d, stored basis %d), max|out - oracle| / |oracle| %.3e, |out - oracle|_2 / |oracle| "
          "%.3e, max|out - run()| / |in| %.3e, | |out| / |in| - 1 | %.3e, 1 - overlap %.3e, replay mismatches %d, vectors %d"
          % (_solver_id(case), a, it, o_it, ref_it, err_max / o_norm, err_2 / o_norm, err_run / in_norm, norm_err, miss,
             stats["replay_mismatches"], stats["workspace_vectors"]))
    assert out.dtype == np.dtype(dtype) and out.shape == (n,)
    assert stats["total_iterations"] == it and stats["n_passes"] == 1 and stats["workspace_vectors"] == 4
    if device_op:
        assert stats["replay_mismatches"] == 0
    if _single(dtype):
        assert abs(it - o_it) <= 2
        assert err_2 <= 1e-3 * o_norm
    else:
        assert abs(it - o_it) <= 1
        assert err_max <= 1e-10 * o_norm
        assert err_run <= 1e-10 * in_norm
        if np.real(a) == 0 and np.imag(a) != 0:
            assert norm_err <= 1e-12
            assert miss <= 10 * ex.eps


# ------------------------------------------------------------------ 3. buffers and memory
def _tfim_run(ctx, inp, where):
    """One run on a fresh 10-site TFIM operator, a = -0.5i: where = 'host', 'device' (distinct output buffer) or 'inplace'.
    Returns (output as a host array, iterations, last_stats, input buffer read back)."""
    op = L.PauliOperator(ctx, TFIM[0], TFIM[1], np.complex128)
    ex = L.Exponentiator(op, 1024)
    try:
        if where == "host":
            out, it = ex.run_two_pass(-0.5j, inp)
            return out, it, ex.last_stats, inp
        d_in = ctx.to_device(inp)
        d_out = d_in if where == "inplace" else ctx.empty(1024, np.complex128)
        got, it = ex.run_two_pass(-0.5j, d_in, out=d_out)
        assert got is d_out
        res = d_out.get(), it, ex.last_stats, d_in.get()
        d_in.free()
        if d_out is not d_in:
            d_out.free()
        return res
    finally:
        op.close()


def test_workspace_is_three_or_four_vectors_and_device_buffers_change_no_bit(ctx, llenv):
    inp = G.start_vector(1024, 1, np.complex128)
    keep = inp.copy()
    host, it, stats, _ = _tfim_run(ctx, inp, "host")
    assert stats["workspace_vectors"] == 4 and stats["replay_mismatches"] == 0 and np.array_equal(inp, keep)
    dev, it_d, stats_d, in_after = _tfim_run(ctx, inp, "device")
    assert stats_d["workspace_vectors"] == 3 and it_d == it
    assert np.array_equal(_bits(in_after), _bits(keep))          # the input buffer is unchanged
    assert np.array_equal(_bits(dev), _bits(host))                # bit for bit the host-buffer run
    inplace, it_i, stats_i, _ = _tfim_run(ctx, inp, "inplace")
    assert stats_i["workspace_vectors"] == 3 and it_i == it and stats_i["replay_mismatches"] == 0
    assert np.array_equal(_bits(inplace), _bits(host))
    # the same bits on poisoned workspace (the hook of tests/test_gpu_poisoned_workspace.py): NaN in every type, then huge and finite
    for fill in (0xFF, 0x7F):
        llenv.setenv("LL_TEST_WORKSPACE_FILL", str(fill))
        for where in ("host", "device", "inplace"):
            got, it_p, stats_p, _ = _tfim_run(ctx, inp, where)
            assert it_p == it and stats_p["replay_mismatches"] == 0, (fill, where)
            assert np.array_equal(_bits(got), _bits(host)), (fill, where)
    llenv.delenv("LL_TEST_WORKSPACE_FILL")


# ------------------------------------------------------------------ 4. edges
def _diag_csr(d, dtype=np.float64):
    n = len(d)
    return np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), np.asarray(d, dtype=dtype)


def test_input_that_is_an_eigenvector_takes_one_iteration(ctx):
    """||in|| = 2, so u_0, alpha_0 = 8 and the update are exact and r_1 = 0: breakdown after one iteration, no replay;
    out = exp(a lambda) in.  a lambda = -2i is exact too, so what remains is the exponential (within 2 units of roundoff) and the
    product g_0 r_0 (2 sqrt(2) units) — below 4 eps, element-wise relative."""
    n = 50
    op = L.CsrOperator(ctx, *_diag_csr(np.arange(1.0, n + 1.0), np.complex128))
    inp = np.zeros(n, dtype=np.complex128)
    inp[7] = -2j
    ex = L.Exponentiator(op, n)
    out, it = ex.run_two_pass(-0.25j, inp)
    op.close()
    exact = complex(np.exp(np.clongdouble(-2j)) * np.clongdouble(inp[7]))
    print("eigenvector input: iterations %d, relative error %.3e" % (it, abs(out[7] - exact) / abs(exact)))
    assert it == 1 and ex.last_stats["replay_mismatches"] == 0
    assert abs(out[7] - exact) <= 4 * EPS * abs(exact)
    assert np.all(np.delete(out, 7) == 0)


def test_max_iteration_gives_the_sum_over_that_krylov_space(ctx):
    """max_iteration = 5: out = ||in|| sum_l coeff_l u_l with coeff = exp(a T_5) e_1, rebuilt here from a plain normalised
    recurrence of five steps in numpy; agreement to 1e-12 ||in||."""
    csr = G.laplace2d(40)
    n, a = 1600, -1j
    inp = G.start_vector(n, 1, np.complex128)
    op = L.CsrOperator(ctx, csr[0], csr[1], csr[2].astype(np.complex128))
    ex = L.Exponentiator(op, n)
    ex.max_iteration = 5
    out, it = ex.run_two_pass(a, inp)
    op.close()
    u = [inp / np.linalg.norm(inp)]
    alpha, beta = [], []
    for k in range(5):
        w = csr_matvec(csr, u[k])
        alpha.append(float(np.real(np.vdot(u[k], w))))
        w = w - alpha[k] * u[k] - (beta[k - 1] * u[k - 1] if k > 0 else 0)
        beta.append(float(np.linalg.norm(w)))
        u.append(w / beta[k])
    T = np.diag(alpha) + np.diag(beta[:4], 1) + np.diag(beta[:4], -1)
    ev, q = np.linalg.eigh(T)
    coeff = q @ (np.exp(a * ev) * q[0])
    expect = np.linalg.norm(inp) * sum(coeff[l] * u[l] for l in range(5))
    err = float(np.max(np.abs(out - expect)))
    print("max_iteration = 5: max|out - sum| / |in| %.3e" % (err / np.linalg.norm(inp)))
    assert it == 5 and ex.last_stats["total_iterations"] == 5 and ex.last_stats["replay_mismatches"] == 0
    assert err <= 1e-12 * np.linalg.norm(inp)


@pytest.mark.parametrize("tid", list(TYPES))
def test_one_by_one_matrix(ctx, tid):
    """One iteration, out = exp(3 a) in: the exponential is formed in double; g_0 rounded to T and one product in T stay below
    4 eps_T."""
    dtype = TYPES[tid]
    cplx = np.dtype(dtype).kind == "c"
    a = -0.5j if cplx else -0.5
    v = (-0.5 + 0.25j) if cplx else -0.5
    op = L.CsrOperator(ctx, np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32), np.array([3.0], dtype=dtype))
    out, it = L.Exponentiator(op, 1).run_two_pass(a, np.array([v], dtype=dtype))
    op.close()
    exact = np.exp(3 * a) * v
    assert it == 1 and out.shape == (1,) and out.dtype == np.dtype(dtype)
    assert abs(out[0] - exact) <= 4 * _eps(dtype) * abs(exact)


def test_a_zero_returns_the_input(ctx):
    """a = 0: coeff = exp(0 T_m) e_1 = Q Q^T e_1, the first column of the identity up to the orthonormality of the tridiagonal
    eigenvectors; the second iteration's overlap is 1 and the run stops with m = 2.  out_i - in_i = (coeff_0 - 1) in_i +
    ||in|| coeff_1 u_1i, so |out - in| <= (|coeff_0 - 1| + |coeff_1|) ||in|| element-wise: 4 eps ||in|| allows two units of
    roundoff in each."""
    inp = G.start_vector(1024, 1, np.complex128)
    op = L.PauliOperator(ctx, TFIM[0], TFIM[1], np.complex128)
    out, it = L.Exponentiator(op, 1024).run_two_pass(0j, inp)
    op.close()
    err = float(np.max(np.abs(out - inp)))
    print("a = 0: iterations %d, max|out - in| / |in| %.3e" % (it, err / np.linalg.norm(inp)))
    assert err <= 4 * EPS * np.linalg.norm(inp)


def test_refusals(ctx):
    inp = G.start_vector(1024, 1, np.complex128)
    op = L.PauliOperator(ctx, TFIM[0], TFIM[1], np.complex128)
    ex = L.Exponentiator(op, 1024)
    ex.full_orthogonalize = True
    with pytest.raises(capi.LanczosHipError) as e:
        ex.run_two_pass(-0.5j, inp)
    assert e.value.code == capi.LL_ERR_INVALID and "full_orthogonalize" in str(e.value)
    assert b"full_orthogonalize" in capi.lib().ll_last_error()
    op.close()
    rp, ci, va = G.laplace2d(40)
    rop = L.CsrOperator(ctx, rp, ci, va)
    with pytest.raises(capi.LanczosHipError) as e:
        L.Exponentiator(rop, 1600).run_two_pass(-0.5j, G.start_vector(1600, 1))
    assert e.value.code == capi.LL_ERR_INVALID and "a_im" in str(e.value)
    rop.close()


def test_refused_on_a_sharded_context(tmp_path):
    """Two ranks on the box's GPU over the host-staged test transport, each with its shard of a Laplacian."""
    from conftest import SHM_TRANSPORT

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name = "/ll_shm_etp_" + uuid.uuid4().hex[:12]
    env = dict(os.environ, LL_COMM_PLUGIN=SHM_TRANSPORT, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen(["timeout", "-k", "10", "120", sys.executable,
                               os.path.join(root, "tests", "shm_expo_two_pass_refused_worker.py"), str(r), "2", name, str(tmp_path)],
                              env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-4000:]
    for r in range(2):
        res = json.load(open(os.path.join(tmp_path, "rank%d.json" % r)))
        assert res["code"] == capi.LL_ERR_INVALID and "sharded" in res["msg"], res
