"""Host reference for whole solver runs in every storage type (numpy / scipy only; tests/test_float_run_model_host.py and
tests/test_gpu_float_runs.py share it).

Traces of a float run cannot be compared with anything: two correct Lanczos processes drift apart.  Invariants can.  This
module holds

  * models of the loops with the storage roundings of the kernels (dev_helpers.hpp): vectors live in the storage type
    (float32 / complex64 / float64 / complex128), every scalar and every sum over elements is a double, and a vector is
    rounded to storage where the kernels round it: y of the operator (narrow<T>), the offset term and the three-term
    update in storage arithmetic (rmul / sub), w after every subtracted basis vector (fnma_acc), the normalisation
    (rmul with the factor rounded to storage), the Ritz / output GEMV (coefficients rounded to storage, one rounding of the
    double sum, lanczos_run.cpp / expo_run.cpp);
  * invariants of what a device run RETURNS (vals, vecs, last_alpha, last_beta; an Exponentiator's output) — no basis —
    in units of the storage epsilon: eps, and u_A = eps (||A||_inf + |offset|) of the matrix as rounded to storage;
  * exact eigenvalues of the test matrices (analytic, eigsh in double, dense eigh), cached per process;
  * BOUNDS: per storage type, max(floor, 4 x the models' worst ratio over the cases), with the ratios beside them.  The host test recomputes the
    ratios and fails when the table is stale; nothing in it comes from a device run.
"""
import functools
import os
import sys

import numpy as np
import scipy.linalg as sl
import scipy.sparse as sp
import scipy.sparse.linalg as spl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:        # (run as a script to print the table)
    sys.path.insert(0, ROOT)
from lambda_lanczos_amd import generators as G  # noqa: E402

WIDE = {np.dtype(np.float32): np.float64, np.dtype(np.complex64): np.complex128,
        np.dtype(np.float64): np.float64, np.dtype(np.complex128): np.complex128}
REAL = {np.dtype(np.float32): np.float32, np.dtype(np.complex64): np.float32,
        np.dtype(np.float64): np.float64, np.dtype(np.complex128): np.float64}
TYPES = {"s": np.float32, "c": np.complex64, "d": np.float64, "z": np.complex128}


def eps_of(storage):
    return float(np.finfo(np.dtype(storage)).eps)


def abs1(v):
    """|re| + |im| (exact_ref.abs1)."""
    v = np.asarray(v)
    return np.abs(v.real) + np.abs(v.imag) if np.iscomplexobj(v) else np.abs(v).astype(np.float64)


# ------------------------------------------------------------------ the operator as the kernels apply it
class Operator:
    """A + offset with A's values rounded to storage first: y = narrow(A x) + offset x, the sum over a row in double, the
    offset term and the addition in storage arithmetic (spmv_shared.hpp)."""

    def __init__(self, csr, storage, offset=0.0):
        self.storage = np.dtype(storage)
        self.wide, self.real = WIDE[self.storage], REAL[self.storage]
        rp, ci, va = csr
        self.n = rp.shape[0] - 1
        va = np.ascontiguousarray(va).astype(self.storage)
        self.csr = (rp, ci, va)                      # what the device operator is created from
        self.A = sp.csr_matrix((va.astype(self.wide), ci, rp), shape=(self.n, self.n))
        self.offset = float(offset)
        self.norm = float(np.max(np.add.reduceat(abs1(va), rp[:-1]))) + abs(self.offset)
        self.eps = eps_of(self.storage)
        self.u_A = self.eps * self.norm

    def apply(self, x):
        y = (self.A @ x.astype(self.wide)).astype(self.storage)
        if self.offset != 0.0:
            y = y + self.real(self.offset) * x
        return y

    def shifted(self):
        """A + offset in double (for residuals of returned vectors)."""
        return self.A + self.offset * sp.identity(self.n, dtype=self.wide, format="csr") if self.offset else self.A


def _unit(v, op):
    """v / ||v||: the norm in double, the factor rounded to storage, one storage multiplication (launch_scale)."""
    w = v.astype(op.wide)
    return (op.real(1.0 / np.sqrt(np.vdot(w, w).real)) * v).astype(op.storage)


class _Sub:
    """fnma_acc on whole vectors: w -= h u in double, w rounded to storage once (in place, buffers reused)."""

    def __init__(self, op):
        self.t = np.empty(op.n, dtype=op.wide)
        self.s = None if op.storage == np.dtype(op.wide) else np.empty(op.n, dtype=op.storage)

    def __call__(self, w, h, u):
        np.multiply(u, h, out=self.t)
        np.subtract(w, self.t, out=w)
        if self.s is not None:
            np.copyto(self.s, w, casting="unsafe")
            np.copyto(w, self.s)
        return w


# ------------------------------------------------------------------ Lanczos with full re-orthogonalisation
def lanczos_model(op, v0, m, passes=2, locked=(), last_two_from=None):
    """m iterations with sequential Gram-Schmidt against the locked and all stored vectors, `passes` times.  Returns
    dict(alpha, beta, U): U[0..m] in storage.  last_two_from = k0 is a MUTANT: from iteration k0 on only the last two stored
    vectors are re-orthogonalised against."""
    S, W = op.storage, op.wide
    n = op.n
    Uw = np.zeros((m + 1, n), dtype=W)                # the stored vectors widened (exact copies)
    Lw = [z.astype(W) for z in locked]
    sub = _Sub(op)
    u0 = v0.astype(S)
    if Lw:                                            # LL:233: the start vector leaves the locked space first
        w = u0.astype(W)
        for z in Lw:
            sub(w, np.vdot(z, w), z)
        u0 = w.astype(S)
    U = np.zeros((m + 1, n), dtype=S)
    U[0] = _unit(u0, op)
    Uw[0] = U[0]
    al, be = [], []
    for k in range(1, m + 1):
        x = U[k - 1]
        y = op.apply(x)
        a = float(np.vdot(Uw[k - 1], y.astype(W)).real)
        w = y
        if k > 1:
            w = w - op.real(be[-1]) * U[k - 2]
        w = (w - op.real(a) * x).astype(W)
        first = 0 if last_two_from is None or k < last_two_from else max(0, k - 2)
        for _ in range(passes):
            for z in Lw:
                sub(w, np.vdot(z, w), z)
            for j in range(first, k):
                sub(w, np.vdot(Uw[j], w), Uw[j])
        b = float(np.sqrt(np.vdot(w, w).real))
        al.append(a)
        be.append(b)
        U[k] = op.real(1.0 / b) * w.astype(S)
        Uw[k] = U[k]
    return dict(alpha=np.array(al), beta=np.array(be), U=U)


# ------------------------------------------------------------------ the one-sweep (lagged, compensated) scheme
def lagged_model(op, v0, m, compensate=True, second_order=True, inject=0.0, inject_at=20):
    """tools/lagged_gs_model.py with the storage roundings of lagged_kernel / lagged_fold_kernel: the raw vector r and the
    completed vectors are stored, x = s r and the three-term update are storage arithmetic, the late update of u_{k-1} and
    the compensation of w round after every subtracted vector.  compensate / second_order / inject as in the tool (MUTANTS
    and the probe of tests/test_lagged_model.py).  Returns dict(alpha, beta, U, raw_last, maxc): raw_last[k] is s r of the
    vector that U[k] is the late-updated form of (k = m only)."""
    S, W, R = op.storage, op.wide, op.real
    n = op.n
    U = np.zeros((m + 1, n), dtype=S)
    Uw = np.zeros((m + 1, n), dtype=W)
    U[0] = _unit(v0.astype(S), op)
    Uw[0] = U[0]
    al, be, maxc = [], [], []
    r = g = t = s = None
    q = 0.0

    sub = _Sub(op)

    def late_update(r, g, s, upto):
        w = r.astype(W)
        for j in range(upto):
            sub(w, g[j], Uw[j])
        return (R(s) * w.astype(S)).astype(S)

    for k in range(1, m + 1):
        if k == inject_at and inject:                 # leave the lagged form once, to plant a known perturbation
            U[k - 1] = late_update(r, g, s, k - 1)
            Uw[k - 1] = U[k - 1]
            r = None
        if r is None:                                  # clean iteration: operator on a complete u_{k-1}
            x = U[k - 1]
            y = op.apply(x)
            a = float(np.vdot(x.astype(W), y.astype(W)).real)
            w = y
            if k > 1:
                w = w - R(be[-1]) * U[k - 2]
            w = (w - R(a) * x).astype(W)
            if k == inject_at and inject:
                w = (w + inject * np.linalg.norm(w) * (Uw[3] - Uw[7])).astype(S).astype(W)
            gn = Uw[:k].conj() @ w
        else:                                          # lagged sweep
            x = (R(s) * r).astype(S)
            y = op.apply(x)
            a = float(np.vdot(x.astype(W), y.astype(W)).real)
            if compensate:
                a -= 2 * float(np.real(g[-1])) + (q if second_order else 0.0)
            wr = y
            if k > 1:
                wr = wr - R(be[-1]) * U[k - 2]
            wr = (wr - R(a) * x).astype(W)
            U[k - 1] = late_update(r, g, s, k - 1)     # the late update
            Uw[k - 1] = U[k - 1]
            mm = Uw[:k - 1].conj() @ wr
            if compensate:
                d = t.copy()
                d[:k - 1] -= a * s * g
                w = wr
                for j in range(k):
                    sub(w, d[j], Uw[j])
                gn = np.concatenate([mm - d[:k - 1], [np.vdot(Uw[k - 1], w)]])
            else:
                w = wr
                gn = np.concatenate([mm, [np.vdot(Uw[k - 1], w)]])
        c1 = float(np.vdot(w, w).real - np.vdot(gn, gn).real)
        if not c1 > 0:
            return dict(alpha=np.array(al), beta=np.array(be), U=None, raw_last=None, maxc=np.array(maxc), failed_at=k)
        b = np.sqrt(c1)
        al.append(a)
        be.append(b)
        c = gn / b
        maxc.append(np.abs(c).max())
        alh, beh = np.array(al), np.array(be)
        tt = np.zeros(k + 1, dtype=gn.dtype)
        tt[:k] += alh * c
        tt[1:k + 1] += beh * c
        tt[:k - 1] += beh[:k - 1] * c[1:]
        q = float(np.real(np.vdot(c, tt[:k])))
        r, g, t, s = w.astype(S), gn, tt, 1.0 / b
    raw_last = (R(s) * r).astype(S)
    U[m] = late_update(r, g, s, m)
    return dict(alpha=np.array(al), beta=np.array(be), U=U, raw_last=raw_last, maxc=np.array(maxc))


# ------------------------------------------------------------------ what a run returns, from a model's basis
def tridiagonal(alpha, beta, m=None):
    m = len(alpha) if m is None else m
    return np.asarray(alpha[:m], dtype=np.float64), np.asarray(beta[:m - 1], dtype=np.float64)


def extreme_pair(alpha, beta, find_maximum, m=None):
    """(theta_1, s) of T_m in double; s has unit norm."""
    d, e = tridiagonal(alpha, beta, m)
    w, q = sl.eigh_tridiagonal(d, e) if len(d) > 1 else (d.copy(), np.ones((1, 1)))
    i = len(d) - 1 if find_maximum else 0
    return float(w[i]), q[:, i]


def ritz_values(alpha, beta, find_maximum, count, m=None):
    """The `count` extreme eigenvalues of T_m, the extreme one first."""
    d, e = tridiagonal(alpha, beta, m)
    w = sl.eigh_tridiagonal(d, e, eigvals_only=True) if len(d) > 1 else d.copy()
    w = w[::-1] if find_maximum else w
    return w[:count]


def model_returns(op, run, find_maximum, m=None, last_vector=None):
    """What the device returns for a window of m iterations of a model run: dict(vals, vecs, last_alpha, last_beta).  The
    Ritz vector is the GEMV of lanczos_run.cpp: coefficients rounded to storage, the sum in double rounded once, normalised.
    last_vector (MUTANT) replaces U[m-1] in the sum."""
    m = len(run["alpha"]) if m is None else m
    theta, s = extreme_pair(run["alpha"], run["beta"], find_maximum, m)
    Uw = run["U"][:m].astype(op.wide)
    if last_vector is not None:
        Uw[m - 1] = last_vector
    coeff = s.astype(op.real).astype(np.float64)
    v = _unit((coeff @ Uw).astype(op.storage), op)
    return dict(vals=np.array([theta - op.offset]), vecs=v[None, :], last_alpha=run["alpha"][:m].copy(),
                last_beta=run["beta"][:m].copy())


def convergence_iteration(op, run, find_maximum):
    """The first m at which beta_m |s_m| <= 1e3 u_A (None if the run never gets there)."""
    for m in range(2, len(run["alpha"]) + 1):
        _, s = extreme_pair(run["alpha"], run["beta"], find_maximum, m)
        if run["beta"][m - 1] * abs(s[-1]) <= 1e3 * op.u_A:
            return m
    return None


# ------------------------------------------------------------------ invariants of a returned run
def residual_norm(op, theta_shifted, v):
    vw = np.asarray(v).astype(op.wide)
    return float(np.linalg.norm(op.A @ vw + (op.offset - theta_shifted) * vw))


def relation(op, ret, find_maximum):
    """(| ||A v - theta v|| - beta_m |s_m| | - double_error) / u_A with (theta, s) of the returned T (single-pass runs)."""
    theta, s = extreme_pair(ret["last_alpha"], ret["last_beta"], find_maximum)
    return max(0.0, abs(residual_norm(op, theta, ret["vecs"][0]) - ret["last_beta"][-1] * abs(s[-1])) - double_error(op)) / op.u_A


def ritz(op, ret, find_maximum):
    theta, _ = extreme_pair(ret["last_alpha"], ret["last_beta"], find_maximum)
    return max(0.0, abs(ret["vals"][0] + op.offset - theta) - double_error(op)) / op.u_A


def interlace(op, ret, find_maximum, exact):
    """max_k (theta_k - lambda_k) / u_A over the extreme exact eigenvalues `exact` (of A, the extreme one first); the sign
    flips for the lower end.  eigsh_error(op), the reference's own error, is taken off first (it only shows in double)."""
    k = min(len(exact), len(ret["last_alpha"]))
    th = ritz_values(ret["last_alpha"], ret["last_beta"], find_maximum, k)
    lam = np.asarray(exact[:k]) + op.offset
    d = th - lam if find_maximum else lam - th
    return (float(np.max(d)) - eigsh_error(op)) / op.u_A


def unit(op, v):
    return abs(float(np.linalg.norm(np.asarray(v).astype(op.wide))) - 1.0) / op.eps


def hermitian(op, val, v, exact):
    """(min_j |theta - lambda_j| - ||A v - theta v||) / u_A over the exact eigenvalues `exact`: at most O(1), an eigenvalue
    lies within the residual of any Rayleigh pair.  `exact` must reach past theta from the end of the spectrum (asserted)
    or hold the whole spectrum, so that the nearest eigenvalue is among them."""
    exact = np.asarray(exact)
    inside = val >= exact.min() if exact[0] >= exact[-1] else val <= exact.max()
    assert len(exact) == op.n or inside, "theta = %r is not inside the range the exact eigenvalues cover" % val
    return (float(np.min(np.abs(val - exact))) - eigsh_error(op) - residual_norm(op, val + op.offset, v)) / op.u_A


def cross(op, vi, vj, m):
    """|<v_i, v_j>| / (cross_bound(m) eps) for two returned vectors of passes of (at most) m iterations."""
    return abs(np.vdot(np.asarray(vi).astype(op.wide), np.asarray(vj).astype(op.wide))) / (cross_bound(m) * op.eps)


def run_invariants(op, ret, find_maximum, exact, with_relation=True):
    """The invariants of case A as a dict of ratios."""
    out = dict(ritz=ritz(op, ret, find_maximum), interlace=interlace(op, ret, find_maximum, exact),
               unit=unit(op, ret["vecs"][0]), hermitian=hermitian(op, ret["vals"][0], ret["vecs"][0], exact))
    if with_relation:
        out["relation"] = relation(op, ret, find_maximum)
    return out


# ------------------------------------------------------------------ the Exponentiator
def expo_coefficients(alpha, beta, a, m):
    d, e = tridiagonal(alpha, beta, m)
    w, q = sl.eigh_tridiagonal(d, e) if m > 1 else (d.copy(), np.ones((1, 1)))
    return (q * np.exp(a * w)) @ q[0].conj()


def expo_model(op, a, v, m, full, coeff_of=None, lagged=False):
    """exp(a A) v by m iterations of the same recurrence (full: with the re-orthogonalisation, else the bare three-term
    recurrence): coefficients ||v|| exp(a T_m) e_1 in double, rounded to storage, the sum in double rounded once
    (expo_run.cpp).  coeff_of = m - 1 is a MUTANT: the coefficients of T_{m-1} (a zero behind them) on m vectors."""
    if lagged:
        run = lagged_model(op, v, m)
    else:
        run = lanczos_model(op, v, m, passes=2 if full else 0)
    vw = v.astype(op.storage).astype(op.wide)
    nrm = float(np.sqrt(np.vdot(vw, vw).real))
    k = m if coeff_of is None else coeff_of
    c = np.zeros(m, dtype=np.complex128)
    c[:k] = expo_coefficients(run["alpha"], run["beta"], a, k)
    c = nrm * c
    if op.wide == np.float64:
        c = c.real
    c = c.astype(op.storage).astype(op.wide)
    return (c @ run["U"][:m].astype(op.wide)).astype(op.storage)


def taylor_model(op, a, v, eps):
    """Exponentiator::taylor_run (EX:175-210): powers A^k v stored, terms until ||A^k v|| |a^k / k!| < eps, one GEMV with the
    factors rounded to storage.  Returns (output, terms)."""
    V = [v.astype(op.storage)]
    factor = 1.0 + 0j
    k = 0
    while True:
        k += 1
        factor *= a / k
        V.append(op.apply(V[-1]))
        if np.linalg.norm(V[-1].astype(op.wide)) * abs(factor) < eps:
            break
    c = np.zeros(len(V), dtype=np.complex128)
    for j in range(len(V) - 1, -1, -1):
        c[j] = factor
        factor *= j / a
    if op.wide == np.float64:
        c = c.real
    c = c.astype(op.storage).astype(op.wide)
    return (c @ np.array(V).astype(op.wide)).astype(op.storage), len(V)


@functools.lru_cache(maxsize=None)
def _dense_eigh(name, size, storage):
    op = Operator(matrix(name, size), storage)
    return sl.eigh(op.A.toarray())


def expo_exact(name, size, storage, a, v):
    """exp(a A) v by dense diagonalisation in double of the storage-rounded matrix (n <= 1700)."""
    w, q = _dense_eigh(name, size, np.dtype(storage).name)
    vw = v.astype(storage).astype(WIDE[np.dtype(storage)])
    out = (q * np.exp(a * w)) @ (q.conj().T @ vw)
    return out.real if WIDE[np.dtype(storage)] == np.float64 else out


# what `exact` of expo_exact and a run of EXPO_M iterations may be off by, relative to ||v||: the selection rule of m (the
# double model within 1e-12 of the dense exponential) and the dense eigh's own error (~1e-13 at n = 1700)
EXPO_ALLOWANCE = 1e-12


def expo_error(op, out, exact, v):
    """(||out - exp(aA) v|| - EXPO_ALLOWANCE ||v||) / (eps ||v||), not below 0."""
    vw = v.astype(op.storage).astype(op.wide)
    nv = float(np.linalg.norm(vw))
    return max(0.0, float(np.linalg.norm(np.asarray(out).astype(op.wide) - exact)) - EXPO_ALLOWANCE * nv) / (op.eps * nv)


def expo_norm(op, out, v):
    """| ||out|| / ||v|| - 1 | / eps (imaginary a)."""
    vw = v.astype(op.storage).astype(op.wide)
    return abs(float(np.linalg.norm(np.asarray(out).astype(op.wide))) / float(np.linalg.norm(vw)) - 1.0) / op.eps


def expo_iterations(name, size, a, v, full, limit=200):
    """The first m at which the model in DOUBLE storage is within 1e-12 ||v|| of the dense exponential."""
    storage = np.complex128 if np.iscomplexobj(v) or np.iscomplexobj(a) else np.float64
    op = Operator(matrix(name, size), storage)
    run = lanczos_model(op, v, limit, passes=2 if full else 0)
    exact = expo_exact(name, size, storage, a, v)
    vw = v.astype(op.wide)
    nrm = float(np.linalg.norm(vw))
    Uw = run["U"].astype(op.wide)
    for m in range(2, limit + 1):
        c = nrm * expo_coefficients(run["alpha"], run["beta"], a, m)
        if np.linalg.norm(c @ Uw[:m] - exact) <= 1e-12 * nrm:
            return m
    raise AssertionError("the Krylov exponential did not reach 1e-12 within %d iterations" % limit)


# ------------------------------------------------------------------ matrices, start vectors, exact eigenvalues
@functools.lru_cache(maxsize=None)
def matrix(name, size):
    return {"randsym": G.randsym_np, "laplace": G.laplace2d_np, "torus": G.torus_np}[name](size)


def dimension(name, size):
    return size if name == "randsym" else size * size


# name -> (find_maximum, offset, start-vector seed)
SETUP = {"randsym": (True, 0.0, 1), "laplace": (True, 0.0, 2), "torus": (False, -10.0, 3)}


def start(name, size, storage):
    wide = WIDE[np.dtype(storage)]
    return G.start_vector(dimension(name, size), SETUP[name][2], wide).astype(storage)


@functools.lru_cache(maxsize=None)
def exact_eigenvalues(name, size, storage_name):
    """Exact eigenvalues of A (no offset) as rounded to storage, the extreme one (SETUP's end) first: the whole analytic
    spectrum for the Laplacian (its entries are exact in every type), the K = 8 extreme ones by eigsh in double with tol 1e-12
    for the others (the torus' band edge is clustered: shift-and-invert from below the spectrum, which separates it; K = 16 on
    the 300 x 300 torus, whose Ritz value after 41 iterations still lies above the eighth eigenvalue)."""
    find_max = SETUP[name][0]
    if name == "laplace":
        c = 2.0 * np.cos(np.arange(1, size + 1) * np.pi / (size + 1))
        lam = np.sort((4.0 - c[:, None] - c[None, :]).reshape(-1))
        return lam[::-1] if find_max else lam
    op = Operator(matrix(name, size), np.dtype(storage_name))
    v0 = np.ones(op.n, dtype=op.wide)
    if name == "torus":
        # the shift a little below a rough lowest Ritz value (which lies above lambda_min): close enough to separate the cluster
        sigma = spl.eigsh(op.A, k=1, which="SA", tol=1e-3, v0=v0, return_eigenvectors=False)[0] - 0.05
        lam, x = spl.eigsh(op.A.tocsc(), k=16 if size >= 300 else 8, sigma=sigma, which="LM", tol=1e-12, v0=v0)
        assert sigma < lam.min()                      # below the spectrum: the nearest K are the lowest K
    else:
        lam, x = spl.eigsh(op.A, k=8, which="LA" if find_max else "SA", tol=1e-12, v0=v0, ncv=48)
    order = np.argsort(lam)
    lam, x = lam[order], x[:, order]
    # the reference's own error: residual^2 / gap (Kato-Temple) must vanish against the rounding of the Rayleigh quotient
    res = np.linalg.norm(op.A @ x - x * lam, axis=0)
    gap = np.min(np.diff(lam))
    assert np.max(res) ** 2 / gap <= EPS_D * op.norm, (res, gap)
    return lam[::-1] if find_max else lam


EPS_D = float(np.finfo(np.float64).eps)


def eigsh_error(op):
    """The reference's own error where exact eigenvalues enter (interlace, hermitian): the accuracy eigsh is asked for,
    tol = 1e-12 relative to ||A||.  1e-5 u_A in float; in double it limits those two checks to 1e-12 ||A||."""
    return 1e-12 * op.norm


def double_error(op):
    """What evaluating `relation` and `ritz` in double is itself off by: theta and s come from a second tridiagonal solver
    (LAPACK here, the library's own on the other side; each is backward stable, |d theta| <= a few eps_d ||T||), and
    every component of A v - theta v carries (nnz + 2) double roundings.  8 eps_d ||A||: 1.5e-8 u_A in float, 8 u_A in
    double — the models share LAPACK with the invariant, so without it their double ratio is 0 and the bound would sit
    below the disagreement of two correct solvers."""
    return 8 * EPS_D * op.norm


# ------------------------------------------------------------------ the case list and the table
# Case A (fixed windows, every form) and case C (default switches at the sizes where the forms switch on by themselves).
# (name, size, types)
CASES_A = [("randsym", 30011, "ds"), ("torus", 120, "zc"), ("laplace", 61, "ds"), ("laplace", 173, "ds")]
# The post-convergence window exists where the float model converges within the 130 iterations searched (a window of at most
# 325).  The 173 x 173 Laplacian does not, so it keeps the early window and a 61 x 61 Laplacian (3 721 rows: odd, no multiple
# of a strip, forced into the streaming forms like the others) runs both windows in its place.
CASES_LATE = CASES_A[:3]
CASES_C = [("randsym", 150001, "s"), ("laplace", 520, "s"), ("torus", 300, "c")]
# Case B (several eigenpairs behind locked vectors): (name, size, type)
CASES_B = [("randsym", 30011, "s"), ("torus", 120, "c")]
WINDOW_EARLY = 41
# Case D: (name, size, a, types)
CASES_D = [("laplace", 41, -0.3, "ds"), ("torus", 40, -0.5j, "zc"), ("torus", 40, -2.0j, "zc")]


def case_key(name, size):
    return "%s%d" % (name, size)


# ---- derived by tests/test_float_run_model_host.py from the models (never from a device run) ----
# the post-convergence window: 2.5 x the first m with beta_m |s_m| <= 1e3 u_A in the float-storage lanczos_model
WINDOW_LATE = {"randsym30011": 185, "torus120": 305, "laplace61": 258}     # (first m: 74, 122 and 103)
# the Exponentiator's m: the first m at which the double-storage model is within 1e-12 of the dense exponential
EXPO_M = {"laplace41:-0.3": 13, "torus40:(-0-0.5j)": 15, "torus40:(-0-2j)": 26}
# invariant: floor (derived in the host test's docstring; cross is in units of cross_bound(m) eps)
FLOORS = dict(relation=1.0, ritz=1.0, hermitian=1.0, interlace=1.0, unit=1.0, cross=1.0, expo_error=1.0, expo_norm=1.0,
              taylor_error=1.0)
# invariant: the models' worst ratio over the case list, per storage type (python tests/float_run_model.py prints them)
MODEL_RATIOS = {"cross": {"c": 0.000591, "s": 0.00397},
                "expo_error": {"c": 1.32, "d": 0.0, "s": 0.365, "z": 0.0},
                "expo_norm": {"c": 0.0599, "z": 2.0},
                "hermitian": {"c": 0.0, "d": 0.0, "s": 0.0, "z": 0.0},
                "interlace": {"c": 0.0737, "d": 0.0, "s": 0.011, "z": 0.0},
                "relation": {"c": 0.535, "d": 0.0, "s": 0.535, "z": 0.0},
                "ritz": {"c": 0.0, "d": 0.0, "s": 0.0, "z": 0.0},
                "taylor_error": {"c": 37.1, "d": 0.0, "s": 0.832, "z": 0.0},
                "unit": {"c": 0.209, "d": 1.0, "s": 0.168, "z": 1.0}}
# invariant: per storage type, max(floor, 4 x that type's worst model ratio)
BOUNDS = {"cross": {"c": 1.0, "s": 1.0},
          "expo_error": {"c": 5.3, "d": 1.0, "s": 1.46, "z": 1.0},
          "expo_norm": {"c": 1.0, "z": 8.0},
          "hermitian": {"c": 1.0, "d": 1.0, "s": 1.0, "z": 1.0},
          "interlace": {"c": 1.0, "d": 1.0, "s": 1.0, "z": 1.0},
          "relation": {"c": 2.14, "d": 1.0, "s": 2.14, "z": 1.0},
          "ritz": {"c": 1.0, "d": 1.0, "s": 1.0, "z": 1.0},
          "taylor_error": {"c": 149.0, "d": 1.0, "s": 3.33, "z": 1.0},
          "unit": {"c": 1.0, "d": 4.0, "s": 1.0, "z": 4.0}}


def cross_bound(m):
    """sqrt(m)/2 + 2 (in eps): each u_k is orthogonal to a locked vector to one storage rounding, v = sum s_k u_k, |s| = 1."""
    return np.sqrt(m) / 2 + 2


# ------------------------------------------------------------------ deriving the table (the host test runs this)
def case_setup(name, size, t):
    find_max, offset, _ = SETUP[name]
    op = Operator(matrix(name, size), TYPES[t], offset)
    return op, start(name, size, TYPES[t]), find_max


def late_window(name, size):
    """2.5 x the first m with beta_m |s_m| <= 1e3 u_A in the float-storage lanczos_model of the case (searched up to m = 130;
    None beyond that: the window would pass 325 iterations)."""
    op, v0, find_max = case_setup(name, size, "c" if name == "torus" else "s")
    conv = convergence_iteration(op, lanczos_model(op, v0, 130), find_max)
    return None if conv is None else int(round(2.5 * conv))


def expo_setup(name, size, t):
    op = Operator(matrix(name, size), TYPES[t])
    return op, start(name, size, TYPES[t])


def expo_key(name, size, a):
    return "%s%d:%s" % (name, size, a)


def _worst(into, inv, t, value):
    into.setdefault(inv, {}).setdefault(t, 0.0)
    into[inv][t] = max(into[inv][t], float(value))


def measure(windows=None, expo_m=None, log=None, parts="ABCD"):
    """(ratios, windows, expo_m): the models' worst ratio per invariant and storage type over the case list."""
    ratios = {}
    if windows is None:
        windows = {case_key(name, size): late_window(name, size) for name, size, _ in CASES_LATE}
    say = log or (lambda *a: None)
    # ---- A: fixed windows, both models
    first_pass = {}
    for name, size, types in CASES_A if "A" in parts else ():
        late = windows.get(case_key(name, size))
        for t in types:
            op, v0, find_max = case_setup(name, size, t)
            exact = exact_eigenvalues(name, size, op.storage.name)
            for model in (lanczos_model, lagged_model):
                run = model(op, v0, late or WINDOW_EARLY)
                if model is lanczos_model and (name, size, t) in CASES_B:
                    first_pass[name, size, t] = run
                for m in (WINDOW_EARLY, late):
                    if m is None:
                        continue
                    inv = run_invariants(op, model_returns(op, run, find_max, m), find_max, exact)
                    say("A", name, t, model.__name__, m, inv)
                    for k, v in inv.items():
                        _worst(ratios, k, t, v)
    # ---- B: restart passes behind locked Ritz vectors (lanczos_model; window = the late one)
    for name, size, t in CASES_B if "B" in parts else ():
        op, v0, find_max = case_setup(name, size, t)
        exact = exact_eigenvalues(name, size, op.storage.name)
        m = windows[case_key(name, size)]
        found = []
        for i in range(3):
            run = first_pass.get((name, size, t)) if i == 0 else None
            run = run or lanczos_model(op, v0, m, locked=[v for _, v in found])
            ret = model_returns(op, run, find_max, m)
            found.append((ret["vals"][0], ret["vecs"][0]))
        for i, (val, v) in enumerate(found):
            inv = dict(unit=unit(op, v), hermitian=hermitian(op, val, v, exact))
            for j in range(i):
                inv["cross"] = max(inv.get("cross", 0.0), cross(op, v, found[j][1], m))
            say("B", name, t, i, inv)
            for k, v_ in inv.items():
                _worst(ratios, k, t, v_)
    # ---- C: window 41 at the sizes where the forms switch on by themselves
    for name, size, t in CASES_C if "C" in parts else ():
        op, v0, find_max = case_setup(name, size, t)
        for model in (lanczos_model, lagged_model):
            ret = model_returns(op, model(op, v0, WINDOW_EARLY), find_max)
            # (interlace and hermitian are thousands of u_A below zero this far from convergence: the device test forms them,
            # the table does not pay half a minute of eigsh per case for a ratio of 0)
            inv = dict(relation=relation(op, ret, find_max), ritz=ritz(op, ret, find_max), unit=unit(op, ret["vecs"][0]))
            say("C", name, size, t, model.__name__, inv)
            for k, v in inv.items():
                _worst(ratios, k, t, v)
    # ---- D: the Exponentiator
    expo_m = dict(expo_m) if expo_m is not None else {}
    for name, size, a, types in CASES_D if "D" in parts else ():
        key = expo_key(name, size, a)
        if key not in expo_m:
            wide = TYPES[types[0]]
            v = start(name, size, wide)
            expo_m[key] = max(expo_iterations(name, size, a, v, full) for full in (False, True))
        m = expo_m[key]
        for t in types:
            op, v = expo_setup(name, size, t)
            exact = expo_exact(name, size, op.storage, a, v)
            outs = [expo_model(op, a, v, m, False), expo_model(op, a, v, m, True), expo_model(op, a, v, m, True, lagged=True)]
            for out in outs:
                _worst(ratios, "expo_error", t, expo_error(op, out, exact, v))
                if np.iscomplexobj(a):
                    _worst(ratios, "expo_norm", t, expo_norm(op, out, v))
            tout, terms = taylor_model(op, a, v, 1e2 * op.eps)
            _worst(ratios, "taylor_error", t, expo_error(op, tout, exact, v))
            say("D", key, t, {k: ratios.get(k, {}).get(t) for k in ("expo_error", "expo_norm", "taylor_error")}, "taylor terms", terms)
    return ratios, windows, expo_m


def bounds_of(ratios):
    return {inv: {t: max(FLOORS[inv], 4.0 * r) for t, r in per_type.items()} for inv, per_type in ratios.items()}


if __name__ == "__main__":          # prints the table above from the models
    import pprint

    r, w, e = measure(log=print)
    print("WINDOW_LATE =", w)
    print("EXPO_M =", e)
    print("MODEL_RATIOS =", pprint.pformat({k: {t: float("%.3g" % x) for t, x in v.items()} for k, v in r.items()}, width=120))
    print("BOUNDS =", pprint.pformat({k: {t: float("%.3g" % x) for t, x in v.items()} for k, v in bounds_of(r).items()}, width=120))
