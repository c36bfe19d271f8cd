"""Executable specification (numpy) of the RAW-BASIS BLOCK form of the Gram-Schmidt step: m <= 8 Lanczos iterations per sweep over
the basis (eight only behind the measured guard of run_guarded, below) and NO late update, written launch by launch the way csrc/gs_block.hip and csrc/lanczos_loop.hpp implement it (block_*
kernels, LoopState::enqueue_block, block_flush, ritz_basis).  Successor of tools/pair_gs_model.py (the pair form, csrc/gs_pair.hip).

The stored vectors are never rewritten.  The basis in memory is a_0, a_1, ...: every a_j is the raw three-term vector of its
iteration, unnormalised (the last two vectors of every block additionally carry the compensation described below).  Beside them
the loop keeps a small record:
    rho_j          the norm of the part of a_j orthogonal to its predecessors
    C_j[l], l < j  the measured, eps-sized coefficients <u_l, a_j>
The orthonormal Lanczos vectors exist only implicitly,
    u_j = (a_j - sum_{l<j} C_j[l] u_l) / rho_j,
and every consumer reaches them to FIRST order in C by transforming its small coefficient vector (ritz_coefficients, flush);
terms of second order in C (1e-28) are dropped, which is what the gate on the largest relative coefficient (the pair form's
kPairGate = 1e-8) is for.

State between blocks: a_0 .. a_k stored (a_{k-1}, a_k are the "seeds": the operands of the next three-term update), rho_j and C_j
for j <= k, alpha_0 .. alpha_{k-1}, beta_j = rho_{j+1} for j < k.  One block of m iterations:
    for i = 1 .. m:   y_i = A x,  e_i = <x, y_i>        operator kernel; x = a_k / rho_k for i = 1, b_{i-1} / |b_{i-1}| after
                      b_i = y_i - e_i x - s x_prev      three-term kernel (s: what x was divided by); also |b_i|^2
    predict           the known coefficient vectors of the two seed inputs over u_0 .. u_k, propagated m times through the
                      recorded tridiagonal: p_i = predicted U^H b_i (eps-sized).  alpha_k = e_1 - 2 Re C_k[k-1] - quad.
    ONE sweep         M[j, i] = <a_j, b_i> for every stored j <= k and the m new vectors;
                      b_m -= sum_j (p_m[j] / rho_j) a_j,  b_{m-1} -= sum_j (p_{m-1}[j] / rho_j) a_j   (BOTH seeds of the next block);
                      the Gram matrix of the new vectors in the strip; writes only those two vectors.
    fold              C rows and rho of the m new vectors, alpha_{k+1} .. alpha_{k+m-1}, beta_k .. beta_{k+m-1}, the gate value.
alpha of the last vector of a block comes from e_1 of the NEXT block (or of the single iteration that follows the form).

    python tools/block_gs_model.py        -> profiles/block_gs_model.txt
    python tools/block_gs_model.py --block8   -> profiles/block8_model.txt  (blocks of eight behind the guard: run_guarded)
"""
import importlib.util
import os
import sys

import numpy as np
import scipy.sparse as sp

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("pair_gs_model", os.path.join(_HERE, "pair_gs_model.py"))
_pair = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_pair)
make_problem, reference, tri_apply = _pair.make_problem, _pair.reference, _pair.tri_apply


class BlockLoop:
    """The device loop.  Every method below is one kernel launch (or one host step) of a device implementation."""

    def __init__(self, A, v0, K, both_seeds=True, plant=None, mutate=None):
        """plant = (relative size, index of the first new vector of the block it goes into, position i in that block): a known
        perturbation along stored vectors in the raw b_i, to exercise the gate.
        mutate(p, M): called in every block once the predictions p (m x W) and the measured columns M (W x m) are formed, to
        change them in place: a stand-in for a device kernel that gets part of them wrong (tests/test_block_model.py)."""
        self.A, self.K, self.plant, self.mutate = A, K, plant, mutate
        n = v0.shape[0]
        self.a = np.zeros((K + 10, n), dtype=v0.dtype)   # the stored raw vectors
        self.a[0] = v0
        self.rho = [1.0]
        self.C = [np.zeros(0, dtype=v0.dtype)]           # C[j]: j coefficients (the K^2 / 2 numbers the host keeps for a pass)
        self.al, self.be = [], []
        self.k = 0
        self.maxcoef = 0.0
        self.both_seeds = both_seeds                      # False: compensate b_m only (shows why both are needed)
        self.gates = {}                                   # index of a stored vector -> its gate value (fold output)

    # ---- entry: the state the pair form enters from (two clean iterations of the one-sweep form: a_0, a_1 complete, a_2 raw with
    # its measured coefficients)
    def start(self):
        A, a = self.A, self.a
        y = A @ a[0]
        a0 = np.vdot(a[0], y).real
        w = y - a0 * a[0]
        w = w - np.vdot(a[0], w) * a[0]
        b0 = np.linalg.norm(w)
        a[1] = w / b0
        self.rho.append(1.0)
        self.C.append(np.zeros(1, dtype=a.dtype))
        y = A @ a[1]
        e = np.vdot(a[1], y).real
        a[2] = y - e * a[1] - b0 * a[0]
        g = a[:2].conj() @ a[2]
        self.C.append(g)
        self.rho.append(np.sqrt(np.vdot(a[2], a[2]).real - np.vdot(g, g).real))
        self.al += [a0, e]
        self.be += [b0, self.rho[2]]
        self.k = 2

    def _d(self, j, width):
        """Coefficients of the operator input a_j / rho_j over u_0 .. u_{width-1}, WITHOUT its own O(1) entry."""
        d = np.zeros(width, dtype=self.a.dtype)
        d[:j] = self.C[j] / self.rho[j]
        return d

    def block(self, m):
        A, a, k = self.A, self.a, self.k
        al, be, rho, C = self.al, self.be, self.rho, self.C
        W = k + 1                                        # stored vectors = the coefficient space of the prediction
        # ---- m x (operator kernel with ScaleIn and fused dot + raw three-term kernel)
        b = np.zeros((m, a.shape[1]), dtype=a.dtype)
        e, nsq = np.zeros(m), np.zeros(m)
        xp, sp_, x, s = a[k - 1], rho[k - 1], a[k], rho[k]
        for i in range(m):
            xs = x / s
            y = A @ xs
            e[i] = np.vdot(xs, y).real
            b[i] = y - e[i] * xs - s * (xp / sp_)
            if self.plant and self.plant[1] == k + 1 and self.plant[2] == i:   # (test: every later launch sees the planted vector)
                b[i] = b[i] + self.plant[0] * np.linalg.norm(b[i]) * (a[3] / rho[3] - a[7] / rho[7] + 0.5 * a[k - 2] / rho[k - 2])
            nsq[i] = np.vdot(b[i], b[i]).real
            xp, sp_, x, s = x, s, b[i], np.sqrt(nsq[i])
        nrm = np.sqrt(nsq)
        # ---- predict (one workgroup).  alpha_k from e_1: the input was a_k / rho_k = u_k + sum d_k[l] u_l
        dk, dk1 = self._d(k, W), self._d(k - 1, W)
        alpha_k = e[0] - 2.0 * C[k][k - 1].real - np.vdot(dk[:k], tri_apply(al, be, dk[:k])).real
        al.append(alpha_k)                               # al now holds alpha_0 .. alpha_k: the whole (k+1) x (k+1) tridiagonal
        # first step: the O(1) self entries (1 on u_k for the input, 1 on u_{k-1} for its predecessor) take part; rows k and k-1
        # cancel exactly in beta_{k-1} = rho_k and leave (alpha_k - e_1) in row k, which is formed from the eps-sized numbers
        p = np.zeros((m, W), dtype=a.dtype)
        p[0] = tri_apply(al, be, dk) - e[0] * dk - rho[k] * dk1
        p[0][k] += alpha_k - e[0]
        # from the second step on the predecessor's self entry is zero: the new direction's back-coupling beta u_k cancels it, and
        # the new directions are not in the space
        pn_prev, pn = dk, p[0] / nrm[0]
        for i in range(1, m):
            p[i] = tri_apply(al, be, pn) - e[i] * pn - nrm[i - 1] * pn_prev
            pn_prev, pn = pn, p[i] / nrm[i]
        # ---- ONE sweep over the stored raw vectors; the stored basis is not touched
        S = a[:W]
        M = S.conj() @ b.T                               # M[j, i] = <a_j, b_i>, raw
        if self.mutate is not None:
            self.mutate(p, M)
        comp = [m - 1] + ([m - 2] if (m >= 2 and self.both_seeds) else [])
        irho = 1.0 / np.asarray(rho[:W])
        for i in comp:
            b[i] = b[i] - (p[i] * irho) @ S
        G = b.conj() @ b.T                               # in-strip Gram matrix (the two compensated vectors as written)
        # ---- fold (one workgroup)
        raw_c = []                                       # coefficient rows of the RAW b_i (what the operator saw)
        for i in range(m):
            j = k + 1 + i                                # index of the new vector
            c = np.zeros(j, dtype=a.dtype)
            c[:W] = M[:, i] * irho                       # stored columns: first order (C^H c is second order)
            for col in (k - 1, k):                       # the two seeds: exact recursion
                c[col] = (M[col, i] - np.vdot(C[col], c[:col])) / rho[col]
            raw = c.copy()
            if i in comp:
                c[:W] -= p[i]                            # by linearity: the vector as written
            for ip in range(i):                          # in-block predecessors: exact recursion
                col = k + 1 + ip
                c[col] = (G[ip, i] - np.vdot(C[col], c[:col])) / rho[col]
                raw[col] = c[col]                        # (the compensation changes these in second order only)
            nn = G[i, i].real
            r2 = max(nn - np.vdot(c, c).real, 0.0)
            C.append(c)
            rho.append(np.sqrt(r2))
            raw_c.append(raw)
            be.append(rho[j])                            # beta_{j-1} couples u_{j-1} and u_j
            self.gates[j] = max(np.abs(raw).max() / nrm[i], np.abs(c).max() / np.sqrt(nn))
            self.maxcoef = max(self.maxcoef, self.gates[j])
            a[j] = b[i]
            if i >= 1:
                # alpha of the PREVIOUS new vector, from this step's e: its input was the raw b_{i-1} / |b_{i-1}|
                #   <b, A b> = rho^2 alpha + 2 rho^2 Re c[prev] + <E, A E>
                jp, cp = j - 1, raw_c[i - 1]
                quad = np.vdot(cp, tri_apply(al, be, cp)).real
                al.append((e[i] * nsq[i - 1] - 2.0 * rho[jp] ** 2 * cp[jp - 1].real - quad) / rho[jp] ** 2)
        self.k = k + m
        # now: al holds alpha_0 .. alpha_{k+m-1}, be holds beta_0 .. beta_{k+m-1}: m iterations recorded

    # ---- consumers of the basis
    def implied_basis(self, count):
        """The orthonormal vectors the record defines (exact back-substitution; model only)."""
        U = np.zeros((count, self.a.shape[1]), dtype=self.a.dtype)
        for j in range(count):
            U[j] = (self.a[j] - self.C[j] @ U[:j]) / self.rho[j]
        return U

    def ritz_coefficients(self, q):
        """Host transform of a coefficient vector over u_0 .. u_{K-1} into one over the stored raw vectors, first order in C:
        c'_j = (q_j - sum_{k>j} C_k[j] q_k / rho_k) / rho_j."""
        K = len(q)
        out = np.array(q, dtype=self.a.dtype)
        for kk in range(K):
            out[:kk] -= self.C[kk] * (q[kk] / self.rho[kk])
        return out / np.asarray(self.rho[:K])

    def flush(self, last=None):
        """Leave the form: complete and normalise the raw vectors a_0 .. a_last IN PLACE, from the highest index down; whatever lies
        behind a_last (later vectors of a block that a gate or a stop cut) is dropped with its records.  The first-order formula
        uses only raw vectors of lower index, which the descending order has not touched yet.  An O(P^2) pass over the basis."""
        a, rho, C = self.a, self.rho, self.C
        if last is not None and last < self.k:
            self.k = last
            del rho[last + 1:], C[last + 1:], self.al[last:], self.be[last:]
        for j in range(self.k, -1, -1):
            a[j] = (a[j] - (C[j] / np.asarray(rho[:j])) @ a[:j]) / rho[j]
        for j in range(self.k + 1):
            rho[j], C[j] = 1.0, np.zeros(j, dtype=a.dtype)

    def clean_iteration(self):
        """One iteration from a flushed (complete, orthonormal) basis: what the device's one-sweep form computes."""
        A, a, k = self.A, self.a, self.k
        y = A @ a[k]
        alpha = np.vdot(a[k], y).real
        w = y - alpha * a[k] - self.be[-1] * a[k - 1]
        for _ in range(2):
            w = w - (a[:k + 1].conj() @ w) @ a[:k + 1]
        beta = np.linalg.norm(w)
        a[k + 1] = w / beta
        self.rho.append(1.0)
        self.C.append(np.zeros(k + 1, dtype=a.dtype))
        self.al.append(alpha)
        self.be.append(beta)
        self.k = k + 1


GATE = 1e-8   # kPairGate


def run_loop(A, v0, K, m, both_seeds=True, plant=None, gate=GATE, mutate=None):
    """K recorded iterations: blocks of m, then of 2 while two remain, an odd last iteration single after the flush.  A vector
    whose gate value exceeds `gate` stands (its coefficients were measured), everything behind it is dropped, the basis is flushed
    and the pass finishes with single iterations, like the pair form's gate trip."""
    L = BlockLoop(A, v0, K, both_seeds, plant, mutate)
    L.start()
    L.gate_trips = 0
    while len(L.al) + 2 <= K and not L.gate_trips:
        k0 = L.k
        L.block(m if len(L.al) + m <= K else 2)
        for j in range(k0 + 1, L.k + 1):
            if not L.gates[j] <= gate:
                L.gate_trips = 1
                L.flush(j)
                break
    if len(L.al) < K:
        L.flush()
        while len(L.al) < K:
            L.clean_iteration()
    return L


# ---- blocks of EIGHT behind a measured guard (csrc/lanczos_loop.hpp: LoopState::collect, enqueue_block_f64)
# Fresh rounding along a converged Ritz direction grows by r = (theta - alpha) / beta per operator application and is measured only
# by the next sweep: a block of m reaches about eps r^(m-1).  From a gate value g measured with blocks of four the value at eight is
# predicted as g (g / eps)^(4/3); a factor 10 under the gate (1e-8) asks for g <= 1.6e-13.  That prediction assumes a STATIONARY r.
# While a Ritz value is still converging r grows from block to block (the outlier matrix below: 5e-16, 1e-13, 1e-12 in the first three
# blocks of four), so one quiet block is no evidence: the guard asks for kBlock8Quiet CONSECUTIVE collected iterations at or below
# kBlock8Tau, and kBlock8Tau sits between what blocks of four publish on matrices without converged outliers (<= 2.3e-14 over the
# problems below, 300 iterations) and what they publish once an outlier has converged (1e-13 .. 5e-12).  The host enqueues a block
# while the block before it is still running, so the guard sees the gate values up to the block BEFORE the previous one (lag = 1).
TAU = 5e-14     # kBlock8Tau
QUIET = 12      # kBlock8Quiet


def run_guarded(A, v0, K, mmax=8, tau=TAU, quiet_need=QUIET, lag=1, plant=None, gate=GATE, mutate=None):
    """K recorded iterations in blocks of 8 (where the guard admits them and eight remain), else 4, 2, 1: never past K.  The gate
    works as in run_loop.  Leaves L.sizes (the block sizes taken) and L.n8 (iterations run in eights)."""
    L = BlockLoop(A, v0, K, True, plant, mutate)
    L.start()
    L.gate_trips, L.n8, L.sizes = 0, 0, []
    blocks = []                                          # the gate values of every block, in order
    while len(L.al) < K and not L.gate_trips:
        rem = K - len(L.al)
        quiet = 0
        for blk in blocks[:len(blocks) - lag]:           # what the host has collected when it enqueues this block
            for g in blk:
                quiet = quiet + 1 if g <= tau else 0
        m = 8 if (mmax >= 8 and rem >= 8 and quiet >= quiet_need) else 4 if rem >= 4 else 2 if rem >= 2 else 1
        k0 = L.k
        L.block(m)
        L.sizes.append(m)
        L.n8 += m if m == 8 else 0
        blocks.append([L.gates[j] for j in range(k0 + 1, L.k + 1)])
        for j in range(k0 + 1, L.k + 1):
            if not L.gates[j] <= gate:
                L.gate_trips = 1
                L.flush(j)
                break
    if len(L.al) < K:
        L.flush()
        while len(L.al) < K:
            L.clean_iteration()
    return L


def _random_rows(n, per_row, lo, complex_, seed, imag=1.0):
    rng = np.random.default_rng(seed)
    rows, cols = np.repeat(np.arange(n), per_row), rng.integers(0, n, per_row * n)
    vals = rng.uniform(lo, 1, per_row * n) + (1j * imag * rng.uniform(-1, 1, per_row * n) if complex_ else 0)
    v0 = rng.uniform(-1, 1, n) + (1j * rng.uniform(-1, 1, n) if complex_ else 0)
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, n)), v0 / np.linalg.norm(v0)


def config3_problem(n, complex_, seed=5):
    """The flagship's type: B + B^H + 7 I, seven entries per row of B in (-1, 1)."""
    B, v0 = _random_rows(n, 7, -1, complex_, seed)
    return (B + B.conj().T + 7 * sp.eye(n)).tocsr(), v0


def outlier_problem(n, complex_, seed=7):
    """Symmetric with a dominant outlier: fifteen entries per row in (0, 1), symmetrised.  The largest Ritz value converges within
    the first blocks and r = (theta - alpha) / beta is about 13 from then on."""
    B, v0 = _random_rows(n, 15, 0, complex_, seed, imag=0.1)
    return ((B + B.conj().T) * 0.5).tocsr(), v0


def norm_inf(A):
    return abs(A).sum(axis=1).max()


def measure8(A, v0, K, ref=None, **kw):
    ra, rb, _ = ref if ref is not None else reference(A, v0, K)
    with np.errstate(all="ignore"):
        L = run_guarded(A, v0, K, **kw)
    a, b = np.array(L.al), np.array(L.be)
    return dict(dalpha=np.abs(a - ra[:K]).max(), dbeta=np.abs(b - rb[:K]).max(), tol=1e-10 * norm_inf(A), maxcoef=L.maxcoef,
                gate_trips=L.gate_trips, n8=L.n8, sizes=L.sizes, alpha=a, beta=b)


def main8():
    out = ["blocks of eight behind the guard (tools/block_gs_model.py --block8): eight only after %d consecutive collected iterations" % QUIET,
           "with a gate value <= %.1e, guard one block late (the host's view); against full re-orthogonalisation; gate 1e-08" % TAU, ""]
    problems = (("the model's problem, n = 3000", lambda c: make_problem(3000, c)),
                ("config-3 type, n = 20000", lambda c: config3_problem(20000, c)))
    for name, mk in problems:
        for cplx in (False, True):
            A, v0 = mk(cplx)
            ref = reference(A, v0, 1024)
            for K in (100, 300, 1024):
                r = measure8(A, v0, K, ref)
                out.append("  %s, %s, K = %4d: max|dalpha| %.1e  max|dbeta| %.1e  (1e-10 ||A|| = %.1e)  largest relative coefficient %.1e  "
                           "gate trips %d  in eights %d (%.0f %%)" % (name, "complex" if cplx else "real", K, r["dalpha"], r["dbeta"], r["tol"],
                                                                   r["maxcoef"], r["gate_trips"], r["n8"], 100.0 * r["n8"] / K))
    out += ["", "the outlier matrix (n = 4000, K = 100), seeds 0 .. 11: runs in which the guard admitted a block of eight, and the"
            " largest coefficient;", "a guard on ONE quiet block (at or below 1.6e-13) for comparison:"]
    for label, kw in (("%d iterations <= %.1e" % (QUIET, TAU), {}), ("one block <= 1.6e-13", dict(tau=1.6e-13, quiet_need=1))):
        for cplx in (False, True):
            admitted, worst, trips = 0, 0.0, 0
            for seed in range(12):
                A, v0 = outlier_problem(4000, cplx, seed)
                with np.errstate(all="ignore"):
                    L = run_guarded(A, v0, 100, **kw)
                admitted += L.n8 > 0
                worst = max(worst, L.maxcoef)
                trips += L.gate_trips
            out.append("  %-26s %s: %2d of 12 runs took a block of eight; largest relative coefficient %.1e; gate trips %d" % (
                label, "complex" if cplx else "real   ", admitted, worst, trips))
    A, v0 = outlier_problem(4000, False)
    with np.errstate(all="ignore"):
        L8, L4 = run_guarded(A, v0, 100), run_loop(A, v0, 100, 4)
    out.append("  seed 7, real: in eights %d; alpha and beta equal to the m = 4 run bit for bit: %s" % (
        L8.n8, np.array_equal(L8.al, L4.al) and np.array_equal(L8.be, L4.be)))
    out += ["", "a component of 1e-6 planted in each position of a block of eight (config-3 type, n = 6000, K = 120; the block starts at",
            "vector 27 with the guard's default warm-up):"]
    A, v0 = config3_problem(6000, False)
    ref = reference(A, v0, 120)
    for pos in range(8):
        r = measure8(A, v0, 120, ref, plant=(1e-6, 27, pos))
        out.append("  position %d: gate trips %d  largest relative coefficient %.1e  max|dalpha| %.1e  max|dbeta| %.1e" % (
            pos + 1, r["gate_trips"], r["maxcoef"], r["dalpha"], r["dbeta"]))
    text = "\n".join(out) + "\n"
    print(text)
    if "--no-write" not in sys.argv:
        with open(os.path.join(os.path.dirname(_HERE), "profiles", "block8_model.txt"), "w") as f:
            f.write(text)


def from_pair(P):
    """The block state from a PairLoop's state between sweeps (P complete vectors, r1 and r2 pending with their measured
    coefficients): the stored vectors are used as they are, the two pending ones become a_P and a_{P+1}."""
    assert P.L == 0
    L = BlockLoop(P.A, P.S[0], P.K)
    n = P.P
    L.a[:n] = P.S[:n]
    L.a[n], L.a[n + 1] = P.r1, P.r2
    L.rho = [1.0] * n + [P.rho1, P.rho2]
    L.C = [np.zeros(j, dtype=L.a.dtype) for j in range(n)] + [np.array(P.g1), np.concatenate([P.g2, [P.gam]])]
    L.al, L.be = list(P.al[:n + 1]), list(P.be[:n + 1])
    L.k = n + 1
    L.gate_trips = 0
    return L


def measure(complex_, m, n=3000, K=200, both_seeds=True, plant=None, gate=GATE):
    """Run the block loop and the reference on the same problem: the numbers the statements in DESIGN.md 8 rest on."""
    A, v0 = make_problem(n, complex_)
    ra, rb, RU = reference(A, v0, K)
    with np.errstate(all="ignore"):
        L = run_loop(A, v0, K, m, both_seeds, plant, gate)
    return compare(L, ra, rb, RU)


def compare(L, ra, rb, RU):
    a, b = np.array(L.al), np.array(L.be)
    it = len(a)
    with np.errstate(all="ignore"):
        U = L.implied_basis(L.k + 1)
    orth_implied = np.abs(U.conj() @ U.T - np.eye(len(U))).max()
    # the Ritz vector of the largest eigenvalue through the transformed coefficients, against the reference's basis
    T = np.diag(a[:it]) + np.diag(b[:it - 1], 1) + np.diag(b[:it - 1], -1)
    q = np.linalg.eigh(T)[1][:, -1]
    v = L.ritz_coefficients(q) @ L.a[:it]
    v_ref = q @ RU[:it]
    ritz = 1.0 - abs(np.vdot(v_ref, v)) / np.linalg.norm(v)
    with np.errstate(all="ignore"):
        L.flush()
    S = L.a[:L.k + 1]
    return dict(iterations=it, dalpha=np.abs(a - ra[:it]).max(), dbeta=np.abs(b - rb[:it]).max(), orth=orth_implied,
                maxcoef=L.maxcoef, ritz=ritz, gate_trips=L.gate_trips, orth_flushed=np.abs(S.conj() @ S.T - np.eye(len(S))).max(),
                dvec_flushed=max(np.linalg.norm(S[j] - RU[j]) for j in range(len(S))))


def pair_entry(complex_, n=1500, K=81, at=21):
    """The pair form up to `at` recorded iterations, the block form from its state on (K odd: the last iteration runs single)."""
    A, v0 = make_problem(n, complex_)
    ra, rb, RU = reference(A, v0, K)
    P = _pair.PairLoop(A, v0, K)
    P.start()
    while len(P.al) < at:
        P.pair()
    L = from_pair(P)
    while len(L.al) + 4 <= K:
        L.block(4)
    while len(L.al) + 2 <= K:
        L.block(2)
    if len(L.al) < K:
        L.flush()
        L.clean_iteration()
    return compare(L, ra, rb, RU)


def stop_in_block(complex_, stop, m=4, n=1500):
    """A stop decided at iteration `stop` inside a block: the results use alpha, beta and the vectors up to that iteration only;
    the later vectors of the block are slots nothing reads.  (Blocks start at iteration 3, 7, 11, ...)"""
    A, v0 = make_problem(n, complex_)
    ra, rb, RU = reference(A, v0, stop + m)
    L = BlockLoop(A, v0, stop + m)
    L.start()
    while len(L.al) < stop:
        L.block(m)
    a, b = np.array(L.al[:stop]), np.array(L.be[:stop])
    T = np.diag(a) + np.diag(b[:stop - 1], 1) + np.diag(b[:stop - 1], -1)
    w, Q = np.linalg.eigh(T)
    Tr = np.diag(ra[:stop]) + np.diag(rb[:stop - 1], 1) + np.diag(rb[:stop - 1], -1)
    wr, Qr = np.linalg.eigh(Tr)
    v = L.ritz_coefficients(Q[:, -1]) @ L.a[:stop]
    v_ref = Qr[:, -1] @ RU[:stop]
    return dict(dropped=len(L.al) - stop, dlambda=abs(w[-1] - wr[-1]), ritz=1.0 - abs(np.vdot(v_ref, v)),
                dnorm=abs(np.linalg.norm(v) - 1.0), dalpha=np.abs(a - ra[:stop]).max(), dbeta=np.abs(b - rb[:stop]).max())


def main():
    out = ["raw-basis block Gram-Schmidt, launch-structured model (tools/block_gs_model.py); n = 3000, 200 iterations,",
           "against full re-orthogonalisation; the suite's tolerance for alpha and beta is 1e-10 ||A|| = 1.2e-09, the gate 1e-08", ""]
    fmt = "  block %d: max|dalpha| %.1e  max|dbeta| %.1e  implied basis max|U^H U - I| %.1e  largest relative coefficient %.1e"
    for cplx in (False, True):
        out.append("complex Hermitian" if cplx else "real symmetric")
        for m in (2, 4, 8):
            r = measure(cplx, m)
            out.append(fmt % (m, r["dalpha"], r["dbeta"], r["orth"], r["maxcoef"]))
            out.append("           Ritz vector through transformed coefficients: 1 - |<v_ref, v>| %.1e;  after the flush: max|S^H S - I| %.1e, "
                       "max|u_j - u_j(ref)| %.1e" % (r["ritz"], r["orth_flushed"], r["dvec_flushed"]))
    out += ["", "only b_m compensated (the other seed keeps its stored-basis components), gate off, real symmetric:"]
    for K in (60, 100, 140):
        r = measure(False, 4, K=K, both_seeds=False, gate=np.inf)
        out.append("  block 4, %3d iterations: max|dalpha| %.1e  max|dbeta| %.1e  largest relative coefficient %.1e" % (
            K, r["dalpha"], r["dbeta"], r["maxcoef"]))
    out += ["", "entry from the pair form's state at 21 iterations, blocks of four, odd last iteration single (n = 1500, 81 iterations):"]
    for cplx in (False, True):
        r = pair_entry(cplx)
        out.append("  %s: max|dalpha| %.1e  max|dbeta| %.1e  largest relative coefficient %.1e  after the flush: max|S^H S - I| %.1e" % (
            "complex" if cplx else "real", r["dalpha"], r["dbeta"], r["maxcoef"], r["orth_flushed"]))
    out += ["", "stop inside a block of four (n = 1500): the results read iterations <= stop only"]
    for cplx in (False, True):
        for stop in (41, 42, 43, 44):
            r = stop_in_block(cplx, stop)
            out.append("  %s, stop at %d (%d later iterations of its block dropped): |dlambda| %.1e  1 - |<v_ref, v>| %.1e  | |v| - 1 | %.1e  "
                       "max|dalpha| %.1e  max|dbeta| %.1e" % ("complex" if cplx else "real", stop, r["dropped"], r["dlambda"], r["ritz"],
                                                             r["dnorm"], r["dalpha"], r["dbeta"]))
    out += ["", "components planted along stored vectors in one raw vector (block of four starting at vector 23; n = 1500, 120 iterations);",
            "above the gate the vector stands, the rest of its block is dropped, the basis is flushed, single iterations finish the pass:"]
    for cplx, size, pos in ((False, 1e-9, 3), (False, 1e-6, 0), (False, 1e-6, 3), (True, 1e-6, 1), (False, 1e-3, 3)):
        r = measure(cplx, 4, n=1500, K=120, plant=(size, 23, pos))
        out.append("  %s, %.0e in vector %d of the block: gate trips %d  largest relative coefficient %.1e  max|dalpha| %.1e  max|dbeta| %.1e  "
                   "after the flush: max|S^H S - I| %.1e" % ("complex" if cplx else "real", size, pos + 1, r["gate_trips"], r["maxcoef"],
                                                            r["dalpha"], r["dbeta"], r["orth_flushed"]))
    text = "\n".join(out) + "\n"
    print(text)
    if "--no-write" not in sys.argv:
        with open(os.path.join(os.path.dirname(_HERE), "profiles", "block_gs_model.txt"), "w") as f:
            f.write(text)


if __name__ == "__main__":
    main8() if "--block8" in sys.argv else main()
