"""Reduced density matrices of 4 to 13 sites on the f64 matrix cores (ll_pauli_rdm_tiled, csrc/pauli_rdm_tiled.hip, planned by
csrc/pauli_rdm_tiled_plan.hpp): every part of every entry against the EXACT host reference — rho[a][a'] = <f_a', f_a> of the two
fibres f_a = psi(a, .) (generators.reduced_density_matrix_np), correctly rounded as exact_ref.dot_exact rounds it — at the
project's bound for a double-accumulated dot in any summation order (exact_ref.dot_bound; the split-K folds are among its n - 1
additions) plus one double rounding; in all four storage types, at the smallest shapes that exercise each mechanism — m = n_sites
(one padded K-step), 2, 4 and 8 environment configurations, the 16- and 32-row padding, one, three and ten macro-tiles, sites
below, across and above the rest and in non-ascending order, KC forced to 4, ksplit forced to 1, 2, 8 — the Hermitian mirror and
the zeros by rule bit for bit, psi in guarded NaN-padded buffers at two alignments and on the host, out on the device, agreement
with ll_pauli_rdm at m = 4, 5, 6, S_z sectors with rows that cannot be completed, entropies with known answers, the block route
and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import contract_cases as K
import exact_ref as E
import lambda_lanczos_amd as L
from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G
from guarded import guarded as _guarded, unguard as _unguard
from test_gpu_pauli_rdm import NAN_FILL, TYPE_IDS, TYPES, _eta, _popc, _refused, check_rho

pytestmark = pytest.mark.gpu

# (n_sites, sites): what each case is for
FULL_CASES = [
    (4, [0, 1, 2, 3]),                    # m = n_sites: K = 1, three zero columns; 16 rows of 64
    (5, [4, 0, 2, 1]),                    # n - m = 1
    (6, [5, 1, 3, 2]),                    # n - m = 2
    (7, [0, 2, 4, 6]),                    # n - m = 3
    (9, [8, 0, 4, 2, 6]),                 # m = 5: 32 rows of 64
    (9, [0, 1, 2, 3, 4, 5]),              # m = 6, the sites below the environment: one full macro-tile
    (9, [8, 7, 6, 5, 4, 3]),              # m = 6, above it, descending
    (9, [8, 1, 3, 0, 5, 6, 2]),           # m = 7: three macro-tiles, one off the diagonal; K = 4
    (12, [2, 3, 5, 7, 8, 10, 11]),        # m = 7, K = 32: two K-steps of 16
    (11, [10, 0, 9, 1, 8, 2, 7, 3]),      # m = 8: ten macro-tiles
]
# (pauli_rdm_tiled_kc, pauli_rdm_tiled_ksplit); the first two are also measured at every placement of psi
TUNINGS = [(None, None), (4, 2), (4, None), (None, 1), (4, 8), (8, 2)]
SECTOR_CASES = [(10, 5, [9, 0, 2, 4, 5, 7, 8]), (12, 4, [0, 1, 3, 6, 8, 10, 11]), (9, 3, [7, 1, 3, 8, 4])]


def _cplx(dtype):
    return np.dtype(dtype).kind == "c"


def fibre_dots(fib, n_down=None):
    """(want, bound) for every entry, as test_gpu_pauli_rdm.reference defines them — want[a][a'] = exact_ref.dot_exact(f_a', f_a),
    bound = exact_ref.dot_bound(f_a', f_a) + one double rounding — with the pairs a <= a' batched through the row-wise exact sum
    that dot_exact itself calls (one row per pair), and mirrored.  A sector's popcount-off-diagonal pairs are zero by rule."""
    dim, k = fib.shape
    ia, iap = np.triu_indices(dim)
    if n_down is not None:
        pc = np.array([_popc(a) for a in range(dim)])
        keep = pc[ia] == pc[iap]
        ia, iap = ia[keep], iap[keep]
    x, y = fib[iap].reshape(-1), fib[ia].reshape(-1)   # <x, y> = sum conj(x) y
    rp = np.arange(ia.shape[0] + 1, dtype=np.int64) * k
    xr, yr = np.real(x).astype(np.float64), np.real(y).astype(np.float64)
    if np.iscomplexobj(fib):
        xi, yi = np.imag(x).astype(np.float64), np.imag(y).astype(np.float64)
        w = E._exact_sums(rp, [(xr, yr), (xi, yi)]) + 1j * E._exact_sums(rp, [(xr, yi), (-xi, yr)])
    else:
        w = E._exact_sums(rp, [(xr, yr)]).astype(np.complex128)
    mag = E.abs1(fib)
    b = 2.0 * (k + 8) * E.EPS_D * np.sum(mag[iap] * mag[ia], axis=1) + 1e-300 + E.EPS_D * np.maximum(np.abs(w.real), np.abs(w.imag))
    for j in np.random.default_rng(3).integers(0, ia.shape[0], 4):   # the batch is the per-pair reference
        one = complex(E.dot_exact(fib[iap[j]], fib[ia[j]]))
        assert one == w[j] and abs(E.dot_bound(fib[iap[j]], fib[ia[j]]) + E.EPS_D * max(abs(one.real), abs(one.imag)) - b[j]) <= 1e-3 * b[j]
    want, bound = np.zeros((dim, dim), np.complex128), np.zeros((dim, dim))
    want[ia, iap], want[iap, ia] = w, w.conj()
    bound[ia, iap] = bound[iap, ia] = b
    return want, bound


_REF = {}


def reference(n_sites, n_down, sites, dtype):
    """(psi, want, bound), computed once per case and storage type and left unchanged."""
    key = (n_sites, n_down, tuple(sites), np.dtype(dtype).char)
    if key not in _REF:
        states = None if n_down is None else G.sector_states(n_sites, n_down)
        n = (1 << n_sites) if states is None else states.shape[0]
        psi = K.start_x(n, dtype)
        _, fib = G.reduced_density_matrix_np(n_sites, sites, psi, states=states)
        want, bound = fibre_dots(fib, n_down)
        for a in (psi, want, bound):
            a.setflags(write=False)
        _REF[key] = (psi, want, bound)
    return _REF[key]


def _tune(ctx, kc, ksplit):
    ctx.set_tuning("pauli_rdm_tiled_kc", None if kc is None else str(kc))
    ctx.set_tuning("pauli_rdm_tiled_ksplit", None if ksplit is None else str(ksplit))


def measure_everywhere(ctx, op, psi, sites, want, bound, dtype, n_down, what):
    """psi in guarded, NaN-padded device buffers at shift 0 and 1 and on the host, out on the host and on the device: every entry
    within its bound, psi unchanged, the same bits for every placement and from call to call.  Returns (worst error / bound, rho)."""
    n, dim = psi.shape[0], 1 << len(sites)
    first, worst = None, 0.0
    for shift in (0, 1):
        buf, view = _guarded(ctx, psi, shift, NAN_FILL)
        for rep in range(2):
            got, nsw = op.reduced_density_matrix_tiled(view, sites, return_sweeps=True)
            assert nsw == 1, (what, shift, nsw)
            worst = max(worst, check_rho(got, want, bound, dtype, n_down, (what, "device", shift)))
            if first is None:
                first = got
            assert np.array_equal(first.view(np.uint8), got.view(np.uint8)), (what, "device", shift, rep)
        dout = ctx.empty(dim * dim, np.complex128)
        try:
            assert op.reduced_density_matrix_tiled(view, sites, out=dout) is dout
            assert np.array_equal(first.view(np.uint8), dout.get().reshape(dim, dim).view(np.uint8)), (what, "out on the device", shift)
        finally:
            dout.free()
        assert np.array_equal(_unguard(buf, n, shift, NAN_FILL), psi), "the measurement changed psi"
        buf.free()
    got = op.reduced_density_matrix_tiled(psi, sites)
    assert np.array_equal(first.view(np.uint8), got.view(np.uint8)), (what, "host psi")
    return worst, first


# ------------------------------------------------------------------ 1. the full space
@pytest.mark.parametrize("n_sites,sites", FULL_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_full_space_against_the_exact_reference(ctx, dtype, n_sites, sites):
    psi, want, bound = reference(n_sites, None, sites, dtype)
    op = L.PauliOperator(ctx, n_sites, G.tfim_terms(n_sites, 1.0, 0.7), dtype)   # the Hamiltonian's terms play no part
    worst = 0.0
    try:
        for j, (kc, ksplit) in enumerate(TUNINGS):
            _tune(ctx, kc, ksplit)
            what = (n_sites, sites, kc, ksplit)
            if j < 2:
                w, rho = measure_everywhere(ctx, op, psi, sites, want, bound, dtype, None, what)
            else:
                rho = op.reduced_density_matrix_tiled(psi, sites)
                w = check_rho(rho, want, bound, dtype, None, what)
            worst = max(worst, w)
        if len(sites) <= 6:   # the one-sweep kernel of up to six sites: each within its own bound of the same reference
            _tune(ctx, None, None)
            old = op.reduced_density_matrix(psi, sites)
            new = op.reduced_density_matrix_tiled(psi, sites)
            diff = np.maximum(np.abs(old.real - new.real), np.abs(old.imag - new.imag))
            print("against ll_pauli_rdm: worst difference / (sum of both bounds)", float(np.max(diff / (2 * bound))))
            assert np.all(diff <= 2 * bound), (n_sites, sites)
    finally:
        _tune(ctx, None, None)
        op.close()
    print("worst error / bound", np.dtype(dtype).char, n_sites, sites, worst)


# ------------------------------------------------------------------ 2. S_z sectors
@pytest.mark.parametrize("n_sites,n_down,sites", SECTOR_CASES, ids=["10-5-m7", "12-4-m7", "9-3-m5"])
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_sector_against_the_exact_reference(ctx, dtype, n_sites, n_down, sites):
    psi, want, bound = reference(n_sites, n_down, sites, dtype)
    m, dim = len(sites), 1 << len(sites)
    dead = [a for a in range(dim) if not 0 <= n_down - _popc(a) <= n_sites - m]
    assert dead, "the case holds a row that no environment configuration completes"
    op = L.PauliSectorOperator(ctx, n_sites, n_down, G.heisenberg_terms(n_sites, 1.0, 0.8, periodic=False), dtype)
    worst = 0.0
    try:
        assert op.n_local == psi.shape[0] == math.comb(n_sites, n_down)
        for j, (kc, ksplit) in enumerate(TUNINGS[:4]):
            _tune(ctx, kc, ksplit)
            what = (n_sites, n_down, sites, kc, ksplit)
            if j < 2:
                w, rho = measure_everywhere(ctx, op, psi, sites, want, bound, dtype, n_down, what)
            else:
                rho = op.reduced_density_matrix_tiled(psi, sites)
                w = check_rho(rho, want, bound, dtype, n_down, what)
            worst = max(worst, w)
            assert not np.any(np.ascontiguousarray(rho[dead, :]).view(np.uint64)), (what, "a row that cannot be completed")
            assert not np.any(np.ascontiguousarray(rho[:, dead]).view(np.uint64)), (what, "a column that cannot be completed")
        if m <= 6:
            _tune(ctx, None, None)
            old, new = op.reduced_density_matrix(psi, sites), op.reduced_density_matrix_tiled(psi, sites)
            assert np.all(np.maximum(np.abs(old.real - new.real), np.abs(old.imag - new.imag)) <= 2 * bound)
    finally:
        _tune(ctx, None, None)
        op.close()
    print("worst error / bound", np.dtype(dtype).char, (n_sites, n_down), sites, worst)


# ------------------------------------------------------------------ 3. physics: states built on the host, exact entropies
def _entropy_with_tolerance(op, n_sites, psi, sites):
    """(S, tolerance): eigenvalues of rho / tr rho move by at most delta = ||entry bounds||_F / tr rho (Weyl), and
    |eta(x) - eta(y)| <= eta(|x - y|) for |x - y| <= 1/2: 2^m eta(delta) — test_gpu_pauli_rdm's derivation."""
    m = len(sites)
    rho = op.reduced_density_matrix_tiled(psi, sites)
    _, fib = G.reduced_density_matrix_np(n_sites, sites, psi)
    mag = E.abs1(fib)
    b = 2.0 * (fib.shape[1] + 8) * E.EPS_D * (mag @ mag.T) * (1.0 + 1e-12) + 1e-300   # dot_bound of every pair of fibres
    parts = 2 if np.iscomplexobj(psi) else 1
    nn = E.dot_exact(psi, psi).real
    assert abs(np.trace(rho).real - nn) <= (1 << m) * E.dot_bound(psi, psi), "tr rho != ||psi||^2"
    delta = math.sqrt(parts * float(np.sum(b * b))) / nn
    assert delta <= 0.5
    return L.entanglement_entropy(rho), (1 << m) * _eta(delta)


def test_singlets_across_the_cut(ctx):
    """16 sites as singlets (i, i + 8), the subsystem sites 0 .. 7: every singlet is cut, S = 8 ln 2 (m = 8: ten macro-tiles)."""
    n_sites = 16
    s = np.arange(1 << n_sites, dtype=np.int64)
    lo, hi = s & 0xFF, s >> 8
    anti = (lo ^ hi) == 0xFF                       # every pair holds one up and one down spin
    sign = np.array([1.0, -1.0])[np.array([_popc(int(v)) for v in range(256)]) & 1][lo]   # (-1)^(down spins on the low half)
    psi = np.where(anti, sign, 0.0) / 16.0
    op = L.PauliOperator(ctx, n_sites, [(0, 1, 1.0)], np.float64)
    try:
        for sites in (list(range(8)), [7, 6, 5, 4, 3, 2, 1, 0], list(range(8, 16))):
            got, tol = _entropy_with_tolerance(op, n_sites, psi, sites)
            print("singlets across the cut", sites, "S", got, "exact", 8 * math.log(2.0), "tolerance", tol)
            assert abs(got - 8 * math.log(2.0)) <= tol
    finally:
        op.close()


@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=["d", "z"])
def test_product_state_has_no_entanglement(ctx, dtype):
    n_sites = 12
    rng = np.random.default_rng(11)
    psi = np.ones(1, dtype)
    for _ in range(n_sites):
        v = rng.uniform(-1, 1, 2) + (1j * rng.uniform(-1, 1, 2) if _cplx(dtype) else 0.0)
        psi = np.kron(v.astype(dtype), psi)
    op = L.PauliOperator(ctx, n_sites, [(0, 1, 1.0)], dtype)
    try:
        for sites in ([0, 1, 2, 3], [11, 4, 9, 2, 7, 0, 5]):
            s, tol = _entropy_with_tolerance(op, n_sites, psi, sites)
            print("product state", np.dtype(dtype).char, sites, "S", s, "tolerance", tol)
            assert abs(s) <= tol
    finally:
        op.close()


def test_a_subsystem_and_its_complement_have_the_same_entropy(ctx):
    n_sites, dtype = 14, np.complex128
    psi = K.start_x(1 << n_sites, dtype, seed=5)
    sites = [0, 2, 3, 6, 9, 11, 12]
    rest = [s for s in range(n_sites) if s not in sites]
    op = L.PauliOperator(ctx, n_sites, [(0, 1, 1.0)], dtype)
    try:
        sa, ta = _entropy_with_tolerance(op, n_sites, psi, sites)
        sb, tb = _entropy_with_tolerance(op, n_sites, psi, rest)
        print("7 of 14 sites", sa, "their complement", sb, "tolerances", ta, tb)
        assert abs(sa - sb) <= ta + tb
    finally:
        op.close()


# ------------------------------------------------------------------ 4. the block route
@pytest.mark.parametrize("kind", ["momentum", "momentum_full", "symmetric"])
def test_block_state_through_expansion(ctx, kind):
    """block.reduced_density_matrix_tiled(c, sites, target) is expand, measure, free: the bits of the call on expand(c)."""
    n_sites, dtype, sites = 12, np.float64, [11, 0, 3, 5, 6, 8, 9]
    if kind == "momentum":
        terms = G.heisenberg_terms(n_sites, 1.0, 0.8, periodic=True)
        block, target = L.PauliMomentumOperator(ctx, n_sites, 6, 0, terms, dtype), L.PauliSectorOperator(ctx, n_sites, 6, terms, dtype)
    else:
        terms = G.tfim_terms(n_sites, 1.0, 0.7, periodic=True)
        target = L.PauliOperator(ctx, n_sites, terms, dtype)
        block = (L.PauliMomentumFullOperator(ctx, n_sites, 0, terms, dtype) if kind == "momentum_full"
                 else L.PauliSymmetricOperator(ctx, n_sites, 0, terms, dtype, parity=1))
    try:
        c = K.start_x(block.n_local, dtype, seed=11)
        got, nsw = block.reduced_density_matrix_tiled(c, sites, target, return_sweeps=True)
        direct = target.reduced_density_matrix_tiled(block.expand(c, target), sites)
        assert nsw == 1 and got.shape == (128, 128) and np.array_equal(got.view(np.uint8), direct.view(np.uint8))
        assert abs(np.trace(got).real - E.dot_exact(c, c)) <= 1e-12 * E.dot_exact(c, c)   # B is an isometry
    finally:
        block.close()
        target.close()


# ------------------------------------------------------------------ 5. refusals, each with its message
def test_refusals(ctx):
    n_sites = 6
    psi = K.start_x(1 << n_sites, np.float64)
    one = [(0, 1, 1.0)]
    csr = L.CsrOperator(ctx, *G.laplace2d_np(4))
    mom = L.PauliMomentumFullOperator(ctx, n_sites, 0, G.tfim_terms(n_sites, 1.0, 0.7, periodic=True), np.float64)
    sym = L.PauliSymmetricOperator(ctx, n_sites, 0, G.tfim_terms(n_sites, 1.0, 0.7, periodic=True), np.float64, parity=1)
    full = L.PauliOperator(ctx, n_sites, one, np.float64)
    big = L.PauliOperator(ctx, 15, one, np.float32)
    try:
        four = [0, 1, 2, 3]
        _refused(lambda: L.pauli_rdm_tiled(csr, K.start_x(csr.n_local, np.float64), four), "a CSR operator")
        _refused(lambda: L.pauli_rdm_tiled(mom, K.start_x(mom.n_local, np.float64), four), "a momentum block of the full space",
                 "symmetry blocks are not built", "expand")
        _refused(lambda: L.pauli_rdm_tiled(sym, K.start_x(sym.n_local, np.float64), four), "a momentum / reflection / spin-inversion block",
                 "expand")
        _refused(lambda: full.reduced_density_matrix_tiled(psi, [0, 1, 2]), "n_sub = 3", "4 to min(13")
        _refused(lambda: full.reduced_density_matrix_tiled(psi, [0, 1, 2, 3, 4, 5, 0]), "n_sub = 7", "n_sites = 6")
        _refused(lambda: big.reduced_density_matrix_tiled(K.start_x(1 << 15, np.float32), list(range(14))), "n_sub = 14")
        _refused(lambda: full.reduced_density_matrix_tiled(psi, [0, 6, 1, 2]), "site 1 of the list (6)", "outside [0, n_sites = 6)")
        _refused(lambda: full.reduced_density_matrix_tiled(psi, [2, 1, 0, 4, 1]), "site 4 of the list (1) is repeated")
        lib = capi.lib()
        sites = (C.c_int32 * 4)(0, 1, 2, 3)
        out = np.zeros(2 * 256)
        outp = capi.ptr(out)
        for args in ((None, full.handle, 4, sites, capi.ptr(psi), outp), (ctx.handle, None, 4, sites, capi.ptr(psi), outp),
                     (ctx.handle, full.handle, 4, None, capi.ptr(psi), outp), (ctx.handle, full.handle, 4, sites, None, outp),
                     (ctx.handle, full.handle, 4, sites, capi.ptr(psi), None)):
            st = lib.ll_pauli_rdm_tiled(*args, None)
            assert st == capi.LL_ERR_INVALID and b"null argument" in lib.ll_last_error(), args
        assert not np.any(out), "a refused call wrote its output"
        # the old entry point keeps its range, and the operator still answers after the refusals
        _refused(lambda: big.reduced_density_matrix(K.start_x(1 << 15, np.float32), [0, 1, 2, 3, 4, 5, 6]), "n_sub = 7")
        rho = full.reduced_density_matrix_tiled(psi, [3, 1, 5, 0])
        assert abs(np.trace(rho).real - E.dot_exact(psi, psi)) <= 16 * E.dot_bound(psi, psi)
    finally:
        for o in (csr, mom, sym, full, big):
            o.close()
