"""Reduced density matrices of up to six sites in one sweep over a state (ll_pauli_rdm, csrc/pauli_rdm.hip, planned by
csrc/pauli_rdm_plan.hpp): every part of every entry against the EXACT host reference — rho[a][a'] = <f_a', f_a> of the two fibres
f_a = psi(a, .) (generators.reduced_density_matrix_np), correctly rounded (exact_ref.dot_exact) — at the project's bound for a
double-accumulated dot (exact_ref.dot_bound, which a float accumulation fails) plus one double rounding; in all four storage
types, on the full space with the subsystem sites below, across and above the tile, on S_z sectors with one and with many batches;
psi in guarded, NaN-padded device buffers at two alignments and on the host (the same bits), the exact Hermitian mirror and the
exact zeros, a cross-check against tomography through ll_pauli_expect, entropies of states with known answers, and the refusals."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import contract_cases as K
import exact_ref as E
import lambda_lanczos_amd as L
from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G
from guarded import guarded as _guarded, unguard as _unguard

pytestmark = pytest.mark.gpu

TYPES = [np.float64, np.complex128, np.float32, np.complex64]
TYPE_IDS = ["d", "z", "s", "c"]
NAN_FILL = 0xFF          # every byte 0xFF: a NaN in all four storage types
FULL_CASES = [(1, [0]), (2, [1]), (3, [0, 2]), (5, [4, 0, 2]), (6, [0, 1, 2, 3, 4, 5]), (9, [0]), (9, [8]), (9, [3, 4, 5, 6]),
              (11, [0, 1, 2, 3, 4, 5]), (11, [10, 9, 8, 7, 6, 5]), (14, [0, 13]), (14, [1, 4, 6, 9, 12]),
              (14, [2, 3, 5, 7, 11, 13])]
TILE_BITS = [None, 6, 9]   # default (the whole vector up to 32 KiB); 64 and 512 states per tile: sites below, across, above
SECTORS = [(6, 0), (6, 6), (9, 4), (12, 6), (13, 4), (14, 7)]
BLOCK_BITS = [None, 4, 7]  # default (what fills 32 KiB); 16 and 128 environment configurations per batch


def sector_site_lists(n_sites):
    """[0], [n - 1], [0, 1, 2], a scattered 4-list and a 6-list (unsorted, the top site included)."""
    n = n_sites
    four = [n - 2, 1, n // 2, 3] if n > 6 else [4, 1, 3, 0]
    six = [0, n - 1, 2, n // 2 + 1, 1, n - 3] if n > 6 else [5, 0, 3, 1, 4, 2]
    assert len(set(four)) == 4 and len(set(six)) == 6
    return [[0], [n - 1], [0, 1, 2], four, six]


def _cplx(dtype):
    return np.dtype(dtype).kind == "c"


def _popc(a):
    return bin(a).count("1")


_REF = {}


def reference(n_sites, n_down, sites, dtype):
    """(psi, want, bound): want[a][a'] = dot_exact(f_a', f_a), bound[a][a'] on each part = dot_bound of the two fibres plus one
    double rounding; computed once per case and storage type for a <= a', mirrored, and left unchanged."""
    key = (n_sites, n_down, tuple(sites), np.dtype(dtype).char)
    if key not in _REF:
        states = None if n_down is None else G.sector_states(n_sites, n_down)
        n = (1 << n_sites) if states is None else states.shape[0]
        psi = K.start_x(n, dtype)
        _, fib = G.reduced_density_matrix_np(n_sites, sites, psi, states=states)
        dim = 1 << len(sites)
        want, bound = np.zeros((dim, dim), np.complex128), np.zeros((dim, dim))
        for a in range(dim):
            for ap in range(a, dim):
                if n_down is not None and _popc(a) != _popc(ap):
                    continue   # exactly zero by rule: want = 0, bound = 0
                w = complex(E.dot_exact(fib[ap], fib[a]))
                b = E.dot_bound(fib[ap], fib[a])
                want[a, ap], want[ap, a] = w, w.conjugate()
                bound[a, ap] = bound[ap, a] = b + E.EPS_D * max(abs(w.real), abs(w.imag))
        psi.setflags(write=False)
        _REF[key] = (psi, want, bound)
    return _REF[key]


def check_rho(got, want, bound, dtype, n_down, what):
    """Every part within its bound; Hermitian bit for bit; the exact zeros.  Returns the worst error / bound."""
    dim = got.shape[0]
    assert got.dtype == np.complex128 and got.shape == want.shape, what
    assert np.all(np.isfinite(got.real)) and np.all(np.isfinite(got.imag)), (what, "a value is not finite: the kernel read past psi")
    re, im = np.ascontiguousarray(got.real), np.ascontiguousarray(got.imag)
    # Hermitian: the real parts have the same bits, the imaginary parts are each other's negation and every zero is +0.0
    assert np.array_equal(re.view(np.uint64), re.T.copy().view(np.uint64)), (what, "real parts are not mirrored bit for bit")
    assert np.array_equal(im, -im.T), (what, "imaginary parts are not mirrored")
    assert not np.any(np.signbit(im[im == 0.0])) and not np.any(np.signbit(re[re == 0.0])), (what, "a zero is -0.0")
    assert not np.any(im.diagonal().view(np.uint64)), (what, "the diagonal has an imaginary part")
    if not _cplx(dtype):
        assert not np.any(im.view(np.uint64)), (what, "real storage with an imaginary part")
    if n_down is not None:
        pc = np.array([_popc(a) for a in range(dim)])
        off = pc[:, None] != pc[None, :]
        assert not np.any(re[off].view(np.uint64)) and not np.any(im[off].view(np.uint64)), (what, "popcount-off-diagonal entry")
    err = np.maximum(np.abs(re - want.real), np.abs(im - want.imag))
    j = np.unravel_index(int(np.argmax(err - bound)), err.shape)
    assert np.all(err <= bound), (what, j, got[j], want[j], bound[j])
    return float(np.max(err / np.maximum(bound, 1e-300)))


def measure_everywhere(ctx, op, psi, sites, want, bound, dtype, n_down, what):
    """psi in guarded, NaN-padded device buffers at shift 0 and 1 and on the host: every entry within its bound, psi unchanged,
    one sweep, the same bits for every placement and from call to call.  Returns the worst error / bound."""
    n = psi.shape[0]
    first, worst = None, 0.0
    for shift in (0, 1):
        buf, view = _guarded(ctx, psi, shift, NAN_FILL)
        for rep in range(2):
            got, nsw = op.reduced_density_matrix(view, sites, return_sweeps=True)
            assert nsw == 1, (what, shift, nsw)
            worst = max(worst, check_rho(got, want, bound, dtype, n_down, (what, "device", shift)))
            if first is None:
                first = got
            assert np.array_equal(first.view(np.uint8), got.view(np.uint8)), (what, "device", shift, rep)
        assert np.array_equal(_unguard(buf, n, shift, NAN_FILL), psi), "the measurement changed psi"
        buf.free()
    got, nsw = op.reduced_density_matrix(psi, sites, return_sweeps=True)
    assert nsw == 1 and np.array_equal(first.view(np.uint8), got.view(np.uint8)), (what, "host psi")
    return worst


# ------------------------------------------------------------------ 1. the full space
@pytest.mark.parametrize("n_sites,sites", FULL_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_full_space_against_the_exact_reference(ctx, dtype, n_sites, sites):
    psi, want, bound = reference(n_sites, None, sites, dtype)
    op = L.PauliOperator(ctx, n_sites, G.tfim_terms(n_sites, 1.0, 0.7), dtype)   # the Hamiltonian's terms play no part
    worst = 0.0
    try:
        for bits in TILE_BITS:
            ctx.set_tuning("pauli_rdm_tile_bits", None if bits is None else str(bits))
            worst = max(worst, measure_everywhere(ctx, op, psi, sites, want, bound, dtype, None, (n_sites, sites, bits)))
    finally:
        ctx.set_tuning("pauli_rdm_tile_bits", None)
        op.close()
    print("worst error / bound", np.dtype(dtype).char, n_sites, sites, worst)


# ------------------------------------------------------------------ 2. S_z sectors
@pytest.mark.parametrize("n_sites,n_down", SECTORS)
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_sector_against_the_exact_reference(ctx, dtype, n_sites, n_down):
    op = L.PauliSectorOperator(ctx, n_sites, n_down, G.heisenberg_terms(n_sites, 1.0, 0.8, periodic=False), dtype)
    worst = 0.0
    try:
        for sites in sector_site_lists(n_sites):
            psi, want, bound = reference(n_sites, n_down, sites, dtype)
            assert op.n_local == psi.shape[0] == math.comb(n_sites, n_down)
            for bits in BLOCK_BITS:
                ctx.set_tuning("pauli_rdm_block_bits", None if bits is None else str(bits))
                worst = max(worst, measure_everywhere(ctx, op, psi, sites, want, bound, dtype, n_down, (n_sites, n_down, sites, bits)))
            if psi.shape[0] == 1:   # one state: one non-zero entry, |psi_0|^2, at the a that the state's bits spell
                got = op.reduced_density_matrix(psi, sites)
                a = sum(1 << k for k in range(len(sites)) if n_down == n_sites)
                assert np.count_nonzero(got) == 1 and got[a, a].imag == 0.0 and got[a, a].real > 0.0
    finally:
        ctx.set_tuning("pauli_rdm_block_bits", None)
        op.close()
    print("worst error / bound", np.dtype(dtype).char, (n_sites, n_down), worst)


# ------------------------------------------------------------------ 3. against the existing kernel: tomography
PAULI = {"I": np.eye(2, dtype=np.complex128), "X": np.array([[0, 1], [1, 0]], np.complex128),
         "Y": np.array([[0, -1j], [1j, 0]], np.complex128), "Z": np.array([[1, 0], [0, -1]], np.complex128)}


@pytest.mark.parametrize("n_sites,n_down,sites", [(10, None, [7, 2, 4]), (12, 6, [9, 3])], ids=["full", "sector"])
def test_tomography_through_the_expectation_kernel(ctx, n_sites, n_down, sites):
    """rho = 2^-m sum_P <P> P with the 4^m strings measured by op.expectation (Re <P> is all a Hermitian P has); both routes
    carry their own bound: sum_P dot_bound(psi, P psi) / 2^m for the reconstruction, the fibre bounds for the direct kernel."""
    dtype = np.complex128
    m = len(sites)
    psi, want, bound = reference(n_sites, n_down, sites, dtype)
    states = None if n_down is None else G.sector_states(n_sites, n_down)
    if n_down is None:
        op = L.PauliOperator(ctx, n_sites, G.tfim_terms(n_sites, 1.0, 0.7), dtype)
    else:
        op = L.PauliSectorOperator(ctx, n_sites, n_down, G.heisenberg_terms(n_sites, 1.0, 0.8, periodic=False), dtype)
    strings, mats = [], []
    for letters in itertools.product("IXYZ", repeat=m):
        x = sum(1 << s for s, c in zip(sites, letters) if c in "XY")
        z = sum(1 << s for s, c in zip(sites, letters) if c in "YZ")
        strings.append((x, z, 1.0))
        mat = np.eye(1, dtype=np.complex128)
        for c in reversed(letters):   # bit k of a is sites[k]: the last letter is the most significant factor
            mat = np.kron(mat, PAULI[c])
        mats.append(mat)
    try:
        vals = op.expectation(psi, strings)
        rho = op.reduced_density_matrix(psi, sites)
    finally:
        op.close()
    tomo = sum(v * mat for v, mat in zip(vals, mats)) / (1 << m)
    tb = sum(E.dot_bound(psi, G.pauli_string_apply_np(n_sites, t, psi, states=states)) + E.EPS_D * abs(v)
             for t, v in zip(strings, vals)) / (1 << m) + 4 ** m * E.EPS_D * float(np.max(np.abs(vals)))   # + the host's sum
    err = np.maximum(np.abs(rho.real - tomo.real), np.abs(rho.imag - tomo.imag))
    print("tomography: worst difference", float(err.max()), "bounds", tb, float(bound.max()))
    assert np.all(err <= tb + bound)


# ------------------------------------------------------------------ 4. physics: states built on the host, exact entropies
def _eta(x):
    return -x * math.log(x) if x > 0.0 else 0.0


def _entropy_with_tolerance(op, n_sites, states, psi, sites):
    """(S, tolerance, rho): eigenvalues of rho / tr rho move by at most delta = ||entry bounds||_F / tr rho (Weyl), and
    |eta(x) - eta(y)| <= eta(|x - y|) for |x - y| <= 1/2: 2^m eta(delta)."""
    m = len(sites)
    rho = op.reduced_density_matrix(psi, sites)
    _, fib = G.reduced_density_matrix_np(n_sites, sites, psi, states=states)
    parts = 2 if np.iscomplexobj(psi) else 1
    b2 = sum(parts * E.dot_bound(fib[ap], fib[a]) ** 2 for a in range(1 << m) for ap in range(1 << m))
    nn = E.dot_exact(psi, psi).real
    assert abs(np.trace(rho).real - nn) <= E.dot_bound(psi, psi), "tr rho != ||psi||^2"
    delta = math.sqrt(b2) / nn
    assert delta <= 0.5
    return L.entanglement_entropy(rho), (1 << m) * _eta(delta), rho


@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=["d", "z"])
def test_product_state_has_no_entanglement(ctx, dtype):
    n_sites = 10
    rng = np.random.default_rng(11)
    psi = np.ones(1, dtype)
    for _ in range(n_sites):
        v = rng.uniform(-1, 1, 2) + (1j * rng.uniform(-1, 1, 2) if _cplx(dtype) else 0.0)
        psi = np.kron(v.astype(dtype), psi)
    op = L.PauliOperator(ctx, n_sites, [(0, 1, 1.0)], dtype)
    try:
        for sites in ([0], [9, 4], [1, 2, 3], [0, 2, 4, 6, 8, 9]):
            s, tol, _ = _entropy_with_tolerance(op, n_sites, None, psi, sites)
            print("product state", np.dtype(dtype).char, sites, "S", s, "tolerance", tol)
            assert abs(s) <= tol
    finally:
        op.close()


@pytest.mark.parametrize("sector", [False, True], ids=["full", "sector"])
def test_chain_of_singlets(ctx, sector):
    """(|01> - |10>) / sqrt 2 on (0,1), (2,3), ...: a block's entropy is ln 2 per singlet that it cuts."""
    n_sites, ln2 = 12, math.log(2.0)
    pair = np.array([0.0, 1.0, -1.0, 0.0]) / math.sqrt(2.0)   # index = bit(site 2j) + 2 bit(site 2j + 1)
    psi = np.ones(1)
    for _ in range(n_sites // 2):
        psi = np.kron(pair, psi)
    states = G.sector_states(n_sites, n_sites // 2) if sector else None
    if sector:
        assert np.count_nonzero(psi) == np.count_nonzero(psi[states])   # the state lies in the sector
        psi = np.ascontiguousarray(psi[states])
        op = L.PauliSectorOperator(ctx, n_sites, n_sites // 2, G.heisenberg_terms(n_sites, 1.0, 1.0, periodic=False), np.float64)
    else:
        op = L.PauliOperator(ctx, n_sites, [(0, 1, 1.0)], np.float64)
    try:
        for sites, want in (([0], ln2), ([0, 1], 0.0), ([1, 2], 2 * ln2), ([0, 2, 4, 6, 8, 10], 6 * ln2)):
            s, tol, rho = _entropy_with_tolerance(op, n_sites, states, psi, sites)
            print("singlets", "sector" if sector else "full", sites, "S", s, "exact", want, "tolerance", tol)
            assert abs(s - want) <= tol
    finally:
        op.close()


# ------------------------------------------------------------------ 5. refusals, each with its message
def _refused(fn, *needles):
    with pytest.raises(L.LanczosHipError) as e:
        fn()
    assert e.value.code == capi.LL_ERR_INVALID, str(e.value)
    for needle in needles:
        assert needle in str(e.value), (needle, str(e.value))


def test_refusals(ctx):
    n_sites = 4
    psi = K.start_x(16, np.float64)
    one = [(0, 1, 1.0)]
    csr = L.CsrOperator(ctx, *G.laplace2d_np(4))
    mom = L.PauliMomentumFullOperator(ctx, n_sites, 0, G.tfim_terms(n_sites, 1.0, 0.7, periodic=True), np.float64)
    sym = L.PauliSymmetricOperator(ctx, n_sites, 0, G.tfim_terms(n_sites, 1.0, 0.7, periodic=True), np.float64, parity=1)
    full = L.PauliOperator(ctx, n_sites, one, np.float64)
    big = L.PauliOperator(ctx, 8, one, np.float64)
    ctx2 = L.Context(0)
    ctx2.init_comm(L.Context.unique_id(), 0, 1)
    shard = L.PauliOperator(ctx2, n_sites, one, np.float64)
    try:
        _refused(lambda: L.pauli_rdm(csr, psi, [0]), "a CSR operator")
        _refused(lambda: L.pauli_rdm(mom, K.start_x(mom.n_local, np.float64), [0]), "a momentum block of the full space",
                 "symmetry blocks are not built")
        _refused(lambda: L.pauli_rdm(sym, K.start_x(sym.n_local, np.float64), [0]), "a momentum / reflection / spin-inversion block")
        _refused(lambda: shard.reduced_density_matrix(psi, [0]), "a context with a communicator")
        _refused(lambda: full.reduced_density_matrix(psi, []), "n_sub = 0")
        _refused(lambda: full.reduced_density_matrix(psi, [0, 1, 2, 3, 0]), "n_sub = 5", "n_sites = 4")
        _refused(lambda: big.reduced_density_matrix(K.start_x(256, np.float64), [0, 1, 2, 3, 4, 5, 6]), "n_sub = 7")
        _refused(lambda: full.reduced_density_matrix(psi, [0, 4]), "site 1 of the list (4)", "outside [0, n_sites = 4)")
        _refused(lambda: full.reduced_density_matrix(psi, [-1]), "site 0 of the list (-1)", "outside")
        _refused(lambda: full.reduced_density_matrix(psi, [2, 1, 2]), "site 2 of the list (2) is repeated")
        lib = capi.lib()
        sites = (C.c_int32 * 1)(0)
        out = np.zeros(8)
        outp = out.ctypes.data_as(C.POINTER(C.c_double))
        for args in ((None, full.handle, 1, sites, capi.ptr(psi), outp), (ctx.handle, None, 1, sites, capi.ptr(psi), outp),
                     (ctx.handle, full.handle, 1, None, capi.ptr(psi), outp), (ctx.handle, full.handle, 1, sites, None, outp),
                     (ctx.handle, full.handle, 1, sites, capi.ptr(psi), None)):
            st = lib.ll_pauli_rdm(*args, None)
            assert st == capi.LL_ERR_INVALID and b"null argument" in lib.ll_last_error(), args
        # the operator still answers after the refusals
        rho = full.reduced_density_matrix(psi, [3, 1])
        assert abs(np.trace(rho).real - E.dot_exact(psi, psi)) <= 4 * E.dot_bound(psi, psi)
    finally:
        for o in (csr, mom, sym, full, big, shard):
            o.close()
        ctx2.close()
