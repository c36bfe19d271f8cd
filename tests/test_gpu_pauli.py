"""The matrix-free sum-of-Pauli-strings operator (ll_op_create_pauli_*, csrc/pauli.hip): every apply against the EXACT host
reference of the expanded matrix (generators.pauli_csr, one entry per term and state) with the bounds the lattice operator is
held to, the same bits for every tile size, whole eigen-solver and Exponentiator runs against the reference library on the
expanded matrix, a 2^24-state ground state against a closed form, and the refusals."""
import ctypes as C
import json
import os
import subprocess
import sys
import time
import uuid

import numpy as np
import pytest

import contract_cases as K
import exact_ref as E
import lambda_lanczos_amd as L
from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G
from pauli_cases import TYPES, TYPE_IDS, WIDE, _checker, _cplx, _run_lanczos, _set_block_bits
from test_gpu_accuracy_contracts import OFFSETS, _check_spmv, _guarded, _unguard
from util import overlap

pytestmark = pytest.mark.gpu

TILE_BITS = [None, 6, 9]          # default (one tile holds every vector below), 64 and 512 states per tile
SITES = [1, 2, 3, 5, 6, 9, 11, 14]  # 2^1 .. 2^14 states: shorter than a tile, one tile, many tiles with remote groups


def j1j2_terms(n_sites, j1=1.0, j2=0.4):
    terms = G.heisenberg_terms(n_sites, j1, 0.7, periodic=False)
    for j in range(n_sites - 2):
        m = (1 << j) | (1 << (j + 2))
        terms += [(m, 0, 0.25 * j2), (m, m, 0.25 * j2), (0, m, 0.25 * j2)]
    return terms


def random_terms(n_sites, cplx, seed=5, count=40):
    """Mixed X / Y / Z strings, several terms per x mask, an identity term, duplicate terms; an even number of Y unless cplx."""
    rng = np.random.default_rng(seed + n_sites)
    full = (1 << n_sites) - 1
    xs = [int(rng.integers(0, full + 1)) for _ in range(6)] + [0, full]
    terms = [(0, 0, 0.75)]
    while len(terms) < count:
        x, z = xs[int(rng.integers(0, len(xs)))], int(rng.integers(0, full + 1))
        if not cplx and bin(x & z).count("1") & 1:
            continue
        terms.append((x, z, float(rng.uniform(-1, 1))))
    return terms + terms[3:6]


def model_terms(model, n_sites, cplx):
    if model == "heisenberg":
        return G.heisenberg_terms(n_sites, 1.0, 1.0, periodic=True)
    if model == "tfim":
        return G.tfim_terms(n_sites, 1.0, 1.5)
    if model == "j1j2":
        return j1j2_terms(n_sites)
    return random_terms(n_sites, cplx)


_REF = {}


def _reference_rows(model, n_sites, tid):
    key = (model, n_sites, tid)
    if key not in _REF:
        dtype = TYPES[TYPE_IDS.index(tid)]
        terms = model_terms(model, n_sites, _cplx(dtype))
        csr = G.pauli_csr(n_sites, terms, WIDE[tid], merge=False)   # coefficients are doubles for every T
        x = K.start_x(1 << n_sites, dtype)
        _REF[key] = (terms, csr, x, E.rows_exact(csr, x))
    return _REF[key]


# ------------------------------------------------------------------ 2. apply against the exact reference
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("model", ["heisenberg", "tfim", "j1j2", "random"])
def test_apply_meets_the_componentwise_contract(ctx, model, dtype):
    tid = TYPE_IDS[TYPES.index(dtype)]
    worst = (0.0, 0.0, 0.0)
    try:
        for n_sites in SITES:
            terms, csr, x, ex = _reference_rows(model, n_sites, tid)
            n = x.shape[0]
            op = L.PauliOperator(ctx, n_sites, terms, dtype)
            assert op.info() == (n, n, len(terms))
            for bits in TILE_BITS:
                _set_block_bits(ctx, "pauli", bits)
                for shift in (0, 1):
                    xb, xv = _guarded(ctx, x, shift)
                    yb, yv = _guarded(ctx, np.zeros(n, dtype), shift)
                    for offset in OFFSETS:
                        alpha = L.spmv(op, xv, yv, offset=offset, want_dot=True)
                        y = _unguard(yb, n, shift).copy()
                        assert np.array_equal(_unguard(xb, n, shift), x), "the apply changed its input"
                        # the lattice operator's checks: products formed exactly in double, floating-point sums
                        r = _check_spmv("pauli", "stencil", False, dtype, csr, x, ex, ex, y, alpha, offset)
                        worst = tuple(max(a, b) for a, b in zip(worst, r))
                    xb.free()
                    yb.free()
            op.close()
    finally:
        _set_block_bits(ctx, "pauli", None)
    print("ratios error/bound (class, storage, alpha)", model, tid, worst)


# ------------------------------------------------------------------ 3. the same bits for every geometry
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_same_bits_for_every_tile_size_and_alignment(ctx, dtype):
    tid = TYPE_IDS[TYPES.index(dtype)]
    try:
        for model, n_sites in [("heisenberg", 14), ("random", 11), ("j1j2", 5)]:
            terms, _, x, _ = _reference_rows(model, n_sites, tid)
            n = x.shape[0]
            op = L.PauliOperator(ctx, n_sites, terms, dtype)
            first = None
            for bits in [None, 0, 1, 2, 6, 9, 12]:
                _set_block_bits(ctx, "pauli", bits)
                for shift in (0, 1):
                    for rep in range(2):
                        xb, xv = _guarded(ctx, x, shift)
                        yb, yv = _guarded(ctx, np.zeros(n, dtype), shift)
                        L.spmv(op, xv, yv, offset=-2.5, want_dot=False)
                        y = _unguard(yb, n, shift).copy()
                        xb.free()
                        yb.free()
                        if first is None:
                            first = y
                        assert np.array_equal(first.view(np.uint8), y.view(np.uint8)), (model, bits, shift, rep)
            op.close()
    finally:
        _set_block_bits(ctx, "pauli", None)


def test_deferred_normalisation_path_against_separate_launches(ctx):
    """fuse_launches = 1: the loop hands the kernel the unnormalised vector and the kernel normalises it on the fly, writes u_k
    and publishes the iteration's scalars (ScaleIn); 2 (default): the one-sweep Gram-Schmidt forms hand it ||w||^2; 0: the
    vector is normalised by a launch of its own.  Runs to the default stop on the open transverse-field chain (a
    non-degenerate ground state with a gap of 2 (h - J)); traces to the tolerance of DESIGN.md section 4 (1e-10 |A|_inf per k)."""
    n_sites = 12
    terms = G.tfim_terms(n_sites, 1.0, 1.5)
    n = 1 << n_sites
    init = G.start_vector(n, 1)
    op = L.PauliOperator(ctx, n_sites, terms)
    norm = op.inf_norm()
    runs = {}
    try:
        ctx.set_tuning("pauli_tile_bits", "9")
        for level in ("0", "1", "2"):
            ctx.set_tuning("fuse_launches", level)
            eng, vals, _ = _run_lanczos(op, n, init, False, -norm)
            runs[level] = (eng.last_alpha, eng.last_beta, vals[0], eng.getIterationCounts())
    finally:
        ctx.set_tuning("fuse_launches", None)      # (remove the settings: an override left behind would outrank the environment)
        ctx.set_tuning("pauli_tile_bits", None)
    op.close()
    base = runs["0"]
    for level in ("1", "2"):
        r = runs[level]
        k = min(len(r[0]), len(base[0]))
        da, db = np.max(np.abs(r[0][:k] - base[0][:k])), np.max(np.abs(r[1][:k] - base[1][:k]))
        print("fuse_launches %s against 0: %s / %s iterations, max |d alpha| = %.3e, max |d beta| = %.3e, |d lambda| = %.3e"
              % (level, r[3], base[3], da, db, abs(r[2] - base[2])))
    for level in ("1", "2"):
        r = runs[level]
        k = min(len(r[0]), len(base[0]))
        assert abs(r[3][0] - base[3][0]) <= 2 and k >= 50
        assert np.max(np.abs(r[0][:k] - base[0][:k])) <= 1e-10 * norm
        assert np.max(np.abs(r[1][:k] - base[1][:k])) <= 1e-10 * norm
        assert abs(r[2] - base[2]) <= 1e-10 * max(1.0, abs(base[2] - norm))


# ------------------------------------------------------------------ 4. whole runs against the real reference
Y_TERMS = [(0b11, 0b01, 0.35), (0b110, 0b100, -0.2), (1 << 13 | 1, 1 << 13, 0.45), (1 << 7, 1 << 7, 0.3)]   # odd numbers of Y


@pytest.mark.parametrize("find_max", [False, True], ids=["smallest", "largest"])
@pytest.mark.parametrize("model", ["heisenberg", "tfim"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["d", "s"])
def test_lanczos_against_the_reference(ctx, model, dtype, find_max):
    n_sites = 14
    n = 1 << n_sites
    terms = model_terms(model, n_sites, False)
    csr = G.pauli_csr(n_sites, terms, np.float64)
    single = np.dtype(dtype) == np.float32
    init = G.start_vector(n, 1).astype(dtype)
    op = L.PauliOperator(ctx, n_sites, terms, dtype)
    norm = op.inf_norm()
    assert abs(norm - sum(abs(c) for _, _, c in terms)) <= 1e-12 * norm
    offset = norm if find_max else -norm
    eng, vals, vecs = _run_lanczos(op, n, init, find_max, offset)
    ref = _checker().lanczos(csr, init.astype(np.float64), find_max, offset=offset, eps=eng.eps)
    scale = max(1.0, abs(ref["eigenvalues"][0] + offset))
    if single:   # the float rules of tests/test_gpu_float.py
        assert abs(vals[0] - ref["eigenvalues"][0]) <= 20 * eng.eps * scale
    else:
        assert abs(vals[0] - ref["eigenvalues"][0]) <= 1e-10 * scale
        assert abs(eng.getIterationCounts()[0] - ref["iter_counts"][0]) <= 2
        r = np.linalg.norm(_spmv_csr(csr, vecs[0]) - vals[0] * vecs[0])
        assert r <= 1e-5 * norm
        if model == "tfim":
            # traces and eigenvectors on the chain only: the ring's largest eigenvalue is the (L + 1)-fold ferromagnetic multiplet
            # and its smallest sits in a spectrum of SU(2) multiplets, so once the first copy has converged the recurrence is
            # driven by the copies that rounding regenerates (no two summation orders share those), and any vector of the
            # multiplet is an eigenvector: there the eigenvalue, the iteration count and the residual are the checks
            k = min(len(eng.last_alpha), len(ref["alpha"]))
            assert np.max(np.abs(eng.last_alpha[:k] - ref["alpha"][:k])) <= 1e-10 * norm
            assert 1 - overlap(vecs[0], ref["eigenvectors"][0]) <= 1e-8
    op.close()


def _spmv_csr(csr, x):
    rp, ci, va = csr
    return np.add.reduceat(va * x[ci], rp[:-1]) if rp[-1] else np.zeros_like(x)


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64], ids=["z", "c"])
def test_lanczos_with_y_terms_and_two_roots(ctx, dtype):
    """A Hamiltonian with odd numbers of Y (a complex Hermitian matrix): smallest pair, then two roots with a restart pass."""
    n_sites = 14
    n = 1 << n_sites
    terms = G.tfim_terms(n_sites, 1.0, 1.5) + Y_TERMS
    csr = G.pauli_csr(n_sites, terms, np.complex128)
    single = np.dtype(dtype) == np.complex64
    init = G.start_vector(n, 1, np.complex128).astype(dtype)
    op = L.PauliOperator(ctx, n_sites, terms, dtype)
    norm = op.inf_norm()
    for num_eigs in (1, 2):
        eng, vals, vecs = _run_lanczos(op, n, init, False, -norm, num_eigs=num_eigs)
        ref = _checker().lanczos(csr, init.astype(np.complex128), False, num_eigs=num_eigs, offset=-norm, eps=eng.eps)
        scale = max(1.0, np.max(np.abs(ref["eigenvalues"] - norm)))
        tol = 20 * eng.eps * scale if single else 1e-10 * scale
        assert len(vals) == num_eigs and np.max(np.abs(vals - ref["eigenvalues"])) <= tol
        assert 1 - overlap(vecs[0].astype(np.complex128), ref["eigenvectors"][0]) <= (1e-3 if single else 1e-8)
        if num_eigs == 2:
            assert len(eng.getIterationCounts()) >= 2     # the second root took a pass of its own
    op.close()


@pytest.mark.parametrize("full_orth", [False, True], ids=["three_term", "full_orthogonalize"])
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64], ids=["z", "c"])
def test_exponentiator_against_the_reference(ctx, dtype, full_orth):
    n_sites = 14
    n = 1 << n_sites
    terms = G.heisenberg_terms(n_sites, 1.0, 0.8) + Y_TERMS
    csr = G.pauli_csr(n_sites, terms, np.complex128)
    single = np.dtype(dtype) == np.complex64
    inp = G.start_vector(n, 2, np.complex128).astype(dtype)
    a = -0.05j
    op = L.PauliOperator(ctx, n_sites, terms, dtype)
    ex = L.Exponentiator(op, n)
    ex.full_orthogonalize = full_orth
    out, it = ex.run(a, inp)
    o_out, o_it, _ = _checker().expo(csr, a, inp.astype(np.complex128), eps=ex.eps, full_orthogonalize=full_orth)
    assert abs(it - o_it) <= 2
    if single:
        assert np.linalg.norm(out - o_out) <= 1e-3 * np.linalg.norm(o_out)
    else:
        assert 1 - overlap(out, o_out) <= 10 * ex.eps
        assert abs(np.linalg.norm(out) / np.linalg.norm(inp) - 1) <= 1e-12
        assert np.max(np.abs(out - o_out)) <= 1e-10 * np.linalg.norm(inp)
    t_out, _ = ex.taylor_run(a, inp)
    r_out, _, _ = _checker().expo(csr, a, inp.astype(np.complex128), eps=ex.eps, taylor=True)   # the reference's own Taylor sum
    assert np.linalg.norm(t_out - r_out) <= (1e-3 if single else 1e-10) * np.linalg.norm(r_out)
    op.close()


# ------------------------------------------------------------------ 5. a size no CSR test reaches
def test_tfim_ground_state_on_2_to_24_states(ctx):
    """Open transverse-field Ising chain, L = 24, J = 1, h = 1.5 (n = 16 777 216): the ground-state energy against the free-fermion
    closed form -sum of the singular values of the L x L bidiagonal matrix (h on the diagonal, J above it), which does not depend
    on the code under test, to 1e-10 |E0| (the project's eigenvalue tolerance).  eigenvalue_offset = -sum |coef|, default eps,
    max_iteration = 300.  With exactly these settings the REFERENCE library, run on the CPU on the expanded matrix of the same
    model, met the tolerance at L = 12 after 87 iterations (relative error 1.3e-15) and at L = 14 after 97 (4.6e-15).
    The CSR image of this matrix would hold >= 12 * 25 * 2^24 B = 5 GB; the operator holds its term tables."""
    n_sites, J, h = 24, 1.0, 1.5
    n = 1 << n_sites
    terms = G.tfim_terms(n_sites, J, h)
    e0 = G.tfim_ground_energy(n_sites, J, h)
    op = L.PauliOperator(ctx, n_sites, terms)
    assert op.device_bytes() < (1 << 20)
    init = G.start_vector_fast(n, 1)
    t0 = time.time()
    eng, vals, vecs = _run_lanczos(op, n, init, False, -op.inf_norm(), max_iteration=300)
    dt = time.time() - t0
    its = eng.getIterationCounts()[0]
    v = ctx.to_device(vecs[0])
    hv = ctx.empty(n, np.float64)
    L.spmv(op, v, hv, offset=0.0)
    res = np.linalg.norm(hv.get() - vals[0] * vecs[0])
    v.free()
    hv.free()
    op.close()
    ctx.release_cache()
    print("TFIM L=24: E0 = %.13f (closed form %.13f), %d iterations, %.2f s (%.1f it/s), residual |Hv - lambda v| = %.3e"
          % (vals[0], e0, its, dt, its / dt, res))
    assert abs(vals[0] - e0) <= 1e-10 * abs(e0)
    assert its < 300


# ------------------------------------------------------------------ 6. refusals
def _create_raw(ctx, sfx, n_sites, n_terms, terms, out=True):
    arr = None
    if terms is not None:
        arr = (capi.PauliTerm * max(len(terms), 1))()
        for k, (x, z, c) in enumerate(terms):
            arr[k].x_mask, arr[k].z_mask, arr[k].coef = x, z, c
    h = C.c_void_p()
    code = getattr(capi.lib(), "ll_op_create_pauli_" + sfx)(ctx.handle, n_sites, n_terms, arr, C.byref(h) if out else None)
    msg = capi.lib().ll_last_error().decode() if code else ""
    if code == 0 and out:
        capi.lib().ll_op_destroy(h)
    return code, msg


@pytest.mark.parametrize("sfx", TYPE_IDS)
def test_invalid_inputs_are_refused_with_their_cause(ctx, sfx):
    ok = [(1, 0, 1.0)]
    INVALID = capi.LL_ERR_INVALID if hasattr(capi, "LL_ERR_INVALID") else 1
    for n_sites in (0, -3, 31, 64):
        code, msg = _create_raw(ctx, sfx, n_sites, 1, ok)
        assert code == INVALID and "n_sites" in msg, (n_sites, code, msg)
    code, msg = _create_raw(ctx, sfx, 4, 2, [(1, 0, 1.0), (1 << 4, 0, 1.0)])
    assert code == INVALID and "term 1" in msg and "mask bit" in msg, msg
    code, msg = _create_raw(ctx, sfx, 4, 1, [(0, 1 << 40, 1.0)])
    assert code == INVALID and "mask bit" in msg, msg
    for bad in (float("nan"), float("inf")):
        code, msg = _create_raw(ctx, sfx, 4, 1, [(1, 0, bad)])
        assert code == INVALID and "not finite" in msg, msg
    code, msg = _create_raw(ctx, sfx, 4, -1, ok)
    assert code == INVALID and "n_terms" in msg, msg
    code, msg = _create_raw(ctx, sfx, 4, 1, None)
    assert code == INVALID and "null" in msg, msg
    code, msg = _create_raw(ctx, sfx, 4, 1, ok, out=False)
    assert code == INVALID and "null" in msg, msg
    code, msg = _create_raw(ctx, sfx, 4, 1, [(0b11, 0b01, 1.0)])     # X0 ... Y: one Y
    if sfx in ("d", "s"):
        assert code == INVALID and "odd number of Y" in msg, msg
    else:
        assert code == 0, msg
    code, msg = _create_raw(ctx, sfx, 30, 1, ok)                       # the largest n_sites: only the tables are allocated
    assert code == 0, msg


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_zero_identity_and_duplicate_terms(ctx, dtype):
    n_sites, n = 7, 128
    x = K.start_x(n, dtype)
    xd, yd = ctx.to_device(x), ctx.empty(n, dtype)
    op = L.PauliOperator(ctx, n_sites, [], dtype)                      # no term: the zero operator
    assert op.info() == (n, n, 0) and op.inf_norm() == 0.0
    L.spmv(op, xd, yd, offset=0.0)
    assert np.all(yd.get() == 0)
    op.close()
    op = L.PauliOperator(ctx, n_sites, [(0, 0, 0.5), (0, 0, 0.25)], dtype)   # identity terms, duplicates add
    assert op.inf_norm() == 0.75
    L.spmv(op, xd, yd, offset=0.0)
    assert np.array_equal(yd.get(), (0.75 * x.astype(WIDE[TYPE_IDS[TYPES.index(dtype)]])).astype(dtype))
    with pytest.raises(capi.LanczosHipError):
        op_sel = L.CsrOperator.select_spmv(op, capi.SPMV_CSR_STREAM)   # noqa: F841 - not a CSR operator, like the lattice operator
    with pytest.raises(capi.LanczosHipError):
        L.CsrOperator.set_accuracy(op, capi.ACCURACY_NORMWISE)
    assert L.CsrOperator.accuracy(op) == capi.ACCURACY_COMPONENTWISE
    assert 0 < op.device_bytes() < 4096
    op.close()
    xd.free()
    yd.free()


def test_refused_on_a_sharded_context(tmp_path):
    """Two ranks on the box's GPU over the test transport: the operator is single-GPU."""
    from conftest import SHM_TRANSPORT

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name = "/ll_shm_pauli_" + uuid.uuid4().hex[:12]
    env = dict(os.environ, LL_COMM_PLUGIN=SHM_TRANSPORT, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(root, "tests", "shm_pauli_worker.py"), str(r), "2", name, str(tmp_path)],
                              env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-4000:]
    for r in range(2):
        res = json.load(open(os.path.join(tmp_path, "rank%d.json" % r)))
        assert res["code"] == capi.LL_ERR_INVALID and "sharded" in res["msg"], res
