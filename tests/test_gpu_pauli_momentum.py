"""The sum-of-Pauli-strings operator on one momentum block of an S_z sector of a ring (ll_op_create_pauli_momentum_*,
csrc/pauli_momentum.hip): every apply against the EXACT host reference of the block B^H H_sector B (generators.pauli_momentum_csr,
one entry per term and state) with the component-wise class, the same bits for every block size and alignment, consistency with
the sector operator through the embedding B, whole eigen-solver and Exponentiator runs against the reference library on the
block's matrix, and the refusals.

The single-type storage-product contract of the CSR kernels is NOT asserted here: an entry of the block is a weight times
sqrt(R_a / R_b) times a phase, formed in double, and in general no number of the storage type (lanczos_hip.h (8), ACCURACY)."""
import json
import math
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import contract_cases as K
import exact_ref as E
import lambda_lanczos_amd as L
from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G
from pauli_cases import (TYPES, TYPE_IDS, WIDE, _apply, _check_apply, _checker, _class_bound, _cplx, _run_lanczos, _runs,
                         _set_block_bits, _tid, dm_ring)
from test_gpu_accuracy_contracts import OFFSETS, _eps
from util import overlap

pytestmark = pytest.mark.gpu

BLOCK_BITS = [None, 4, 8, 10]      # default, 16, 256 and 1024 indices per block (1024: four states per lane; D_m = 2704 still takes three blocks)
# (n_sites, n_down, momentum): short orbits inside the block ((4,2,0), (6,3,0), (6,2,3), (12,6,0), (12,6,6), (16,8,0), (9,3,3): R = 3) and
# excluded from it ((4,2,1), (4,2,3), (6,3,3) drops R = 2, (12,6,5), (16,8,5), (8,4,3)), blocks of one state ((1,0,0), (2,1,0), (2,1,1),
# (4,2,1), (4,2,3)), complex phases, real blocks at m = 0 and L / 2; D_m = 810 at L = 16, 2704 at (18,9,9): more than one block at every setting
SHAPES = [(1, 0, 0), (2, 1, 0), (2, 1, 1), (3, 1, 1), (4, 2, 0), (4, 2, 1), (4, 2, 2), (4, 2, 3), (5, 2, 1), (6, 3, 0), (6, 3, 2),
          (6, 3, 3), (6, 2, 3), (8, 4, 3), (9, 3, 3), (12, 6, 0), (12, 6, 6), (12, 6, 5), (16, 8, 0), (16, 8, 5), (18, 9, 9)]


def model_terms(model, n_sites):
    if model == "heisenberg":
        return G.heisenberg_terms(n_sites, 1.0, 1.0, periodic=True)
    if model == "xxz_field":
        return G.heisenberg_terms(n_sites, 1.0, 0.8, periodic=True) + G.zfield_terms(n_sites, 0.3)
    if model == "xxz_dm":
        return G.heisenberg_terms(n_sites, 1.0, 0.8, periodic=True) + dm_ring(n_sites, 0.35)
    raise KeyError(model)


_REF = {}


def _reference_rows(model, shape, tid):
    """(terms, csr with one entry per term and state, x, exact rows): computed once per module, never changed."""
    key = (model, shape, tid)
    if key not in _REF:
        dtype = TYPES[TYPE_IDS.index(tid)]
        terms = model_terms(model, shape[0])
        csr = G.pauli_momentum_csr(*shape, terms, WIDE[tid], merge=False)   # entries are doubles for every T
        x = K.start_x(csr[0].shape[0] - 1, dtype)
        _REF[key] = (terms, csr, x, E.rows_exact(csr, x))
    return _REF[key]


# ------------------------------------------------------------------ 1. apply against the exact reference
# (the Dzyaloshinskii-Moriya terms carry one Y each: complex types only)
APPLY_CASES = [(m, t) for m in ("heisenberg", "xxz_field", "xxz_dm") for t in TYPE_IDS if m != "xxz_dm" or t in ("z", "c")]


@pytest.mark.parametrize("model,tid", APPLY_CASES, ids=["%s-%s" % c for c in APPLY_CASES])
def test_apply_meets_the_componentwise_contract(ctx, model, tid):
    dtype = TYPES[TYPE_IDS.index(tid)]
    worst = (0.0, 0.0)
    ran = 0
    try:
        for shape in SHAPES:
            n_sites, n_down, m = shape
            if not _runs(dtype, n_sites, m):
                continue
            terms, csr, x, ex = _reference_rows(model, shape, tid)
            n = x.shape[0]
            assert n == G.momentum_basis(*shape)[0].shape[0]
            op = L.PauliMomentumOperator(ctx, n_sites, n_down, m, terms, dtype)
            assert op.info() == (n, n, len(terms))
            assert (op.n, op.n_local, op.n_sites, op.n_down, op.momentum) == (n, n, n_sites, n_down, m)
            assert op.device_bytes() >= 4 * math.comb(n_sites, n_down) + 5 * n    # orbit[], the representatives, their periods
            for bits in BLOCK_BITS:
                _set_block_bits(ctx, "momentum", bits)
                for shift in (0, 1):
                    for offset in OFFSETS:
                        y, alpha = _apply(ctx, op, x, shift, offset, True)
                        r = _check_apply(dtype, x, ex, y, alpha, offset, "%s %s %s" % (model, tid, shape))
                        worst = tuple(max(a, b) for a, b in zip(worst, r))
            op.close()
            ran += 1
    finally:
        _set_block_bits(ctx, "momentum", None)
    assert ran == (len(SHAPES) if _cplx(dtype) else sum(1 for s in SHAPES if (2 * s[2]) % s[0] == 0))
    print("ratios error/bound (class, alpha)", model, tid, worst)


# ------------------------------------------------------------------ 2. the same bits for every geometry
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_same_bits_for_every_block_size_and_alignment(ctx, dtype):
    tid = _tid(dtype)
    cases = [("heisenberg", (18, 9, 9)), ("xxz_field", (12, 6, 0)), ("xxz_field", (6, 2, 3))]
    if _cplx(dtype):
        cases += [("xxz_dm", (16, 8, 5)), ("xxz_dm", (9, 3, 3))]
    try:
        for model, shape in cases:
            terms, _, x, _ = _reference_rows(model, shape, tid)
            op = L.PauliMomentumOperator(ctx, *shape, terms, dtype)
            first = None
            for bits in [None, 0, 1, 4, 8, 12]:
                _set_block_bits(ctx, "momentum", bits)
                for shift in (0, 1):
                    for rep in range(2):
                        y, _ = _apply(ctx, op, x, shift, -2.5, False)      # _apply asserts that the input is left unchanged
                        if first is None:
                            first = y
                        assert np.array_equal(first.view(np.uint8), y.view(np.uint8)), (model, shape, bits, shift, rep)
            assert np.any(first != 0)
            op.close()
    finally:
        _set_block_bits(ctx, "momentum", None)


# ------------------------------------------------------------------ 3. consistency with the sector operator on the GPU
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64], ids=["z", "c"])
@pytest.mark.parametrize("model", ["heisenberg", "xxz_dm"])
def test_consistent_with_the_sector_operator_through_the_embedding(ctx, dtype, model):
    """y_m = B^H H_sector (B x) for every block of (12, 6).  Bound: the momentum apply's class bound, plus the sector apply's
    class bound and the rounding of its input (B x formed on the host in double, one complex product per element, then rounded to
    T: <= 4 eps_T per element, which H carries to <= 4 eps_T sum |a||x|) pushed through |B|^T, plus the host projection (a column
    of B holds <= L entries: (L + 4) eps_d |B|^T |Y|)."""
    n_sites, n_down = 12, 6
    tid = _tid(dtype)
    eps = _eps(dtype)
    terms = model_terms(model, n_sites)
    sec = L.PauliSectorOperator(ctx, n_sites, n_down, terms, dtype)
    sec_csr = G.pauli_sector_csr(n_sites, n_down, terms, np.complex128, merge=False)
    total = 0
    worst = 0.0
    for m in range(n_sites):
        _, _, x, ex = _reference_rows(model, (n_sites, n_down, m), tid)
        col, val = G.momentum_embedding(n_sites, n_down, m, dense=False)
        inb = col >= 0
        total += x.shape[0]
        X = np.zeros(col.shape[0], np.complex128)
        X[inb] = val[inb] * x.astype(np.complex128)[col[inb]]
        X = X.astype(dtype)
        Y, _ = _apply(ctx, sec, X, 0, 0.0, False)
        sec_ex = E.rows_exact(sec_csr, X)
        sec_cls = E.componentwise_bound(sec_ex, eps) + eps * E.abs1(Y) + 4 * eps * sec_ex.absrow

        def push(v):   # |B|^T v
            return np.bincount(col[inb], weights=E.abs1(val[inb]) * v[inb], minlength=x.shape[0])

        proj = np.zeros(x.shape[0], np.complex128)
        np.add.at(proj, col[inb], np.conj(val[inb]) * Y.astype(np.complex128)[inb])
        mom = L.PauliMomentumOperator(ctx, n_sites, n_down, m, terms, dtype)
        y, _ = _apply(ctx, mom, x, 0, 0.0, False)
        mom.close()
        cls, _ = _class_bound(dtype, x, ex, y, 0.0)
        bound = cls + push(sec_cls) + (n_sites + 4) * E.EPS_D * push(E.abs1(Y))
        ok, r = E.within(E.part_errors(y, proj), (bound, bound))
        assert ok, (model, m, r)
        worst = max(worst, r)
        assert np.any(y != 0)
    sec.close()
    assert total == math.comb(n_sites, n_down)
    print("momentum apply against B^H (sector apply) B: worst error / bound", model, tid, worst)


# ------------------------------------------------------------------ 4. deferred normalisation
def test_deferred_normalisation_path_against_separate_launches(ctx):
    """fuse_launches = 1 and 2 (the kernel normalises its input on the fly through ScaleIn) against 0 (a launch of its own) on
    the Heisenberg ring, block (16, 8, 0), 256 indices per block: traces to 1e-10 |A|_inf per k, iteration counts within 2."""
    shape = (16, 8, 0)
    terms = model_terms("heisenberg", shape[0])
    op = L.PauliMomentumOperator(ctx, *shape, terms)
    n = op.n
    init = G.start_vector(n, 1)
    norm = op.inf_norm()
    runs = {}
    try:
        ctx.set_tuning("pauli_momentum_block_bits", "8")
        for level in ("0", "1", "2"):
            ctx.set_tuning("fuse_launches", level)
            eng, vals, _ = _run_lanczos(op, n, init, False, -norm)
            runs[level] = (eng.last_alpha, eng.last_beta, vals[0], eng.getIterationCounts())
    finally:
        ctx.set_tuning("fuse_launches", None)
        ctx.set_tuning("pauli_momentum_block_bits", None)
    op.close()
    base = runs["0"]
    for level in ("1", "2"):
        r = runs[level]
        k = min(len(r[0]), len(base[0]))
        print("fuse_launches %s against 0: %s / %s iterations, max |d alpha| = %.3e, max |d beta| = %.3e, |d lambda| = %.3e"
              % (level, r[3], base[3], np.max(np.abs(r[0][:k] - base[0][:k])), np.max(np.abs(r[1][:k] - base[1][:k])),
                 abs(r[2] - base[2])))
    for level in ("1", "2"):
        r = runs[level]
        k = min(len(r[0]), len(base[0]))
        assert abs(r[3][0] - base[3][0]) <= 2 and k >= 10
        assert np.max(np.abs(r[0][:k] - base[0][:k])) <= 1e-10 * norm
        assert np.max(np.abs(r[1][:k] - base[1][:k])) <= 1e-10 * norm
        assert abs(r[2] - base[2]) <= 1e-10 * max(1.0, abs(base[2] - norm))


# ------------------------------------------------------------------ 5. whole runs against the real reference
# d, s at m = 0 and m = L / 2 (real blocks); z, c at m = 5 of the XXZ + DM ring (complex phases, complex H)
EIGEN_CASES = [("d", "xxz_field", 0), ("d", "xxz_field", 6), ("s", "xxz_field", 0), ("s", "xxz_field", 6), ("z", "xxz_dm", 5),
               ("c", "xxz_dm", 5)]


@pytest.mark.parametrize("num_eigs", [1, 3])
@pytest.mark.parametrize("find_max", [False, True], ids=["smallest", "largest"])
@pytest.mark.parametrize("tid,model,m", EIGEN_CASES, ids=["%s-%s-m%d" % c for c in EIGEN_CASES])
def test_lanczos_against_the_reference(ctx, tid, model, m, find_max, num_eigs):
    n_sites, n_down = 12, 6
    dtype = TYPES[TYPE_IDS.index(tid)]
    terms = model_terms(model, n_sites)
    csr = G.pauli_momentum_csr(n_sites, n_down, m, terms, WIDE[tid])
    n = csr[0].shape[0] - 1
    init = G.start_vector(n, 1).astype(dtype)
    op = L.PauliMomentumOperator(ctx, n_sites, n_down, m, terms, dtype)
    assert op.n == n
    norm = op.inf_norm()
    assert abs(norm - sum(abs(c) for _, _, c in terms)) <= 1e-12 * norm
    offset = norm if find_max else -norm
    eng, vals, vecs = _run_lanczos(op, n, init, find_max, offset, num_eigs=num_eigs)
    ref = _checker().lanczos(csr, init.astype(WIDE[tid]), find_max, num_eigs=num_eigs, offset=offset, eps=eng.eps)
    scale = max(1.0, np.max(np.abs(ref["eigenvalues"] + offset)))
    err = np.max(np.abs(vals - ref["eigenvalues"]))
    print("block (12, 6, %d) %s %s: max |lambda - reference| = %.3e, bound %.3e" % (m, tid, model, err, 20 * eng.eps * scale))
    assert len(vals) == num_eigs
    assert err <= 20 * eng.eps * scale
    op.close()


def test_lowest_block_energy_of_16_sites_is_the_sector_ground_energy_at_momentum_zero(ctx):
    n_sites, n_down = 16, 8
    terms = model_terms("heisenberg", n_sites)
    D = math.comb(n_sites, n_down)
    sec = L.PauliSectorOperator(ctx, n_sites, n_down, terms, np.complex128)
    norm = sec.inf_norm()
    eng, val_sec, _ = _run_lanczos(sec, D, G.start_vector(D, 1).astype(np.complex128), False, -norm)
    sec.close()
    lows, total = [], 0
    for m in range(n_sites):
        op = L.PauliMomentumOperator(ctx, n_sites, n_down, m, terms, np.complex128)
        total += op.n
        _, vals, _ = _run_lanczos(op, op.n, G.start_vector(op.n, 1).astype(np.complex128), False, -norm)
        lows.append(vals[0])
        op.close()
    assert total == D
    scale = max(1.0, abs(val_sec[0] - norm))
    print("Heisenberg ring L = 16: sector E0 = %.13f, block minima %s" % (val_sec[0], " ".join("%.10f" % v for v in lows)))
    assert abs(min(lows) - val_sec[0]) <= 20 * eng.eps * scale
    assert int(np.argmin(lows)) == 0


# ------------------------------------------------------------------ 6. Exponentiator
@pytest.mark.parametrize("full_orth", [False, True], ids=["three_term", "full_orthogonalize"])
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64], ids=["z", "c"])
def test_exponentiator_against_the_reference(ctx, dtype, full_orth):
    shape = (12, 6, 5)
    terms = model_terms("xxz_dm", shape[0])
    csr = G.pauli_momentum_csr(*shape, terms, np.complex128)
    n = csr[0].shape[0] - 1
    single = np.dtype(dtype) == np.complex64
    inp = G.start_vector(n, 2, np.complex128).astype(dtype)
    a = -0.05j
    op = L.PauliMomentumOperator(ctx, *shape, terms, dtype)
    ex = L.Exponentiator(op, n)
    ex.full_orthogonalize = full_orth
    out, it = ex.run(a, inp)
    o_out, o_it, _ = _checker().expo(csr, a, inp.astype(np.complex128), eps=ex.eps, full_orthogonalize=full_orth)
    assert abs(it - o_it) <= 2
    if single:   # the float rule of the sector operator's test
        assert np.linalg.norm(out - o_out) <= 1e-3 * np.linalg.norm(o_out)
    else:
        assert 1 - overlap(out, o_out) <= 10 * ex.eps
        assert abs(np.linalg.norm(out) / np.linalg.norm(inp) - 1) <= 1e-12
    op.close()


# ------------------------------------------------------------------ 7. refusals
def _refused(ctx, n_sites, n_down, m, terms, dtype=np.float64):
    with pytest.raises(capi.LanczosHipError) as e:
        L.PauliMomentumOperator(ctx, n_sites, n_down, m, terms, dtype).close()
    assert e.value.code == capi.LL_ERR_INVALID, str(e.value)
    return str(e.value)


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_invalid_inputs_are_refused_with_their_cause(ctx, dtype):
    ring = G.heisenberg_terms(6, 1.0, 1.0)
    for m in (-1, 6):
        assert "momentum must lie in [0, n_sites)" in _refused(ctx, 6, 3, m, ring, dtype)
    if not _cplx(dtype):
        msg = _refused(ctx, 6, 3, 1, ring, dtype)
        assert "real storage type" in msg and "momentum 0 and n_sites / 2" in msg, msg
    else:
        L.PauliMomentumOperator(ctx, 6, 3, 1, ring, dtype).close()
    msg = _refused(ctx, 6, 3, 0, G.heisenberg_terms(6, 1.0, 1.0, periodic=False), dtype)      # an open chain: bond (5, 0) is missing
    assert "does not commute with the one-site translation" in msg and "x_mask 0x30, z_mask 0x0" in msg, msg
    bent = list(ring)
    bent[4] = (bent[4][0], bent[4][1], float(np.nextafter(bent[4][2], 1.0)))                  # YY of bond 1, last bit changed:
    msg = _refused(ctx, 6, 3, 0, bent, dtype)                                                 # XX + YY no longer cancels there
    assert "conserve S_z" in msg, msg
    bent = list(ring)
    bent[5] = (bent[5][0], bent[5][1], float(np.nextafter(bent[5][2], 1.0)))                  # ZZ of bond 1, last bit changed
    msg = _refused(ctx, 6, 3, 0, bent, dtype)
    assert "does not commute with the one-site translation" in msg and "term 2 (x_mask 0x0, z_mask 0x3)" in msg, msg
    msg = _refused(ctx, 6, 3, 0, G.tfim_terms(6, 1.0, 1.5, periodic=True), dtype)             # leaves the sector: the sector's message
    assert "conserve S_z" in msg and "x mask 0x1 " in msg, msg
    msg = _refused(ctx, 6, 0, 3, ring, dtype)                                                 # the all-up state has momentum 0 only
    assert "momentum block is empty" in msg, msg
    for n_down in (-1, 7):
        assert "n_down" in _refused(ctx, 6, n_down, 0, ring, dtype)
    assert "n_sites" in _refused(ctx, 31, 15, 0, ring, dtype)
    ok = L.PauliMomentumOperator(ctx, 6, 3, 0, ring, dtype)
    assert ok.n == 4
    with pytest.raises(capi.LanczosHipError):
        L.CsrOperator.select_spmv(ok, capi.SPMV_CSR_STREAM)           # not a CSR operator, like the sector operator
    with pytest.raises(capi.LanczosHipError):
        L.CsrOperator.set_accuracy(ok, capi.ACCURACY_NORMWISE)
    assert L.CsrOperator.accuracy(ok) == capi.ACCURACY_COMPONENTWISE
    ok.close()


# ------------------------------------------------------------------ 8. degenerate operators
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_zero_and_diagonal_operators(ctx, dtype):
    n_sites, n_down = 8, 3
    for m in (0, 4) if not _cplx(dtype) else (0, 3, 4):
        n = G.momentum_basis(n_sites, n_down, m)[0].shape[0]
        x = K.start_x(n, dtype)
        xd, yd = ctx.to_device(x), ctx.empty(n, dtype)
        op = L.PauliMomentumOperator(ctx, n_sites, n_down, m, [], dtype)                  # no term: the zero operator
        assert op.info() == (n, n, 0) and op.inf_norm() == 0.0
        L.spmv(op, xd, yd, offset=0.0)
        assert np.all(yd.get() == 0)
        op.close()
        op = L.PauliMomentumOperator(ctx, n_sites, n_down, m, [(0, 0, 0.5)] + G.zfield_terms(n_sites, 0.25), dtype)
        L.spmv(op, xd, yd, offset=0.0)                                                    # 0.5 - 0.25 (L - 2 n_down): exact in every T
        want = (0.5 - 0.25 * (n_sites - 2 * n_down)) * x.astype(WIDE[_tid(dtype)])
        assert np.array_equal(yd.get(), want.astype(dtype))
        op.close()
        xd.free()
        yd.free()


def test_refused_on_a_sharded_context(tmp_path):
    """Two ranks on the box's GPU over the test transport: the operator is single-GPU."""
    from conftest import SHM_TRANSPORT

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name = "/ll_shm_pmom_" + uuid.uuid4().hex[:12]
    env = dict(os.environ, LL_COMM_PLUGIN=SHM_TRANSPORT, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(root, "tests", "shm_pauli_refused_worker.py"), str(r), "2", name,
                               str(tmp_path), "momentum"], env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-4000:]
    for r in range(2):
        res = json.load(open(os.path.join(tmp_path, "rank%d.json" % r)))
        assert res["code"] == capi.LL_ERR_INVALID and "sharded" in res["msg"], res
