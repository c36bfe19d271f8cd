"""The sum-of-Pauli-strings operator on one momentum block of the FULL 2^n_sites space of a ring
(ll_op_create_pauli_momentum_full_*, csrc/pauli_momentum_full.hip): every apply against the EXACT host reference of the block
B^H H B (generators.pauli_momentum_full_csr, one entry per term and state) with the component-wise class, the same bits for every
block size and alignment, consistency on the GPU with PauliOperator through the embedding B and with the S_z-sector momentum
operator, whole eigen-solver and Exponentiator runs against the reference library on the block's matrix, the image's size
(O(D_m): no table over the 2^n_sites states) and the refusals.

As for the sector's momentum operator the single-type storage-product contract of the CSR kernels is NOT asserted: an entry of
the block is a weight times sqrt(R_a / R_b) times a phase, formed in double (lanczos_hip.h (9), ACCURACY)."""
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
from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G
from pauli_cases import (TYPES, TYPE_IDS, WIDE, _apply, _check_apply, _checker, _class_bound, _cplx, _run_lanczos, _runs,
                         _set_block_bits, _tid, dm_ring)
from test_gpu_accuracy_contracts import OFFSETS, _eps
from util import overlap

pytestmark = pytest.mark.gpu

BLOCK_BITS = [None, 4, 8, 10]      # default, 16, 256 and 1024 indices per block (1024: four states per lane)
# (n_sites, momentum).  D_m = 2, 3, 1, 2: one-state and tiny blocks; (4, *): D_m = 6, 3, 4, 3 with R = 1, 2 inside and excluded;
# (5, 2): prime L, complex phases; (6, *): D_m = 14, 11, 10 with R = 2, 3 in and out; (8, 3), (9, 3): R = 3 inside at L = 9;
# (12, *): D_m = 352, 348, 335 — more than one block at 2^8; (16, *): D_m = 4116, 4114, 4080 — 17 blocks; (16, 0): 512 buckets of
# up to 65 representatives, (16, 5): 256 buckets of up to 128 — a search of 7 halvings in both
SHAPES = [(1, 0), (2, 0), (2, 1), (3, 1), (4, 0), (4, 1), (4, 2), (4, 3), (5, 2), (6, 0), (6, 2), (6, 3), (8, 3), (9, 3), (12, 0),
          (12, 6), (12, 5), (16, 0), (16, 8), (16, 5)]
DIMS = {(1, 0): 2, (2, 0): 3, (2, 1): 1, (3, 1): 2, (4, 0): 6, (4, 1): 3, (4, 2): 4, (4, 3): 3, (6, 0): 14, (6, 2): 11, (6, 3): 10,
        (12, 0): 352, (12, 6): 348, (16, 0): 4116, (16, 8): 4114, (18, 9): 14542}
COMPLEX_MODELS = ("xyz_dm_x",)     # the Dzyaloshinskii-Moriya terms carry one Y each


def model_terms(model, n_sites):
    if model == "tfim":
        return G.tfim_terms(n_sites, 1.0, 0.7, periodic=True)
    if model == "tfim_z":   # the z field breaks the spin-flip parity
        return G.tfim_terms(n_sites, 1.0, 0.7, periodic=True) + G.zfield_terms(n_sites, 0.3)
    if model == "xyz":
        return G.xyz_terms(n_sites, 1.0, 0.6, 0.8)
    if model == "xyz_dm_x":
        return G.xyz_terms(n_sites, 1.0, 0.6, 0.8) + dm_ring(n_sites, 0.35) + [(1 << j, 0, -0.45) for j in range(n_sites)]
    if model == "heisenberg":  # conserves S_z: accepted here too
        return G.heisenberg_terms(n_sites, 1.0, 1.0, periodic=True)
    raise KeyError(model)


_REF = {}


def _reference_rows(model, shape, tid):
    """(terms, csr with one entry per term and state, x, exact rows): computed once per module, never changed."""
    key = (model, shape, tid)
    if key not in _REF:
        dtype = TYPES[TYPE_IDS.index(tid)]
        terms = model_terms(model, shape[0])
        csr = G.pauli_momentum_full_csr(*shape, terms, WIDE[tid], merge=False)   # entries are doubles for every T
        x = K.start_x(csr[0].shape[0] - 1, dtype)
        _REF[key] = (terms, csr, x, E.rows_exact(csr, x))
    return _REF[key]


# ------------------------------------------------------------------ 1. apply against the exact reference
APPLY_CASES = [(m, t) for m in ("tfim", "tfim_z", "xyz", "xyz_dm_x", "heisenberg") for t in TYPE_IDS
               if m not in COMPLEX_MODELS or t in ("z", "c")]


@pytest.mark.parametrize("model,tid", APPLY_CASES, ids=["%s-%s" % c for c in APPLY_CASES])
def test_apply_meets_the_componentwise_contract(ctx, model, tid):
    dtype = TYPES[TYPE_IDS.index(tid)]
    worst = (0.0, 0.0)
    ran = 0
    try:
        for shape in SHAPES:
            n_sites, m = shape
            if not _runs(dtype, n_sites, m):
                continue
            terms, csr, x, ex = _reference_rows(model, shape, tid)
            n = x.shape[0]
            assert n == G.full_momentum_basis(*shape)[0].shape[0] and n == DIMS.get(shape, n)
            op = L.PauliMomentumFullOperator(ctx, n_sites, m, terms, dtype)
            assert op.info() == (n, n, len(terms))
            assert (op.n, op.n_local, op.n_sites, op.momentum) == (n, n, n_sites, m)
            assert op.device_bytes() <= 8 * n + 2 ** 16      # reps, periods, the bucket table and the small tables: O(D_m)
            if n_sites == 16:
                assert op.device_bytes() < 4 * 2 ** 16       # a table over the 2^16 states alone would be that large
            for bits in BLOCK_BITS:
                _set_block_bits(ctx, "momentum_full", bits)
                for shift in (0, 1):
                    for offset in OFFSETS:
                        y, alpha = _apply(ctx, op, x, shift, offset, True)
                        r = _check_apply(dtype, x, ex, y, alpha, offset, "%s %s %s" % (model, tid, shape))
                        worst = tuple(max(a, b) for a, b in zip(worst, r))
            op.close()
            ran += 1
    finally:
        _set_block_bits(ctx, "momentum_full", None)
    assert ran == (len(SHAPES) if _cplx(dtype) else sum(1 for s in SHAPES if (2 * s[1]) % s[0] == 0))
    print("ratios error/bound (class, alpha)", model, tid, worst)


# ------------------------------------------------------------------ 2. the same bits for every geometry
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_same_bits_for_every_block_size_and_alignment(ctx, dtype):
    cases = [("tfim", (18, 9)), ("tfim_z", (12, 0)), ("xyz", (6, 3))]
    if _cplx(dtype):
        cases += [("xyz_dm_x", (16, 5)), ("xyz_dm_x", (9, 3))]
    try:
        for model, shape in cases:
            terms = model_terms(model, shape[0])
            op = L.PauliMomentumFullOperator(ctx, *shape, terms, dtype)
            assert op.n == DIMS.get(shape, op.n)
            x = K.start_x(op.n, dtype)
            first = None
            for bits in [None, 0, 1, 4, 8, 12]:
                _set_block_bits(ctx, "momentum_full", bits)
                for shift in (0, 1):
                    for rep in range(2):
                        y, _ = _apply(ctx, op, x, shift, -2.5, False)      # _apply asserts that the input is left unchanged
                        if first is None:
                            first = y
                        assert np.array_equal(first.view(np.uint8), y.view(np.uint8)), (model, shape, bits, shift, rep)
            assert np.any(first != 0)
            op.close()
    finally:
        _set_block_bits(ctx, "momentum_full", None)


# ------------------------------------------------------------------ 3. consistency with PauliOperator on the GPU
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64], ids=["z", "c"])
@pytest.mark.parametrize("model", ["tfim_z", "xyz_dm_x"])
def test_consistent_with_the_full_operator_through_the_embedding(ctx, dtype, model):
    """y_m = B^H H (B x) for every block of 12 sites, H applied by PauliOperator on the 4096 states.  Bound, formed as
    test_gpu_pauli_momentum.test_consistent_with_the_sector_operator_through_the_embedding forms it: the block apply's class
    bound, plus the full apply's class bound and the rounding of its input (B x formed on the host in double, one complex product
    per element, then rounded to T: <= 4 eps_T per element, which H carries to <= 4 eps_T sum |a||x|) pushed through |B|^T, plus
    the host projection (a column of B holds <= L entries: (L + 4) eps_d |B|^T |Y|)."""
    n_sites = 12
    tid = _tid(dtype)
    eps = _eps(dtype)
    terms = model_terms(model, n_sites)
    full = L.PauliOperator(ctx, n_sites, terms, dtype)
    full_csr = G.pauli_csr(n_sites, terms, np.complex128, merge=False)
    total = 0
    worst = 0.0
    for m in range(n_sites):
        _, _, x, ex = _reference_rows(model, (n_sites, m), tid)
        col, val = G.full_momentum_embedding(n_sites, m, dense=False)
        inb = col >= 0
        total += x.shape[0]
        X = np.zeros(col.shape[0], np.complex128)
        X[inb] = val[inb] * x.astype(np.complex128)[col[inb]]
        X = X.astype(dtype)
        Y, _ = _apply(ctx, full, X, 0, 0.0, False)
        full_ex = E.rows_exact(full_csr, X)
        full_cls = E.componentwise_bound(full_ex, eps) + eps * E.abs1(Y) + 4 * eps * full_ex.absrow

        def push(v):   # |B|^T v
            return np.bincount(col[inb], weights=E.abs1(val[inb]) * v[inb], minlength=x.shape[0])

        proj = np.zeros(x.shape[0], np.complex128)
        np.add.at(proj, col[inb], np.conj(val[inb]) * Y.astype(np.complex128)[inb])
        mom = L.PauliMomentumFullOperator(ctx, n_sites, m, terms, dtype)
        y, _ = _apply(ctx, mom, x, 0, 0.0, False)
        mom.close()
        cls, _ = _class_bound(dtype, x, ex, y, 0.0)
        bound = cls + push(full_cls) + (n_sites + 4) * E.EPS_D * push(E.abs1(Y))
        ok, r = E.within(E.part_errors(y, proj), (bound, bound))
        assert ok, (model, m, r)
        worst = max(worst, r)
        assert np.any(y != 0)
    full.close()
    assert total == 4096
    print("block apply against B^H (full apply) B: worst error / bound", model, tid, worst)


# ------------------------------------------------------------------ 4. consistency with the sector's momentum operator
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_consistent_with_the_sector_momentum_operator(ctx, dtype):
    """Heisenberg ring of 12 sites (conserves S_z): on a vector supported on the representatives of ONE n_down the full-space
    block acts as that sector's block (the direct sum of test_pauli_momentum_full_host).  Tolerance: the two applies' class
    bounds added — not equal bits: a group that leaves the sector enters here with weight 0 and may change the sign of a zero."""
    n_sites = 12
    tid = _tid(dtype)
    terms = model_terms("heisenberg", n_sites)
    ran = 0
    for m in (0, 5, 6):
        if not _runs(dtype, n_sites, m):
            continue
        reps, _ = G.full_momentum_basis(n_sites, m)
        n_down = np.array([bin(int(r)).count("1") for r in reps])
        full_csr = G.pauli_momentum_full_csr(n_sites, m, terms, WIDE[tid], merge=False)
        fop = L.PauliMomentumFullOperator(ctx, n_sites, m, terms, dtype)
        xall = K.start_x(reps.shape[0], dtype)
        seen = 0
        for nd in range(n_sites + 1):
            here = n_down == nd
            sec_reps, _ = G.momentum_basis(n_sites, nd, m)
            assert np.array_equal(reps[here], sec_reps)
            seen += sec_reps.shape[0]
            if sec_reps.shape[0] == 0:
                continue    # an empty block of the sector (the sector operator refuses it)
            x = np.where(here, xall, 0).astype(dtype)
            y, _ = _apply(ctx, fop, x, 0, 0.0, False)
            sop = L.PauliMomentumOperator(ctx, n_sites, nd, m, terms, dtype)
            xs = np.ascontiguousarray(x[here])
            ys, _ = _apply(ctx, sop, xs, 0, 0.0, False)
            sop.close()
            assert np.all(y[~here] == 0), (m, nd)
            cls_f, _ = _class_bound(dtype, x, E.rows_exact(full_csr, x), y, 0.0)
            sec_csr = G.pauli_momentum_csr(n_sites, nd, m, terms, WIDE[tid], merge=False)
            cls_s, _ = _class_bound(dtype, xs, E.rows_exact(sec_csr, xs), ys, 0.0)
            bound = cls_f[here] + cls_s
            ok, r = E.within(E.part_errors(y[here], ys.astype(np.complex128 if _cplx(dtype) else np.float64)), (bound, bound))
            assert ok, (m, nd, r)
            ran += 1
        assert seen == reps.shape[0]
        fop.close()
    # the non-empty (m, n_down) pairs: 13 at m = 0, 11 at m = 5 and at m = 6 (n_down = 0 and 12 have R = 1: block 0 only)
    assert ran == (35 if _cplx(dtype) else 24)


# ------------------------------------------------------------------ 5. deferred normalisation
@pytest.mark.parametrize("shape,model,dtype", [((12, 5), "xyz_dm_x", np.complex128), ((12, 6), "tfim_z", np.float64)],
                         ids=["12-5-z", "12-6-d"])
def test_deferred_normalisation_path_against_separate_launches(ctx, shape, model, dtype):
    """fuse_launches = 1 and 2 (the kernel normalises its input on the fly through ScaleIn) against 0 (a launch of its own), 16
    indices per block: traces to 1e-10 |A|_inf per k, iteration counts within 2 (the rule of the sector operator's test)."""
    terms = model_terms(model, shape[0])
    op = L.PauliMomentumFullOperator(ctx, *shape, terms, dtype)
    n = op.n
    init = G.start_vector(n, 1).astype(dtype)
    norm = op.inf_norm()
    runs = {}
    try:
        _set_block_bits(ctx, "momentum_full", 4)
        for level in ("0", "1", "2"):
            ctx.set_tuning("fuse_launches", level)
            eng, vals, _ = _run_lanczos(op, n, init, False, -norm)
            runs[level] = (eng.last_alpha, eng.last_beta, vals[0], eng.getIterationCounts())
    finally:
        ctx.set_tuning("fuse_launches", None)
        _set_block_bits(ctx, "momentum_full", None)
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


# ------------------------------------------------------------------ 6. whole runs against the real reference
# d, s at m = 0 and m = L / 2 (real blocks) of the TFIM ring with a z field; z, c at m = 5 of the XYZ + DM + x-field ring
EIGEN_CASES = [("d", "tfim_z", 0), ("d", "tfim_z", 6), ("s", "tfim_z", 0), ("s", "tfim_z", 6), ("z", "xyz_dm_x", 5),
               ("c", "xyz_dm_x", 5)]


@pytest.mark.parametrize("num_eigs", [1, 3])
@pytest.mark.parametrize("find_max", [False, True], ids=["smallest", "largest"])
@pytest.mark.parametrize("tid,model,m", EIGEN_CASES, ids=["%s-%s-m%d" % c for c in EIGEN_CASES])
def test_lanczos_against_the_reference(ctx, tid, model, m, find_max, num_eigs):
    n_sites = 12
    dtype = TYPES[TYPE_IDS.index(tid)]
    terms = model_terms(model, n_sites)
    csr = G.pauli_momentum_full_csr(n_sites, m, terms, WIDE[tid])
    n = csr[0].shape[0] - 1
    init = G.start_vector(n, 1).astype(dtype)
    op = L.PauliMomentumFullOperator(ctx, n_sites, m, terms, dtype)
    assert op.n == n
    norm = op.inf_norm()
    assert abs(norm - sum(abs(c) for _, _, c in terms)) <= 1e-12 * norm
    offset = norm if find_max else -norm
    eng, vals, vecs = _run_lanczos(op, n, init, find_max, offset, num_eigs=num_eigs)
    ref = _checker().lanczos(csr, init.astype(WIDE[tid]), find_max, num_eigs=num_eigs, offset=offset, eps=eng.eps)
    scale = max(1.0, np.max(np.abs(ref["eigenvalues"] + offset)))
    err = np.max(np.abs(vals - ref["eigenvalues"]))
    print("block (12, %d) %s %s: max |lambda - reference| = %.3e, bound %.3e" % (m, tid, model, err, 20 * eng.eps * scale))
    assert len(vals) == num_eigs
    assert err <= 20 * eng.eps * scale
    op.close()


# ------------------------------------------------------------------ 7. Exponentiator
@pytest.mark.parametrize("full_orth", [False, True], ids=["three_term", "full_orthogonalize"])
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64], ids=["z", "c"])
def test_exponentiator_against_the_reference(ctx, dtype, full_orth):
    shape = (12, 5)
    terms = model_terms("xyz_dm_x", shape[0])
    csr = G.pauli_momentum_full_csr(*shape, terms, np.complex128)
    n = csr[0].shape[0] - 1
    single = np.dtype(dtype) == np.complex64
    inp = G.start_vector(n, 2, np.complex128).astype(dtype)
    a = -0.05j
    op = L.PauliMomentumFullOperator(ctx, *shape, terms, dtype)
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


# ------------------------------------------------------------------ 8. physics
def test_ground_energy_of_the_16_site_tfim_ring_lies_in_the_block_of_momentum_zero(ctx):
    """TFIM ring, L = 16, fp64: the lowest energy of the block m = 0 (4116 states) is the lowest energy PauliOperator finds on
    all 65 536 states (the ground state of the ferromagnetic ring is translation invariant)."""
    n_sites = 16
    terms = model_terms("tfim", n_sites)
    full = L.PauliOperator(ctx, n_sites, terms, np.float64)
    norm = full.inf_norm()
    eng, val_full, _ = _run_lanczos(full, full.n, G.start_vector(full.n, 1), False, -norm)
    full.close()
    op = L.PauliMomentumFullOperator(ctx, n_sites, 0, terms, np.float64)
    assert op.n == 4116 and op.inf_norm() == norm
    _, vals, _ = _run_lanczos(op, op.n, G.start_vector(op.n, 1), False, -norm)
    op.close()
    scale = max(1.0, abs(val_full[0] - norm))
    print("TFIM ring L = 16: E0 on 65536 states %.13f, on the block m = 0 %.13f" % (val_full[0], vals[0]))
    assert abs(vals[0] - val_full[0]) <= 20 * eng.eps * scale


# ------------------------------------------------------------------ 9. refusals
def _refused(ctx, n_sites, m, terms, dtype=np.float64):
    with pytest.raises(capi.LanczosHipError) as e:
        L.PauliMomentumFullOperator(ctx, n_sites, m, terms, dtype).close()
    assert e.value.code == capi.LL_ERR_INVALID, str(e.value)
    return str(e.value)


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_invalid_inputs_are_refused_with_their_cause(ctx, dtype):
    ring = G.tfim_terms(6, 1.0, 0.7, periodic=True)
    for m in (-1, 6):
        assert "momentum must lie in [0, n_sites)" in _refused(ctx, 6, m, ring, dtype)
    odd_y = model_terms("xyz_dm_x", 6)
    if not _cplx(dtype):
        msg = _refused(ctx, 6, 1, ring, dtype)
        assert "real storage type" in msg and "momentum 0 and n_sites / 2" in msg, msg
        msg = _refused(ctx, 6, 0, odd_y, dtype)
        assert "odd number of Y" in msg, msg
    else:
        L.PauliMomentumFullOperator(ctx, 6, 1, ring, dtype).close()
        L.PauliMomentumFullOperator(ctx, 6, 0, odd_y, dtype).close()
    msg = _refused(ctx, 6, 0, G.tfim_terms(6, 1.0, 0.7, periodic=False), dtype)       # an open chain: bond (5, 0) is missing
    assert "does not commute with the one-site translation" in msg and "term 4 (x_mask 0x0, z_mask 0x30)" in msg, msg
    for n_sites in (0, 31):
        assert "n_sites" in _refused(ctx, n_sites, 0, ring, dtype)
    assert "a mask bit at or above n_sites" in _refused(ctx, 6, 0, ring + [(1 << 6, 0, 1.0)], dtype)
    assert "not finite" in _refused(ctx, 6, 0, ring + [(0, 0, float("nan"))], dtype)
    ok = L.PauliMomentumFullOperator(ctx, 6, 0, model_terms("heisenberg", 6), dtype)   # an H that conserves S_z is accepted
    assert ok.n == 14
    with pytest.raises(capi.LanczosHipError):
        L.CsrOperator.select_spmv(ok, capi.SPMV_CSR_STREAM)           # not a CSR operator, like the sector operator
    with pytest.raises(capi.LanczosHipError):
        L.CsrOperator.set_accuracy(ok, capi.ACCURACY_NORMWISE)
    assert L.CsrOperator.accuracy(ok) == capi.ACCURACY_COMPONENTWISE
    ok.close()


# ------------------------------------------------------------------ 10. degenerate operators
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_zero_and_diagonal_operators(ctx, dtype):
    n_sites = 8
    for m in (0, 4) if not _cplx(dtype) else (0, 3, 4):
        reps, _ = G.full_momentum_basis(n_sites, m)
        n = reps.shape[0]
        x = K.start_x(n, dtype)
        xd, yd = ctx.to_device(x), ctx.empty(n, dtype)
        op = L.PauliMomentumFullOperator(ctx, n_sites, m, [], dtype)                      # no term: the zero operator
        assert op.info() == (n, n, 0) and op.inf_norm() == 0.0
        L.spmv(op, xd, yd, offset=0.0)
        assert np.all(yd.get() == 0)
        op.close()
        op = L.PauliMomentumFullOperator(ctx, n_sites, m, [(0, 0, 0.5)], dtype)           # the identity term: coef x
        L.spmv(op, xd, yd, offset=0.0)
        assert np.array_equal(yd.get(), (0.5 * x.astype(WIDE[_tid(dtype)])).astype(dtype))
        op.close()
        op = L.PauliMomentumFullOperator(ctx, n_sites, m, [(0, 0, 0.5)] + G.zfield_terms(n_sites, 0.25), dtype)
        L.spmv(op, xd, yd, offset=0.0)                                # 0.5 - 0.25 (L - 2 popcount(r)): exact in every T
        down = np.array([bin(int(r)).count("1") for r in reps])
        want = (0.5 - 0.25 * (n_sites - 2 * down)) * x.astype(WIDE[_tid(dtype)])
        assert np.array_equal(yd.get(), want.astype(dtype))
        op.close()
        xd.free()
        yd.free()


# ------------------------------------------------------------------ 11. sharded contexts
def test_refused_on_a_sharded_context(tmp_path):
    """Two ranks on the box's GPU over the test transport: the operator is single-GPU."""
    from conftest import SHM_TRANSPORT

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name = "/ll_shm_pmf_" + uuid.uuid4().hex[:12]
    env = dict(os.environ, LL_COMM_PLUGIN=SHM_TRANSPORT, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(root, "tests", "shm_pauli_refused_worker.py"), str(r), "2", name,
                               str(tmp_path), "momentum_full"], env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-4000:]
    for r in range(2):
        res = json.load(open(os.path.join(tmp_path, "rank%d.json" % r)))
        assert res["code"] == capi.LL_ERR_INVALID and "sharded" in res["msg"], res
