"""The sum-of-Pauli-strings operator on one block of a ring under momentum, reflection and spin inversion
(ll_op_create_pauli_symmetric_*, csrc/pauli_symmetric.hip): every apply against the EXACT host reference of the block B^H H B
(generators.pauli_symmetric_csr, one entry per term and state) with the component-wise class, the same bits for every block
size and alignment, the same bits as PauliMomentumFullOperator with every flag 0, consistency on the GPU with PauliOperator and
PauliSectorOperator through the embedding B, whole eigen-solver and Exponentiator runs against the reference library on the
block's matrix, the image's size and the refusals.

As for the momentum operators the single-type storage-product contract of the CSR kernels is NOT asserted: an entry of the
block is a weight times sqrt(R_a / R_b) times a phase, formed in double (lanczos_hip.h (10), ACCURACY)."""
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
from pauli_cases import (TYPES, TYPE_IDS, WIDE, _apply, _check_apply, _checker, _class_bound, _cplx, _run_lanczos,
                         _set_block_bits, _tid, dm_ring)
from test_gpu_accuracy_contracts import OFFSETS, _eps
from util import overlap

pytestmark = pytest.mark.gpu

BLOCK_BITS = [None, 4, 8, 10]      # default, 16, 256 and 1024 indices per block (1024: four states per lane)
SIGNS = [(1, 1), (1, -1), (-1, 1), (-1, -1)]
# (n_sites, m, parity, inversion) -> D, pinned: the cases of the issue at 12 sites, and at 16 sites from the host generator, tied
# by the sum rule D(m,+,+) + D(m,+,-) + D(m,-,+) + D(m,-,-) = D_m (4116 at m = 0, 4114 at m = 8; asserted below)
DIMS = {(12, 0, 1, 1): 122, (12, 6, -1, -1): 102, (12, 0, 1, 0): 224, (16, 0, 1, 1): 1162, (16, 8, -1, -1): 1088}
DIMS_HALF = {(12, 0, 1, 1): 35, (12, 6, -1, -1): 27, (12, 0, 1, 0): 50}        # with n_down = 6
COMPLEX_MODELS = ("xyz_dm_x",)     # the Dzyaloshinskii-Moriya terms carry one Y each


def model_terms(model, n_sites):
    if model == "tfim":
        return G.tfim_terms(n_sites, 1.0, 0.7, periodic=True)
    if model == "xyz":
        return G.xyz_terms(n_sites, 1.0, 0.6, 0.8)
    if model in ("heisenberg", "heisenberg_sector"):
        return G.heisenberg_terms(n_sites, 1.0, 1.0, periodic=True)
    if model == "xyz_dm_x":     # commutes with the translation only
        return G.xyz_terms(n_sites, 1.0, 0.6, 0.8) + dm_ring(n_sites, 0.35) + [(1 << j, 0, -0.45) for j in range(n_sites)]
    raise KeyError(model)


def _all_blocks(n_sites):
    """Every (n_sites, m, parity, inversion) with 2 m mod n_sites = 0."""
    return [(n_sites, m, p, z) for m in sorted({0, n_sites // 2} if n_sites % 2 == 0 else {0}) for p in (0, 1, -1)
            for z in (0, 1, -1)]


# L = 2, 3: one- and two-state blocks; L = 4, 6, 8: every (m, p, z) with 2 m mod L = 0 — short orbits, representatives excluded by
# parity alone and by inversion alone, the empty ones skipped (and counted); L = 9 and (5, 2): complex phases with the spin flip
# (z / c only); L = 12: the pinned cases; L = 16: more than one block at 2^8 indices and a search of several halvings
SHAPES = (_all_blocks(2) + _all_blocks(3) + _all_blocks(4) + _all_blocks(6) + _all_blocks(8) +
          [(9, 3, 0, 1), (9, 3, 0, -1), (9, 1, 0, -1), (5, 2, 0, 1), (5, 2, 0, -1)] +
          [(12, 0, 1, 1), (12, 6, -1, -1), (12, 0, 1, 0), (12, 0, 1, -1), (12, 0, -1, 1), (12, 0, -1, -1)] +
          [(16, 0, 1, 1), (16, 8, -1, -1)])
PLAIN_SHAPES = [(2, 1, 0, 0), (3, 1, 0, 0), (4, 1, 0, 0), (5, 2, 0, 0), (6, 0, 0, 0), (8, 3, 0, 0), (9, 3, 0, 0), (12, 5, 0, 0),
                (16, 5, 0, 0)]


def _n_down(model, n_sites):
    return n_sites // 2 if model == "heisenberg_sector" else None


def _shapes(model, dtype):
    if model in COMPLEX_MODELS:
        return PLAIN_SHAPES
    out = []
    for s in SHAPES:
        n_sites, m, p, z = s
        if not (_cplx(dtype) or (2 * m) % n_sites == 0):
            continue                                     # d / s run only where the block is real
        if _n_down(model, n_sites) is not None and z and n_sites % 2:
            continue                                     # the spin flip needs half filling
        out.append(s)
    return out


_REF = {}


def _reference_rows(model, shape, tid):
    """(terms, csr with one entry per term and state, x, exact rows) or None for an empty block: computed once per module."""
    key = (model, shape, tid)
    if key not in _REF:
        dtype = TYPES[TYPE_IDS.index(tid)]
        n_sites, m, p, z = shape
        terms = model_terms(model, n_sites)
        nd = _n_down(model, n_sites)
        if G.symmetric_basis(n_sites, m, p, z, nd)[0].shape[0] == 0:
            _REF[key] = None
        else:
            csr = G.pauli_symmetric_csr(n_sites, m, p, z, terms, WIDE[tid], n_down=nd, merge=False)   # doubles for every T
            x = K.start_x(csr[0].shape[0] - 1, dtype)
            _REF[key] = (terms, csr, x, E.rows_exact(csr, x))
    return _REF[key]


def _op(ctx, shape, terms, dtype, n_down=None):
    n_sites, m, p, z = shape
    return L.PauliSymmetricOperator(ctx, n_sites, m, terms, dtype, parity=p, inversion=z, n_down=n_down)


def test_the_pinned_dimensions_obey_the_sum_rules():
    for m, total in ((0, 4116), (8, 4114)):
        assert sum(G.symmetric_basis(16, m, p, z)[0].shape[0] for p, z in SIGNS) == total
        assert G.full_momentum_basis(16, m)[0].shape[0] == total
    for (n_sites, m, p, z), D in DIMS.items():
        assert G.symmetric_basis(n_sites, m, p, z)[0].shape[0] == D


# ------------------------------------------------------------------ 1. apply against the exact reference
APPLY_CASES = [(m, t) for m in ("tfim", "xyz", "heisenberg", "heisenberg_sector", "xyz_dm_x") for t in TYPE_IDS
               if m not in COMPLEX_MODELS or t in ("z", "c")]


@pytest.mark.parametrize("model,tid", APPLY_CASES, ids=["%s-%s" % c for c in APPLY_CASES])
def test_apply_meets_the_componentwise_contract(ctx, model, tid):
    dtype = TYPES[TYPE_IDS.index(tid)]
    worst = (0.0, 0.0)
    ran = empty = 0
    try:
        for shape in _shapes(model, dtype):
            n_sites, m, p, z = shape
            nd = _n_down(model, n_sites)
            ref = _reference_rows(model, shape, tid)
            if ref is None:                              # an empty block: refused (section 7 checks the message)
                with pytest.raises(capi.LanczosHipError):
                    _op(ctx, shape, model_terms(model, n_sites), dtype, nd)
                empty += 1
                continue
            terms, csr, x, ex = ref
            n = x.shape[0]
            assert n == G.symmetric_basis(n_sites, m, p, z, nd)[0].shape[0]
            assert n == (DIMS if nd is None else DIMS_HALF).get(shape, n)
            op = _op(ctx, shape, terms, dtype, nd)
            assert op.info() == (n, n, len(terms))
            assert (op.n, op.n_local, op.n_sites, op.momentum, op.parity, op.inversion, op.n_down) == (n, n, n_sites, m, p, z, nd)
            assert op.device_bytes() <= 8 * n + 192 * 1024   # reps, orbit lengths, the bucket table, the small tables: O(D)
            for bits in BLOCK_BITS:
                _set_block_bits(ctx, "symmetric", bits)
                for shift in (0, 1):
                    for offset in OFFSETS:
                        y, alpha = _apply(ctx, op, x, shift, offset, True)
                        r = _check_apply(dtype, x, ex, y, alpha, offset, "%s %s %s" % (model, tid, shape))
                        worst = tuple(max(a, b) for a, b in zip(worst, r))
            op.close()
            ran += 1
    finally:
        _set_block_bits(ctx, "symmetric", None)
    assert ran + empty == len(_shapes(model, dtype)) and ran >= 9
    if model not in COMPLEX_MODELS and model != "heisenberg_sector":
        assert empty >= 3                                 # (4, 0, -1, *) at least
    print("ratios error/bound (class, alpha)", model, tid, worst, "blocks", ran, "empty", empty)


# ------------------------------------------------------------------ 2. the same bits for every geometry
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_same_bits_for_every_block_size_and_alignment(ctx, dtype):
    cases = [("tfim", (16, 0, 1, 1), None), ("heisenberg", (12, 6, -1, -1), 6)]
    if _cplx(dtype):
        cases += [("xyz", (9, 3, 0, -1), None)]
    try:
        for model, shape, nd in cases:
            terms = model_terms(model, shape[0])
            op = _op(ctx, shape, terms, dtype, nd)
            assert op.n == (DIMS if nd is None else DIMS_HALF).get(shape, op.n)
            x = K.start_x(op.n, dtype)
            first = None
            for bits in [None, 0, 1, 4, 8, 12]:
                _set_block_bits(ctx, "symmetric", bits)
                for shift in (0, 1):
                    for rep in range(2):
                        y, _ = _apply(ctx, op, x, shift, -2.5, False)      # _apply asserts that the input is left unchanged
                        if first is None:
                            first = y
                        assert np.array_equal(first.view(np.uint8), y.view(np.uint8)), (model, shape, bits, shift, rep)
            assert np.any(first != 0)
            op.close()
    finally:
        _set_block_bits(ctx, "symmetric", None)


# ------------------------------------------------------------------ 3. the same bits as the full-space momentum operator
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_same_bits_as_the_momentum_operator_of_the_full_space_with_every_flag_zero(ctx, dtype):
    cases = [("tfim", 12, 0), ("xyz", 6, 3)]
    if _cplx(dtype):
        cases += [("xyz_dm_x", 16, 5)]
    for model, n_sites, m in cases:
        terms = model_terms(model, n_sites)
        ref = L.PauliMomentumFullOperator(ctx, n_sites, m, terms, dtype)
        op = L.PauliSymmetricOperator(ctx, n_sites, m, terms, dtype)
        assert op.n == ref.n and (op.parity, op.inversion, op.n_down) == (0, 0, None)
        x = K.start_x(op.n, dtype)
        for offset in (0.0, -2.5):
            y0, a0 = _apply(ctx, ref, x, 0, offset, True)
            y1, a1 = _apply(ctx, op, x, 0, offset, True)
            assert np.array_equal(y0.view(np.uint8), y1.view(np.uint8)), (model, n_sites, m, offset)
            assert a0 == a1
        assert np.any(y0 != 0)
        ref.close()
        op.close()


# ------------------------------------------------------------------ 4. consistency on the GPU through the embedding
CONSISTENCY = [("tfim", (12, 0, 1, 1), None), ("xyz", (12, 6, -1, -1), None), ("xyz", (12, 0, 1, 0), None),
               ("xyz", (12, 5, 0, -1), None), ("heisenberg", (12, 0, 1, 1), 6), ("heisenberg", (12, 6, -1, -1), 6),
               ("heisenberg", (12, 0, 1, 0), 6)]


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64], ids=["z", "c"])
@pytest.mark.parametrize("model,shape,nd", CONSISTENCY, ids=["%s-%s-%s" % c for c in CONSISTENCY])
def test_consistent_with_the_full_and_sector_operators_through_the_embedding(ctx, dtype, model, shape, nd):
    """y = B^H H (B x), H applied by PauliOperator on the 4096 states (PauliSectorOperator on the 924 of n_down = 6).  Bound, formed
    as test_gpu_pauli_momentum_full forms it: the block apply's class bound, plus the big apply's class bound and the rounding of
    its input (B x formed on the host in double, one complex product per element, then rounded to T: <= 4 eps_T per element,
    which H carries to <= 4 eps_T sum |a||x|) pushed through |B|^T, plus the host projection (a column of B holds <= 4 L entries:
    (4 L + 4) eps_d |B|^T |Y|)."""
    n_sites, m, p, z = shape
    eps = _eps(dtype)
    terms = model_terms(model, n_sites)
    if nd is None:
        big = L.PauliOperator(ctx, n_sites, terms, dtype)
        big_csr = G.pauli_csr(n_sites, terms, np.complex128, merge=False)
    else:
        big = L.PauliSectorOperator(ctx, n_sites, nd, terms, dtype)
        big_csr = G.pauli_sector_csr(n_sites, nd, terms, np.complex128, merge=False)
    csr = G.pauli_symmetric_csr(n_sites, m, p, z, terms, np.complex128, n_down=nd, merge=False)
    x = K.start_x(csr[0].shape[0] - 1, dtype)
    ex = E.rows_exact(csr, x)
    col, val = G.symmetric_embedding(n_sites, m, p, z, nd, dense=False)
    inb = col >= 0
    X = np.zeros(col.shape[0], np.complex128)
    X[inb] = val[inb] * x.astype(np.complex128)[col[inb]]
    X = X.astype(dtype)
    Y, _ = _apply(ctx, big, X, 0, 0.0, False)
    big.close()
    big_ex = E.rows_exact(big_csr, X)
    big_cls = E.componentwise_bound(big_ex, eps) + eps * E.abs1(Y) + 4 * eps * big_ex.absrow

    def push(v):   # |B|^T v
        return np.bincount(col[inb], weights=E.abs1(val[inb]) * v[inb], minlength=x.shape[0])

    proj = np.zeros(x.shape[0], np.complex128)
    np.add.at(proj, col[inb], np.conj(val[inb]) * Y.astype(np.complex128)[inb])
    op = _op(ctx, shape, terms, dtype, nd)
    y, _ = _apply(ctx, op, x, 0, 0.0, False)
    op.close()
    cls, _ = _class_bound(dtype, x, ex, y, 0.0)
    bound = cls + push(big_cls) + (4 * n_sites + 4) * E.EPS_D * push(E.abs1(Y))
    ok, r = E.within(E.part_errors(y, proj), (bound, bound))
    assert ok, (model, shape, nd, r)
    assert np.any(y != 0)
    print("block apply against B^H (big apply) B: error / bound", model, shape, nd, r)


# ------------------------------------------------------------------ 5. deferred normalisation
@pytest.mark.parametrize("shape,model,dtype", [((12, 5, 0, -1), "xyz", np.complex128), ((12, 6, -1, -1), "tfim", np.float64)],
                         ids=["12-5-z", "12-6-d"])
def test_deferred_normalisation_path_against_separate_launches(ctx, shape, model, dtype):
    """fuse_launches = 1 and 2 (the kernel normalises its input on the fly through ScaleIn) against 0 (a launch of its own), 16
    indices per block: traces to 1e-10 |A|_inf per k, iteration counts within 2 (the rule of the momentum operators' tests)."""
    terms = model_terms(model, shape[0])
    op = _op(ctx, shape, terms, dtype)
    n = op.n
    init = G.start_vector(n, 1).astype(dtype)
    norm = op.inf_norm()
    runs = {}
    try:
        _set_block_bits(ctx, "symmetric", 4)
        for level in ("0", "1", "2"):
            ctx.set_tuning("fuse_launches", level)
            eng, vals, _ = _run_lanczos(op, n, init, False, -norm)
            runs[level] = (eng.last_alpha, eng.last_beta, vals[0], eng.getIterationCounts())
    finally:
        ctx.set_tuning("fuse_launches", None)
        _set_block_bits(ctx, "symmetric", None)
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
EIGEN_CASES = [("d", "tfim", (12, 0, 1, 1)), ("s", "tfim", (12, 0, 1, 1)), ("z", "xyz", (12, 5, 0, -1))]


@pytest.mark.parametrize("num_eigs", [1, 3])
@pytest.mark.parametrize("find_max", [False, True], ids=["smallest", "largest"])
@pytest.mark.parametrize("tid,model,shape", EIGEN_CASES, ids=["%s-%s-%s" % c for c in EIGEN_CASES])
def test_lanczos_against_the_reference(ctx, tid, model, shape, find_max, num_eigs):
    n_sites, m, p, z = shape
    dtype = TYPES[TYPE_IDS.index(tid)]
    terms = model_terms(model, n_sites)
    csr = G.pauli_symmetric_csr(n_sites, m, p, z, terms, WIDE[tid])
    n = csr[0].shape[0] - 1
    init = G.start_vector(n, 1).astype(dtype)
    op = _op(ctx, shape, terms, dtype)
    assert op.n == n
    norm = op.inf_norm()
    assert abs(norm - sum(abs(c) for _, _, c in terms)) <= 1e-12 * norm
    offset = norm if find_max else -norm
    eng, vals, vecs = _run_lanczos(op, n, init, find_max, offset, num_eigs=num_eigs)
    ref = _checker().lanczos(csr, init.astype(WIDE[tid]), find_max, num_eigs=num_eigs, offset=offset, eps=eng.eps)
    scale = max(1.0, np.max(np.abs(ref["eigenvalues"] + offset)))
    err = np.max(np.abs(vals - ref["eigenvalues"]))
    print("block %s %s %s: max |lambda - reference| = %.3e, bound %.3e" % (shape, tid, model, err, 20 * eng.eps * scale))
    assert len(vals) == num_eigs
    assert err <= 20 * eng.eps * scale
    op.close()


def test_exponentiator_against_the_reference(ctx):
    shape = (12, 5, 0, -1)
    terms = model_terms("xyz", shape[0])
    csr = G.pauli_symmetric_csr(*shape, terms, np.complex128)
    n = csr[0].shape[0] - 1
    inp = G.start_vector(n, 2, np.complex128)
    a = -0.05j
    op = _op(ctx, shape, terms, np.complex128)
    ex = L.Exponentiator(op, n)
    out, it = ex.run(a, inp)
    o_out, o_it, _ = _checker().expo(csr, a, inp, eps=ex.eps)
    assert abs(it - o_it) <= 2
    assert 1 - overlap(out, o_out) <= 10 * ex.eps
    assert abs(np.linalg.norm(out) / np.linalg.norm(inp) - 1) <= 1e-12
    op.close()


def test_ground_energy_of_the_16_site_tfim_ring_lies_in_the_fully_symmetric_block(ctx):
    """TFIM ring, L = 16, fp64: the lowest energy of the block (m, p, z) = (0, +1, +1) — 1162 of the 65 536 states — is the exact
    ground energy of the ring (generators.tfim_ring_ground_energy: free fermions; generators.tfim_ground_energy is the OPEN
    chain's and lies 0.7 above), and the lowest energy of the block (0, -1, +1) lies clearly above it."""
    n_sites = 16
    terms = model_terms("tfim", n_sites)
    e0 = G.tfim_ring_ground_energy(n_sites, 1.0, 0.7)
    op = _op(ctx, (n_sites, 0, 1, 1), terms, np.float64)
    norm = op.inf_norm()
    assert op.n == 1162
    eng, vals, _ = _run_lanczos(op, op.n, G.start_vector(op.n, 1), False, -norm)
    op.close()
    odd = _op(ctx, (n_sites, 0, -1, 1), terms, np.float64)
    assert odd.n == 906
    _, vals_odd, _ = _run_lanczos(odd, odd.n, G.start_vector(odd.n, 1), False, -norm)
    odd.close()
    scale = max(1.0, abs(e0 - norm))
    print("TFIM ring L = 16: exact E0 %.13f, block (0,+,+) %.13f, block (0,-,+) %.13f" % (e0, vals[0], vals_odd[0]))
    assert abs(vals[0] - e0) <= 20 * eng.eps * scale
    assert vals_odd[0] > e0 + 0.1


# ------------------------------------------------------------------ 7. refusals
def _refused(ctx, n_sites, m, terms, dtype=np.float64, **kw):
    with pytest.raises(capi.LanczosHipError) as e:
        L.PauliSymmetricOperator(ctx, n_sites, m, terms, dtype, **kw).close()
    assert e.value.code == capi.LL_ERR_INVALID, str(e.value)
    return str(e.value)


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_invalid_inputs_are_refused_with_their_cause(ctx, dtype):
    ring = G.xyz_terms(6, 1.0, 0.6, 0.8)
    heis = G.heisenberg_terms(6, 1.0, 1.0, periodic=True)
    # everything the full-space momentum operator refuses
    for m in (-1, 6):
        assert "momentum must lie in [0, n_sites)" in _refused(ctx, 6, m, ring, dtype)
    odd_y = model_terms("xyz_dm_x", 6)
    if not _cplx(dtype):
        msg = _refused(ctx, 6, 1, ring, dtype)
        assert "real storage type" in msg and "momentum 0 and n_sites / 2" in msg, msg
        assert "odd number of Y" in _refused(ctx, 6, 0, odd_y, dtype)
    else:
        L.PauliSymmetricOperator(ctx, 6, 1, ring, dtype, inversion=-1).close()
        L.PauliSymmetricOperator(ctx, 6, 0, odd_y, dtype).close()
    msg = _refused(ctx, 6, 0, G.tfim_terms(6, 1.0, 0.7, periodic=False), dtype, parity=1)   # an open chain: bond (5, 0) is missing
    assert "does not commute with the one-site translation" in msg and "term 4 (x_mask 0x0, z_mask 0x30)" in msg, msg
    for n_sites in (0, 31):
        assert "n_sites" in _refused(ctx, n_sites, 0, ring, dtype)
    assert "a mask bit at or above n_sites" in _refused(ctx, 6, 0, ring + [(1 << 6, 0, 1.0)], dtype)
    assert "not finite" in _refused(ctx, 6, 0, ring + [(0, 0, float("nan"))], dtype)
    # the flags
    for bad in (2, -2):
        assert "parity must be 0" in _refused(ctx, 6, 0, ring, dtype, parity=bad)
        assert "inversion must be 0" in _refused(ctx, 6, 0, ring, dtype, inversion=bad)
    if _cplx(dtype):
        msg = _refused(ctx, 6, 1, ring, dtype, parity=1)
        assert "parity != 0 takes momentum 0 and n_sites / 2 only" in msg, msg
    # H against the reflection: the first Dzyaloshinskii-Moriya term of the ring (x_mask 0x3, z_mask 0x2)
    if _cplx(dtype):
        msg = _refused(ctx, 6, 0, heis + dm_ring(6, 0.35), dtype, parity=1)
        assert "does not commute with the reflection" in msg and "term %d (x_mask 0x3, z_mask 0x2)" % len(heis) in msg, msg
        L.PauliSymmetricOperator(ctx, 6, 0, heis + dm_ring(6, 0.35), dtype).close()     # fine without the reflection
    # a term pair that the translation keeps and the reflection does not: Z_j Z_{j+1} X_{j+3} on every site
    chiral = [(1 << ((j + 3) % 6), (1 << j) | (1 << ((j + 1) % 6)), 0.3) for j in range(6)]
    msg = _refused(ctx, 6, 0, ring + chiral, dtype, parity=1)
    assert "does not commute with the reflection" in msg and "term %d (x_mask 0x8, z_mask 0x3)" % len(ring) in msg, msg
    # H against the global flip: a longitudinal field
    msg = _refused(ctx, 6, 0, ring + G.zfield_terms(6, 0.3), dtype, inversion=1)
    assert "does not commute with the global spin flip" in msg and "term %d (x_mask 0x0, z_mask 0x1)" % len(ring) in msg, msg
    L.PauliSymmetricOperator(ctx, 6, 0, ring + G.zfield_terms(6, 0.3) + G.zfield_terms(6, -0.3), dtype, inversion=1).close()
    # n_down
    for nd in (-2, 7):
        assert "n_down must lie in [-1, n_sites]" in _refused(ctx, 6, 0, heis, dtype, n_down=nd)
    assert "do not conserve S_z" in _refused(ctx, 6, 0, ring, dtype, n_down=3)
    msg = _refused(ctx, 6, 0, heis, dtype, inversion=1, n_down=2)
    assert "needs 2 n_down = n_sites" in msg, msg
    # empty blocks
    for kw in (dict(parity=-1), dict(parity=-1, inversion=1), dict(parity=-1, inversion=-1)):
        assert "is empty" in _refused(ctx, 4, 0, G.xyz_terms(4, 1.0, 0.6, 0.8), dtype, **kw)
    assert "is empty" in _refused(ctx, 6, 0, ring, dtype, parity=-1, inversion=1)
    # the queries of a non-CSR operator
    ok = L.PauliSymmetricOperator(ctx, 6, 0, heis, dtype, parity=1, inversion=1, n_down=3)
    assert ok.n == G.symmetric_basis(6, 0, 1, 1, 3)[0].shape[0]
    with pytest.raises(capi.LanczosHipError):
        L.CsrOperator.select_spmv(ok, capi.SPMV_CSR_STREAM)
    with pytest.raises(capi.LanczosHipError):
        L.CsrOperator.set_accuracy(ok, capi.ACCURACY_NORMWISE)
    assert L.CsrOperator.accuracy(ok) == capi.ACCURACY_COMPONENTWISE
    ok.close()


# ------------------------------------------------------------------ 8. degenerate operators
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_zero_and_diagonal_operators(ctx, dtype):
    n_sites = 8
    for m, p, z in [(0, 1, 1), (4, -1, -1), (0, -1, 0)] + ([(3, 0, -1)] if _cplx(dtype) else []):
        reps, _ = G.symmetric_basis(n_sites, m, p, z)
        n = reps.shape[0]
        x = K.start_x(n, dtype)
        xd, yd = ctx.to_device(x), ctx.empty(n, dtype)
        op = _op(ctx, (n_sites, m, p, z), [], dtype)                                   # no term: the zero operator
        assert op.info() == (n, n, 0) and op.inf_norm() == 0.0
        L.spmv(op, xd, yd, offset=0.0)
        assert np.all(yd.get() == 0)
        op.close()
        op = _op(ctx, (n_sites, m, p, z), [(0, 0, 0.5)], dtype)                        # the identity term: coef x
        L.spmv(op, xd, yd, offset=0.0)
        assert np.array_equal(yd.get(), (0.5 * x.astype(WIDE[_tid(dtype)])).astype(dtype))
        op.close()
        zz = [(0, (1 << j) | (1 << ((j + 1) % n_sites)), 0.25) for j in range(n_sites)]  # ZZ only: diagonal, even under the flip
        op = _op(ctx, (n_sites, m, p, z), [(0, 0, 0.5)] + zz, dtype)
        L.spmv(op, xd, yd, offset=0.0)                                 # 0.5 + 0.25 (L - 2 domain walls): exact in every T
        r = reps.astype(np.int64)
        rot = ((r << 1) | (r >> (n_sites - 1))) & ((1 << n_sites) - 1)
        walls = np.array([bin(int(v)).count("1") for v in r ^ rot])
        want = (0.5 + 0.25 * (n_sites - 2 * walls)) * x.astype(WIDE[_tid(dtype)])
        assert np.array_equal(yd.get(), want.astype(dtype))
        op.close()
        xd.free()
        yd.free()


# ------------------------------------------------------------------ 9. sharded contexts
def test_refused_on_a_sharded_context(tmp_path):
    """Two ranks on the box's GPU over the test transport: the operator is single-GPU."""
    from conftest import SHM_TRANSPORT

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name = "/ll_shm_psy_" + uuid.uuid4().hex[:12]
    env = dict(os.environ, LL_COMM_PLUGIN=SHM_TRANSPORT, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(root, "tests", "shm_pauli_refused_worker.py"), str(r), "2", name,
                               str(tmp_path), "symmetric"], env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-4000:]
    for r in range(2):
        res = json.load(open(os.path.join(tmp_path, "rank%d.json" % r)))
        assert res["code"] == capi.LL_ERR_INVALID and "sharded" in res["msg"], res
