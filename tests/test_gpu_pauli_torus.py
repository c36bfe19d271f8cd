"""The sum-of-Pauli-strings operator on one translation block of an Lx x Ly torus (ll_op_create_pauli_torus,
csrc/pauli_torus.hip): every apply against the EXACT host reference of the block B^H H B (generators.pauli_torus_csr, one entry
per term and state) with the component-wise class, the same bits for every block size and alignment, the same bits as
PauliSymmetricOperator(parity = inversion = 0) where the torus is a ring, consistency on the GPU with PauliOperator and
PauliSectorOperator through the embedding B, whole eigen-solver, two-pass and Exponentiator runs, expectation values on the
block, the refusals and the image's size.

As for the ring's blocks the single-type storage-product contract of the CSR kernels is NOT asserted: an entry of the block is a
weight times sqrt(R_a / R_b) times a phase, formed in double (lanczos_hip.h (11), ACCURACY)."""
import numpy as np
import pytest

import contract_cases as K
import exact_ref as E
import lambda_lanczos_amd as L
from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G
from pauli_cases import TYPES, TYPE_IDS, WIDE, _apply, _check_apply, _checker, _class_bound, _cplx, _run_lanczos, _tid
from test_gpu_accuracy_contracts import OFFSETS, _eps
from util import overlap

pytestmark = pytest.mark.gpu

BITS_KEY = "pauli_torus_block_bits"
BLOCK_BITS = [None, 4, 8, 10]      # default, 16, 256 and 1024 indices per block (1024: four states per lane)
E0_4X4 = -11.228483208428853       # the 4 x 4 Heisenberg torus (32 bonds), block (0, 0) at n_down = 8: numpy eigvalsh
SHAPES = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 2), (2, 3), (3, 3), (4, 2), (4, 3), (3, 4), (4, 4)]
COMPLEX_ONLY_SHAPE = ((5, 2), (2, 1))   # at (mx, my) = (2, 1), z / c
MODELS = ("tfim", "xyz_dm_x", "j1j2", "j1j2_sector")
COMPLEX_MODELS = ("xyz_dm_x",)     # the Dzyaloshinskii-Moriya terms carry one Y each


def _set_bits(ctx, bits):
    ctx.set_tuning(BITS_KEY, None if bits is None else str(bits))   # None removes the setting


def xyz_dm_torus_terms(lx, ly):
    """XYZ couplings that differ along x and y, a Dzyaloshinskii-Moriya term on every directed bond (x, y) -> (x + 1, y) and a
    transverse field: commutes with the two translations and with nothing else (complex Hermitian, S_z not conserved)."""
    terms = []
    for (dx, dy), (jx, jy, jz) in (((1, 0), (1.0, 0.6, 0.8)), ((0, 1), (0.9, 0.5, 0.7))):
        for a, b in G.torus_bonds(lx, ly, dx, dy):
            m = (1 << a) | (1 << b)
            terms += [(m, 0, jx), (m, m, jy), (0, m, jz)]
    if lx > 1:
        for y in range(ly):
            for x in range(lx):
                a, b = 1 << (x + lx * y), 1 << ((x + 1) % lx + lx * y)
                terms += [(a | b, b, 0.35), (a | b, a, -0.35)]
    return terms + [(1 << j, 0, -0.45) for j in range(lx * ly)]


def model_terms(model, lx, ly):
    if model == "tfim":
        return G.tfim_torus_terms(lx, ly, 1.0, 0.7)
    if model == "xyz_dm_x":
        return xyz_dm_torus_terms(lx, ly)
    if model in ("j1j2", "j1j2_sector"):
        return G.heisenberg_torus_terms(lx, ly, 1.0, 0.5)
    raise KeyError(model)


def _n_down(model, lx, ly):
    return (lx * ly) // 2 if model == "j1j2_sector" else None


def _momenta(shape, dtype):
    """d / s: every (mx, my) at which the block is real.  z / c: all of them up to 3 x 3; on the larger shapes the real ones and
    two with complex phases."""
    lx, ly = shape
    real = [(mx, my) for mx in range(lx) for my in range(ly) if (2 * mx) % lx == 0 and (2 * my) % ly == 0]
    if not _cplx(dtype):
        return real
    if lx * ly <= 9:
        return [(mx, my) for mx in range(lx) for my in range(ly)]
    return real + [(1, 1), (lx - 1, 0)]


def _cases(model, dtype):
    out = [(s, m) for s in SHAPES for m in _momenta(s, dtype)]
    if _cplx(dtype):
        out.append(COMPLEX_ONLY_SHAPE)
    return out


_REF = {}


def _reference_rows(model, shape, mom, tid):
    """(terms, csr with one entry per term and state, x, exact rows) or None for an empty block: computed once per module."""
    key = (model, shape, mom, tid)
    if key not in _REF:
        dtype = TYPES[TYPE_IDS.index(tid)]
        (lx, ly), (mx, my) = shape, mom
        terms = model_terms(model, lx, ly)
        nd = _n_down(model, lx, ly)
        if G.torus_basis(lx, ly, mx, my, nd)[0].shape[0] == 0:
            _REF[key] = None
        else:
            csr = G.pauli_torus_csr(lx, ly, mx, my, terms, WIDE[tid], n_down=nd, merge=False)   # doubles for every T
            x = K.start_x(csr[0].shape[0] - 1, dtype)
            _REF[key] = (terms, csr, x, E.rows_exact(csr, x))
    return _REF[key]


def _op(ctx, shape, mom, terms, dtype, n_down=None):
    return L.PauliTorusOperator(ctx, shape[0], shape[1], mom[0], mom[1], terms, dtype, n_down=n_down)


# ------------------------------------------------------------------ 1. apply against the exact reference
APPLY_CASES = [(m, t, s) for m in MODELS for t in TYPE_IDS if m not in COMPLEX_MODELS or t in ("z", "c")
               for s in SHAPES + ([COMPLEX_ONLY_SHAPE[0]] if t in ("z", "c") else [])]


@pytest.mark.parametrize("model,tid,shape", APPLY_CASES, ids=["%s-%s-%dx%d" % (m, t, s[0], s[1]) for m, t, s in APPLY_CASES])
def test_apply_meets_the_componentwise_contract(ctx, model, tid, shape):
    dtype = TYPES[TYPE_IDS.index(tid)]
    lx, ly = shape
    nd = _n_down(model, lx, ly)
    momenta = [COMPLEX_ONLY_SHAPE[1]] if shape == COMPLEX_ONLY_SHAPE[0] else _momenta(shape, dtype)
    worst = (0.0, 0.0)
    ran = empty = 0
    try:
        for mom in momenta:
            ref = _reference_rows(model, shape, mom, tid)
            if ref is None:                              # an empty block: refused (section 7 checks the message)
                with pytest.raises(capi.LanczosHipError) as e:
                    _op(ctx, shape, mom, model_terms(model, lx, ly), dtype, nd)
                assert "is empty" in str(e.value)
                empty += 1
                continue
            terms, csr, x, ex = ref
            n = x.shape[0]
            op = _op(ctx, shape, mom, terms, dtype, nd)
            assert op.info() == (n, n, len(terms))
            assert (op.n, op.n_local, op.lx, op.ly, op.mx, op.my, op.n_sites, op.n_down) == (n, n, lx, ly, mom[0], mom[1], lx * ly, nd)
            assert op.device_bytes() <= 8 * n + 192 * 1024   # reps, orbit lengths, the bucket table, the small tables: O(D)
            for bits in (None, 4):                       # several kernel blocks at 2^4 indices (section 2: every size, the same bits)
                _set_bits(ctx, bits)
                for shift in (0, 1):
                    for offset in OFFSETS:
                        y, alpha = _apply(ctx, op, x, shift, offset, True)
                        r = _check_apply(dtype, x, ex, y, alpha, offset, "%s %s %s %s" % (model, tid, shape, mom))
                        worst = tuple(max(a, b) for a, b in zip(worst, r))
            op.close()
            ran += 1
    finally:
        _set_bits(ctx, None)
    assert ran + empty == len(momenta) and ran >= 1
    if nd is None:
        assert empty == 0                                # no full-space block of the listed shapes is empty
    print("ratios error/bound (class, alpha)", model, tid, shape, worst, "blocks", ran, "empty", empty)


def test_at_least_nine_in_ten_of_the_listed_blocks_are_not_empty():
    """What test_apply_meets_the_componentwise_contract runs, counted from the generator: an empty block is refused there and runs
    no apply."""
    listed = run = 0
    for model, tid, shape in APPLY_CASES:
        dtype = TYPES[TYPE_IDS.index(tid)]
        momenta = [COMPLEX_ONLY_SHAPE[1]] if shape == COMPLEX_ONLY_SHAPE[0] else _momenta(shape, dtype)
        for mx, my in momenta:
            listed += 1
            run += G.torus_basis(shape[0], shape[1], mx, my, _n_down(model, *shape))[0].shape[0] > 0
    print("listed blocks", listed, "with an apply", run)
    assert run >= 0.9 * listed


# ------------------------------------------------------------------ 2. the same bits for every geometry
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_same_bits_for_every_block_size_and_alignment(ctx, dtype):
    cases = [("tfim", (4, 4), (0, 0), None), ("j1j2", (4, 3), (2, 0), 6), ("j1j2", (4, 4), (2, 2), None)]
    if _cplx(dtype):
        cases += [("xyz_dm_x", (3, 4), (1, 3), None), ("j1j2", (4, 4), (1, 2), 8)]
    try:
        for model, shape, mom, nd in cases:
            op = _op(ctx, shape, mom, model_terms(model, *shape), dtype, nd)
            assert op.n == G.torus_basis(shape[0], shape[1], mom[0], mom[1], nd)[0].shape[0]
            x = K.start_x(op.n, dtype)
            first = None
            for bits in BLOCK_BITS:
                _set_bits(ctx, bits)
                for shift in (0, 1):
                    for rep in range(2):
                        y, _ = _apply(ctx, op, x, shift, -2.5, False)      # _apply asserts that the input is left unchanged
                        if first is None:
                            first = y
                        assert np.array_equal(first.view(np.uint8), y.view(np.uint8)), (model, shape, mom, bits, shift, rep)
            assert np.any(first != 0)
            op.close()
    finally:
        _set_bits(ctx, None)


# ------------------------------------------------------------------ 3. a torus of one row or one column is the ring
RING_CASES = [((8, 1), 5, "z", None), ((1, 8), 5, "z", None), ((12, 1), 5, "z", None), ((12, 1), 5, "z", 6), ((9, 1), 3, "z", None),
              ((1, 8), 4, "d", None), ((8, 1), 0, "s", 4), ((1, 8), 5, "c", None)]


@pytest.mark.parametrize("shape,m,tid,nd", RING_CASES, ids=["%dx%d-m%d-%s-nd%s" % (s[0], s[1], m, t, nd) for s, m, t, nd in RING_CASES])
def test_same_bits_as_the_ring_operator(ctx, shape, m, tid, nd):
    dtype = TYPES[TYPE_IDS.index(tid)]
    n_sites = shape[0] * shape[1]
    if nd is not None:
        terms = G.heisenberg_terms(n_sites, 1.0, 0.8, periodic=True)
    elif _cplx(dtype):
        terms = G.xyz_terms(n_sites, 1.0, 0.6, 0.8) + G.dm_terms(n_sites, 0.35, periodic=True) + [(1 << j, 0, -0.45) for j in range(n_sites)]
    else:
        terms = G.xyz_terms(n_sites, 1.0, 0.6, 0.8) + [(1 << j, 0, -0.45) for j in range(n_sites)]
    mom = (m, 0) if shape[1] == 1 else (0, m)
    ring = L.PauliSymmetricOperator(ctx, n_sites, m, terms, dtype, parity=0, inversion=0, n_down=nd)
    op = _op(ctx, shape, mom, terms, dtype, nd)
    assert op.n == ring.n
    x = K.start_x(op.n, dtype)
    for offset in (0.0, -2.5):
        y0, a0 = _apply(ctx, ring, x, 0, offset, True)
        y1, a1 = _apply(ctx, op, x, 0, offset, True)
        assert np.array_equal(y0.view(np.uint8), y1.view(np.uint8)), (shape, m, offset)
        assert a0 == a1
    assert np.any(y0 != 0)
    ring.close()
    op.close()


# ------------------------------------------------------------------ 4. consistency on the GPU through the embedding
CONSISTENCY = [("tfim", (3, 3), (0, 0), None), ("xyz_dm_x", (3, 3), (1, 2), None), ("j1j2", (3, 3), (2, 0), 4),
               ("j1j2", (4, 3), (0, 0), 6), ("j1j2", (4, 3), (1, 2), 6), ("xyz_dm_x", (4, 3), (2, 1), None)]


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64], ids=["z", "c"])
@pytest.mark.parametrize("model,shape,mom,nd", CONSISTENCY, ids=["%s-%dx%d-%d%d-%s" % (c[0], *c[1], *c[2], c[3]) for c in CONSISTENCY])
def test_consistent_with_the_full_and_sector_operators_through_the_embedding(ctx, dtype, model, shape, mom, nd):
    """B (H_block c) against H (B c), H applied by PauliOperator (PauliSectorOperator with n_down), compared in the block:
    y = B^H H (B x).  Bound, formed as tests/test_gpu_pauli_symmetric.py forms it: the block apply's class bound, plus the big apply's
    class bound and the rounding of its input (B x formed on the host in double, one complex product per element, then rounded to
    T: <= 4 eps_T per element, which H carries to <= 4 eps_T sum |a||x|) pushed through |B|^T, plus the host projection (a column
    of B holds <= Lx Ly entries: (Lx Ly + 4) eps_d |B|^T |Y|)."""
    (lx, ly), (mx, my) = shape, mom
    n_sites = lx * ly
    eps = _eps(dtype)
    terms = model_terms(model, lx, ly)
    if nd is None:
        big = L.PauliOperator(ctx, n_sites, terms, dtype)
        big_csr = G.pauli_csr(n_sites, terms, np.complex128, merge=False)
    else:
        big = L.PauliSectorOperator(ctx, n_sites, nd, terms, dtype)
        big_csr = G.pauli_sector_csr(n_sites, nd, terms, np.complex128, merge=False)
    csr = G.pauli_torus_csr(lx, ly, mx, my, terms, np.complex128, n_down=nd, merge=False)
    x = K.start_x(csr[0].shape[0] - 1, dtype)
    ex = E.rows_exact(csr, x)
    col, val = G.torus_embedding(lx, ly, mx, my, nd, dense=False)
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
    op = _op(ctx, shape, mom, terms, dtype, nd)
    y, _ = _apply(ctx, op, x, 0, 0.0, False)
    op.close()
    cls, _ = _class_bound(dtype, x, ex, y, 0.0)
    bound = cls + push(big_cls) + (n_sites + 4) * E.EPS_D * push(E.abs1(Y))
    ok, r = E.within(E.part_errors(y, proj), (bound, bound))
    assert ok, (model, shape, mom, nd, r)
    assert np.any(y != 0)
    print("block apply against B^H (big apply) B: error / bound", model, shape, mom, nd, r)


# ------------------------------------------------------------------ 5. whole runs
_GROUND = {}


def _ground_4x4():
    """(terms, csr of the block (0, 0) at n_down = 8, its lowest eigenvalue and eigenvector by numpy): once per module."""
    if not _GROUND:
        terms = G.heisenberg_torus_terms(4, 4)
        csr = G.pauli_torus_csr(4, 4, 0, 0, terms, np.float64, n_down=8)
        n = csr[0].shape[0] - 1
        w, V = np.linalg.eigh(np.asarray(K.dense_of(csr, n), dtype=np.float64))
        assert n == 822 and abs(w[0] - E0_4X4) <= 1e-12
        V[:, 0].setflags(write=False)
        _GROUND.update(terms=terms, csr=csr, n=n, e0=w[0], v0=V[:, 0])
    return _GROUND


@pytest.mark.parametrize("tid", ["d", "z"])
def test_lanczos_and_two_pass_reach_the_ground_energy_of_the_4_by_4_heisenberg_torus(ctx, tid):
    g = _ground_4x4()
    dtype = TYPES[TYPE_IDS.index(tid)]
    n = g["n"]
    op = _op(ctx, (4, 4), (0, 0), g["terms"], dtype, 8)
    try:
        assert op.n == n
        norm = op.inf_norm()
        assert abs(norm - sum(abs(c) for _, _, c in g["terms"])) <= 1e-12 * norm
        init = G.start_vector(n, 1).astype(dtype)
        eng, vals, vecs = _run_lanczos(op, n, init, False, -norm)
        scale = max(1.0, abs(E0_4X4 - norm))
        print("4 x 4 Heisenberg torus %s: stored basis %.15f, exact %.15f, bound %.3e" % (tid, vals[0], E0_4X4, 20 * eng.eps * scale))
        assert abs(vals[0] - E0_4X4) <= 20 * eng.eps * scale
        assert 1 - overlap(vecs[0], g["v0"].astype(vecs[0].dtype)) <= 1e-8
        two = L.LambdaLanczos(op, n, False, 1)
        two.eigenvalue_offset = -norm
        two.init_vector = lambda v, *_: np.copyto(v, init)
        val, vec, info = two.run_two_pass()
        print("two-pass %.15f after %d iterations" % (val, info["iterations"]))
        assert abs(val - E0_4X4) <= 20 * two.eps * scale
        assert 1 - overlap(vec, g["v0"].astype(vec.dtype)) <= 1e-8
    finally:
        op.close()


def test_exponentiator_against_the_reference(ctx):
    shape, mom = (4, 3), (1, 2)
    terms = model_terms("xyz_dm_x", *shape)
    csr = G.pauli_torus_csr(*shape, *mom, terms, np.complex128)
    n = csr[0].shape[0] - 1
    inp = G.start_vector(n, 2, np.complex128)
    a = -0.05j
    op = _op(ctx, shape, mom, terms, np.complex128)
    ex = L.Exponentiator(op, n)
    out, it = ex.run(a, inp)
    o_out, o_it, _ = _checker().expo(csr, a, inp, eps=ex.eps)
    assert abs(it - o_it) <= 2
    assert 1 - overlap(out, o_out) <= 10 * ex.eps
    assert abs(np.linalg.norm(out) / np.linalg.norm(inp) - 1) <= 1e-12
    op.close()


# ------------------------------------------------------------------ 6. expectation values on the block
def _expect_reference(lx, ly, mx, my, nd, c, obs):
    """want_k = coef_k Re <Psi, P_k Psi> correctly rounded, Psi = B c in double, with the bound of
    tests/pauli_expect_block_cases.reference: (2 (D S_k + 8) + 32) eps_d scale_k + eps_d |want_k|, scale_k = |coef_k| sum |Psi||P_k Psi|,
    S_k the distinct strings of the average over the translations, D = the block's dimension."""
    n_sites = lx * ly
    col, val = G.torus_embedding(lx, ly, mx, my, nd, dense=False)
    cw = np.asarray(c).astype(np.complex128)
    psi = np.where(col >= 0, val * cw[np.maximum(col, 0)], 0.0).astype(np.complex128)
    states = None if nd is None else G.sector_states(n_sites, nd)
    want, bound = np.zeros(len(obs)), np.zeros(len(obs))
    for k, t in enumerate(obs):
        q = G.pauli_string_apply_np(n_sites, t, psi, states=states)
        want[k] = t[2] * E.dot_exact(psi, q).real
        s_k = len(G.torus_symmetrised_strings(lx, ly, t))
        bound[k] = (2 * (cw.shape[0] * s_k + 8) + 32) * E.EPS_D * abs(t[2]) * E.dot_abs(psi, q) + E.EPS_D * abs(want[k])
    return want, bound


@pytest.mark.parametrize("tid", ["d", "z", "s"])
def test_spin_correlations_of_the_4_by_4_ground_state(ctx, tid):
    """<Z_0 Z_r> for every r, and sum_r (-1)^(x_r + y_r) <S_0 . S_r> (the staggered structure factor S(pi, pi)) from XX, YY and ZZ."""
    g = _ground_4x4()
    dtype = TYPES[TYPE_IDS.index(tid)]
    c = g["v0"].astype(dtype)
    op = _op(ctx, (4, 4), (0, 0), g["terms"], dtype, 8)
    try:
        zz = [(0, 1 | (1 << r), 1.0) for r in range(1, 16)]
        want, bound = _expect_reference(4, 4, 0, 0, 8, c, zz)
        got, sweeps = op.expectation(c, zz, return_sweeps=True)
        assert sweeps == 1
        assert np.all(np.abs(got - want) <= bound), np.max(np.abs(got - want) / bound)
        # two observables of one translation orbit: Z_(0,0) Z_(1,1) and Z_(2,1) Z_(3,2) — the same tables, the same bits
        pair = op.expectation(c, [(0, 1 | (1 << 5), 1.0), (0, (1 << 6) | (1 << 11), 1.0)])
        assert pair[0] == pair[1] == got[4]
        # S_0 . S_r = (XX + YY + ZZ) / 4; YY is real: measured in every type
        sss = []
        for r in range(1, 16):
            m = 1 | (1 << r)
            sign = -1.0 if ((r % 4) + (r // 4)) % 2 else 1.0
            sss += [(m, 0, 0.25 * sign), (m, m, 0.25 * sign), (0, m, 0.25 * sign)]
        want3, bound3 = _expect_reference(4, 4, 0, 0, 8, c, sss)
        got3, sweeps = op.expectation(c, sss, return_sweeps=True)
        assert sweeps == 2                              # 45 observables, 32 per sweep
        assert np.all(np.abs(got3 - want3) <= bound3)
        nn = E.dot_exact(c, c).real
        s_pipi = 0.75 * nn + float(np.sum(got3))
        ref = 0.75 * nn + float(np.sum(want3))
        assert abs(s_pipi - ref) <= float(np.sum(bound3)) + 64 * E.EPS_D * abs(ref)
        assert s_pipi / nn > 3.0                        # antiferromagnetic order: far above the 0.75 of uncorrelated spins
        print("4 x 4 ground state %s: S(pi, pi) = %.12f, max error / bound %.3g" % (tid, s_pipi / nn, np.max(np.abs(got - want) / bound)))
    finally:
        op.close()


@pytest.mark.parametrize("tid", TYPE_IDS)
def test_expectations_on_a_tfim_torus_state(ctx, tid):
    """X_0, the identity, ZZ and XX pairs on a seeded random state of the 4 x 3 block; for z / c a block with complex phases and
    Y-carrying strings (X_0 Y_1, Y_0 Z_5 X_6)."""
    dtype = TYPES[TYPE_IDS.index(tid)]
    shape, mom = (4, 3), ((1, 2) if _cplx(dtype) else (2, 0))
    op = _op(ctx, shape, mom, model_terms("tfim", *shape), dtype)
    try:
        c = K.start_x(op.n, dtype, seed=11)
        obs = [(1, 0, 1.0), (0, 0, 1.0), (0, 1 | (1 << 5), -0.5), (3, 0, 2.0), (1 | (1 << 4), 0, 0.7), (0, 1, 1.5),
               (3, 2, 1.25), (1 | (1 << 6), 1 | (1 << 5), -0.75), (3, 3, 0.3)]
        want, bound = _expect_reference(4, 3, mom[0], mom[1], None, c, obs)
        got = op.expectation(c, obs)
        for k, t in enumerate(obs):
            if not _cplx(dtype) and bin(t[0] & t[1]).count("1") % 2:
                assert got[k] == 0.0 and not np.signbit(got[k])          # an odd nY on a real type: exactly +0.0
            else:
                assert abs(got[k] - want[k]) <= bound[k], (t, got[k], want[k], bound[k])
        assert got[0] != 0.0 and got[1] != 0.0
        moved = op.expectation(c, [(2, 0, 1.0), (1 << 9, 0, 1.0)])       # X on two other sites: the orbit of X_0
        assert moved[0] == moved[1] == got[0]
    finally:
        op.close()


# ------------------------------------------------------------------ 7. refusals
def _refused(ctx, lx, ly, mx, my, terms, dtype=np.float64, n_down=None):
    with pytest.raises(capi.LanczosHipError) as e:
        L.PauliTorusOperator(ctx, lx, ly, mx, my, terms, dtype, n_down=n_down).close()
    assert e.value.code == capi.LL_ERR_INVALID, str(e.value)
    return str(e.value)


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_invalid_inputs_are_refused_with_their_cause(ctx, dtype):
    heis = G.heisenberg_torus_terms(4, 3)
    # an open cylinder: the bonds (x, 2) - (x, 0) are missing; T_x holds, T_y does not
    open_y = [t for t in heis if not any((t[0] | t[1]) == (1 << x) | (1 << (x + 8)) for x in range(4))]
    msg = _refused(ctx, 4, 3, 0, 0, open_y, dtype)
    assert "does not commute with T_y" in msg and "along y" in msg and "x_mask 0x" in msg and "z_mask 0x" in msg, msg
    open_x = [t for t in heis if not any((t[0] | t[1]) == (1 << (4 * y)) | (1 << (4 * y + 3)) for y in range(3))]
    msg = _refused(ctx, 4, 3, 0, 0, open_x, dtype)
    assert "does not commute with T_x" in msg and "along x" in msg, msg
    # a ring of 16 sites is no 4 x 4 torus: T_x takes the bond (2, 3) to (3, 0), which the ring does not hold
    ring16 = G.heisenberg_terms(16, 1.0, 1.0, periodic=True)
    msg = _refused(ctx, 4, 4, 0, 0, ring16, dtype)
    assert G.torus_translation_fault(4, 4, ring16) == ("x", 6)
    assert "does not commute with T_x" in msg and "term 6 (x_mask 0xc, z_mask 0x0)" in msg, msg
    L.PauliTorusOperator(ctx, 16, 1, 0, 0, ring16, dtype).close()
    h44 = G.heisenberg_torus_terms(4, 4)
    if not _cplx(dtype):
        msg = _refused(ctx, 4, 4, 1, 0, h44, dtype)
        assert "real storage type" in msg and "lx / 2" in msg, msg
        msg = _refused(ctx, 4, 4, 0, 3, h44, dtype)
        assert "real storage type" in msg, msg
        assert "odd number of Y" in _refused(ctx, 4, 3, 0, 0, xyz_dm_torus_terms(4, 3), dtype)
    else:
        L.PauliTorusOperator(ctx, 4, 4, 1, 0, h44, dtype, n_down=8).close()
    # S_z: the transverse field leaves the sector
    assert "do not conserve S_z" in _refused(ctx, 4, 3, 0, 0, G.tfim_torus_terms(4, 3, 1.0, 0.7), dtype, n_down=6)
    for nd in (-2, 13):
        assert "n_down must lie in [-1, lx * ly]" in _refused(ctx, 4, 3, 0, 0, heis, dtype, n_down=nd)
    # the shape and the momenta
    assert "lx * ly must be at most 30" in _refused(ctx, 8, 4, 0, 0, [], dtype)
    for lx, ly in ((0, 4), (4, 0), (-1, 3)):
        assert "lx and ly must be at least 1" in _refused(ctx, lx, ly, 0, 0, [], dtype)
    for mx in (-1, 4):
        assert "mx must lie in [0, lx)" in _refused(ctx, 4, 3, mx, 0, heis, dtype)
    for my in (-1, 3):
        assert "my must lie in [0, ly)" in _refused(ctx, 4, 3, 0, my, heis, dtype)
    assert "a mask bit at or above n_sites" in _refused(ctx, 4, 3, 0, 0, heis + [(1 << 12, 0, 1.0)], dtype)
    assert "not finite" in _refused(ctx, 4, 3, 0, 0, heis + [(0, 0, float("nan"))], dtype)
    # an empty block: one flipped spin on 2 x 2 has a full orbit, two on the diagonal are fixed by T_x T_y: n_down = 0 admits (0, 0) only
    assert "is empty" in _refused(ctx, 2, 2, 1, 0, G.heisenberg_torus_terms(2, 2), dtype, n_down=0)


def test_an_unknown_storage_code_is_refused(ctx):
    import ctypes as C

    arr = (capi.PauliTerm * 1)()
    h = C.c_void_p()
    for code in (0, ord("x"), ord("D"), 1):
        st = capi.lib().ll_op_create_pauli_torus(ctx.handle, code, 2, 2, -1, 0, 0, 0, arr, C.byref(h))
        assert st == capi.LL_ERR_INVALID and b"storage must be one of 'd', 'z', 's', 'c'" in capi.lib().ll_last_error()
    for code in "dzsc":
        capi.check(capi.lib().ll_op_create_pauli_torus(ctx.handle, ord(code), 2, 2, -1, 0, 0, 0, arr, C.byref(h)))
        capi.check(capi.lib().ll_op_destroy(h))


def test_what_is_not_built_for_a_torus_block_is_refused_by_name(ctx):
    terms = G.heisenberg_torus_terms(3, 2)
    op = L.PauliTorusOperator(ctx, 3, 2, 0, 0, terms, np.float64)
    other = L.PauliTorusOperator(ctx, 3, 2, 0, 1, terms, np.float64)
    full = L.PauliOperator(ctx, 6, terms, np.float64)
    ring = L.PauliMomentumFullOperator(ctx, 6, 0, G.heisenberg_terms(6), np.float64)
    kind = "a translation block of a torus"
    try:
        c = K.start_x(op.n, np.float64)
        psi = K.start_x(64, np.float64)

        def refused(call):
            with pytest.raises(capi.LanczosHipError) as e:
                call()
            assert e.value.code == capi.LL_ERR_INVALID and kind in str(e.value), str(e.value)

        refused(lambda: L.pauli_block_expand(op, c, full))
        refused(lambda: L.pauli_block_project(op, psi, full))
        refused(lambda: L.pauli_block_transfer(op, other, [(0, 1, 1.0)], c))
        refused(lambda: L.pauli_block_transfer(ring, op, [(0, 1, 1.0)], K.start_x(ring.n, np.float64)))
        refused(lambda: L.pauli_expect(op, c, [(0, 1, 1.0)]))
        refused(lambda: L.pauli_rdm(op, c, [0, 1]))
        refused(lambda: L.pauli_rdm_tiled(op, c, [0, 1, 2, 3]))
        with pytest.raises(capi.LanczosHipError):
            L.CsrOperator.select_spmv(op, capi.SPMV_CSR_STREAM)
        with pytest.raises(capi.LanczosHipError):
            L.CsrOperator.set_accuracy(op, capi.ACCURACY_NORMWISE)
        assert L.CsrOperator.accuracy(op) == capi.ACCURACY_COMPONENTWISE
        # the operator still applies and measures
        nn = E.dot_exact(c, c).real
        assert abs(op.expectation(c, [(0, 0, 1.0)])[0] - nn) <= E.dot_bound(c, c) + E.EPS_D * nn
    finally:
        for o in (op, other, full, ring):
            o.close()


# ------------------------------------------------------------------ 8. the image's size
@pytest.mark.parametrize("nd", [None, 8], ids=["full", "nd8"])
def test_image_size_at_4_by_4(ctx, nd):
    op = L.PauliTorusOperator(ctx, 4, 4, 0, 0, G.heisenberg_torus_terms(4, 4, 1.0, 0.5), np.complex128, n_down=nd)
    assert op.n == (4156 if nd is None else 822)
    assert op.device_bytes() <= 8 * op.n + 192 * 1024
    op.close()
