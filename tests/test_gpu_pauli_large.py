"""The five matrix-free spin-1/2 kernels (csrc/pauli.hip, pauli_sector.hip, pauli_momentum.hip, pauli_momentum_full.hip,
pauli_symmetric.hip) on rings of 20 to 30 sites — the sizes they exist for — against the EXACT rows of the host references
(generators.pauli_*_csr with one entry per term and state, exact_ref.rows_exact), in every type the block admits.  What the
smaller rings of the kernels' own files never reach: bits 18 to 29 of a state or a mask (the rotations and the bit reversal near
L = 30, the sentinel above every state, rank tables of 2^15 entries, remote tiles beyond 2^14 states, 32-bit masks through
ctypes), the bucket search with (nearly) the whole basis in one bucket, and the third and fourth trip of the grid-stride loops
(more than 3 * 2048 blocks).  The cases, their term lists and the pinned dimensions: tests/pauli_large_cases.py; the sum rules
that tie the dimensions: tests/test_pauli_large_host.py.

No new tolerance: the component-wise class and the fused alpha exactly as test_gpu_pauli_momentum._check_apply forms them, the
embedding bound of the 12-site consistency tests, the eigenvalue comparison of the files' test_lanczos_against_the_reference."""
import math

import numpy as np
import pytest

import contract_cases as K
import exact_ref as E
import lambda_lanczos_amd as L
import pauli_large_cases as C
from lambda_lanczos_amd import generators as G
from pauli_cases import BITS_KEY, WIDE, _apply, _check_apply, _checker, _class_bound, _run_lanczos
from test_gpu_accuracy_contracts import OFFSETS, _eps

pytestmark = pytest.mark.gpu

TYPES = {"d": np.float64, "z": np.complex128, "s": np.float32, "c": np.complex64}


def _momentum_of(kind, shape):
    return {"sector": None, "momentum": shape[-1], "momentum_full": shape[1], "symmetric": shape[1]}[kind]


def _tids(kind, shape, model):
    """d, z, s, c where the block is real (2 m mod L = 0, no term with an odd number of Y), else z and c."""
    m = _momentum_of(kind, shape)
    real = model != "dm" and (m is None or (2 * m) % shape[0] == 0)
    return ("d", "z", "s", "c") if real else ("z", "c")


BLOCKS = ([("sector", s, model) for s, model in C.SECTOR] + [("momentum", s, "heisenberg") for s in C.MOMENTUM] +
          [("momentum_full", s, model) for s, (model, _) in C.MOMENTUM_FULL.items()] +
          [("symmetric", s, model) for s, (model, _) in C.SYMMETRIC.items()])
APPLY_CASES = [(kind, shape, model, t) for kind, shape, model in BLOCKS for t in _tids(kind, shape, model)]


def _id(case):
    return "-".join([case[0]] + ["x" if v is None else str(v) for v in case[1]] + [str(v) for v in case[3:]])


def _dim(kind, shape):
    if kind == "sector":
        return math.comb(*shape)
    if kind == "momentum":
        return C.MOMENTUM[shape]
    return (C.MOMENTUM_FULL if kind == "momentum_full" else C.SYMMETRIC)[shape][1]


def _csr(kind, shape, terms, dtype, merge):
    if kind == "sector":
        return G.pauli_sector_csr(*shape, terms, dtype, merge=merge)
    if kind == "momentum":
        return G.pauli_momentum_csr(*shape, terms, dtype, merge=merge)
    if kind == "momentum_full":
        return G.pauli_momentum_full_csr(*shape, terms, dtype, merge=merge)
    n_sites, m, p, z, nd = shape
    return G.pauli_symmetric_csr(n_sites, m, p, z, terms, dtype, n_down=nd, merge=merge)


def _operator(ctx, kind, shape, terms, dtype):
    if kind == "sector":
        return L.PauliSectorOperator(ctx, *shape, terms, dtype)
    if kind == "momentum":
        return L.PauliMomentumOperator(ctx, *shape, terms, dtype)
    if kind == "momentum_full":
        return L.PauliMomentumFullOperator(ctx, *shape, terms, dtype)
    n_sites, m, p, z, nd = shape
    return L.PauliSymmetricOperator(ctx, n_sites, m, terms, dtype, parity=p, inversion=z, n_down=nd)


_REF = {}


def _reference_rows(kind, shape, model, tid):
    """(terms, x, exact rows of the csr with one entry per term and state): computed once per module, never changed."""
    key = (kind, shape, tid)
    if key not in _REF:
        terms = C.model_terms(model, shape[0])
        csr = _csr(kind, shape, terms, WIDE[tid], False)          # entries are doubles for every T
        x = K.start_x(csr[0].shape[0] - 1, TYPES[tid])
        _REF[key] = (terms, x, E.rows_exact(csr, x))
    return _REF[key]


def _check_image(kind, shape, op, n):
    """The pinned dimension, and the size of the image by the bound the kernel's own test file states."""
    assert op.n == n == _dim(kind, shape) and op.n_local == n and op.n_sites == shape[0]
    if kind == "momentum":
        assert (op.n_down, op.momentum) == shape[1:]
        assert op.device_bytes() >= 4 * math.comb(shape[0], shape[1]) + 5 * n    # orbit[], the representatives, their periods
    elif kind == "momentum_full":
        assert op.momentum == shape[1]
        assert op.device_bytes() <= 8 * n + 2 ** 16          # reps, periods, the bucket table and the small tables: O(D_m)
    elif kind == "symmetric":
        assert (op.momentum, op.parity, op.inversion, op.n_down) == shape[1:]
        assert op.device_bytes() <= 8 * n + 192 * 1024       # reps, orbit lengths, the bucket table, the small tables: O(D)
    else:
        assert op.n_down == shape[1]


# ------------------------------------------------------------------ 1. applies against the exact rows
@pytest.mark.parametrize("case", APPLY_CASES, ids=[_id(c) for c in APPLY_CASES])
def test_apply_against_the_exact_rows(ctx, case):
    """Default block bits, and the largest bits at which the grid-stride loop still takes at least three trips with a ragged last
    one (one index per block where D is too small for that: pauli_large_cases.BELOW_WRAP); both at alignment shift 0 and 1 and
    every offset."""
    kind, shape, model, tid = case
    dtype = TYPES[tid]
    terms, x, ex = _reference_rows(kind, shape, model, tid)
    n = x.shape[0]
    small = C.small_bits(n)
    if (kind, shape) in C.BELOW_WRAP:
        assert small == 0 and n < 3 * 2048 + 1               # too few states for a third trip everywhere: the case table says so
    else:
        assert -(-n // (1 << small)) >= 3 * 2048 + 1         # kMaxGrid = 2048 workgroups: three trips of blk += gridDim.x, or more
    op = _operator(ctx, kind, shape, terms, dtype)
    worst = (0.0, 0.0)
    try:
        assert op.info() == (n, n, len(terms))
        _check_image(kind, shape, op, n)
        for bits in (None, small):
            ctx.set_tuning(BITS_KEY[kind], None if bits is None else str(bits))
            for shift in (0, 1):
                for offset in OFFSETS:
                    y, alpha = _apply(ctx, op, x, shift, offset, True)
                    r = _check_apply(dtype, x, ex, y, alpha, offset, "%s bits %s shift %d offset %g" % (_id(case), bits, shift, offset))
                    worst = tuple(max(a, b) for a, b in zip(worst, r))
        assert np.any(y != 0)
    finally:
        ctx.set_tuning(BITS_KEY[kind], None)
        op.close()
    print("ratios error/bound (class, alpha)", kind, tid, shape, "D", n, "small bits", small, worst)


# ------------------------------------------------------------------ 1b. PauliOperator on all 2^20 states
_PAULI_REF = {}


def _pauli_reference(tid):
    """(terms, sample, x, exact rows of the sample): generators.pauli_csr(states=sample) — all 2^20 rows would hold 5e7 entries."""
    if tid not in _PAULI_REF:
        terms = C.pauli_terms(tid in ("z", "c"))
        sample = C.pauli_sample()
        csr = G.pauli_csr(C.PAULI_SITES, terms, WIDE[tid], merge=False, states=sample)
        x = K.start_x(1 << C.PAULI_SITES, TYPES[tid])
        _PAULI_REF[tid] = (terms, sample, x, E.rows_exact(csr, x))
    return _PAULI_REF[tid]


@pytest.mark.parametrize("tid", list(TYPES))
def test_pauli_operator_on_20_sites(ctx, tid):
    """The TFIM ring plus strings on sites 14 to 19 (two with an odd number of Y in z and c), default tile and tiles of 64 states:
    the sampled rows of y against the exact rows with the component-wise class, alpha over the whole vector, and outside the
    sample the symmetry Re<u, H v> = Re<H u, v> for two start vectors.

    The symmetry's tolerance is dot_bound of both sides.  For d and z it covers the applies' own rounding with room to spare (an
    element of H v is off by a few eps_d |y|, dot_bound allows 2 n eps_d per product, n = 2^20).  For s and c an element is off
    by up to eps_f / 2 |y| with no common sign: the sum moves by about eps_f / 2 sqrt(n) rms(|u||y|), 0.06 of the bound at
    n = 2^20 — while ONE wrong element of size 1 moves it by hundreds of times the bound."""
    dtype = TYPES[tid]
    terms, sample, x, ex = _pauli_reference(tid)
    n = x.shape[0]
    assert sample.shape[0] == C.PAULI_SAMPLE and n == 1 << 20
    assert sum(1 for xm, zm, _ in terms if (xm | zm) >> 14) >= 4 + 13     # the strings, the ring's 7 bonds and 6 fields up there
    assert sum(1 for xm, zm, _ in terms if bin(xm & zm).count("1") & 1) == (2 if tid in ("z", "c") else 0)
    assert (n >> 6) == 8 * 2048                                          # kMaxGrid = 2048 workgroups: eight tiles of 64 states each
    op = L.PauliOperator(ctx, C.PAULI_SITES, terms, dtype)
    worst = (0.0, 0.0)
    xs = np.ascontiguousarray(x[sample])
    try:
        assert op.info() == (n, n, len(terms))
        for bits in (None, 6):
            ctx.set_tuning("pauli_tile_bits", None if bits is None else str(bits))
            for shift in (0, 1):
                for offset in OFFSETS:
                    y, alpha = _apply(ctx, op, x, shift, offset, True)
                    ys = np.ascontiguousarray(y[sample])
                    cls, xw = _class_bound(dtype, xs, ex, ys, offset)          # _check_apply's two checks, the first on the sample
                    ok, r_cls = E.within(E.part_errors(ys, ex.y + offset * xw), (cls, cls))
                    assert ok, "pauli %s bits %s shift %d offset %g: class bound violated (ratio %.3g)" % (tid, bits, shift, offset, r_cls)
                    d, db = E.dot_exact(x, y), E.dot_bound(x, y)
                    assert abs(alpha - np.real(d)) <= db, (tid, bits, shift, offset, alpha, d, db)
                    worst = (max(worst[0], r_cls), max(worst[1], abs(alpha - np.real(d)) / db))
        u = K.start_x(n, dtype, seed=2)
        ratios = []
        for bits in (None, 6):
            ctx.set_tuning("pauli_tile_bits", None if bits is None else str(bits))
            hv, _ = _apply(ctx, op, x, 0, 0.0, False)
            hu, _ = _apply(ctx, op, u, 0, 0.0, False)
            lhs, rhs = np.real(E.dot_exact(u, hv)), np.real(E.dot_exact(hu, x))
            tol = E.dot_bound(u, hv) + E.dot_bound(hu, x)
            ratios.append(abs(lhs - rhs) / tol)
            assert abs(lhs - rhs) <= tol, (tid, bits, lhs, rhs, tol)
            assert abs(lhs) > tol and np.any(hv != 0)         # the two sides are numbers of size, not zeros
    finally:
        ctx.set_tuning("pauli_tile_bits", None)
        op.close()
    print("ratios error/bound (class, alpha)", "pauli", tid, (20,), "D", n, worst, "symmetry", max(ratios))


# ------------------------------------------------------------------ 2. through the embedding, against the sector kernel
EMBED_BLOCKS = ([("momentum", s) for s in C.MOMENTUM] + [("symmetric", s) for s in C.SYMMETRIC if s[4] is not None])
EMBED_CASES = [(kind, shape, "heisenberg", t) for kind, shape in EMBED_BLOCKS for t in ("z", "c")]
_EMBED = {}


def _embedding(kind, shape):
    if (kind, shape) not in _EMBED:
        if kind == "momentum":
            _EMBED[(kind, shape)] = G.momentum_embedding(*shape, dense=False)
        else:
            _EMBED[(kind, shape)] = G.symmetric_embedding(*shape, dense=False)
    return _EMBED[(kind, shape)]


@pytest.mark.parametrize("case", EMBED_CASES, ids=[_id(c) for c in EMBED_CASES])
def test_consistent_with_the_sector_operator_through_the_embedding(ctx, case):
    """y = B^H H_sector (B x) with PauliSectorOperator on the same ring: a check that does not go through the block matrix of the
    host generator.  Bound, formed as the 12-site tests of test_gpu_pauli_momentum and test_gpu_pauli_symmetric form it: the block
    apply's class bound, plus the sector apply's class bound and the rounding of its input (B x formed on the host in double, one
    complex product per element, then rounded to T: <= 4 eps_T per element, which H carries to <= 4 eps_T sum |a||x|) pushed
    through |B|^T, plus the host projection (a column of B holds <= L entries, <= 4 L with the reflection and the flip:
    (L + 4) or (4 L + 4) eps_d |B|^T |Y|)."""
    kind, shape, model, tid = case
    dtype = TYPES[tid]
    n_sites = shape[0]
    n_down = shape[1] if kind == "momentum" else shape[4]
    eps = _eps(dtype)
    terms, x, ex = _reference_rows(kind, shape, model, tid)
    col, val = _embedding(kind, shape)
    inb = col >= 0
    assert col.shape[0] == math.comb(n_sites, n_down) and int(col.max()) == x.shape[0] - 1
    X = np.zeros(col.shape[0], np.complex128)
    X[inb] = val[inb] * x.astype(np.complex128)[col[inb]]
    X = X.astype(dtype)
    sec = L.PauliSectorOperator(ctx, n_sites, n_down, terms, dtype)
    Y, _ = _apply(ctx, sec, X, 0, 0.0, False)
    sec.close()
    sec_ex = C.sector_abs_rows(n_sites, n_down, terms, X)
    sec_cls = E.componentwise_bound(sec_ex, eps) + eps * E.abs1(Y) + 4 * eps * sec_ex.absrow

    def push(v):   # |B|^T v
        return np.bincount(col[inb], weights=E.abs1(val[inb]) * v[inb], minlength=x.shape[0])

    proj = np.zeros(x.shape[0], np.complex128)
    np.add.at(proj, col[inb], np.conj(val[inb]) * Y.astype(np.complex128)[inb])
    op = _operator(ctx, kind, shape, terms, dtype)
    y, _ = _apply(ctx, op, x, 0, 0.0, False)
    op.close()
    cls, _ = _class_bound(dtype, x, ex, y, 0.0)
    column = (4 * n_sites if kind == "symmetric" else n_sites) + 4
    bound = cls + push(sec_cls) + column * E.EPS_D * push(E.abs1(Y))
    ok, r = E.within(E.part_errors(y, proj), (bound, bound))
    assert ok, (case, r)
    assert np.any(y != 0)
    print("block apply against B^H (sector apply) B: error / bound", kind, tid, shape, r)


@pytest.mark.parametrize("tid", list(TYPES))
def test_same_bits_as_the_momentum_operator_of_the_full_space_with_every_flag_zero(ctx, tid):
    dtype = TYPES[tid]
    n_sites, m = 20, 10
    terms = C.model_terms("tfim", n_sites)
    ref = L.PauliMomentumFullOperator(ctx, n_sites, m, terms, dtype)
    op = L.PauliSymmetricOperator(ctx, n_sites, m, terms, dtype)
    try:
        assert op.n == ref.n == C.MOMENTUM_FULL[(n_sites, m)][1] and (op.parity, op.inversion, op.n_down) == (0, 0, None)
        x = K.start_x(op.n, dtype)
        for offset in (0.0, -2.5):
            y0, a0 = _apply(ctx, ref, x, 0, offset, True)
            y1, a1 = _apply(ctx, op, x, 0, offset, True)
            assert np.array_equal(y0.view(np.uint8), y1.view(np.uint8)), (tid, offset)
            assert a0 == a1
        assert np.any(y0 != 0)
    finally:
        ref.close()
        op.close()


# ------------------------------------------------------------------ 3. one solver run per table kernel
EIGEN_CASES = [("symmetric", (30, 15, -1, 0, 5), "heisenberg", "d"), ("momentum", (30, 5, 7), "heisenberg", "z")]


@pytest.mark.parametrize("case", EIGEN_CASES, ids=[_id(c) for c in EIGEN_CASES])
def test_lanczos_against_the_reference(ctx, case):
    """The smallest eigenvalue against the reference library on the block's matrix: the comparison and the tolerance of
    test_lanczos_against_the_reference in test_gpu_pauli_symmetric and test_gpu_pauli_momentum."""
    kind, shape, model, tid = case
    dtype = TYPES[tid]
    terms = C.model_terms(model, shape[0])
    csr = _csr(kind, shape, terms, WIDE[tid], True)
    n = csr[0].shape[0] - 1
    init = G.start_vector(n, 1).astype(dtype)
    op = _operator(ctx, kind, shape, terms, dtype)
    try:
        assert op.n == n == _dim(kind, shape)
        norm = op.inf_norm()
        assert abs(norm - sum(abs(c) for _, _, c in terms)) <= 1e-12 * norm
        offset = -norm
        eng, vals, vecs = _run_lanczos(op, n, init, False, offset)
        ref = _checker().lanczos(csr, init.astype(WIDE[tid]), False, num_eigs=1, offset=offset, eps=eng.eps)
        scale = max(1.0, np.max(np.abs(ref["eigenvalues"] + offset)))
        err = np.max(np.abs(vals - ref["eigenvalues"]))
        print("block %s %s %s: lambda %.13f, max |lambda - reference| = %.3e, bound %.3e, %s iterations"
              % (shape, tid, model, vals[0], err, 20 * eng.eps * scale, eng.getIterationCounts()))
        assert len(vals) == 1
        assert err <= 20 * eng.eps * scale
    finally:
        op.close()
