"""No kernel reads past its inputs: every primitive and every operator form with POISONED surroundings.

Each case runs the same call three times on the same buffers at the same device addresses.  Between the calls every byte around
the inputs — both guards, the row gaps [n, ld) of a basis slab, its rows beyond nb — and the previous contents of every pure
output are refilled with one byte: 0x00 (the control: what the other tests give the kernels), 0xFF (NaN in float and in double:
it survives any arithmetic, a multiplication by zero included) and 0x7F (3.4e38 as float, 1.4e306 as double: a max|x| scan, which
drops NaN, takes it, and a sum overflows on it).  Asserted: the three results, returned scalars included, agree bit for bit; the
0x00 result meets the exact-reference bound the existing tests hold that primitive to (exact_ref.py, contract_cases.py,
util.check_orth_h; no tolerance of this file's own); after each call every byte outside the outputs still holds the fill.
pb_atomic adds in arrival order: there the contract bound is asserted for every fill instead of bit equality.
Every buffer is a guarded.GuardedSlab: an allocation of the test's own with 64 elements of fill on either side."""
import numpy as np
import pytest

import contract_cases as K
import exact_ref as E
import lambda_lanczos_amd as L
import test_gpu_accuracy_contracts as AC
from guarded import GuardedSlab
from pauli_cases import BITS_KEY, TYPE_IDS, TYPES, _check_apply, _cplx, _runs
from util import check_orth_h

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xFF, 0x7F)
GEOMETRIES = [("0", "streaming"), (str(1 << 40), "small")]   # LL_BLAS_SMALL_BYTES: either strip geometry on every length
COUNTS = {}   # family -> [compared bit for bit, compared by bound]


def _count(family, bits=0, bound=0):
    c = COUNTS.setdefault(family, [0, 0])
    c[0] += bits
    c[1] += bound


def _report(family):
    print("poisoned reads, %s: %d cases compared bit for bit, %d by bound" % (family, *COUNTS.get(family, [0, 0])))


def _bytes(v):
    return np.atleast_1d(np.asarray(v)).view(np.uint8)


def _same_bits(runs, what):
    """runs: one dict of results (arrays and scalars) per fill, in the order of FILLS."""
    for fill, r in zip(FILLS[1:], runs[1:]):
        for k, v in runs[0].items():
            assert np.array_equal(_bytes(v), _bytes(r[k])), "%s: %s differs between the fills 0x00 and 0x%02X" % (what, k, fill)


def sizes(dtype):
    """1, 7, 20011, and one below / one above a wave strip of the small geometry (64 lanes x 16 bytes) and a strip of the streaming
    geometry (256 lanes x 64 bytes)."""
    isz = np.dtype(dtype).itemsize
    small, stream = 64 * 16 // isz, 256 * 64 // isz
    return [1, 7, small - 1, small + 1, stream - 1, stream + 1, 20011]


# ------------------------------------------------------------------ BLAS-1 and the recurrence kernel
def _blas1_run(ctx, bufs, data, n, fill):
    for k, b in bufs.items():
        b.refill(fill, data[k])
    a, b, w, up, uc, y, x, p, psi = (bufs[k] for k in ("a", "b", "w", "up", "uc", "y", "x", "p", "psi"))
    r = {}

    def unchanged(*names):
        for k in names:
            assert np.array_equal(bufs[k].rows(fill), data[k]), "input %s changed" % k

    r["dot"] = L.dot(ctx, a, b, n)
    r["nrm2"] = L.nrm2(ctx, a, n)
    unchanged("a", "b")
    r["normalize"] = L.normalize(ctx, a, n)
    r["normalized"] = a.rows(fill)
    L.scal(ctx, -0.75, b, n)
    r["scaled"] = b.rows(fill)
    L.three_term(ctx, w, up, uc, 0.3, -1.7, n)
    r["three_term"] = w.rows(fill)
    w.refill(fill, data["w"])
    L.three_term(ctx, w, None, uc, 0.0, 0.9, n)
    r["three_term_first"] = w.rows(fill)
    unchanged("up", "uc")
    L.recur_accum(ctx, y, x, p, -1.7, 0.3, 0.625, psi, n)
    r["recur_y"], r["recur_psi"] = y.rows(fill), psi.rows(fill)
    y.refill(fill, data["y"])
    psi.refill(fill, data["psi"])
    L.recur_accum(ctx, y, x, None, -1.7, 0.3, 0.625, psi, n)
    r["recur_y_nop"], r["recur_psi_nop"] = y.rows(fill), psi.rows(fill)
    unchanged("x", "p")
    return r


def _blas1_check(dtype, data, r, n):
    """The bounds of test_gpu_accuracy_contracts.test_blas1_single_precision_against_exact_sums (dot, norm, s / c elements),
    test_gpu_kernels.test_blas1 (d / z elements) and test_gpu_two_pass.test_recur_accum_against_exact_arithmetic."""
    single, cplx = AC._single(dtype), _cplx(dtype)
    eps = AC._eps(dtype)
    a, b = data["a"], data["b"]
    assert abs(r["dot"] - E.dot_exact(a, b)) <= E.dot_bound(a, b) * (1.5 if cplx else 1.0)
    nn = E.dot_exact(a, a).real
    nrm = r["nrm2"]
    assert abs(nrm * nrm - nn) <= 2 * E.dot_bound(a, a) + 4 * E.EPS_D * nn
    assert r["normalize"] == nrm
    got = r["normalized"]
    if single:
        want_v = (a * np.float32(1.0 / nrm)).astype(dtype)
        assert np.array_equal(got, want_v) or np.max(np.abs(got - a / nrm)) <= E.EPS_F * np.max(np.abs(a / nrm)) * 1.01
        assert np.array_equal(r["scaled"], (b * np.float32(-0.75)).astype(dtype))
    else:
        assert np.allclose(got, a * (1.0 / nrm), rtol=4 * E.EPS_D, atol=0)
        assert np.array_equal(r["scaled"], -0.75 * b)
    wide = np.clongdouble if cplx else np.longdouble
    w, up, uc = (data[k].astype(wide) for k in ("w", "up", "uc"))
    for key, exact, scale in (("three_term", w - wide(0.3) * up + wide(1.7) * uc, np.abs(w) + 0.3 * np.abs(up) + 1.7 * np.abs(uc)),
                              ("three_term_first", w - wide(0.9) * uc, np.abs(w) + 0.9 * np.abs(uc))):
        err = np.abs(r[key].astype(wide) - exact).astype(np.float64)
        assert np.all(err <= (3 * E.EPS_F * scale.astype(np.float64) if single else 8 * E.EPS_D)), key
    y, x, p, psi = (data[k] for k in ("y", "x", "p", "psi"))
    for sfx, bp in (("", 0.3), ("_nop", 0.0)):
        y_exact = y.astype(wide) - wide(-1.7) * x.astype(wide) - wide(bp) * p.astype(wide)
        q_exact = psi.astype(wide) + wide(0.625) * y_exact
        S = (np.abs(y) + 1.7 * np.abs(x) + bp * np.abs(p)).astype(np.float64)
        by = 3 * eps * S * 1.01
        bq = eps * (np.abs(psi).astype(np.float64) + 5 * 0.625 * S) * 1.01
        assert np.all(np.abs(r["recur_y" + sfx].astype(wide) - y_exact).astype(np.float64) <= by), sfx
        assert np.all(np.abs(r["recur_psi" + sfx].astype(wide) - q_exact).astype(np.float64) <= bq), sfx


@pytest.mark.parametrize("geometry", [g for g, _ in GEOMETRIES], ids=[i for _, i in GEOMETRIES])
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_blas1_and_recurrence_read_nothing_outside_their_vectors(ctx, llenv, dtype, geometry):
    """dot, nrm2, normalize, scal, three_term (with and without u_prev) and recur_accum (with and without p) at pointer shifts 0
    and 1, in both geometries, over sizes()."""
    llenv.setenv("LL_BLAS_SMALL_BYTES", geometry)
    names = ("a", "b", "w", "up", "uc", "y", "x", "p", "psi")
    for n in sizes(dtype):
        data = {k: K.start_x(n, dtype, 11 + i) for i, k in enumerate(names)}
        for shift in (0, 1):
            bufs = {k: GuardedSlab(ctx, dtype, n, shift=shift) for k in names}
            try:
                runs = [_blas1_run(ctx, bufs, data, n, fill) for fill in FILLS]
            finally:
                for b in bufs.values():
                    b.free()
            _same_bits(runs, "blas1 n = %d shift %d" % (n, shift))
            _blas1_check(dtype, data, runs[0], n)
            _count("blas1", bits=len(runs[0]))
    _report("blas1")


# ------------------------------------------------------------------ Gram-Schmidt and the GEMV over the basis
_ORTH = {}


def _orth_inputs(n, nb, dtype):
    key = (n, nb, np.dtype(dtype).str)
    if key not in _ORTH:
        basis, w = AC._orth_case(n, nb, dtype)
        rng = np.random.default_rng(9)
        coeff = rng.uniform(-1, 1, (3, nb)) + (1j * rng.uniform(-1, 1, (3, nb)) if _cplx(dtype) else 0)
        _ORTH[key] = (basis, w, coeff)
    return _ORTH[key]


def _orth_shapes(dtype):
    """(n, nb, ld): ld = n + {0, 1, 3} and round_up(n, 256) with nb = 5; nb = 1 and nb = 40 with an odd and with the rounded ld; nb
    never above n (the rows are orthonormal); and the (2053, 1703) case of test_orth_and_gemv_single_precision_exact, more rows
    than one launch takes."""
    out = []
    for n in sizes(dtype):
        r256 = -(-n // 256) * 256
        for nb, lds in ((5, (n, n + 1, n + 3, r256)), (1, (n + 3, r256)), (40, (n + 1, r256))):
            out += [(n, nb, ld) for ld in lds if nb <= n]
    return out + [(2053, 1703, 2053 + 1)]


def _orth_run(ctx, slab, wv, out, inputs, n, nb, ld, mode, fill):
    basis, w, coeff = inputs
    slab.refill(fill, basis)
    wv.refill(fill, w)
    out.refill(fill)                      # a pure output: its previous contents are the fill
    nrm, h = L.orth_block(ctx, slab, nb, ld, wv, n, mode=mode, want_h=True)
    r = {"norm": nrm, "h": np.array(h), "w": wv.rows(fill)}
    L.gemv_basis(ctx, slab, nb, ld, coeff, out, out.ld, n)
    r["gemv"] = out.rows(fill, "gemv_basis wrote into the gap between its output rows")
    assert np.array_equal(slab.rows(fill, "a kernel wrote into the basis slab"), basis)
    return r


def _orth_check(ctx, llenv, oracle, slab, inputs, r, n, nb, ld, mode, dtype):
    """h: util.check_orth_h (DGKS and MGS, as the float tests use it).  w, the norm and the GEMV: s / c by the bounds of
    test_gpu_accuracy_contracts.test_orth_and_gemv_single_precision_exact (CGS2, which that test does not run: the mode-independent
    bounds of test_gpu_float.test_orth_and_gemv_single_precision), d / z by those of test_gpu_kernels (test_orth_block_matches_mgs_oracle,
    test_gemv_basis)."""
    basis, w, coeff = inputs
    single, cplx = AC._single(dtype), _cplx(dtype)
    wide = np.complex128
    got, nrm, h = r["w"], r["norm"], r["h"]
    if mode != L.ORTH_CGS2:
        check_orth_h(ctx, llenv, slab, basis, ld, w, mode, h)   # (its own calls read the slab with the last fill around it)
    bw = basis.astype(wide)
    scale = np.linalg.norm(w)
    if single:
        nn = E.dot_exact(got, got).real
        assert abs(nrm * nrm - nn) <= 2 * E.dot_bound(got, got) + 4 * E.EPS_D * nn, (nrm, np.sqrt(nn))
        if mode == L.ORTH_CGS2:
            want = w.astype(wide) - (bw.conj() @ w.astype(wide)) @ bw
            assert np.linalg.norm(got - want) <= 20 * E.EPS_F * scale
            assert abs(nrm - np.linalg.norm(want)) <= 20 * E.EPS_F * scale
            assert np.max(np.abs(bw.conj() @ got)) <= 20 * E.EPS_F * scale
        else:
            hw = np.asarray(h, dtype=wide)
            want = w.astype(wide) - hw @ bw
            sc = np.abs(w.astype(wide)) + np.abs(hw) @ np.abs(bw)
            bound = (2 * nb + 2) * 0.5 * E.EPS_F * sc * (2 if cplx else 1) + 1e-30
            assert np.all(np.abs(got.astype(wide) - want) <= bound)
        for row in range(coeff.shape[0]):
            ex = coeff[row] @ bw
            absum = E.abs1(coeff[row]) @ E.abs1(basis)
            de = 2 * (2 * nb + 4) * E.EPS_D * absum
            b = (0.5 * E.EPS_F * (1 + E.EPS_F) * (np.abs(ex.real) + de) + de + 1e-38,
                 0.5 * E.EPS_F * (1 + E.EPS_F) * (np.abs(ex.imag) + de) + de + 1e-38)
            assert E.within(E.part_errors(r["gemv"][row], ex), b)[0], row
    else:
        want = oracle.schmidt_orth(bw, w.astype(wide))
        if not cplx:
            want = want.real
        assert np.linalg.norm(got - want) <= 50 * E.EPS_D * scale * np.sqrt(nb)
        assert abs(nrm - np.linalg.norm(want)) <= 50 * E.EPS_D * scale * np.sqrt(nb)
        assert np.max(np.abs(basis.conj() @ got)) <= 20 * E.EPS_D * scale
        assert np.allclose(h, basis.conj() @ w, rtol=0, atol=50 * E.EPS_D * scale)
        assert np.max(np.abs(r["gemv"] - coeff.astype(dtype) @ basis)) <= 8 * E.EPS_D * nb * 2


@pytest.mark.parametrize("geometry", [g for g, _ in GEOMETRIES], ids=[i for _, i in GEOMETRIES])
@pytest.mark.parametrize("mode", [L.ORTH_CGS_DGKS, L.ORTH_CGS2, L.ORTH_MGS], ids=["dgks", "cgs2", "mgs"])
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_orth_block_and_gemv_basis_read_only_n_elements_of_nb_rows(ctx, llenv, oracle, dtype, mode, geometry):
    """The slab holds nb + 2 rows of ld elements; the gaps [n, ld) of every row, the two spare rows and the guards are poisoned, w
    sits one element into its buffer, and gemv_basis writes rows of ld_out = n + 5 elements whose gaps must keep the fill."""
    llenv.setenv("LL_BLAS_SMALL_BYTES", geometry)
    for n, nb, ld in _orth_shapes(dtype):
        inputs = _orth_inputs(n, nb, dtype)
        slab = GuardedSlab(ctx, dtype, n, nb=nb, ld=ld, nb_alloc=nb + 2)
        wv = GuardedSlab(ctx, dtype, n, shift=1)
        out = GuardedSlab(ctx, dtype, n, nb=3, ld=n + 5, nb_alloc=3, shift=1)
        try:
            runs = [_orth_run(ctx, slab, wv, out, inputs, n, nb, ld, mode, fill) for fill in FILLS]
            what = "orth n = %d nb = %d ld = %d" % (n, nb, ld)
            _same_bits(runs, what)
            _orth_check(ctx, llenv, oracle, slab, inputs, runs[0], n, nb, ld, mode, dtype)
        finally:
            for b in (slab, wv, out):
                b.free()
        _count("orth_block / gemv_basis", bits=4)
    _report("orth_block / gemv_basis")


# ------------------------------------------------------------------ ll_spmv: every form of test_gpu_accuracy_contracts.FORMS
SPMV_SIZES = {"csr": [1, 2, 3, 5003], "sym": [3, 5003], "dense": [3, 1027, 1028], "stencil": AC.SIZES["stencil"]}
SPMV_OFFSETS = [0.0, -2.5]


def _spmv_runs(ctx, op, x, shift, offset):
    n = x.shape[0]
    xb = GuardedSlab(ctx, x.dtype, n, shift=shift)
    yb = GuardedSlab(ctx, x.dtype, n, shift=shift)
    runs = []
    try:
        for fill in FILLS:
            xb.refill(fill, x)
            yb.refill(fill)               # y is a pure output: poisoned too
            alpha = L.spmv(op, xb, yb, offset=offset, want_dot=True)
            runs.append({"y": yb.rows(fill, "the SpMV wrote outside y"), "alpha": alpha})
            assert np.array_equal(xb.rows(fill, "the SpMV wrote around x"), x), "the SpMV changed its input"
    finally:
        xb.free()
        yb.free()
    return runs


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("form_name", list(AC.FORMS))
def test_spmv_reads_nothing_around_x_and_writes_every_row_of_y(ctx, llenv, form_name, dtype):
    """x and y inside poisoned buffers, y itself poisoned before the call: at offset 0 the empty rows of the matrices of
    contract_cases.py (the first and the last row among them) must come back as written zeros."""
    kind, kernel, accuracy, hooks, fixed = AC.FORMS[form_name]
    for k, v in hooks.items():
        llenv.setenv(k, v)
    family = "spmv " + form_name
    for size in SPMV_SIZES[kind]:
        factory, csr, x, ex, sp = AC._inputs(kind, size, dtype)
        op = factory(ctx, AC.FORMS[form_name])
        if kind in ("csr", "sym"):
            assert op.selected_spmv() == kernel, (form_name, size, op.selected_spmv())
        empty = np.flatnonzero(np.diff(csr[0]) == 0)
        try:
            for shift in (0, 1):
                for offset in SPMV_OFFSETS:
                    runs = _spmv_runs(ctx, op, x, shift, offset)
                    what = "%s n = %s shift %d offset %s" % (form_name, size, shift, offset)
                    checked = runs if form_name == "pb_atomic" else runs[:1]
                    for r in checked:
                        AC._check_spmv(form_name, kind, fixed, dtype, csr, x, ex, sp, r["y"], r["alpha"], offset)
                        if offset == 0.0:
                            assert np.all(r["y"][empty] == 0), what + ": an empty row is not a written zero"
                    if form_name == "pb_atomic":
                        _count(family, bound=1)
                    else:
                        _same_bits(runs, what)
                        _count(family, bits=1)
        finally:
            op.close()
    _report(family)


# ------------------------------------------------------------------ the five Pauli-sum families
def _pauli_cases(ctx, family, dtype):
    """(reference rows, operator factory) of the smallest rings of the family's own test module, one model each."""
    tid = TYPE_IDS[TYPES.index(dtype)]
    if family == "pauli":
        import test_gpu_pauli as P
        return [(P._reference_rows("heisenberg", s, tid), lambda t, s=s: L.PauliOperator(ctx, s, t, dtype)) for s in (1, 2, 3, 5, 9)]
    if family == "sector":
        import test_gpu_pauli_sector as P
        return [(P._reference_rows("heisenberg", s, d, tid), lambda t, s=s, d=d: L.PauliSectorOperator(ctx, s, d, t, dtype))
                for s, d in P.SECTORS[:8]]
    if family == "momentum":
        import test_gpu_pauli_momentum as P
        return [(P._reference_rows("heisenberg", sh, tid), lambda t, sh=sh: L.PauliMomentumOperator(ctx, *sh, t, dtype))
                for sh in P.SHAPES[:15] if _runs(dtype, sh[0], sh[2])]
    if family == "momentum_full":
        import test_gpu_pauli_momentum_full as P
        return [(P._reference_rows("tfim", sh, tid), lambda t, sh=sh: L.PauliMomentumFullOperator(ctx, *sh, t, dtype))
                for sh in P.SHAPES[:14] if _runs(dtype, sh[0], sh[1])]
    import test_gpu_pauli_symmetric as P
    shapes = [sh for sh in P._shapes("tfim", dtype) if sh[0] <= 9]
    return [(P._reference_rows("tfim", sh, tid), lambda t, sh=sh: P._op(ctx, sh, t, dtype)) for sh in shapes]



@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("family", list(BITS_KEY))
def test_pauli_sum_applies_read_nothing_around_x(ctx, family, dtype):
    """Rings of 1 to 9 sites; pointer shift 0 takes the vectorised form of a kernel where it has one, shift 1 the element-wise
    one (as in the families' own tests)."""
    ran = 0
    for ref, factory in _pauli_cases(ctx, family, dtype):
        if ref is None:                   # an empty symmetry block: no operator
            continue
        terms, csr, x, ex = ref
        op = factory(terms)
        try:
            for shift in (0, 1):
                for offset in SPMV_OFFSETS:
                    runs = _spmv_runs(ctx, op, x, shift, offset)
                    what = "%s %s n = %d shift %d offset %s" % (family, TYPE_IDS[TYPES.index(dtype)], x.shape[0], shift, offset)
                    _same_bits(runs, what)
                    if family in ("pauli", "sector"):   # each family by the checker of its own test module
                        AC._check_spmv(family, "stencil", False, dtype, csr, x, ex, ex, runs[0]["y"], runs[0]["alpha"], offset)
                    else:
                        _check_apply(dtype, x, ex, runs[0]["y"], runs[0]["alpha"], offset, what)
                    _count("pauli " + family, bits=1)
        finally:
            op.close()
        ran += 1
    assert ran >= 4
    _report("pauli " + family)
