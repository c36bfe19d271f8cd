"""The accuracy contracts of include/lanczos_hip.h checked against an EXACT host reference (tests/exact_ref.py), for every SpMV
kernel form, every storage type and the BLAS / Gram-Schmidt kernels in float: per row, the bound of the stated accuracy class
against the correctly rounded A x, and for float / complex float the sharper "each product rounded to the storage type once, the
sum in double or fixed point" contract against the exact sum of those rounded products.  x and y are also passed one element
into larger buffers whose guard zones must come back untouched, and the fixed-point forms must give the same bits under every
geometry knob."""

import numpy as np
import pytest

import contract_cases as K
import exact_ref as E
import lambda_lanczos_amd as L
from guarded import GUARD, guarded as _guarded, unguard as _unguard  # noqa: F401 (fill 0xA5)
from lambda_lanczos_amd import _capi as capi
from util import check_orth_h

pytestmark = pytest.mark.gpu

TYPES = [np.float64, np.complex128, np.float32, np.complex64]
TYPE_IDS = ["d", "z", "s", "c"]
OFFSETS = [0.0, -2.5, 0.1]


def _eps(dtype):
    return E.EPS_F if np.dtype(dtype) in (np.float32, np.complex64) else E.EPS_D


def _single(dtype):
    return np.dtype(dtype) in (np.float32, np.complex64)


# ------------------------------------------------------------------ SpMV: every form x type x offset x pointer shift
# form -> (constructor kind, accuracy, hooks / switches, fixed point?, products the kernel forms for s/c: "storage" or "exact")
FORMS = {
    "csr": ("csr", capi.SPMV_CSR_STREAM, None, {}, False),
    "csr_rp64": ("csr", capi.SPMV_CSR_STREAM, None, {"LL_FORCE_RP64": "1"}, False),
    "pb_fixed": ("csr", capi.SPMV_PB, capi.ACCURACY_NORMWISE, {}, True),
    "pb_ordered": ("csr", capi.SPMV_PB, None, {"LL_PB_PHASE2": "ordered"}, False),
    "pb_atomic": ("csr", capi.SPMV_PB, None, {"LL_PB_PHASE2": "atomic"}, False),
    "tiled_fixed": ("csr", capi.SPMV_TILED, capi.ACCURACY_NORMWISE, {"LL_TL_FORCE": "1"}, True),
    "tiled_ordered": ("csr", capi.SPMV_TILED, capi.ACCURACY_COMPONENTWISE, {"LL_TL_FORCE": "1"}, False),
    "sym": ("sym", capi.SPMV_SYM, None, {}, True),
    "dense": ("dense", None, None, {}, False),
    "stencil_vec": ("stencil", None, None, {}, False),
    "stencil_scalar": ("stencil", None, None, {"LL_STENCIL_VEC": "0"}, False),
}
CSR_SIZES = [1, 2, 3, 5003, 30002]          # n = 1, 2, 3 and n = 3, 2 (mod 4)
# dense: the kernel takes its vectorised form (16-byte loads of the row and of x) when n is a multiple of 16 / sizeof(T) and x is
# 16-byte aligned; n = 1028 reaches it for every type at pointer shift 0 and the scalar form at shift 1 (complex double: shift 1
# stays aligned, vectorised both times); n = 1027 reaches the scalar form only (complex double: vectorised)
SIZES = {"csr": CSR_SIZES, "sym": [3, 5003, 20001], "dense": [1, 2, 3, 1027, 1028], "stencil": [(37, 64), (5, 8, 8)]}
_CACHE = {}


def _inputs(kind, size, dtype):
    """(operator factory, csr the reference sums, x, products formed in storage type?) — cached per module."""
    key = (kind, size, np.dtype(dtype).str)
    if key in _CACHE:
        return _CACHE[key]
    if kind == "csr":
        csr, x = K.edge_matrix(size, dtype)
        out = (lambda ctx, form: L.CsrOperator(ctx, *csr, accuracy=form[2], kernel=form[1]), csr, x)
    elif kind == "sym":
        tri, full, x = K.sym_triangle(size, dtype)
        out = (lambda ctx, form: L.CsrOperator.from_triangle(ctx, *tri, uplo="U", kernel=capi.SPMV_SYM), full, x)
    elif kind == "dense":
        a, csr, x = K.dense_matrix(size, dtype)
        out = (lambda ctx, form: L.DenseOperator(ctx, a), csr, x)
    else:
        dims = size
        n = int(np.prod(dims))
        rng = np.random.default_rng(n)
        onsite = rng.uniform(-1, 1, n)
        hop = [-1.0] * len(dims) if np.dtype(dtype).kind != "c" else [-1.0 + 0.5j, -0.5 - 0.25j, 0.75 + 0.0j][: len(dims)]
        # the on-site terms are kept in the real type of T (float for s / c); the kernel adds them to diag in double
        os_ref = onsite.astype(np.float32).astype(np.float64) if _single(dtype) else onsite
        csr = K.stencil_csr(dims, hop, 0.25, os_ref, dtype)
        x = K.start_x(n, dtype)
        out = (lambda ctx, form: L.StencilOperator(ctx, dims, diag=0.25, hop=hop, periodic=True, onsite=onsite, dtype=dtype),
               csr, x)
    ex = E.rows_exact(out[1], out[2])
    sp = E.rows_storage_products(out[1], out[2], dtype) if _single(dtype) else None
    _CACHE[key] = out + (ex, sp)
    return _CACHE[key]


def _products_exact(kind, form_name, csr):
    """Rows whose products the kernel forms EXACTLY in double (fma of the widened operands) instead of rounding them to the
    storage type: CSR-stream's rows of more than 1024 entries (one workgroup strides over the row), the dense and the lattice
    operator (lanczos_hip.h, ACCURACY, last paragraph)."""
    n = csr[0].shape[0] - 1
    if kind in ("dense", "stencil"):
        return np.ones(n, dtype=bool)
    if form_name.startswith("csr"):
        return np.diff(csr[0]) > 1024
    return np.zeros(n, dtype=bool)


def _check_spmv(form_name, kind, fixed, dtype, csr, x, ex, sp, y, alpha, offset):
    """Assert the class bound against rows_exact, the storage-product contract (s/c) and alpha against dot_exact.  Returns the
    largest error / bound ratios (class, storage, alpha)."""
    eps = _eps(dtype)
    xw = x.astype(np.complex128 if np.dtype(dtype).kind == "c" else np.float64)
    target = ex.y + offset * xw
    xmax = float(np.max(np.abs(np.real(x)) + np.abs(np.imag(x)))) if x.size else 0.0
    cls = E.normwise_bound(ex, xmax, eps) if fixed else E.componentwise_bound(ex, eps)
    cls = cls + eps * (np.abs(offset) * (np.abs(xw.real) + np.abs(xw.imag)) + np.abs(y.real) + np.abs(np.imag(y))) + 1e-300
    ok, r_cls = E.within(E.part_errors(y, target), (cls, cls))
    assert ok, "%s: class bound violated (ratio %.3g)" % (form_name, r_cls)
    r_sto = 0.0
    if _single(dtype):
        exact_rows = _products_exact(kind, form_name, csr)
        s_target = np.where(exact_rows, ex.y, sp.y)
        rows = E.Rows(s_target, ex.absrow, ex.rowsum, ex.nnz)
        se = E.double_sum_error(rows, fixed_point=fixed, xmax=xmax)
        sb = E.storage_bound(y, x, offset, dtype, se)
        # target: the exact sum of the formed products plus offset * x_i (storage_bound charges the float offset term's rounding)
        ok, r_sto = E.within(E.part_errors(y, s_target + offset * xw), sb)
        assert ok, "%s: storage-product contract violated (ratio %.3g)" % (form_name, r_sto)
    # alpha = Re<x, y> of the RETURNED y, accumulated in double
    d = E.dot_exact(x, y)
    db = E.dot_bound(x, y)
    assert abs(alpha - np.real(d)) <= db, (form_name, alpha, d, db)
    return r_cls, r_sto, abs(alpha - np.real(d)) / db


RATIOS = {}


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("form_name", list(FORMS))
def test_spmv_meets_its_contract(ctx, llenv, form_name, dtype):
    kind, kernel, accuracy, hooks, fixed = FORMS[form_name]
    for k, v in hooks.items():
        llenv.setenv(k, v)
    for size in SIZES[kind]:
        factory, csr, x, ex, sp = _inputs(kind, size, dtype)
        op = factory(ctx, FORMS[form_name])
        if kind in ("csr", "sym"):
            assert op.selected_spmv() == kernel, (form_name, size, op.selected_spmv())
        n = x.shape[0]
        first = None
        for shift in (0, 1):
            xb, xv = _guarded(ctx, x, shift)
            yb, yv = _guarded(ctx, np.zeros(n, dtype), shift)
            for offset in OFFSETS:
                alpha = L.spmv(op, xv, yv, offset=offset, want_dot=True)
                y = _unguard(yb, n, shift).copy()
                assert np.array_equal(_unguard(xb, n, shift), x), "the SpMV changed its input"
                r = _check_spmv(form_name, kind, fixed, dtype, csr, x, ex, sp, y, alpha, offset)
                key = (form_name, np.dtype(dtype).char)
                RATIOS[key] = tuple(max(a, b) for a, b in zip(RATIOS.get(key, (0, 0, 0)), r))
                if kind in ("csr", "sym") and form_name != "pb_atomic":   # a fixed order: the same bits for any placement of x / y
                    if first is None:
                        first = {}
                    if offset in first:
                        assert np.array_equal(first[offset].view(np.uint8), y.view(np.uint8)), (form_name, size, offset)
                    first[offset] = y
            xb.free()
            yb.free()
        op.close()
    print("ratios error/bound (class, storage, alpha)", form_name, np.dtype(dtype).char, RATIOS[(form_name, np.dtype(dtype).char)])


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("form_name", ["pb_fixed", "tiled_fixed", "sym"])
def test_normwise_forms_on_a_decades_vector(ctx, llenv, form_name, dtype):
    """A vector spanning 300 decades (d / z; 30 for s / c, inside the float range): the norm-wise bound holds with its grid term
    binding, the float storage-product contract with the grid's sum error, and for d / z some row is NOT component-wise accurate
    — the input separates the two classes (as the header says of localised vectors)."""
    kind, kernel, accuracy, hooks, fixed = FORMS[form_name]
    for k, v in hooks.items():
        llenv.setenv(k, v)
    n = 5003
    if kind == "sym":
        tri, csr, _ = K.sym_triangle(n, dtype)
        op = L.CsrOperator.from_triangle(ctx, *tri, uplo="U", kernel=capi.SPMV_SYM)
    else:
        csr, _ = K.edge_matrix(n, dtype)
        op = L.CsrOperator(ctx, *csr, accuracy=accuracy, kernel=kernel)
    assert op.selected_spmv() == kernel
    x = K.decades_x(n, dtype, 30 if _single(dtype) else 300)
    ex = E.rows_exact(csr, x)
    sp = E.rows_storage_products(csr, x, dtype) if _single(dtype) else None
    xd, yd = ctx.to_device(x), ctx.empty(n, dtype)
    alpha = L.spmv(op, xd, yd, offset=0.0, want_dot=True)
    y = yd.get()
    op.close()
    r = _check_spmv(form_name, kind, True, dtype, csr, x, ex, sp, y, alpha, 0.0)
    eps = _eps(dtype)
    grid = ex.nnz * 2.0 ** -60 * ex.rowsum * float(np.max(E.abs1(x)))
    assert np.any(grid > 2 * eps * ex.absrow)          # the grid term is the binding one on some rows
    if not _single(dtype):
        cw = E.componentwise_bound(ex, eps) + 1e-300
        assert not E.within(E.part_errors(y, ex.y), (cw, cw))[0]
    print("decades ratios error/bound (class, storage, alpha)", form_name, np.dtype(dtype).char, r)


# ------------------------------------------------------------------ geometry knobs: the fixed-point forms bit for bit
KNOBS = [
    {"LL_PB_PAD": "4"}, {"LL_PB_PAD": "16"}, {"LL_PB_THREADS1": "256"}, {"LL_PB_THREADS1": "512"}, {"LL_PB_THREADS1": "1024"},
    {"LL_PB_XPRE": "0"}, {"LL_PB_ROW_BLOCK": "300", "LL_PB_COL_BLOCK": "1100"}, {"pb_placements": "1"},
    {"pb_placements": "16"},   # (a tuning key of the context: ll_ctx_set_tuning)
]
TL_KNOBS = [{}, {"LL_TL_XCD": "0"}, {"LL_TL_WALK": "0"}, {"LL_TL_XCD": "0", "LL_TL_WALK": "0"}]


def _y_of(ctx, op, x, offset=-2.5):
    xd, yd = ctx.to_device(x), ctx.empty(x.shape[0], x.dtype)
    L.spmv(op, xd, yd, offset=offset)
    y = yd.get()
    xd.free()
    yd.free()
    return y


def _with(ctx, llenv, settings):
    """LL_* names through the llenv fixture (switches and util.HOOK_KEYS hooks), lower-case tuning keys on the context itself."""
    for k, v in settings.items():
        if k.startswith("LL_"):
            llenv.setenv(k, v)
        else:
            ctx.set_tuning(k, v)


def _without(ctx, llenv, settings):
    for k in settings:
        if k.startswith("LL_"):
            llenv.delenv(k)
        else:
            ctx.set_tuning(k, None)


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_fixed_point_forms_give_the_same_bits_for_every_geometry(ctx, llenv, dtype):
    """The fixed-point forms promise the same y for every launch, block geometry and placement (lanczos_hip.h, ACCURACY): the
    default PB operator's bits under every PB knob, the tiled kernel's under its walk / XCD knobs, and on a symmetric matrix the
    one-triangle kernel's as well.  The floating-point forms under the same knobs: the component-wise bound and run-to-run bits."""
    tri, full, x = K.sym_triangle(20001, dtype)
    ex = E.rows_exact(full, x)
    op = L.CsrOperator(ctx, *full, accuracy=capi.ACCURACY_NORMWISE, kernel=capi.SPMV_PB)
    assert op.selected_spmv() == capi.SPMV_PB
    ref = _y_of(ctx, op, x)
    op.close()
    shown = []
    try:
        _knob_runs(ctx, llenv, full, x, ex, ref, dtype, shown)
    finally:
        for knob in KNOBS + TL_KNOBS:
            _without(ctx, llenv, {k: v for k, v in knob.items() if not k.startswith("LL_")})
    op = L.CsrOperator.from_triangle(ctx, *tri, uplo="U", kernel=capi.SPMV_SYM)
    assert op.selected_spmv() == capi.SPMV_SYM
    assert np.array_equal(_y_of(ctx, op, x).view(np.uint8), ref.view(np.uint8))
    op.close()
    print("bit-identical to the default PB operator:", shown, "and the one-triangle kernel")


def _knob_runs(ctx, llenv, full, x, ex, ref, dtype, shown):
    for knob in KNOBS:
        _with(ctx, llenv, knob)
        op = L.CsrOperator(ctx, *full, accuracy=capi.ACCURACY_NORMWISE, kernel=capi.SPMV_PB)
        assert op.selected_spmv() == capi.SPMV_PB
        assert np.array_equal(_y_of(ctx, op, x).view(np.uint8), ref.view(np.uint8)), knob
        op.close()
        for phase2 in ("ordered",):
            llenv.setenv("LL_PB_PHASE2", phase2)
            op = L.CsrOperator(ctx, *full, kernel=capi.SPMV_PB)
            assert op.selected_spmv() == capi.SPMV_PB
            y1, y2 = _y_of(ctx, op, x), _y_of(ctx, op, x)
            assert np.array_equal(y1.view(np.uint8), y2.view(np.uint8)), knob
            b = E.componentwise_bound(ex, _eps(dtype)) + _eps(dtype) * (2.5 * np.abs(x) + np.abs(y1)) * 2 + 1e-300
            ok, _ = E.within(E.part_errors(y1, ex.y - 2.5 * x.astype(ex.y.dtype)), (b, b))
            assert ok, (knob, phase2)
            op.close()
            llenv.delenv("LL_PB_PHASE2")
        _without(ctx, llenv, knob)
        shown.append(knob)
    llenv.setenv("LL_TL_FORCE", "1")
    for knob in TL_KNOBS:
        _with(ctx, llenv, knob)
        op = L.CsrOperator(ctx, *full, accuracy=capi.ACCURACY_NORMWISE, kernel=capi.SPMV_TILED)
        assert op.selected_spmv() == capi.SPMV_TILED
        assert np.array_equal(_y_of(ctx, op, x).view(np.uint8), ref.view(np.uint8)), knob
        op.close()
        op = L.CsrOperator(ctx, *full, accuracy=capi.ACCURACY_COMPONENTWISE, kernel=capi.SPMV_TILED)
        assert op.selected_spmv() == capi.SPMV_TILED
        y1, y2 = _y_of(ctx, op, x), _y_of(ctx, op, x)
        assert np.array_equal(y1.view(np.uint8), y2.view(np.uint8)), knob
        op.close()
        _without(ctx, llenv, knob)
        shown.append(("tiled", knob))
    llenv.delenv("LL_TL_FORCE")
    # CSR-stream with the other tile builder: the component-wise bound and run-to-run bits
    llenv.setenv("LL_SPMV_TILE_BALANCE", "0")
    op = L.CsrOperator(ctx, *full, kernel=capi.SPMV_CSR_STREAM)
    assert op.selected_spmv() == capi.SPMV_CSR_STREAM
    y1, y2 = _y_of(ctx, op, x), _y_of(ctx, op, x)
    assert np.array_equal(y1.view(np.uint8), y2.view(np.uint8))
    b = E.componentwise_bound(ex, _eps(dtype)) + _eps(dtype) * (2.5 * np.abs(x) + np.abs(y1)) * 2 + 1e-300
    assert E.within(E.part_errors(y1, ex.y - 2.5 * x.astype(ex.y.dtype)), (b, b))[0]
    op.close()


# ------------------------------------------------------------------ BLAS-1 and Gram-Schmidt in float, double-level bounds
SINGLE = [np.float32, np.complex64]


@pytest.mark.parametrize("dtype", SINGLE, ids=["s", "c"])
@pytest.mark.parametrize("n", [1, 7, 9, 4097, 100003])
def test_blas1_single_precision_against_exact_sums(ctx, dtype, n):
    a, b = K.start_x(n, dtype, 11), K.start_x(n, dtype, 12)
    for shift in (0, 1):
        ab, av = _guarded(ctx, a, shift)
        bb, bv = _guarded(ctx, b, shift)
        d = L.dot(ctx, av, bv, n)
        want = E.dot_exact(a, b)
        assert abs(d - want) <= E.dot_bound(a, b) * (1.5 if np.dtype(dtype).kind == "c" else 1.0), (d, want)
        nrm = L.nrm2(ctx, av, n)
        nn = E.dot_exact(a, a).real
        assert abs(nrm * nrm - nn) <= 2 * E.dot_bound(a, a) + 4 * E.EPS_D * nn
        nrm2 = L.normalize(ctx, av, n)
        assert nrm2 == nrm
        got = _unguard(ab, n, shift)
        # normalize = scal(1 / ||a||): each element one product rounded to float (the factor itself rounded to float first)
        f = np.float32(1.0 / nrm)
        want_v = (a * f).astype(dtype)
        assert np.array_equal(got, want_v) or np.max(np.abs(got - a / nrm)) <= E.EPS_F * np.max(np.abs(a / nrm)) * 1.01
        # three_term and scal on guarded vectors: the guards stay, the values are one float expression per element
        L.scal(ctx, 2.0, av, n)
        _unguard(ab, n, shift)
        w, up, uc = (K.start_x(n, dtype, s) for s in (21, 22, 23))
        wb, wv = _guarded(ctx, w, shift)
        ub, uv = _guarded(ctx, up, shift)
        cb, cv = _guarded(ctx, uc, shift)
        L.three_term(ctx, wv, uv, cv, 0.3, -1.7, n)
        gw = _unguard(wb, n, shift)
        exact = w.astype(np.complex128) - 0.3 * up.astype(np.complex128) + 1.7 * uc.astype(np.complex128)
        scale = np.abs(w) + 0.3 * np.abs(up) + 1.7 * np.abs(uc)
        assert np.all(np.abs(gw - exact) <= 3 * E.EPS_F * scale)
        for buf in (ab, bb, wb, ub, cb):
            buf.free()


def _orth_case(n, nb, dtype, seed=4):
    rng = np.random.default_rng(seed)
    wide = np.complex128 if np.dtype(dtype).kind == "c" else np.float64
    m = rng.uniform(-1, 1, (n, nb)) + (1j * rng.uniform(-1, 1, (n, nb)) if wide == np.complex128 else 0)
    q, _ = np.linalg.qr(m)
    basis = np.ascontiguousarray(q.T).astype(dtype)
    w = (K.start_x(n, dtype, 31).astype(wide) + 3.0 * q[:, 0]).astype(dtype)
    return basis, w


@pytest.mark.parametrize("geometry", ["0", str(1 << 40)], ids=["streaming", "small"])
@pytest.mark.parametrize("n,nb,ldpad", [(20011, 23, 0), (66, 9, 1), (7, 5, 0), (513, 40, 3), (2053, 1703, 0)])
@pytest.mark.parametrize("dtype", SINGLE, ids=["s", "c"])
@pytest.mark.parametrize("mode", [L.ORTH_CGS_DGKS, L.ORTH_MGS], ids=["dgks", "mgs"])
def test_orth_and_gemv_single_precision_exact(ctx, llenv, dtype, mode, n, nb, ldpad, geometry):
    """h against the exact projections of the input w (pass 1) — for MGS / a second pass against the exact projections of the
    w each step sees; the returned norm against the exact norm of the returned w; w against a bound derived from the rounding
    sequence; gemv_basis against the exact sum rounded once.  ld = n + ldpad: odd ld leaves basis rows off 16-byte alignment."""
    llenv.setenv("LL_BLAS_SMALL_BYTES", geometry)
    basis, w = _orth_case(n, nb, dtype)
    ld = n + ldpad
    slab = np.zeros((nb, ld), dtype=dtype)
    slab[:, :n] = basis
    bd = ctx.to_device(slab)
    wb, wv = _guarded(ctx, w, 1)
    nrm, h = L.orth_block(ctx, bd, nb, ld, wv, n, mode=mode, want_h=True)
    got = _unguard(wb, n, 1)
    # h against exact projections at the double-level bound (util.check_orth_h: pass 1 / every MGS step exactly; a float-level
    # term only for the corrections of a second DGKS pass that really ran)
    check_orth_h(ctx, llenv, bd, basis, ld, w, mode, h)
    # the norm against the exact norm of the RETURNED w: the norm sum runs in double over the stored floats
    nn = E.dot_exact(got, got).real
    assert abs(nrm * nrm - nn) <= 2 * E.dot_bound(got, got) + 4 * E.EPS_D * nn, (nrm, np.sqrt(nn))
    # w: fnma_acc(float&, double h, float u) rounds w to float once per basis vector and pass (dev_helpers.hpp), each rounding
    # at most u_f |w_current|, |w_current| <= |w| + sum_j |h_j||u_j| elementwise; the coefficients are double (error of the
    # double sums only).  Two passes at most: |w_got - (w - sum h_j u_j)| <= 2 nb u_f (|w| + sum|h_j||u_j|) + double terms.
    wide = np.complex128
    hw = np.asarray(h, dtype=wide)
    want = w.astype(wide) - hw @ basis.astype(wide)
    scale = np.abs(w.astype(wide)) + np.abs(hw) @ np.abs(basis.astype(wide))
    bound = (2 * nb + 2) * 0.5 * E.EPS_F * scale * (2 if np.dtype(dtype).kind == "c" else 1) + 1e-30
    assert np.all(np.abs(got.astype(wide) - want) <= bound)
    # gemv_basis: out = sum_k coeff_k basis_k; ld_out > n leaves a gap between the rows that must keep its pattern
    rng = np.random.default_rng(9)
    nout = 3
    coeff = rng.uniform(-1, 1, (nout, nb)) + (1j * rng.uniform(-1, 1, (nout, nb)) if np.dtype(dtype).kind == "c" else 0)
    ld_out = n + 5
    pattern = np.frombuffer(np.full(nout * ld_out * np.dtype(dtype).itemsize, 0xA5, np.uint8).tobytes(), dtype=dtype)
    ob, ov = _guarded(ctx, pattern, 1)   # the whole output block starts as the guard pattern: the gaps must keep it
    L.gemv_basis(ctx, bd, nb, ld, coeff, ov, ld_out, n)
    raw = _unguard(ob, nout * ld_out, 1).reshape(nout, ld_out)
    fill = np.frombuffer(np.full(5 * raw.dtype.itemsize, 0xA5, np.uint8).tobytes(), dtype=raw.dtype)
    for r in range(nout):
        assert np.array_equal(raw[r, n:].view(np.uint8), fill.view(np.uint8)), "gemv_basis wrote into the gap between rows"
        # the exact sum (double coefficients) rounded once to T, plus the error of a double sum over nb terms (two roundings per
        # term and part for complex); nb = 1703 spans several launches, whose partial sums stay in double
        ex = coeff[r] @ basis.astype(np.complex128)
        absum = E.abs1(coeff[r]) @ E.abs1(basis)
        de = 2 * (2 * nb + 4) * E.EPS_D * absum
        b = (0.5 * E.EPS_F * (1 + E.EPS_F) * (np.abs(ex.real) + de) + de + 1e-38,
             0.5 * E.EPS_F * (1 + E.EPS_F) * (np.abs(ex.imag) + de) + de + 1e-38)
        e = E.part_errors(raw[r, :n], ex)
        assert E.within(e, b)[0], r
    ob.free()
    wb.free()
    bd.free()
