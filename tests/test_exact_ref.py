"""tests/exact_ref.py against fractions.Fraction, and proof that each bound helper tells right from wrong: emulated outputs of
plausibly wrong kernels, on the inputs the GPU tests use (contract_cases.py), must be rejected.  CPU only."""
import math
from fractions import Fraction

import numpy as np
import pytest

import contract_cases as K
import exact_ref as E


def _frac_rows(csr, x):
    rp, ci, va = csr
    out = []
    for i in range(rp.shape[0] - 1):
        re = im = Fraction(0)
        for k in range(rp[i], rp[i + 1]):
            a, b = complex(va[k]), complex(x[ci[k]])
            re += Fraction(a.real) * Fraction(b.real) - Fraction(a.imag) * Fraction(b.imag)
            im += Fraction(a.real) * Fraction(b.imag) + Fraction(a.imag) * Fraction(b.real)
        out.append((re, im))
    return out


def _assert_matches_fraction(csr, x):
    got = E.rows_exact(csr, x).y
    for i, (re, im) in enumerate(_frac_rows(csr, x)):
        assert np.real(got[i]) == E._frac_to_float(re), (i, got[i], float(re))
        if np.iscomplexobj(got):
            assert np.imag(got[i]) == E._frac_to_float(im), i


@pytest.mark.parametrize("dtype", [np.float64, np.complex128, np.float32, np.complex64])
def test_rows_exact_matches_fractions_on_random_rows(dtype):
    rng = np.random.default_rng(2)
    n = 40
    rp = np.concatenate([[0], np.cumsum(rng.integers(0, 12, n))]).astype(np.int64)
    ci = rng.integers(0, n, rp[-1]).astype(np.int32)
    va = (rng.standard_normal(rp[-1]) * 10.0 ** rng.integers(-8, 8, rp[-1]))
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
    if np.dtype(dtype).kind == "c":
        va = va + 1j * rng.standard_normal(rp[-1])
        x = x - 1j * rng.standard_normal(n)
    _assert_matches_fraction((rp, ci, va.astype(dtype)), x.astype(dtype))


def test_rows_exact_on_cancellation_and_extreme_magnitudes():
    tiny, huge = 5e-324, 1.7e308
    rows = [([0, 1, 2], [1e16, 1.0, -1e16]),            # cancellation: a naive double sum gives 0
            ([0, 1], [tiny, 3 * tiny]),                    # denormal products (the split is not exact there)
            ([0, 2], [1e-200, -1e-200]),                   # products below the smallest denormal that cancel
            ([0, 1, 2], [huge, huge, -huge]),              # partial sums beyond the largest double, exact sum finite
            ([0, 1], [huge, huge]),                        # an exact sum beyond the largest double: +inf
            ([0, 1, 0], [0.1, 0.2, 0.3])]
    rp = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int64)
    ci = np.concatenate([c for c, _ in rows]).astype(np.int32)
    va = np.concatenate([v for _, v in rows]).astype(np.float64)
    x = np.array([1.0, 1.0, 1.0])
    got = E.rows_exact((rp, ci, va), x).y
    assert got[0] == 1.0 and got[1] == 4 * tiny and got[2] == 0.0 and got[3] == huge and got[4] == math.inf
    _assert_matches_fraction((rp, ci, va), x)
    x2 = np.array([1e-200, 0.5, 1e-200])
    _assert_matches_fraction((rp, ci, va), x2)
    assert E.rows_exact((rp, ci, va), x2).y[2] == 0.0
    # complex with the same magnitudes
    vz = va * (1 - 0.5j)
    _assert_matches_fraction((rp, ci, vz), x2 * (0.25 + 1j))


def test_dot_exact_is_conjugate_linear_in_its_first_argument():
    a = np.array([1 + 2j, 1e16, -1e16 + 1j])
    b = np.array([3 - 1j, 1.0, 1.0])
    re = sum(Fraction(p.real) * Fraction(q.real) + Fraction(p.imag) * Fraction(q.imag) for p, q in zip(a, b))
    im = sum(Fraction(p.real) * Fraction(q.imag) - Fraction(p.imag) * Fraction(q.real) for p, q in zip(a, b))
    got = E.dot_exact(a, b)
    assert got == complex(float(re), float(im))
    assert E.dot_exact(np.array([1e16, 1.0, -1e16]), np.ones(3)) == 1.0


def test_storage_products_round_like_the_device():
    a = np.array([1 + 1e-3j], dtype=np.complex64)
    x = np.array([1 - 1e-3j], dtype=np.complex64)
    p = E.storage_products(a, x, np.complex64)[0]
    ar, ai, xr, xi = (np.float32(v) for v in (a[0].real, a[0].imag, x[0].real, x[0].imag))
    assert p.real == np.float32(np.float32(ar * xr) - np.float32(ai * xi))
    assert p.imag == np.float32(np.float32(ar * xi) + np.float32(ai * xr))
    # a product that is not exact in float: exactly one rounding
    f = E.storage_products(np.array([1 / 3], np.float32), np.array([3.0000002], np.float32), np.float32)[0]
    assert f == np.float32(float(np.float32(1 / 3)) * float(np.float32(3.0000002)))


# ------------------------------------------------------------------ the helpers reject emulated wrong kernels
def _seq_sum(p, dtype):
    """Sum in the storage type, in stored order (a kernel that accumulates in float)."""
    acc = np.zeros((), dtype=dtype)
    for v in p:
        acc = (acc + v).astype(dtype)
    return acc


def _emulate(csr, x, dtype, how):
    rp, ci, va = csr
    n = rp.shape[0] - 1
    p = E.storage_products(va, x[ci], dtype)
    y = np.zeros(n, dtype=dtype)
    for i in range(n):
        seg = p[rp[i]:rp[i + 1]]
        if how == "float_accumulation":
            y[i] = _seq_sum(seg, dtype)
        elif how == "product_to_narrower_type":   # the storage product rounded once more, to half precision
            q = seg.astype(np.complex128 if np.iscomplexobj(seg) else np.float64)
            r = lambda v: np.float32(np.float64(np.float16(v)) if abs(v) < 6e4 else v)   # noqa: E731
            q = np.array([complex(r(v.real), r(v.imag)) for v in np.atleast_1d(q)]) if np.iscomplexobj(q) else \
                np.array([r(v) for v in q])
            y[i] = math.fsum(np.real(q)) + (1j * math.fsum(np.imag(q)) if np.iscomplexobj(q) else 0)
        elif how == "widened_complex_product":   # complex float products formed in double and rounded to float once
            q = E.storage_products(va[rp[i]:rp[i + 1]], x[ci[rp[i]:rp[i + 1]]], np.complex128).astype(dtype)
            y[i] = math.fsum(np.real(q).astype(np.float64)) + 1j * math.fsum(np.imag(q).astype(np.float64))
        else:
            y[i] = math.fsum(np.real(seg).astype(np.float64)) + (1j * math.fsum(np.imag(seg).astype(np.float64))
                                                                    if np.iscomplexobj(seg) else 0)
    return y


def _storage_ok(csr, x, dtype, y, fixed=False, offset=0.0):
    sp = E.rows_storage_products(csr, x, dtype)
    xmax = float(np.max(np.abs(np.real(x)) + np.abs(np.imag(x))))
    se = E.double_sum_error(sp, fixed_point=fixed, xmax=xmax)
    xw = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    return E.within(E.part_errors(y, sp.y + offset * xw), E.storage_bound(y, x, offset, dtype, se))[0]


@pytest.mark.parametrize("dtype", [np.float32, np.complex64], ids=["s", "c"])
@pytest.mark.parametrize("fixed", [False, True], ids=["double_sums", "fixed_point"])
def test_storage_bound_rejects_wrong_kernels(dtype, fixed):
    csr, x = K.edge_matrix(5003, dtype)
    right = _emulate(csr, x, dtype, "right")
    assert _storage_ok(csr, x, dtype, right, fixed)
    # an offset applied as the device applies it stays inside the bound; 0.1 in double instead of float does too, within it
    for off in (-2.5, 0.1):
        y = (right + E.offset_term(x, off, dtype)).astype(dtype)
        assert _storage_ok(csr, x, dtype, y, fixed, off)
    assert not _storage_ok(csr, x, dtype, _emulate(csr, x, dtype, "float_accumulation"), fixed)
    assert not _storage_ok(csr, x, dtype, _emulate(csr, x, dtype, "product_to_narrower_type"), fixed)
    if np.dtype(dtype).kind == "c":
        # a realistic other rounding sequence: the complex product formed in double (exact real products, one rounding of their
        # difference) and rounded to float once — rounded twice, not the device's fl(fl(ar xr) - fl(ai xi))
        assert not _storage_ok(csr, x, dtype, _emulate(csr, x, dtype, "widened_complex_product"), fixed)
    skipped = right.copy()
    skipped[K.designed_rows(5003)["small_terms"]] = 0          # a row left at 0
    assert not _storage_ok(csr, x, dtype, skipped, fixed)
    half = right.astype(np.complex64 if np.iscomplexobj(right) else np.float32)
    coarse = (half.real.astype(np.float16).astype(np.float32) + (1j * half.imag.astype(np.float16).astype(np.float32)
                                                                  if np.iscomplexobj(half) else 0)).astype(dtype)
    assert not _storage_ok(csr, x, dtype, coarse, fixed)        # y rounded to a narrower type (half)


@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=["d", "z"])
def test_class_bounds_reject_wrong_kernels(dtype):
    csr, x = K.edge_matrix(5003, dtype)
    ex = E.rows_exact(csr, x)
    xmax = float(np.max(np.abs(np.real(x)) + np.abs(np.imag(x))))
    for bound in (E.componentwise_bound(ex, E.EPS_D), E.normwise_bound(ex, xmax, E.EPS_D)):
        def ok(y):
            return E.within(E.part_errors(y, ex.y), (bound, bound))[0]
        assert ok(ex.y.astype(dtype))
        single = np.complex64 if np.dtype(dtype).kind == "c" else np.float32
        assert not ok(_emulate(csr, x.astype(single), single, "float_accumulation"))      # float accumulation
        assert not ok(_emulate(csr, x, single, "right"))                                   # inputs and products rounded to float
        skipped = ex.y.copy()
        skipped[K.designed_rows(5003)["cancel"]] = 0
        assert not ok(skipped)                                                             # a row left at 0
        assert not ok(ex.y.astype(single))                                                 # y rounded to float


@pytest.mark.parametrize("dtype", [np.float32, np.complex64, np.float64], ids=["s", "c", "d"])
def test_dot_bound_rejects_a_float_accumulated_alpha(dtype):
    csr, x = K.edge_matrix(30002, dtype)
    y = E.rows_exact(csr, x).y.astype(dtype)
    d = E.dot_exact(x, y).real
    assert abs(float(np.vdot(x.astype(np.complex128), y.astype(np.complex128)).real) - d) <= E.dot_bound(x, y)
    single = np.float32
    terms = (np.real(x).astype(single) * np.real(y).astype(single) + np.imag(x).astype(single) * np.imag(y).astype(single))
    alpha_f = float(_seq_sum(terms, single))
    assert abs(alpha_f - d) > E.dot_bound(x, y)
