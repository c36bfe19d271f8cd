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


# ------------------------------------------------------------------ the column-split forms of a sharded context
def _split_bound_ok(csr, x, dtype, world, y, offset, exact_above=1024):
    """The storage contract of the column-split CSR-stream operator exactly as tests/test_gpu_sharded_contracts.py asserts it."""
    own, rem = E.split_rows(csr, x, dtype, world, exact_above)
    se_o, se_r = E.double_sum_error(own), E.double_sum_error(rem)
    xw = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    b = E.split_storage_bound(y, x, offset, dtype, own, rem, se_o, se_r)
    return E.within(E.part_errors(y, own.y + rem.y + offset * xw), b)[0]


def _class_ok(csr, x, y, offset, eps):
    ex = E.rows_exact(csr, x)
    xw = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    b = E.class_bound(ex, x, y, offset, eps, False)
    return E.within(E.part_errors(y, ex.y + offset * xw), (b, b))[0]


def _emulate_split(csr, x, dtype, world, offset, how):
    """Host emulation of a column-split CSR-stream kernel on `world` ranks, stitched over the ranks: "right", or one of the
    plausibly wrong ones."""
    n = x.shape[0]
    col0, col1 = E.owner_ranges(n, world)
    own_csr, rem_csr = E.split_csr(csr, col0, col1)
    xo = xr = x
    if how == "boundary_to_wrong_rank":
        # ownership test off by one (col <= col1): the next rank's first column counts as own and is read one past the local
        # shard, where the padded send buffer holds a zero
        rp, ci, va = csr
        rows = np.repeat(np.arange(n), np.diff(rp))
        va = np.where(ci == col1[rows], 0, va).astype(va.dtype)
        own_csr, rem_csr = E.split_csr((rp, ci, va), col0, col1)
    if how == "padded_tail_as_data":
        # the gathered vector has the stride ceil(n / P) per rank, the last shard is shorter and its tail is padding; a kernel
        # that places the last shard at the END of the buffer reads the padding (zeros) as data and every column of that shard shifted
        stride = -(-n // world)
        pad = world * stride - n
        assert pad > 0
        rp, ci, va = rem_csr
        xr = np.concatenate([x, np.zeros(pad, x.dtype)])
        last = (world - 1) * stride
        xr[last + pad:] = x[last:]
        xr[last:last + pad] = 0
    so = E.formed_products_rows(own_csr, xo, dtype, 1024)
    sr = E.formed_products_rows(rem_csr, xr, dtype, 1024)
    if how == "remote_part_in_float":
        rp, ci, va = rem_csr
        p = E.storage_products(va, x[ci], dtype)
        v = np.array([_seq_sum(p[rp[i]:rp[i + 1]], dtype) for i in range(n)], dtype=dtype)
        w = (so.y.astype(dtype) + E.offset_term(x, offset, dtype)).astype(dtype)
        return (w + v).astype(dtype)
    return E.split_chain(so.y, sr.y, x, offset, dtype, offset_twice=(how == "offset_in_both_parts"))


@pytest.mark.parametrize("dtype", [np.float32, np.complex64], ids=["s", "c"])
@pytest.mark.parametrize("world", [2, 3])
def test_split_storage_bound_rejects_wrong_split_kernels(dtype, world):
    csr, x, special = K.sharded_edge_matrix(5003, dtype)
    for offset in (0.0, -2.5, 0.1):
        assert _split_bound_ok(csr, x, dtype, world, _emulate_split(csr, x, dtype, world, offset, "right"), offset), offset
    for how in ("remote_part_in_float", "boundary_to_wrong_rank", "offset_in_both_parts", "padded_tail_as_data"):
        assert 5003 % world != 0   # the last shard is short: there is a padded tail to misread
        offset = 0.0 if how != "offset_in_both_parts" else 0.1
        assert not _split_bound_ok(csr, x, dtype, world, _emulate_split(csr, x, dtype, world, offset, how), offset), how
    # the split form is not the unsplit contract: two narrowings and two additions in T leave the one-rounding bound
    assert not _storage_ok(csr, x, dtype, _emulate_split(csr, x, dtype, world, 0.0, "right"), offset=0.0)
    # the > 1024 rule goes by the length of each part: on 3 ranks the own parts of both long rows stay below it
    own, rem = E.split_rows(csr, x, dtype, world, 1024)
    whole = E.formed_products_rows(csr, x, dtype, 1024)
    long2 = special["long2"]
    assert whole.nnz[long2] > 1024
    if world == 3:
        assert own.nnz[long2] <= 1024 < rem.nnz[long2] and own.nnz[special["long1"]] <= 1024 and rem.nnz[special["long1"]] <= 1024


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["d", "s"])
@pytest.mark.parametrize("world", [2, 3])
def test_class_bound_rejects_a_misplaced_boundary_column_and_a_padded_tail(dtype, world):
    csr, x, special = K.sharded_edge_matrix(5003, dtype)
    eps = E.EPS_D if dtype == np.float64 else E.EPS_F
    for offset in (0.0, -2.5):
        assert _class_ok(csr, x, _emulate_split(csr, x, dtype, world, offset, "right"), offset, eps)
    assert not _class_ok(csr, x, _emulate_split(csr, x, dtype, world, 0.0, "boundary_to_wrong_rank"), 0.0, eps)
    assert not _class_ok(csr, x, _emulate_split(csr, x, dtype, world, 0.0, "padded_tail_as_data"), 0.0, eps)
    assert not _class_ok(csr, x, _emulate_split(csr, x, dtype, world, -2.5, "offset_in_both_parts"), -2.5, eps)


def test_sharded_edge_matrix_puts_rows_on_every_cut():
    n = 5003
    csr, x, special = K.sharded_edge_matrix(n, np.float32)
    base, _ = K.edge_matrix(n, np.float32)
    assert special["cuts"] == [1668, 2502, 3336] and special["cut_rows"] == [1666, 1669, 2500, 2503, 3335, 3336]
    rp, ci, va = csr
    for c, (lo, hi) in zip(special["cuts"], zip(special["cut_rows"][0::2], special["cut_rows"][1::2])):
        for i in (lo, hi):
            cols = list(ci[rp[i]:rp[i + 1]])
            assert set(cols) == {c - 1, c, 0, n - 1, i} and cols.count(c) == 2 and len(cols) == len(set(cols)) + 1
            assert cols != sorted(cols)
    # every other row is edge_matrix's
    changed = set(special["cut_rows"])
    for i in range(n):
        if i not in changed:
            a, b = slice(rp[i], rp[i + 1]), slice(base[0][i], base[0][i + 1])
            assert np.array_equal(ci[a], base[1][b]) and np.array_equal(va[a], base[2][b])
    # shard_rows: the row blocks of the ranks stitch back to the matrix, column indices global
    for world in (2, 3):
        stride = -(-n // world)
        parts = [K.shard_rows(csr, min(n, r * stride), min(n, (r + 1) * stride) - min(n, r * stride)) for r in range(world)]
        assert np.array_equal(np.concatenate([p[1] for p in parts]), ci)
        assert np.array_equal(np.concatenate([p[0][1:] + rp[min(n, r * stride)] for r, p in enumerate(parts)]), rp[1:])
        assert all(p[0][0] == 0 for p in parts)
