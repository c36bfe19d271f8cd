"""Exact host reference for the operator and BLAS kernels (numpy + the standard library only: no torch, no GPU).

Every sum here is the CORRECTLY ROUNDED double of the exact real sum: products are split exactly into two doubles
(TwoProduct with Veltkamp's split) and each row's terms go through math.fsum, which rounds the exact sum once.  Rows whose
magnitudes leave the range where that is exact (denormal or near-overflow terms) are summed in integer arithmetic instead.

The bound helpers state, one function per accuracy class of include/lanczos_hip.h, the largest error a kernel of that class may
make; tests/test_exact_ref.py shows that each of them rejects the outputs of plausibly wrong kernels (float accumulation, a
product rounded to a narrower type or in another sequence, a skipped row, y rounded to the wrong type, a fused dot product accumulated in float;
for the column-split forms of a sharded context: the remote part accumulated in float, a boundary column read from the wrong
rank, the offset added by both parts, the padded tail of a short last shard read as data)."""
import math
from fractions import Fraction

import numpy as np

EPS_D = float(np.finfo(np.float64).eps)   # 2^-52
EPS_F = float(np.finfo(np.float32).eps)   # 2^-23
_SPLIT = 134217729.0                       # 2^27 + 1 (Veltkamp)
_SAFE = 2.0 ** 450                         # |a|, |x| in [2^-450, 2^450]: products, their error terms and the split stay exact


def _two_product(a, b):
    """p + e == a * b exactly (element-wise, float64; |a|, |b| within the safe range)."""
    p = a * b
    t = _SPLIT * a
    ah = t - (t - a)
    al = a - ah
    t = _SPLIT * b
    bh = t - (t - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def _frac_to_float(f):
    """Correctly rounded double of a Fraction (+-inf beyond the largest double)."""
    try:
        return float(f)
    except OverflowError:
        return math.inf if f > 0 else -math.inf


def _row_terms(csr, x):
    """Per stored entry: the real factor pairs whose products make up Re and Im of a_ij x_j (complex: four products)."""
    rp, ci, va = csr
    va = np.asarray(va)
    xa = np.asarray(x)[np.asarray(ci, dtype=np.int64)]
    if np.iscomplexobj(va) or np.iscomplexobj(xa):
        ar, ai = np.real(va).astype(np.float64), np.imag(va).astype(np.float64)
        xr, xi = np.real(xa).astype(np.float64), np.imag(xa).astype(np.float64)
        re = [(ar, xr), (-ai, xi)]
        im = [(ar, xi), (ai, xr)]
        return re, im
    return [(va.astype(np.float64), xa.astype(np.float64))], None


def _exact_sums(rp, pairs):
    """Correctly rounded sum over each row of sum_k a_k * b_k for the factor pairs `pairs` (lists of equal-length arrays)."""
    rp = np.asarray(rp, dtype=np.int64)
    n = rp.shape[0] - 1
    out = np.zeros(n)
    if n == 0:
        return out
    nnz = int(rp[-1])
    mags = [np.abs(a) for a, _ in pairs] + [np.abs(b) for _, b in pairs]
    bad = np.zeros(nnz, dtype=bool)
    for m in mags:
        bad |= (m != 0) & ((m < 1.0 / _SAFE) | (m > _SAFE) | ~np.isfinite(m))
    terms = []
    for a, b in pairs:
        p, e = _two_product(np.where(bad, 0.0, a), np.where(bad, 0.0, b))
        terms += [p, e]
    stacked = np.stack(terms, axis=1) if terms else np.zeros((nnz, 0))
    bad_rows = np.zeros(n, dtype=bool)
    if bad.any():
        rows = np.repeat(np.arange(n), np.diff(rp))
        bad_rows[rows[bad]] = True
    for i in range(n):
        lo, hi = int(rp[i]), int(rp[i + 1])
        if lo == hi:
            continue
        if bad_rows[i]:
            s = Fraction(0)
            nonfinite = []
            for a, b in pairs:
                for k in range(lo, hi):
                    if not (math.isfinite(a[k]) and math.isfinite(b[k])):
                        nonfinite.append(float(a[k]) * float(b[k]))
                    else:
                        s += Fraction(float(a[k])) * Fraction(float(b[k]))
            out[i] = math.fsum(nonfinite) if nonfinite else _frac_to_float(s)
        else:
            out[i] = math.fsum(stacked[lo:hi].ravel())
    return out


def abs1(v):
    """|re| + |im| element-wise (|v| for real v), in double."""
    v = np.asarray(v)
    if np.iscomplexobj(v):
        return np.abs(np.real(v)).astype(np.float64) + np.abs(np.imag(v)).astype(np.float64)
    return np.abs(v).astype(np.float64)


class Rows:
    """Result of rows_exact / rows_storage_products.  y: the correctly rounded row sums (complex when the inputs are);
    absrow: sum_j |a_ij| |x_j|; rowsum: sum_j |a_ij|; nnz: entries per row (|.| of a complex number is |re| + |im|, the
    magnitude the kernels' fixed-point scales are built from, dev_helpers.hpp abs1)."""

    def __init__(self, y, absrow, rowsum, nnz):
        self.y, self.absrow, self.rowsum, self.nnz = y, absrow, rowsum, nnz


def _row_reduce(rp, v):
    """sum over each row of the non-negative v (float64; used for the scales of the bounds only)."""
    rp = np.asarray(rp, dtype=np.int64)
    out = np.zeros(rp.shape[0] - 1)
    nz = np.flatnonzero(np.diff(rp) > 0)
    if nz.size:
        out[nz] = np.add.reduceat(np.asarray(v, dtype=np.float64), rp[:-1][nz])
    return out


def rows_exact(csr, x):
    """(A x)_i correctly rounded to double, with sum_j |a_ij||x_j|, sum_j |a_ij| and nnz_i (see Rows)."""
    rp, ci, va = csr
    re, im = _row_terms(csr, x)
    y = _exact_sums(rp, re)
    if im is not None:
        y = y + 1j * _exact_sums(rp, im)
    xa = np.asarray(x)[np.asarray(ci, dtype=np.int64)]
    absrow = _row_reduce(rp, abs1(va) * abs1(xa))
    rowsum = _row_reduce(rp, abs1(va))
    return Rows(y, absrow, rowsum, np.diff(np.asarray(rp, dtype=np.int64)))


def storage_products(a, x, dtype):
    """The device's mul(a, x) in the storage type (dev_helpers.hpp; the library is built with -ffp-contract=off):
    float: one rounding of the exact product; complex float: {fl(fl(ar xr) - fl(ai xi)), fl(fl(ar xi) + fl(ai xr))}, each real
    product and the difference / sum rounded to float.  double / complex double: the same with double roundings."""
    dtype = np.dtype(dtype)
    a, x = np.asarray(a).astype(dtype), np.asarray(x).astype(dtype)
    if dtype.kind != "c":
        return a * x
    ar, ai, xr, xi = a.real, a.imag, x.real, x.imag
    pre = ar * xr - ai * xi   # numpy rounds every operation of the storage dtype once, like the device
    pim = ar * xi + ai * xr
    out = np.empty(a.shape, dtype=dtype)
    out.real, out.imag = pre, pim
    return out


def rows_storage_products(csr, x, dtype):
    """Like rows_exact, but over the products rounded to the storage type first (storage_products): the exact target of a
    float / complex-float kernel that rounds every product once and sums in double or fixed point (lanczos_hip.h, ACCURACY)."""
    rp, ci, va = csr
    p = storage_products(va, np.asarray(x)[np.asarray(ci, dtype=np.int64)], dtype)
    ones = np.ones(p.shape[0])
    y = _exact_sums(rp, [(np.real(p).astype(np.float64), ones)])
    if np.dtype(dtype).kind == "c":
        y = y + 1j * _exact_sums(rp, [(np.imag(p).astype(np.float64), ones)])
    base = rows_exact(csr, x)
    return Rows(y, base.absrow, base.rowsum, base.nnz)


def dot_exact(a, b):
    """<a, b> = sum conj(a_i) b_i correctly rounded (conjugate-linear in the FIRST argument, LA:29-51): a float for real
    inputs, a complex (both parts correctly rounded) otherwise.  Re<a, b> is .real of it."""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    rp = np.array([0, a.shape[0]], dtype=np.int64)
    if np.iscomplexobj(a) or np.iscomplexobj(b):
        ar, ai = np.real(a).astype(np.float64), np.imag(a).astype(np.float64)
        br, bi = np.real(b).astype(np.float64), np.imag(b).astype(np.float64)
        re = _exact_sums(rp, [(ar, br), (ai, bi)])[0]
        im = _exact_sums(rp, [(ar, bi), (-ai, br)])[0]
        return complex(re, im)
    return float(_exact_sums(rp, [(a.astype(np.float64), b.astype(np.float64))])[0])


def dot_abs(a, b):
    """sum |a_i| |b_i| (|.| = |re| + |im|): the scale of the dot-product bounds."""
    return float(np.sum(abs1(a) * abs1(b)))


# ------------------------------------------------------------------ the accuracy classes of include/lanczos_hip.h
# Every helper returns the per-row bound on |computed - exact| (complex: on each of the real and imaginary parts).

def componentwise_bound(rows, eps):
    """CSR-stream, PB / tiled with floating-point sums (header, ACCURACY): |y_i - (A x)_i| <= ~nnz_i eps sum_j |a_ij||x_j|.
    Constant 8 (nnz_i + 2): a complex entry is four real products and two sums (x 4), the tree folds of the kernels add a
    rounding per level on top of the nnz_i additions (x 2), +2 for the final narrowing and the diagonal term kept outside the
    streams.  Same constant as tests/test_gpu_round3.py."""
    return 8.0 * eps * (rows.nnz + 2) * rows.absrow


def normwise_bound(rows, xmax, eps):
    """PB / tiled / one-triangle with fixed-point sums (header, ACCURACY):
        |y_i - (A x)_i| <= 2 eps sum_j |a_ij||x_j| + nnz_i 2^-60 (sum_j |a_ij|) max_k |x_k|,   max_k over the WHOLE vector.
    The header's constant 2 counts the roundings outside the grid: each product rounded to T (real: eps/2 |a x|; complex: up to
    eps (|ar xr| + |ai xi|) per part — two products and their difference), the integer sum converted back to a double (eps/2),
    the first diagonal entry's product added outside the streams (eps/2)."""
    return 2.0 * eps * rows.absrow + rows.nnz * 2.0 ** -60 * rows.rowsum * xmax


def double_sum_error(rows, fixed_point=False, xmax=0.0):
    """Error of summing a row's (already rounded) products in double (floating point: 2 (nnz_i + 2) eps_d sum|p|, a rounding per
    addition and per tree level) or in 64-bit fixed point (nnz_i 2^-60 rowsum max|x| for the grid plus 2 eps_d sum|p| for the
    conversions).  sum|p| <= (1 + 2 eps_f) sum_j |a_ij||x_j| for storage-type products."""
    absp = rows.absrow * (1.0 + 4.0 * EPS_F)
    if fixed_point:
        return rows.nnz * 2.0 ** -60 * rows.rowsum * xmax + 2.0 * EPS_D * absp
    return 2.0 * EPS_D * (rows.nnz + 2) * absp


def offset_term(x, offset, dtype):
    """offset * x_i as the device forms it (dev_helpers.hpp rmul): double for d/z; for s/c the offset is rounded to float first
    and the product rounded to float (complex: each part)."""
    dtype = np.dtype(dtype)
    x = np.asarray(x).astype(dtype)
    if dtype in (np.float64, np.complex128):
        return offset * x
    return np.float32(offset) * x


def offset_error(x, offset, dtype):
    """|offset_term - offset * x_i| per part, exactly (the products of two doubles are split exactly)."""
    t = offset_term(x, offset, dtype)
    xs = np.asarray(x).astype(np.dtype(dtype))

    def part(tp, xp):
        p, e = _two_product(np.full(xp.shape, float(offset)), xp.astype(np.float64))
        return np.abs((tp.astype(np.float64) - p) - e)

    if np.iscomplexobj(t):
        return part(t.real, xs.real), part(t.imag, xs.imag)
    return part(t, xs), None


def storage_bound(y, x, offset, dtype, sum_err):
    """Bound on |y_i - (S_i + offset x_i)| per part, for a float / complex-float kernel whose row value v_i = fl_f(acc_i) comes
    from an accumulator acc_i in double with |acc_i - S_i| <= sum_err (S_i: the exact sum of the products the kernel forms,
    rows_storage_products, or rows_exact for the kernels that form exact products), and y_i = fl_f(v_i + t_i),
    t_i = fl_f(fl_f(offset) x_i) (offset_term):
        |y - (S + offset x)| <= |acc - S| + |v - acc| + |y - (v + t)| + |t - offset x|
                             <= sum_err + u_f |v| (1 + u_f) + u_f |y| + offset_error,        u_f = eps_f / 2,
    and |v| <= (|y - t| + u_f |y|) (1 + u_f).  With offset == 0 the last addition adds a zero: y = v, no u_f |y| term.
    Returns (bound of the real part, bound of the imaginary part or None)."""
    u = 0.5 * EPS_F
    t = offset_term(x, offset, dtype)
    oe = offset_error(x, offset, dtype)

    def part(yp, tp, se, op_err):
        yp, tp = yp.astype(np.float64), tp.astype(np.float64)
        v = (np.abs(yp - tp) + u * np.abs(yp)) * (1 + u)
        b = se + u * v * (1 + 2 * u) + op_err
        if offset != 0.0:
            b = b + u * np.abs(yp)
        return b * (1 + 4 * u) + 1e-300   # (1 + 4 u_f): the second-order terms left out above

    if np.iscomplexobj(y):
        return part(y.real, t.real, sum_err, oe[0]), part(y.imag, t.imag, sum_err, oe[1])
    return part(y, t, sum_err, oe[0]), None


def class_bound(rows, x, y, offset, eps, fixed_point):
    """The bound of the operator's accuracy class on |y_i - ((A x)_i + offset x_i)| per part, as the GPU contract tests assert it:
    normwise_bound (max |x| over the WHOLE vector) for the fixed-point forms, componentwise_bound otherwise, plus
    eps (|offset x_i| + |y_i|) for the offset product and the addition in T."""
    x = np.asarray(x)
    xw = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    xmax = float(np.max(abs1(x))) if x.size else 0.0
    cls = normwise_bound(rows, xmax, eps) if fixed_point else componentwise_bound(rows, eps)
    return cls + eps * (np.abs(offset) * abs1(xw) + abs1(y)) + 1e-300


# ------------------------------------------------------------------ column-split operators of a sharded context
# A rank of a sharded context owns the rows AND the columns [cut_r, cut_{r+1}) (cut_r = min(n, r ceil(n / P))).  The CSR-stream and
# the dense operator multiply the own columns first (under the all-gather) and add the other ranks' columns in a second kernel
# (lanczos_hip.h, ACCURACY, "column-split forms").

def owner_ranges(n, world):
    """(col0, col1) per row: the column range the row's rank owns."""
    stride = -(-n // world)
    r = np.arange(n) // max(stride, 1)
    return np.minimum(n, r * stride), np.minimum(n, (r + 1) * stride)


def split_csr(csr, col0, col1):
    """(own, rem): the entries of every row inside / outside [col0_i, col1_i), the order inside a row kept, column indices
    global in both (the host twin of csr_split_kernel, which rebases the own part)."""
    rp, ci, va = csr
    rp = np.asarray(rp, dtype=np.int64)
    n = rp.shape[0] - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    ci64 = np.asarray(ci, dtype=np.int64)
    own = (ci64 >= np.asarray(col0)[rows]) & (ci64 < np.asarray(col1)[rows])
    out = []
    for keep in (own, ~own):
        cnt = np.bincount(rows[keep], minlength=n)
        out.append((np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), np.asarray(ci)[keep], np.asarray(va)[keep]))
    return out[0], out[1]


def formed_products_rows(csr, x, dtype, exact_above):
    """Rows of the exact sums of the products a float / complex-float kernel FORMS: rounded to the storage type once
    (rows_storage_products) in rows of at most `exact_above` entries, exact (rows_exact) in longer rows — CSR-stream:
    exact_above = 1024, counted in the image the kernel walks; dense: exact_above = -1, every product exact."""
    ex = rows_exact(csr, x)
    if exact_above < 0:
        return ex
    sp = rows_storage_products(csr, x, dtype)
    return Rows(np.where(ex.nnz > exact_above, ex.y, sp.y), ex.absrow, ex.rowsum, ex.nnz)


def split_rows(csr, x, dtype, world, exact_above):
    """(own, rem): formed_products_rows of the two halves of the column split on `world` ranks.  The > 1024 rule of CSR-stream
    goes by the length of the row's PART: a row of 3000 entries whose own part holds 900 forms those 900 products in the storage
    type."""
    n = np.asarray(csr[0]).shape[0] - 1
    own, rem = split_csr(csr, *owner_ranges(n, world))
    return formed_products_rows(own, x, dtype, exact_above), formed_products_rows(rem, x, dtype, exact_above)


def split_chain(s_own, s_rem, x, offset, dtype, offset_twice=False):
    """What a right column-split kernel returns when its two accumulators are exact: fl_T(fl_T(fl_T(S_own) + t) + fl_T(S_rem)),
    t = offset_term (numpy rounds every operation of the storage type once, like the device)."""
    dtype = np.dtype(dtype)
    t = offset_term(x, offset, dtype)
    w = np.asarray(s_own).astype(dtype) + t
    v = np.asarray(s_rem).astype(dtype)
    if offset_twice:   # a wrong kernel: the offset term added by both parts
        v = v + t
    return (w + v).astype(dtype)


def split_storage_bound(y, x, offset, dtype, own, rem, se_own, se_rem):
    """Bound on |y_i - (S_own,i + S_rem,i + offset x_i)| per part for a float / complex-float column-split kernel (own, rem:
    split_rows; se_*: double_sum_error of each part).  Part 1 leaves w_i = fl_f(v_o + t_i), v_o = fl_f(acc_o), t_i = offset_term;
    part 2 returns y_i = fl_f(w_i + v_r), v_r = fl_f(acc_r); acc_* are double accumulators with |acc_* - S_*| <= se_*:
        |y - (S_o + S_r + offset x)| <= |acc_o - S_o| + |acc_r - S_r|      the two sums                  se_own + se_rem
                                      + |v_o - acc_o| + |v_r - acc_r|      TWO narrowings to T           u_f (|S_o| + se_own) + u_f (|S_r| + se_rem)
                                      + |w - (v_o + t)|                     the addition of part 1        u_f |w|
                                      + |y - (w + v_r)|                     the addition of part 2        u_f |y|
                                      + |t - offset x|                      offset_error
    with |w| <= (|v_o| + |t|)(1 + u_f), |v_o| <= (|S_o| + se_own)(1 + u_f).  storage_bound has one narrowing and one addition.
    With offset == 0 part 1 adds a zero (w = v_o: no u_f |w|); in a row without remote entries part 2 adds a zero (y = w: no
    u_f |y|).  Returns (bound of the real part, bound of the imaginary part or None)."""
    u = 0.5 * EPS_F
    t = offset_term(x, offset, dtype)
    oe = offset_error(x, offset, dtype)
    has_rem = rem.nnz > 0

    def part(yp, tp, so, sr, op_err):
        yp, tp = np.abs(yp.astype(np.float64)), np.abs(tp.astype(np.float64))
        vo = (np.abs(so) + se_own) * (1 + u)
        b = se_own + se_rem + u * (np.abs(so) + se_own) + u * (np.abs(sr) + se_rem) + op_err
        if offset != 0.0:
            b = b + u * (vo + tp) * (1 + u)
        b = b + np.where(has_rem, u * yp, 0.0)
        return b * (1 + 4 * u) + 1e-300   # (1 + 4 u_f): the second-order terms left out above

    so, sr = np.asarray(own.y), np.asarray(rem.y)
    if np.iscomplexobj(y):
        return part(y.real, t.real, so.real, sr.real, oe[0]), part(y.imag, t.imag, so.imag, sr.imag, oe[1])
    return part(y, t, np.real(so), np.real(sr), oe[0]), None


def dot_bound(x, y, n=None):
    """Fused alpha / ll_dot: Re<x, y> accumulated in double from products exact in double (float inputs) or rounded once
    (double inputs): |alpha - dot_exact| <= 2 (n + 8) eps_d sum |x_i||y_i| — a rounding per addition of any summation order
    (n - 1 of them) and per product, x 2 for the four-product complex terms, + 8 for the cross-workgroup folds.  At every n
    this file meets it is below float resolution, so a float accumulation fails it."""
    n = np.asarray(x).size if n is None else n
    return 2.0 * (n + 8) * EPS_D * dot_abs(x, y) + 1e-300


def part_errors(y, target):
    """|y - target| per part (real / imaginary), in double; target may carry more precision than y."""
    y, target = np.asarray(y), np.asarray(target)
    if np.iscomplexobj(y) or np.iscomplexobj(target):
        yc, tc = y.astype(np.complex128), target.astype(np.complex128)
        return np.abs(yc.real - tc.real), np.abs(yc.imag - tc.imag)
    return np.abs(y.astype(np.float64) - target.astype(np.float64)), None


def within(errs, bounds):
    """True when every part of every row meets its bound; also returns the largest error / bound ratio."""
    worst = 0.0
    ok = True
    for e, b in zip(errs, bounds):
        if e is None:
            continue
        b = np.broadcast_to(np.asarray(b, dtype=np.float64), e.shape)
        ok = ok and bool(np.all(e <= b))
        if e.size:
            worst = max(worst, float(np.max(e / np.maximum(b, 1e-300))))
    return ok, worst
