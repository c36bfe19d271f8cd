"""Inputs of the accuracy-contract tests (numpy only): matrices built where SpMV kernels go wrong, shared by the host checks of the
bound helpers (test_exact_ref.py) and the GPU tests (test_gpu_accuracy_contracts.py), so that both see the same rows."""
import numpy as np

# |x_j| in [1/2, 1] with random signs: the designed rows below rely on it
SMALL = 2.0 ** -25      # terms of the designed row: below half an ulp of its O(1) term in float
BIG = 2.0 ** 26         # the cancellation row: +BIG x_c + x_d - BIG x_c (products exact in every type)


def start_x(n, dtype, seed=1):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n)
    if np.dtype(dtype).kind == "c":
        x = x + 1j * rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n)
    return x.astype(dtype)


def decades_x(n, dtype, decades):
    """x_j = +-10^-(j mod decades) (complex: times e^{ij}): every row of a band sees the whole dynamic range, so the fixed-point
    grid term nnz 2^-60 rowsum max|x| of the norm-wise class is the binding one on many rows."""
    rng = np.random.default_rng(7)
    x = 10.0 ** (-(np.arange(n) % decades).astype(np.float64)) * rng.choice([-1.0, 1.0], n)
    if np.dtype(dtype).kind == "c":
        x = x * np.exp(1j * np.arange(n))
    return x.astype(dtype)


def _vals(rng, k, dtype):
    v = rng.uniform(-1, 1, k)
    if np.dtype(dtype).kind == "c":
        v = v + 1j * rng.uniform(-1, 1, k)
    v[rng.random(k) < 0.03] = 0.0          # explicit zeros
    return v


def _finish(rows, n, dtype):
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum([len(c) for c, _ in rows])
    ci = np.concatenate([np.asarray(c, dtype=np.int32) for c, _ in rows]) if rp[-1] else np.zeros(0, np.int32)
    va = np.concatenate([np.asarray(v) for _, v in rows]).astype(dtype) if rp[-1] else np.zeros(0, dtype)
    return rp, ci, va


def designed_rows(n):
    """Row indices of the special rows of edge_matrix(n) (None where n is too small for them)."""
    if n < 64:
        return {}
    return {"empty": [0, 7, 8, n - 1], "two_diag": 5, "long1": n // 2, "long2": n // 2 + 1, "small_terms": n // 3,
            "cancel": n // 3 + 1}


def edge_matrix(n, dtype, seed=0, band=300, long_rows=(1500, 3000), small_terms=4096):
    """General (not symmetric) n x n CSR matrix: unsorted columns, the diagonal entry not first, explicit zeros, empty rows
    (the first and the last among them), a row with two diagonal entries, two long rows (> 1024 entries: CSR-stream's
    whole-workgroup path; spanning every column block of PB), a row of one O(1) term and `small_terms` terms of 2^-25 |x_j|
    (float accumulation loses all of them), and a cancellation row (2^26 x_c + x_d - 2^26 x_c, the column c twice).
    Small n (1, 2, 3): every entry kind that fits.  Values are exact in float (rounded to dtype here)."""
    rng = np.random.default_rng(seed + 17 * n)
    x = start_x(n, dtype)
    sign = np.sign(np.real(x)).astype(np.float64)
    if n <= 3:
        tables = {1: [([0], [1.5])],
                  2: [([], []), ([1, 0, 1], [0.75, -2.0, 0.0])],
                  3: [([2, 0, 0], [0.5, 1.25, -0.25]), ([2, 1, 0], [1.0, 0.0, 3.0]), ([], [])]}
        rows = [(c, np.asarray(v, dtype=np.float64) * (1 + 0.5j if np.dtype(dtype).kind == "c" else 1)) for c, v in tables[n]]
        return _finish(rows, n, dtype), x
    special = designed_rows(n)
    rows = []
    for i in range(n):
        k = int(rng.integers(1, 10))
        lo, hi = max(0, i - band), min(n, i + band + 1)
        cols = rng.choice(np.arange(lo, hi), size=min(k, hi - lo), replace=False)
        cols = cols[cols != i]
        cols = np.insert(cols, int(rng.integers(0, cols.size + 1)), i)   # the diagonal somewhere in the row, not first
        rows.append((cols, _vals(rng, cols.size, dtype)))
    for i in special["empty"]:
        rows[i] = ([], np.zeros(0))
    i = special["two_diag"]
    rows[i] = ([i + 3, i, i - 2, i], _vals(rng, 4, dtype))
    for i, k in zip((special["long1"], special["long2"]), long_rows):
        cols = rng.choice(n, size=min(k, n), replace=False)
        rows[i] = (cols, _vals(rng, cols.size, dtype))
    i = special["small_terms"]
    m = min(small_terms, n - 2)
    cols = rng.choice(np.setdiff1d(np.arange(n), [i]), size=m, replace=False)
    rows[i] = (np.concatenate([[i], cols]), np.concatenate([[1.0], SMALL * sign[cols]]))
    i = special["cancel"]
    c, d = (i + 11) % n, (i + 29) % n
    rows[i] = ([c, d, c], [BIG, 1.0, -BIG])
    return _finish(rows, n, dtype), x


def dense_of(csr, n):
    rp, ci, va = csr
    a = np.zeros((rp.shape[0] - 1, n), dtype=va.dtype)
    rows = np.repeat(np.arange(rp.shape[0] - 1), np.diff(rp))
    np.add.at(a, (rows, ci), va)
    return a


def dense_matrix(n, dtype, seed=0):
    """Dense n x n matrix (no duplicates): random entries, explicit zeros, a small-terms row and a cancellation row where n
    allows; returned as (dense, csr of the same values in row-major order, x)."""
    rng = np.random.default_rng(seed + 5 * n)
    x = start_x(n, dtype)
    a = _vals(rng, n * n, dtype).reshape(n, n)
    if n >= 8:
        i = n // 3
        a[i] = SMALL * np.sign(np.real(x))
        a[i, i] = 1.0
        j = i + 1
        a[j] = 0.0
        a[j, 0], a[j, 1] = BIG, 1.0   # + BIG x_0 + x_1 - BIG x_0 (the column twice is impossible in a dense row: two columns
        a[j, 2] = -BIG                 # whose x agree instead)
        x[2] = x[0]
        a[j + 1] = 0.0                 # an empty row
    a = a.astype(dtype)
    rp = np.arange(n + 1, dtype=np.int64) * n
    ci = np.tile(np.arange(n, dtype=np.int32), n)
    return a, (rp, ci, a.ravel().copy()), x


def stencil_csr(dims, hop, diag, onsite, dtype):
    """CSR of the lattice operator of lanczos_hip.h (periodic in every dimension):
    (A x)(r) = (diag + onsite[r]) x(r) + sum_d (hop_d x(r + e_d) + conj(hop_d) x(r - e_d)).  The diagonal stays double
    (the kernel multiplies it in double); hops are exact in every type here."""
    dims = list(dims)
    n = int(np.prod(dims))
    idx = np.arange(n).reshape(dims)
    cols, vals = [[] for _ in range(n)], [[] for _ in range(n)]
    for r in range(n):
        cols[r].append(r)
        vals[r].append(diag + onsite[r])
    for d, t in enumerate(hop):
        up = np.roll(idx, -1, axis=d).ravel()
        dn = np.roll(idx, 1, axis=d).ravel()
        for r in range(n):
            cols[r] += [int(up[r]), int(dn[r])]
            vals[r] += [t, np.conj(t)]
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum([len(c) for c in cols])
    wide = np.complex128 if np.dtype(dtype).kind == "c" else np.float64
    return rp, np.concatenate(cols).astype(np.int32), np.concatenate(vals).astype(wide)


def sym_triangle(n, dtype, seed=0, band=200, long_row=1500):
    """Upper triangle T (col >= row) of a symmetric / Hermitian matrix, eligible for the one-triangle kernel: a band, unsorted
    columns, explicit zeros, empty rows (first and last), a row with two diagonal entries, a long row (its mirrored entries land
    in many rows), a small-terms row.  Returns (triangle csr, expanded full csr in the storage type, x); the expanded matrix holds
    every stored entry once and the mirror conj(a) of every off-diagonal one (lanczos_hip.h: A = T + T^H - diag(T))."""
    rng = np.random.default_rng(seed + 3 * n)
    x = start_x(n, dtype)
    sign = np.sign(np.real(x))
    rows = []
    for i in range(n):
        k = int(rng.integers(0, 6))
        hi = min(n, i + band + 1)
        cols = rng.choice(np.arange(i + 1, hi), size=min(k, hi - i - 1), replace=False) if hi > i + 1 else np.zeros(0, int)
        cols = np.insert(cols, int(rng.integers(0, cols.size + 1)), i)
        v = _vals(rng, cols.size, dtype)
        if np.dtype(dtype).kind == "c":
            v[cols == i] = v[cols == i].real   # Hermitian: real diagonal
        rows.append((cols, v))
    if n >= 64:
        rows[0] = ([], np.zeros(0))
        rows[n - 1] = ([], np.zeros(0))
        rows[3] = ([9, 3, 3], np.array([0.5, 1.25, -0.75]))   # two diagonal entries, not first
        i = 10
        cols = np.sort(rng.choice(np.arange(i + 1, n), size=min(long_row, n - i - 1), replace=False))[::-1]
        v = _vals(rng, cols.size + 1, dtype)
        v[0] = 1.0
        rows[i] = (np.concatenate([[i], cols]), v)
        i = n // 2
        m = min(n - i - 1, band)
        cols = np.arange(i + 1, i + 1 + m)
        rows[i] = (np.concatenate([[i], cols]), np.concatenate([[1.0], SMALL * sign[cols]]))
    tri = _finish(rows, n, dtype)
    rp, ci, va = tri
    r = np.repeat(np.arange(n), np.diff(rp))
    off = ci != r
    fr = np.concatenate([r, ci[off]])
    fc = np.concatenate([ci, r[off]])
    fv = np.concatenate([va, np.conj(va[off])])
    order = np.argsort(fr, kind="stable")
    full = (np.concatenate([[0], np.cumsum(np.bincount(fr, minlength=n))]).astype(np.int64), fc[order].astype(np.int32),
            fv[order])
    return tri, full, x
