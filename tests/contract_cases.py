"""Inputs of the accuracy-contract tests (numpy only): matrices built where SpMV kernels go wrong, shared by the host checks of the
bound helpers (test_exact_ref.py) and the GPU tests (test_gpu_accuracy_contracts.py; test_gpu_sharded_contracts.py and its rank
processes for sharded contexts), so that all see the same rows."""
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


def shard_rows(csr, row_begin, n_local):
    """Rows [row_begin, row_begin + n_local) of a CSR matrix, as a CSR row block with GLOBAL column indices (what a rank of a
    sharded context passes to its operator)."""
    rp, ci, va = csr
    rp = np.asarray(rp, dtype=np.int64)
    lo, hi = int(rp[row_begin]), int(rp[row_begin + n_local])
    return rp[row_begin: row_begin + n_local + 1] - lo, ci[lo:hi].copy(), va[lo:hi].copy()


def shard_cuts(n, worlds):
    """First rows of the second, third, ... shard for every number of ranks in `worlds`: k * ceil(n / P), 0 < k < P, below n."""
    cuts = set()
    for p in worlds:
        stride = -(-n // p)
        cuts |= {k * stride for k in range(1, p) if 0 < k * stride < n}
    return sorted(cuts)


def sharded_edge_matrix(n, dtype, worlds=(2, 3)):
    """edge_matrix(n, dtype) with two ordinary rows per shard cut replaced by rows that sit on the cut: for every cut c (the
    first row of a shard, shard_cuts) the row just below and the row at the cut hold exactly the columns
    {c - 1, c, 0, n - 1, the row's own index}, unsorted, the column c twice — the last column of one rank and the first of the
    next, the first and the last column of the whole vector, and a duplicate whose two copies a column split must send the same
    way.  The rows are c - 1 and c; where one of them is a designed row of edge_matrix (n = 5003: the long rows lie on the
    2-rank cut, the small-terms and the cancellation row on the first 3-rank cut) the designed row stays and the nearest
    ordinary row outward (c - 2, c + 1) takes the columns instead.  Everything else of edge_matrix stays: empty rows, the long
    rows (1500 and 3000 random columns: on 3 ranks their own parts hold fewer, the second one's remote part more than 1024
    entries), the small-terms row, the cancellation row.  n <= 3: edge_matrix itself.
    Returns (csr, x, designed row indices — those of designed_rows plus "cuts": the cuts, "cut_rows": the replaced rows)."""
    csr, x = edge_matrix(n, dtype)
    special = dict(designed_rows(n))
    special["cuts"], special["cut_rows"] = shard_cuts(n, worlds) if n >= 64 else [], []
    if n < 64:
        return csr, x, special
    rp, ci, va = csr
    rows = [(ci[rp[i]:rp[i + 1]], va[rp[i]:rp[i + 1]]) for i in range(n)]
    taken = set(special["empty"]) | {special[k] for k in ("two_diag", "long1", "long2", "small_terms", "cancel")}
    rng = np.random.default_rng(1000 + n)
    for c in special["cuts"]:
        for i, step in ((c - 1, -1), (c, 1)):
            while i in taken:
                i += step
            assert 0 < i < n - 1, "no ordinary row next to the cut"
            taken.add(i)
            # c first and last; between them n - 1, the row's own index, c - 1 and 0, each once (the row may itself be c - 1 or c)
            cols = [c] + [j for j in dict.fromkeys([n - 1, i, c - 1, 0]) if j != c] + [c]
            v = rng.uniform(0.25, 1.0, len(cols)) * rng.choice([-1.0, 1.0], len(cols))   # no explicit zero on a cut
            if np.dtype(dtype).kind == "c":
                v = v + 1j * rng.uniform(-1, 1, len(cols))
            rows[i] = (np.asarray(cols), v)
            special["cut_rows"].append(i)
    return _finish(rows, n, dtype), x, special


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


def open_boundaries(csr, dims, periodic):
    """stencil_csr's matrix (rows: the diagonal, then per dimension the upper and the lower neighbour) without the bonds that wrap
    around a dimension that is not periodic."""
    dims = list(dims)
    if all(periodic):
        return csr
    rp, ci, va = csr
    n = int(np.prod(dims))
    coords = np.stack(np.unravel_index(np.arange(n), dims), axis=1)
    keep = np.ones(ci.shape[0], dtype=bool)
    for d, per in enumerate(periodic):
        if not per:
            keep[rp[:-1] + 1 + 2 * d] = coords[:, d] + 1 < dims[d]   # the upper neighbour
            keep[rp[:-1] + 2 + 2 * d] = coords[:, d] > 0             # the lower neighbour
    rows = np.repeat(np.arange(n), np.diff(rp))
    cnt = np.bincount(rows[keep], minlength=n)
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), ci[keep], va[keep]


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
