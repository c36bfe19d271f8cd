"""The matrix of the long block-form runs (tests/test_gpu_block_long.py on the device, tests/test_block_model.py in the numpy model):
a chain whose six separated eigenvalues converge within a few dozen iterations, so that every later iteration of a long window
depends on the re-orthogonalisation alone."""
import numpy as np

N_LONG = 2048 * 3 + 5      # three 16 KiB strips of doubles and a ragged tail
T_LONG = 0.1
NORM_INF = 2.4             # 2.2 + 2 t


def long_diagonal(n):
    d = np.linspace(0.0, 1.0, n)
    d[:2] = [-1.0, -0.6]
    d[-4:] = [1.3, 1.5, 1.8, 2.2]
    return d


def long_chain(n, cplx, t=T_LONG):
    """CSR of diag(linspace(0, 1, n)) with d[:2] = -1.0, -0.6 and d[-4:] = 1.3, 1.5, 1.8, 2.2, nearest-neighbour coupling t
    (complex: i t below, -i t above the diagonal, as test_gpu_block.chain)."""
    d = long_diagonal(n)
    i = np.arange(n)
    cols = np.stack([i - 1, i, i + 1], 1)
    lo, up = (1j * t, -1j * t) if cplx else (t, t)
    vals = np.stack([np.full(n, lo), d.astype(complex if cplx else float), np.full(n, up)], 1)
    ok = (cols >= 0) & (cols < n)
    rp = np.concatenate([[0], np.cumsum(ok.sum(1))]).astype(np.int64)
    return rp, cols[ok].astype(np.int32), np.ascontiguousarray(vals[ok])


def as_sparse(csr):
    import scipy.sparse as sp

    rp, ci, va = csr
    n = rp.shape[0] - 1
    return sp.csr_matrix((va, ci, rp), shape=(n, n))
