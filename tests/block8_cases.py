"""Matrices and the recorded case of tests/test_gpu_block8.py (blocks of eight Lanczos iterations per sweep).  The two
matrices are those of tools/block_gs_model.py at the device tests' n = 3 x 2 048 + 5."""
import hashlib

import numpy as np
import scipy.sparse as sp

N = 2048 * 3 + 5


def _csr(A):
    A = A.tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.int32), np.ascontiguousarray(A.data)


def _rows(n, per_row, lo, cplx, seed, imag=1.0):
    rng = np.random.default_rng(seed)
    rows, cols = np.repeat(np.arange(n), per_row), rng.integers(0, n, per_row * n)
    vals = rng.uniform(lo, 1, per_row * n) + (1j * imag * rng.uniform(-1, 1, per_row * n) if cplx else 0)
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, n))


def flagship_type(n, cplx, seed=5):
    """B + B^H + 7 I, seven entries per row of B in (-1, 1): the type of the benchmark's matrix.  No Ritz value converges to an
    outlier: blocks of four publish gate values of 1e-15 .. 2e-14 and the guard admits blocks of eight after its warm-up."""
    B = _rows(n, 7, -1, cplx, seed)
    return _csr(B + B.conj().T + 7 * sp.eye(n))


def outlier(n, cplx, seed=7):
    """Fifteen entries per row in (0, 1), symmetrised: one dominant eigenvalue, to which a Ritz value converges within the first
    blocks; blocks of four then publish 1e-13 .. 5e-12 and the guard admits no block of eight."""
    B = _rows(n, 15, 0, cplx, seed, imag=0.1)
    return _csr((B + B.conj().T) * 0.5)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def recorded_case(L, G, ctx, block_gs_max):
    """Window 100 on the real flagship-type matrix with the CSR-stream SpMV (no creation-time kernel choice), streaming geometry
    forced, at the given value of the tuning key block_gs_max.  tests/golden/block8_parent_bits.json holds what the commit before
    blocks of eight returned for it."""
    csr, init = flagship_type(N, False), G.start_vector(N, 5, np.float64)
    keys = {"spmv_kernel": "csr", "blas_small_bytes": "0", "sweep_pipeline": "2", "block_gs_max": str(block_gs_max)}
    try:
        for k, v in keys.items():
            ctx.set_tuning(k, v)
        op = L.CsrOperator(ctx, *csr)
        eng = L.LambdaLanczos(op, N, True, 1)
        eng.init_vector = lambda out, *_: np.copyto(out, init)
        eng.max_iteration = 100
        eng.eps = 0.0
        vals, vecs = eng.run()
        st = dict(eng.last_stats)
        out = dict(iters=[int(i) for i in eng.getIterationCounts()], alpha=[float(a).hex() for a in eng.last_alpha],
                   beta=[float(b).hex() for b in eng.last_beta], value=float(vals[0]).hex(), vector_sha256=sha(vecs[0]),
                   block_iterations=int(st["block_iterations"]), pair_iterations=int(st["pair_iterations"]))
        op.close()
        return out
    finally:
        for k in keys:
            ctx.set_tuning(k, None)
