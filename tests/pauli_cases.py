"""What the GPU tests of the five matrix-free spin-1/2 operators share (tests/test_gpu_pauli.py, _sector.py, _momentum.py,
_momentum_full.py, _symmetric.py, _large.py): the storage types, the block-geometry keys, the guarded apply with its
component-wise class, and the eigen-solver run with its checker.  No test."""
import numpy as np

import exact_ref as E
import lambda_lanczos_amd as L
import oracle_lib
from lambda_lanczos_amd import generators as G
from test_gpu_accuracy_contracts import _eps, _guarded, _unguard

TYPES = [np.float64, np.complex128, np.float32, np.complex64]
TYPE_IDS = ["d", "z", "s", "c"]
WIDE = {"d": np.float64, "z": np.complex128, "s": np.float64, "c": np.complex128}
# kind -> the tuning key of its kernel's block (tile) size
BITS_KEY = {"pauli": "pauli_tile_bits", "sector": "pauli_sector_block_bits", "momentum": "pauli_momentum_block_bits",
            "momentum_full": "pauli_momentum_full_block_bits", "symmetric": "pauli_symmetric_block_bits"}


def _cplx(dtype):
    return np.dtype(dtype).kind == "c"


def _tid(dtype):
    return TYPE_IDS[TYPES.index(dtype)]


def dm_ring(n_sites, D):
    """One Dzyaloshinskii-Moriya bond j -> (j + 1) mod L per site; generators.dm_terms keeps ONE bond at L = 2 (an open chain)."""
    if n_sites != 2:
        return G.dm_terms(n_sites, D, periodic=True)
    return [(3, 2, float(D)), (3, 1, -float(D)), (3, 1, float(D)), (3, 2, -float(D))]


def _runs(dtype, n_sites, m):
    """d / s run only where the block is real."""
    return _cplx(dtype) or (2 * m) % n_sites == 0


def _set_block_bits(ctx, kind, bits):
    ctx.set_tuning(BITS_KEY[kind], None if bits is None else str(bits))   # None removes the setting


def _apply(ctx, op, x, shift, offset, want_dot):
    n = x.shape[0]
    xb, xv = _guarded(ctx, x, shift)
    yb, yv = _guarded(ctx, np.zeros(n, x.dtype), shift)
    alpha = L.spmv(op, xv, yv, offset=offset, want_dot=want_dot)
    y = _unguard(yb, n, shift).copy()
    assert np.array_equal(_unguard(xb, n, shift), x), "the apply changed its input"
    xb.free()
    yb.free()
    return y, alpha


def _class_bound(dtype, x, ex, y, offset):
    """The component-wise class exactly as test_gpu_accuracy_contracts._check_spmv forms `cls`: componentwise_bound plus the offset
    and narrowing terms.  Holds by derivation: a kernel entry carries at most about 4 double roundings (weight x sqrt factor x phase,
    complex) and the chain adds nnz / 2 — below the class's 8 (nnz + 2)."""
    eps = _eps(dtype)
    xw = x.astype(np.complex128 if _cplx(dtype) else np.float64)
    cls = E.componentwise_bound(ex, eps)
    return cls + eps * (np.abs(offset) * (np.abs(xw.real) + np.abs(xw.imag)) + np.abs(y.real) + np.abs(np.imag(y))) + 1e-300, xw


def _check_apply(dtype, x, ex, y, alpha, offset, what):
    cls, xw = _class_bound(dtype, x, ex, y, offset)
    ok, r_cls = E.within(E.part_errors(y, ex.y + offset * xw), (cls, cls))
    assert ok, "%s: class bound violated (ratio %.3g)" % (what, r_cls)
    d, db = E.dot_exact(x, y), E.dot_bound(x, y)   # alpha = Re<x, y> of the RETURNED y, accumulated in double
    assert abs(alpha - np.real(d)) <= db, (what, alpha, d, db)
    return r_cls, abs(alpha - np.real(d)) / db


def _run_lanczos(op, n, init, find_max, offset, num_eigs=1, max_iteration=None):
    eng = L.LambdaLanczos(op, n, find_max, num_eigs)
    eng.eigenvalue_offset = offset
    eng.init_vector = lambda v, *_: np.copyto(v, init)
    if max_iteration is not None:
        eng.max_iteration = max_iteration
    vals, vecs = eng.run()
    return eng, vals, vecs


def _checker():
    return oracle_lib.reference() if oracle_lib.have_reference() else oracle_lib.oracle()
