"""Shared helpers for the parity tests."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def c2list(a):
    a = np.asarray(a)
    if np.iscomplexobj(a):
        return {"re": a.real.tolist(), "im": a.imag.tolist()}
    return a.tolist()


def list2c(v):
    if isinstance(v, dict):
        return np.asarray(v["re"]) + 1j * np.asarray(v["im"])
    return np.asarray(v)


def overlap(a, b):
    """|<a,b>| / (|a||b|): 1 for parallel vectors, sign/phase independent (T2:66-72)."""
    return abs(np.vdot(a, b)) / (np.linalg.norm(a) * np.linalg.norm(b))


def csr_matvec(csr, x):
    rp, ci, va = csr
    import scipy.sparse as sp

    n = rp.shape[0] - 1
    return sp.csr_matrix((va, ci, rp), shape=(n, x.shape[0])) @ x


def residual(csr, lam, v):
    return np.linalg.norm(csr_matvec(csr, v) - lam * v)


def inf_norm(csr):
    rp, ci, va = csr
    return np.max(np.add.reduceat(np.abs(va), rp[:-1]))


# ------------------------------------------------------------------ tuning hooks of the harness
# The library reads only the user-facing LL_* switches from the environment.  The test hooks and
# geometry overrides are per-context settings (ll_ctx_set_tuning); the harness keeps NAMING them like environment variables —
# so that a test can hand them to a worker process in its environment — and applies them itself, to every context it creates.
HOOK_KEYS = {
    "LL_PB_BLOCK": "pb_block", "LL_PB_ROW_BLOCK": "pb_row_block", "LL_PB_COL_BLOCK": "pb_col_block",
    "LL_PB_THREADS1": "pb_threads1", "LL_PB_PAD": "pb_pad", "LL_PB_XPRE": "pb_xpre",
    "LL_PB_TEST_ALL_REMOTE": "pb_test_all_remote", "LL_FORCE_RP64": "force_rp64",
    "LL_SPMV_TILE_BALANCE": "spmv_tile_balance", "LL_STENCIL_VEC": "stencil_vec",
    "LL_TL_FORCE": "tl_force", "LL_TL_XCD": "tl_xcd", "LL_TL_WALK": "tl_walk",
    "LL_TEST_PAIR_SPLIT": "pair_split", "LL_TEST_PAIR_MAX_STORED": "pair_max_stored",
    "LL_TEST_LAGGED_PIECES": "lagged_pieces", "LL_TEST_LAGGED_MIN_BYTES": "lagged_min_bytes",
    "LL_TRIDIAG_TEST_JITTER_US": "tridiag_test_jitter_us", "LL_STALL_TRACE": "stall_trace",
    "LL_TEST_WORKSPACE_FILL": "test_workspace_fill",
}


def sync_hooks(ctx):
    """Make the context's hook settings equal to what os.environ says under the harness names above."""
    for name, key in HOOK_KEYS.items():
        v = os.environ.get(name)
        ctx.set_tuning(key, v if v else None)


def install_hook_sync():
    """Every Context created from now on (this process) takes the hook settings of os.environ: call once in conftest.py and at
    the top of every worker script."""
    import lambda_lanczos_amd as L

    if sync_hooks not in L.CONTEXT_CREATED_HOOKS:
        L.CONTEXT_CREATED_HOOKS.append(sync_hooks)


# ------------------------------------------------------------------ Gram-Schmidt coefficients against exact projections
def check_orth_h(ctx, llenv, basis_dev, basis, ld, w, mode, h):
    """h of ll_orth_block_* (returned with the default settings) against EXACT projections at the double-level bound of
    exact_ref.dot_bound.  MGS: h_j against the exact projection of the w that step j sees — the output of the same call over
    the first j basis vectors (the steps are strictly sequential, so the first j are the same launches).  DGKS: with
    LL_DGKS_THRESHOLD=0 (no second pass) h must be the projections of the INPUT w; the default call may add a second pass,
    whose corrections are float-level (they remove the roundings of w to float): only then a float-level term is allowed.
    Returns True when the default call ran a second pass."""
    import exact_ref as E
    import lambda_lanczos_amd as L

    n, nb = w.shape[0], basis.shape[0]
    if mode == L.ORTH_MGS:
        steps = range(nb) if nb <= 64 else sorted({0, 1, 2, nb // 2, nb - 1})
        for j in steps:
            wj = w
            if j > 0:
                wd = ctx.to_device(w)
                L.orth_block(ctx, basis_dev, j, ld, wd, n, mode=mode)
                wj = wd.get()
                wd.free()
            assert abs(h[j] - E.dot_exact(basis[j], wj)) <= E.dot_bound(basis[j], wj), ("mgs", j)
        return False
    llenv.setenv("LL_DGKS_THRESHOLD", "0")
    wd = ctx.to_device(w)
    _, h1 = L.orth_block(ctx, basis_dev, nb, ld, wd, n, mode=mode, want_h=True)
    wd.free()
    llenv.delenv("LL_DGKS_THRESHOLD")
    for j in range(nb):
        assert abs(h1[j] - E.dot_exact(basis[j], w)) <= E.dot_bound(basis[j], w), ("pass 1", j)
    if np.array_equal(h, h1):
        return False   # no second pass: h is the pass-1 h asserted above
    # a second pass ran: its corrections are the projections of w's roundings to float after pass 1 (nb roundings per element,
    # fnma_acc) and of the float basis' departure from orthonormality (2 u_f per pair) times sum |h1|
    hw = np.asarray(h1, dtype=np.complex128)
    scale = np.abs(w.astype(np.complex128)) + np.abs(hw) @ np.abs(basis.astype(np.complex128))
    extra = (nb + 2) * E.EPS_F * np.linalg.norm(scale) + 2 * E.EPS_F * np.sum(np.abs(hw))
    for j in range(nb):
        assert abs(h[j] - h1[j]) <= extra, ("pass 2", j)
    return True
