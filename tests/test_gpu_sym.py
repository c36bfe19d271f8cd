"""Symmetric / Hermitian CSR operators stored as one triangle (ll_op_create_csr_sym_*, CsrOperator.from_triangle).

The one-triangle kernel (LL_SPMV_SYM) must give the same bits as the fixed-point PB kernel (and the tiled kernel) on the
expanded full matrix, the expanded fallback the bits of the full operator with the same kernel, and the solvers the runs
of the full-storage operator."""
import numpy as np
import pytest

import exact_ref as E
import lambda_lanczos_amd as L
from lambda_lanczos_amd import generators as G

pytestmark = pytest.mark.gpu
C = L.capi


# ------------------------------------------------------------------ triangles and their expansion (host)
def triangle(csr, uplo):
    rp, ci, va = csr
    n = rp.shape[0] - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    keep = ci >= rows if uplo == "U" else ci <= rows
    trp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int64)
    return trp, np.ascontiguousarray(ci[keep], np.int32), np.ascontiguousarray(va[keep])


def expand(tri, uplo):
    """The full matrix of a triangle, every row in the order the library sums it: upper — the mirrored entries (by source
    row), then the row's own; lower — the row's own, then the mirrored ones."""
    rp, ci, va = tri
    n = rp.shape[0] - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    seq = np.arange(rows.shape[0])
    strict = ci != rows
    r = np.concatenate([rows, ci[strict].astype(np.int64)])
    c = np.concatenate([ci.astype(np.int64), rows[strict]])
    v = np.concatenate([va, np.conj(va[strict]) if np.iscomplexobj(va) else va[strict]])
    own_first = 0 if uplo == "L" else 1
    group = np.concatenate([np.full(rows.shape[0], own_first), np.full(int(strict.sum()), 1 - own_first)])
    s = np.concatenate([seq, seq[strict]])
    order = np.lexsort((s, group, r))
    frp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int64)
    return frp, c[order].astype(np.int32), np.ascontiguousarray(v[order])


def cast(csr, dtype):
    return csr[0], csr[1], np.ascontiguousarray(csr[2]).astype(dtype)


def matrices():
    lap = G.laplace2d_np(300)
    band = G.randsym_np(20000, band=500)
    tor = G.torus_np(64)
    return {"laplace": lap, "band": band, "torus": tor}


_M = {}


def mat(name, dtype):
    if not _M:
        _M.update(matrices())
    m = _M[name]
    if name == "torus":
        dtype = np.complex128 if np.dtype(dtype) in (np.float64, np.complex128) else np.complex64
    elif np.dtype(dtype).kind == "c":
        m = (m[0], m[1], m[2] + 0j)
    return cast(m, dtype)


def apply(ctx, op, x, offset=0.0, want_dot=False):
    xd = ctx.to_device(x)
    yd = ctx.empty(x.shape, x.dtype)
    d = L.spmv(op, xd, yd, offset=offset, want_dot=want_dot)
    y = yd.get()
    xd.free()
    yd.free()
    return y, d


def same_bits(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb])


def start(n, dtype, seed=3):
    x = G.start_vector(n, seed, np.complex128 if np.dtype(dtype).kind == "c" else np.float64)
    return x.astype(dtype)


# ------------------------------------------------------------------ 1. bits
@pytest.mark.parametrize("dtype", [np.float64, np.complex128, np.float32, np.complex64])
@pytest.mark.parametrize("name", ["laplace", "band", "torus"])
@pytest.mark.parametrize("uplo", ["U", "L"])
def test_sym_bits_match_pb_and_tiled(ctx, dtype, name, uplo):
    full0 = mat(name, dtype)
    tri = triangle(full0, uplo)
    full = expand(tri, uplo)
    n = tri[0].shape[0] - 1
    sym = L.CsrOperator.from_triangle(ctx, *tri, uplo=uplo)
    assert sym.selected_spmv() == C.SPMV_SYM
    pb = L.CsrOperator(ctx, *full, kernel=C.SPMV_PB, accuracy=C.ACCURACY_NORMWISE)
    try:
        tl = L.CsrOperator(ctx, *full, kernel=C.SPMV_TILED, accuracy=C.ACCURACY_NORMWISE)
    except L.capi.LanczosHipError:
        tl = None
    x = start(n, full[2].dtype)
    for offset in (0.0, -2.5):
        y_s, d_s = apply(ctx, sym, x, offset, True)
        y_p, d_p = apply(ctx, pb, x, offset, True)
        assert same_bits(y_s, y_p), (name, uplo, offset, np.max(np.abs(y_s - y_p)))
        if tl is not None:
            assert same_bits(y_s, apply(ctx, tl, x, offset)[0])
        assert same_bits(y_s, apply(ctx, sym, x, offset)[0])  # a second launch
        # alpha = Re<x, y> of the returned y, accumulated in double (lanczos_hip.h): against the exact dot product in every type
        assert abs(d_s - E.dot_exact(x, y_s).real) <= E.dot_bound(x, y_s), (name, uplo, offset)
        if np.dtype(dtype) in (np.float64, np.complex128):
            assert abs(d_s - d_p) <= 1e-12 * max(1.0, abs(d_p))
        else:  # the same y bits: both alphas within the double-level bound of the same exact value
            assert abs(d_s - d_p) <= 2 * E.dot_bound(x, y_s)
    # Inf in x: every row NaN, as PB
    xi = x.copy()
    xi[n // 3] = np.inf
    assert same_bits(apply(ctx, sym, xi)[0], apply(ctx, pb, xi)[0])
    for o in (sym, pb, tl):
        if o is not None:
            o.close()


@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
def test_sym_inf_in_one_row(ctx, dtype):
    full0 = mat("band", dtype)
    rp, ci, va = triangle(full0, "U")
    va = va.copy()
    va[rp[700] + 1] = np.inf  # an off-diagonal entry of row 700: rows 700 and its column become NaN
    tri = (rp, ci, va)
    full = expand(tri, "U")
    sym = L.CsrOperator.from_triangle(ctx, *tri, uplo="U")
    pb = L.CsrOperator(ctx, *full, kernel=C.SPMV_PB, accuracy=C.ACCURACY_NORMWISE)
    x = start(rp.shape[0] - 1, dtype)
    y_s, y_p = apply(ctx, sym, x, 1.0)[0], apply(ctx, pb, x, 1.0)[0]
    assert np.isnan(y_s[700]) and np.isnan(y_s[ci[rp[700] + 1]])
    assert same_bits(y_s, y_p)
    sym.close()
    pb.close()


def edge_triangles():
    out = {}
    # empty rows and a duplicate diagonal entry; n smaller than one row block
    rp = np.array([0, 3, 3, 5, 5, 7, 7], np.int64)
    ci = np.array([0, 0, 3, 2, 5, 4, 5], np.int32)
    va = np.array([2.0, 1.5, -1.0, 3.0, 0.25, 1.0, -0.5])
    out["edges"] = (rp, ci, va)
    out["n1"] = (np.array([0, 1], np.int64), np.array([0], np.int32), np.array([4.0]))
    ring = G.ring_csr(1000)
    out["ring"] = triangle(ring, "U")
    return out


@pytest.mark.parametrize("which", ["edges", "n1", "ring"])
@pytest.mark.parametrize("dtype", [np.float64, np.complex128, np.float32, np.complex64])
def test_sym_edge_cases(ctx, which, dtype):
    tri = cast(edge_triangles()[which], dtype)
    if np.dtype(dtype).kind == "c":
        tri = (tri[0], tri[1], tri[2] * np.asarray(1 + 0.5j, dtype))
    full = expand(tri, "U")
    sym = L.CsrOperator.from_triangle(ctx, *tri, uplo="U")
    assert sym.selected_spmv() == C.SPMV_SYM
    try:
        pb = L.CsrOperator(ctx, *full, kernel=C.SPMV_PB, accuracy=C.ACCURACY_NORMWISE)
    except L.capi.LanczosHipError:  # (a shape the PB image does not take: the tiled kernel sums the same integers)
        pb = L.CsrOperator(ctx, *full, kernel=C.SPMV_TILED, accuracy=C.ACCURACY_NORMWISE)
    x = start(tri[0].shape[0] - 1, dtype)
    for offset in (0.0, 0.75):
        assert same_bits(apply(ctx, sym, x, offset)[0], apply(ctx, pb, x, offset)[0])
    sym.close()
    pb.close()


# ------------------------------------------------------------------ 2. fallback
@pytest.mark.parametrize("which", ["random", "wide"])
def test_sym_fallback_expands(ctx, which):
    full0 = G.randsym_np(5000) if which == "random" else G.randsym_np(40000, band=6000)
    tri = triangle(full0, "L")
    full = expand(tri, "L")
    op = L.CsrOperator.from_triangle(ctx, *tri, uplo="L")
    k = op.selected_spmv()
    assert k in (C.SPMV_CSR_STREAM, C.SPMV_PB, C.SPMV_TILED)
    ref = L.CsrOperator(ctx, *full, kernel=k)
    x = start(full[0].shape[0] - 1, np.float64)
    assert same_bits(apply(ctx, op, x, 0.5)[0], apply(ctx, ref, x, 0.5)[0])
    assert op.info()[2] == tri[0][-1]
    with pytest.raises(L.capi.LanczosHipError) as e:
        L.CsrOperator.from_triangle(ctx, *tri, uplo="L", kernel=C.SPMV_SYM)
    assert e.value.code == C.LL_ERR_INVALID
    op.close()
    ref.close()


@pytest.mark.parametrize("kernel", [C.SPMV_CSR_STREAM, C.SPMV_PB])
def test_sym_forced_full_kernel(ctx, kernel):
    tri = triangle(G.laplace2d_np(100), "U")
    full = expand(tri, "U")
    op = L.CsrOperator.from_triangle(ctx, *tri, uplo="U", kernel=kernel)
    assert op.selected_spmv() == kernel
    ref = L.CsrOperator(ctx, *full, kernel=kernel)
    x = start(10000, np.float64)
    assert same_bits(apply(ctx, op, x)[0], apply(ctx, ref, x)[0])
    op.close()
    ref.close()


# ------------------------------------------------------------------ 3. queries and errors
@pytest.mark.parametrize("name", ["laplace", "band"])
def test_sym_queries(ctx, name):
    full0 = mat(name, np.float64)
    tri = triangle(full0, "U")
    full = expand(tri, "U")
    sym = L.CsrOperator.from_triangle(ctx, *tri, uplo="U")
    ref = L.CsrOperator(ctx, *full)
    assert sym.inf_norm() == ref.inf_norm()
    n = tri[0].shape[0] - 1
    assert sym.info() == (n, n, int(tri[0][-1]))
    assert sym.device_bytes() <= 0.6 * ref.device_bytes(), (sym.device_bytes(), ref.device_bytes())
    assert sym.accuracy() == C.ACCURACY_NORMWISE
    assert sym.tiled_layout() == (0, 0)
    assert sym.autotune_ms_of(C.SPMV_SYM) == -1.0
    sym.select_spmv(C.SPMV_SYM)
    with pytest.raises(L.capi.LanczosHipError):
        sym.select_spmv(C.SPMV_PB)
    with pytest.raises(L.capi.LanczosHipError) as e:
        sym.set_accuracy(C.ACCURACY_COMPONENTWISE)
    assert e.value.code == C.LL_ERR_INVALID
    sym.set_accuracy(C.ACCURACY_NORMWISE)
    with pytest.raises(L.capi.LanczosHipError):
        ref.select_spmv(C.SPMV_SYM)  # a full-storage operator has no one-triangle image
    sym.close()
    ref.close()


def test_sym_componentwise_takes_the_expanded_image(ctx):
    tri = triangle(G.laplace2d_np(100), "U")
    op = L.CsrOperator.from_triangle(ctx, *tri, uplo="U", accuracy=C.ACCURACY_COMPONENTWISE)
    assert op.selected_spmv() != C.SPMV_SYM
    assert op.accuracy() == C.ACCURACY_COMPONENTWISE
    with pytest.raises(L.capi.LanczosHipError):
        L.CsrOperator.from_triangle(ctx, *tri, uplo="U", accuracy=C.ACCURACY_COMPONENTWISE, kernel=C.SPMV_SYM)
    op.close()


def test_sym_invalid_triangles(ctx):
    tri = triangle(G.laplace2d_np(30), "U")
    rp, ci, va = tri
    bad_side = ci.copy()
    bad_side[rp[10]] = 5  # row 10 holds column 5: below the diagonal of an upper triangle
    bad_col = ci.copy()
    bad_col[-1] = 900
    cases = [((rp, bad_side, va), "U"), ((rp, ci, va), "L"), ((rp, bad_col, va), "U")]
    for t, uplo in cases:
        with pytest.raises(L.capi.LanczosHipError) as e:
            L.CsrOperator.from_triangle(ctx, *t, uplo=uplo)
        assert e.value.code == C.LL_ERR_INVALID
    h = L.capi.C.c_void_p()
    opt = C.CsrOptions()
    L.capi.check(L.capi.lib().ll_csr_options_default(L.capi.C.byref(opt)))
    code = L.capi.lib().ll_op_create_csr_sym_d(ctx.handle, 900, 7, L.capi.ptr(rp), L.capi.ptr(ci), L.capi.ptr(va),
                                               L.capi.C.byref(opt), L.capi.C.byref(h))
    assert code == C.LL_ERR_INVALID and "uplo" in L.capi.lib().ll_last_error().decode()
    assert not h.value  # no operator was handed out


# ------------------------------------------------------------------ 4. solvers
def _run(op, n, find_max, num_eigs, offset, init):
    eng = L.LambdaLanczos(op, n, find_max, num_eigs)
    eng.init_vector = lambda v, *_: v.__setitem__(slice(None), init)
    eng.eigenvalue_offset = offset
    vals, vecs = eng.run()
    return np.asarray(vals), eng.getIterationCounts()


@pytest.mark.parametrize("case", ["laplace_smallest", "band_largest"])
def test_sym_lanczos_matches_full(ctx, oracle, case):
    if case == "laplace_smallest":
        tri = triangle(G.laplace2d_np(60), "U")
        find_max, k, offset = False, 1, -8.0
    else:
        tri = triangle(G.randsym_np(4000, band=200), "L")
        find_max, k, offset = True, 3, 0.0
    uplo = "U" if case == "laplace_smallest" else "L"
    full = expand(tri, uplo)
    n = tri[0].shape[0] - 1
    init = G.start_vector(n)
    sym = L.CsrOperator.from_triangle(ctx, *tri, uplo=uplo)
    assert sym.selected_spmv() == C.SPMV_SYM
    ref = L.CsrOperator(ctx, *full, kernel=C.SPMV_PB, accuracy=C.ACCURACY_NORMWISE)
    v_s, it_s = _run(sym, n, find_max, k, offset, init)
    v_f, it_f = _run(ref, n, find_max, k, offset, init)
    norm = ref.inf_norm()
    assert it_s == it_f
    assert np.max(np.abs(v_s - v_f)) <= 1e-10 * norm
    ora = oracle.lanczos(full, init, find_max, num_eigs=k, offset=offset)
    assert np.max(np.abs(v_s - np.asarray(ora["eigenvalues"][:k]))) <= 1e-10 * norm
    sym.close()
    ref.close()


def test_sym_exponentiator_hermitian(ctx):
    tri = triangle(G.torus_np(32), "U")
    full = expand(tri, "U")
    n = tri[0].shape[0] - 1
    inp = G.start_vector(n, 1, np.complex128)
    sym = L.CsrOperator.from_triangle(ctx, *tri, uplo="U")
    assert sym.selected_spmv() == C.SPMV_SYM
    ref = L.CsrOperator(ctx, *full)
    out_s, _ = L.Exponentiator(sym, n).run(-0.1j, inp)
    out_f, _ = L.Exponentiator(ref, n).run(-0.1j, inp)
    assert np.max(np.abs(out_s - out_f)) <= 1e-10
    sym.close()
    ref.close()


def test_sym_refused_on_a_sharded_context(tmp_path):
    """Two ranks on the box's GPU over the test transport: a triangle cannot be sharded by rows."""
    import json
    import os
    import subprocess
    import sys
    import uuid

    from conftest import SHM_TRANSPORT

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name = "/ll_shm_sym_" + uuid.uuid4().hex[:12]
    env = dict(os.environ, LL_COMM_PLUGIN=SHM_TRANSPORT, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(root, "tests", "shm_sym_worker.py"), str(r), "2", name, str(tmp_path)],
                              env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-4000:]
    for r in range(2):
        res = json.load(open(os.path.join(tmp_path, "rank%d.json" % r)))
        assert res["code"] == C.LL_ERR_INVALID and "sharded" in res["msg"], res


# ------------------------------------------------------------------ device input, eligibility bounds, complex norm
@pytest.mark.parametrize("case", ["band_d", "torus_z", "random_d"])
def test_sym_from_device_arrays(ctx, case):
    """arrays_on_device = 1: the triangle is read from HBM; the operator is the one the host arrays give (same kernel, same bits)."""
    if case == "band_d":
        full0, kind = mat("band", np.float64), C.SPMV_SYM
    elif case == "torus_z":
        full0, kind = mat("torus", np.complex128), C.SPMV_SYM
    else:
        full0, kind = G.randsym_np(5000), None
    tri = triangle(full0, "U")
    host = L.CsrOperator.from_triangle(ctx, *tri, uplo="U")
    dev_arrays = [ctx.to_device(a) for a in tri]
    dev = L.CsrOperator.from_triangle(ctx, *dev_arrays, uplo="U")
    for a in dev_arrays:
        a.free()  # the operator holds its own image
    assert dev.selected_spmv() == host.selected_spmv()
    if kind is not None:
        assert dev.selected_spmv() == kind
    else:
        assert dev.selected_spmv() != C.SPMV_SYM
    assert dev.info() == host.info() and dev.inf_norm() == host.inf_norm()
    x = start(tri[0].shape[0] - 1, tri[2].dtype)
    for offset in (0.0, 1.25):
        assert same_bits(apply(ctx, dev, x, offset)[0], apply(ctx, host, x, offset)[0])
    dev.close()
    host.close()


@pytest.mark.parametrize("dtype,n,h", [(np.float64, 5000, 2000), (np.complex128, 3000, 2048), (np.float32, 20000, 2048),
                                       (np.complex64, 9000, 2048)])
def test_sym_half_bandwidth_2048_is_eligible(ctx, dtype, n, h):
    """Any triangle of half-bandwidth <= 2048 takes the one-triangle kernel, whatever n."""
    rows = np.arange(n, dtype=np.int64)
    diag = (rows, rows, np.full(n, 3.0))
    far = rows[: n - h]
    band = (far, far + h, np.full(n - h, -0.5))
    near = rows[: n - 1]
    nb = (near, near + 1, np.full(n - 1, -1.0))
    r = np.concatenate([diag[0], band[0], nb[0]])
    c = np.concatenate([diag[1], band[1], nb[1]])
    v = np.concatenate([diag[2], band[2], nb[2]]).astype(dtype)
    if np.dtype(dtype).kind == "c":
        v = v * np.asarray(1 + 0.25j, dtype)
        v[:n] = v[:n].real  # (any diagonal works; a real one keeps the test readable)
    order = np.lexsort((c, r))
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int64)
    tri = (rp, c[order].astype(np.int32), np.ascontiguousarray(v[order]))
    sym = L.CsrOperator.from_triangle(ctx, *tri, uplo="U")
    assert sym.selected_spmv() == C.SPMV_SYM
    full = expand(tri, "U")
    try:
        pb = L.CsrOperator(ctx, *full, kernel=C.SPMV_PB, accuracy=C.ACCURACY_NORMWISE)
    except L.capi.LanczosHipError:  # (a shape the PB image does not take: the tiled kernel sums the same integers)
        pb = L.CsrOperator(ctx, *full, kernel=C.SPMV_TILED, accuracy=C.ACCURACY_NORMWISE)
    x = start(n, dtype)
    assert same_bits(apply(ctx, sym, x, -0.5)[0], apply(ctx, pb, x, -0.5)[0])
    assert sym.inf_norm() == pb.inf_norm()
    sym.close()
    pb.close()


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64, np.float32])
def test_sym_inf_norm_other_types(ctx, dtype):
    full0 = mat("torus" if np.dtype(dtype).kind == "c" else "band", dtype)
    tri = triangle(full0, "L")
    sym = L.CsrOperator.from_triangle(ctx, *tri, uplo="L")
    ref = L.CsrOperator(ctx, *expand(tri, "L"))
    assert sym.selected_spmv() == C.SPMV_SYM
    assert sym.inf_norm() == ref.inf_norm()
    sym.close()
    ref.close()
