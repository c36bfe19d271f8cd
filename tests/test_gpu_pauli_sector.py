"""The sum-of-Pauli-strings operator on one S_z sector (ll_op_create_pauli_sector_*, csrc/pauli_sector.hip): every apply against
the EXACT host reference of the sector block of the expanded matrix (generators.pauli_sector_csr, one entry per term and state)
with the bounds the lattice operator is held to, the same bits for every block size, the same bits as the full-space operator
on an embedded vector, whole eigen-solver and Exponentiator runs against the reference library on the sector's matrix, and the
refusals."""
import json
import math
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import contract_cases as K
import exact_ref as E
import lambda_lanczos_amd as L
from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G
from pauli_cases import TYPES, TYPE_IDS, WIDE, _apply, _checker, _cplx, _run_lanczos, _set_block_bits
from test_gpu_accuracy_contracts import OFFSETS, _check_spmv
from util import overlap

pytestmark = pytest.mark.gpu

BLOCK_BITS = [None, 4, 8]          # default (one block holds every sector below but the largest), 16 and 256 indices per block
SECTORS = [(1, 0), (1, 1), (2, 1), (4, 2), (5, 0), (5, 5), (6, 3), (9, 4), (12, 6), (14, 7), (16, 3)]   # D = 1 .. 3432


def j1j2_terms(n_sites, j1=1.0, j2=0.4, delta=0.7):
    terms = G.heisenberg_terms(n_sites, j1, delta, periodic=False)
    for j in range(n_sites - 2):
        m = (1 << j) | (1 << (j + 2))
        terms += [(m, 0, 0.25 * j2), (m, m, 0.25 * j2), (0, m, 0.25 * j2)]
    return terms


def model_terms(model, n_sites):
    if model == "heisenberg":
        return G.heisenberg_terms(n_sites, 1.0, 1.0, periodic=True)
    if model == "j1j2_field":
        return j1j2_terms(n_sites) + G.zfield_terms(n_sites, 0.3)
    if model == "j1j2":
        return j1j2_terms(n_sites)
    if model == "dm":
        return G.dm_terms(n_sites, 0.35, periodic=True) + G.heisenberg_terms(n_sites, 1.0, 0.8, periodic=True)
    raise KeyError(model)


_REF = {}


def _reference_rows(model, n_sites, n_down, tid):
    key = (model, n_sites, n_down, tid)
    if key not in _REF:
        dtype = TYPES[TYPE_IDS.index(tid)]
        terms = model_terms(model, n_sites)
        csr = G.pauli_sector_csr(n_sites, n_down, terms, WIDE[tid], merge=False)   # coefficients are doubles for every T
        x = K.start_x(math.comb(n_sites, n_down), dtype)
        _REF[key] = (terms, csr, x, E.rows_exact(csr, x))
    return _REF[key]


# ------------------------------------------------------------------ 1. apply against the exact reference
# (the Dzyaloshinskii-Moriya terms carry one Y each: complex types only)
APPLY_CASES = [(m, t) for m in ("heisenberg", "j1j2_field", "dm") for t in TYPE_IDS if m != "dm" or t in ("z", "c")]


@pytest.mark.parametrize("model,tid", APPLY_CASES, ids=["%s-%s" % c for c in APPLY_CASES])
def test_apply_meets_the_componentwise_contract(ctx, model, tid):
    dtype = TYPES[TYPE_IDS.index(tid)]
    worst = (0.0, 0.0, 0.0)
    try:
        for n_sites, n_down in SECTORS:
            terms, csr, x, ex = _reference_rows(model, n_sites, n_down, tid)
            n = x.shape[0]
            op = L.PauliSectorOperator(ctx, n_sites, n_down, terms, dtype)
            assert op.info() == (n, n, len(terms)) and (op.n, op.n_local, op.n_sites, op.n_down) == (n, n, n_sites, n_down)
            for bits in BLOCK_BITS:
                _set_block_bits(ctx, "sector", bits)
                for shift in (0, 1):
                    for offset in OFFSETS:
                        y, alpha = _apply(ctx, op, x, shift, offset, True)
                        # the lattice operator's checks: products formed exactly in double, floating-point sums
                        r = _check_spmv("pauli_sector", "stencil", False, dtype, csr, x, ex, ex, y, alpha, offset)
                        worst = tuple(max(a, b) for a, b in zip(worst, r))
            op.close()
    finally:
        _set_block_bits(ctx, "sector", None)
    print("ratios error/bound (class, storage, alpha)", model, tid, worst)


# ------------------------------------------------------------------ 2. the same bits for every geometry
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_same_bits_for_every_block_size_and_alignment(ctx, dtype):
    tid = TYPE_IDS[TYPES.index(dtype)]
    try:
        for model, n_sites, n_down in [("heisenberg", 14, 7), ("j1j2_field", 12, 6), ("dm" if _cplx(dtype) else "j1j2_field", 9, 4)]:
            terms, _, x, _ = _reference_rows(model, n_sites, n_down, tid)
            op = L.PauliSectorOperator(ctx, n_sites, n_down, terms, dtype)
            first = None
            for bits in [None, 0, 1, 4, 8, 12]:
                _set_block_bits(ctx, "sector", bits)
                for shift in (0, 1):
                    for rep in range(2):
                        y, _ = _apply(ctx, op, x, shift, -2.5, False)
                        if first is None:
                            first = y
                        assert np.array_equal(first.view(np.uint8), y.view(np.uint8)), (model, bits, shift, rep)
            op.close()
    finally:
        _set_block_bits(ctx, "sector", None)


# ------------------------------------------------------------------ 3. the same bits as the full-space operator
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_same_bits_as_the_full_space_operator_on_an_embedded_vector(ctx, dtype):
    """Holds by construction: the groups the sector kernel skips have weight exactly 0 and a zero partner in the embedded vector,
    and with offset 0 nothing else is added — if it fails, the two kernels do not implement the same sum."""
    tid = TYPE_IDS[TYPES.index(dtype)]
    for model, n_sites, n_down in [("heisenberg", 14, 7), ("j1j2_field", 12, 5), ("dm" if _cplx(dtype) else "j1j2_field", 5, 2)]:
        terms, _, x, _ = _reference_rows(model, n_sites, n_down, tid)
        states = G.sector_states(n_sites, n_down).astype(np.int64)
        sec = L.PauliSectorOperator(ctx, n_sites, n_down, terms, dtype)
        full = L.PauliOperator(ctx, n_sites, terms, dtype)
        y, _ = _apply(ctx, sec, x, 0, 0.0, False)
        xf = np.zeros(1 << n_sites, dtype)
        xf[states] = x
        yf, _ = _apply(ctx, full, xf, 0, 0.0, False)
        assert np.array_equal(yf[states].view(np.uint8), y.view(np.uint8)), (model, n_sites, n_down)
        other = np.ones(1 << n_sites, bool)
        other[states] = False
        assert np.all(yf[other] == 0), (model, n_sites, n_down)
        assert np.any(y != 0)
        sec.close()
        full.close()


# ------------------------------------------------------------------ 4. deferred normalisation
def test_deferred_normalisation_path_against_separate_launches(ctx):
    """fuse_launches = 1 and 2 (the kernel normalises its input on the fly through ScaleIn) against 0 (a launch of its own) on
    the Heisenberg ring, sector (12, 6), 256 indices per block: traces to 1e-10 |A|_inf per k, iteration counts within 2."""
    n_sites, n_down = 12, 6
    terms = model_terms("heisenberg", n_sites)
    n = math.comb(n_sites, n_down)
    init = G.start_vector(n, 1)
    op = L.PauliSectorOperator(ctx, n_sites, n_down, terms)
    norm = op.inf_norm()
    runs = {}
    try:
        ctx.set_tuning("pauli_sector_block_bits", "8")
        for level in ("0", "1", "2"):
            ctx.set_tuning("fuse_launches", level)
            eng, vals, _ = _run_lanczos(op, n, init, False, -norm)
            runs[level] = (eng.last_alpha, eng.last_beta, vals[0], eng.getIterationCounts())
    finally:
        ctx.set_tuning("fuse_launches", None)
        ctx.set_tuning("pauli_sector_block_bits", None)
    op.close()
    base = runs["0"]
    for level in ("1", "2"):
        r = runs[level]
        k = min(len(r[0]), len(base[0]))
        print("fuse_launches %s against 0: %s / %s iterations, max |d alpha| = %.3e, max |d beta| = %.3e, |d lambda| = %.3e"
              % (level, r[3], base[3], np.max(np.abs(r[0][:k] - base[0][:k])), np.max(np.abs(r[1][:k] - base[1][:k])),
                 abs(r[2] - base[2])))
    for level in ("1", "2"):
        r = runs[level]
        k = min(len(r[0]), len(base[0]))
        assert abs(r[3][0] - base[3][0]) <= 2 and k >= 10
        assert np.max(np.abs(r[0][:k] - base[0][:k])) <= 1e-10 * norm
        assert np.max(np.abs(r[1][:k] - base[1][:k])) <= 1e-10 * norm
        assert abs(r[2] - base[2]) <= 1e-10 * max(1.0, abs(base[2] - norm))


# ------------------------------------------------------------------ 5. whole runs against the real reference
def _spmv_csr(csr, x):
    rp, ci, va = csr
    return np.add.reduceat(va * x[ci], rp[:-1]) if rp[-1] else np.zeros_like(x)


@pytest.mark.parametrize("num_eigs", [1, 3])
@pytest.mark.parametrize("find_max", [False, True], ids=["smallest", "largest"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["d", "s"])
def test_lanczos_against_the_reference(ctx, dtype, find_max, num_eigs):
    n_sites, n_down = 12, 6
    n = math.comb(n_sites, n_down)
    terms = model_terms("j1j2", n_sites)
    csr = G.pauli_sector_csr(n_sites, n_down, terms, np.float64)
    single = np.dtype(dtype) == np.float32
    init = G.start_vector(n, 1).astype(dtype)
    op = L.PauliSectorOperator(ctx, n_sites, n_down, terms, dtype)
    norm = op.inf_norm()
    assert abs(norm - sum(abs(c) for _, _, c in terms)) <= 1e-12 * norm
    offset = norm if find_max else -norm
    eng, vals, vecs = _run_lanczos(op, n, init, find_max, offset, num_eigs=num_eigs)
    ref = _checker().lanczos(csr, init.astype(np.float64), find_max, num_eigs=num_eigs, offset=offset, eps=eng.eps)
    scale = max(1.0, np.max(np.abs(ref["eigenvalues"] + offset)))
    assert len(vals) == num_eigs
    if single:   # the float rules of tests/test_gpu_float.py
        assert np.max(np.abs(vals - ref["eigenvalues"])) <= 20 * eng.eps * scale
    else:
        assert np.max(np.abs(vals - ref["eigenvalues"])) <= 1e-10 * scale
        assert abs(eng.getIterationCounts()[0] - ref["iter_counts"][0]) <= 2
        r = np.linalg.norm(_spmv_csr(csr, vecs[0]) - vals[0] * vecs[0])
        assert r <= 1e-5 * norm
        # the open XXZ chain with a second-neighbour bond has no multiplets inside a sector: traces and eigenvectors too
        k = min(len(eng.last_alpha), len(ref["alpha"]))
        if num_eigs == 1:
            assert np.max(np.abs(eng.last_alpha[:k] - ref["alpha"][:k])) <= 1e-10 * norm
        assert 1 - overlap(vecs[0], ref["eigenvectors"][0]) <= 1e-8
    op.close()


@pytest.mark.parametrize("full_orth", [False, True], ids=["three_term", "full_orthogonalize"])
@pytest.mark.parametrize("model", ["j1j2", "dm"])
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64], ids=["z", "c"])
def test_exponentiator_against_the_reference(ctx, dtype, model, full_orth):
    n_sites, n_down = 12, 6
    n = math.comb(n_sites, n_down)
    terms = model_terms(model, n_sites)
    csr = G.pauli_sector_csr(n_sites, n_down, terms, np.complex128)
    single = np.dtype(dtype) == np.complex64
    inp = G.start_vector(n, 2, np.complex128).astype(dtype)
    a = -0.05j
    op = L.PauliSectorOperator(ctx, n_sites, n_down, terms, dtype)
    ex = L.Exponentiator(op, n)
    ex.full_orthogonalize = full_orth
    out, it = ex.run(a, inp)
    o_out, o_it, _ = _checker().expo(csr, a, inp.astype(np.complex128), eps=ex.eps, full_orthogonalize=full_orth)
    assert abs(it - o_it) <= 2
    if single:
        assert np.linalg.norm(out - o_out) <= 1e-3 * np.linalg.norm(o_out)
    else:
        assert 1 - overlap(out, o_out) <= 10 * ex.eps
        assert abs(np.linalg.norm(out) / np.linalg.norm(inp) - 1) <= 1e-12
        assert np.max(np.abs(out - o_out)) <= 1e-10 * np.linalg.norm(inp)
    t_out, _ = ex.taylor_run(a, inp)
    r_out, _, _ = _checker().expo(csr, a, inp.astype(np.complex128), eps=ex.eps, taylor=True)   # the reference's own Taylor sum
    assert np.linalg.norm(t_out - r_out) <= (1e-3 if single else 1e-10) * np.linalg.norm(r_out)
    op.close()


def test_four_site_ring_has_its_singlet_at_minus_two_j(ctx):
    J = 1.5
    op = L.PauliSectorOperator(ctx, 4, 2, G.heisenberg_terms(4, J, 1.0, periodic=True))
    assert op.n == 6
    _, vals, _ = _run_lanczos(op, 6, G.start_vector(6, 1), False, -op.inf_norm())
    op.close()
    assert abs(vals[0] + 2.0 * J) <= 1e-10 * 2.0 * J


def test_ground_energy_of_18_sites_equals_the_full_space_one(ctx):
    """Heisenberg ring, L = 18: the ground state is a singlet, so it lies in the sector n_down = 9 (D = 48 620 of 262 144)."""
    n_sites, n_down = 18, 9
    terms = model_terms("heisenberg", n_sites)
    n = math.comb(n_sites, n_down)
    sec = L.PauliSectorOperator(ctx, n_sites, n_down, terms)
    full = L.PauliOperator(ctx, n_sites, terms)
    norm = sec.inf_norm()
    assert n == 48620 and norm == full.inf_norm()
    assert sec.device_bytes() >= 4 * n and sec.device_bytes() < 4 * n + (1 << 16)   # the states and two small tables
    eng_sec, val_sec, _ = _run_lanczos(sec, n, G.start_vector(n, 1), False, -norm)
    eng_full, val_full, _ = _run_lanczos(full, 1 << n_sites, G.start_vector(1 << n_sites, 1), False, -norm)
    print("Heisenberg ring L = 18: sector (18, 9) E0 = %.13f after %d iterations, full space E0 = %.13f after %d iterations"
          % (val_sec[0], eng_sec.getIterationCounts()[0], val_full[0], eng_full.getIterationCounts()[0]))
    sec.close()
    full.close()
    assert abs(val_sec[0] - val_full[0]) <= 1e-10 * norm


# ------------------------------------------------------------------ 6. refusals
def _refused(ctx, n_sites, n_down, terms, dtype=np.float64):
    with pytest.raises(capi.LanczosHipError) as e:
        L.PauliSectorOperator(ctx, n_sites, n_down, terms, dtype).close()
    assert e.value.code == capi.LL_ERR_INVALID, str(e.value)
    return str(e.value)


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_invalid_inputs_are_refused_with_their_cause(ctx, dtype):
    heis = G.heisenberg_terms(6, 1.0, 1.0)
    msg = _refused(ctx, 6, 3, G.tfim_terms(6, 1.0, 1.5), dtype)        # a field along x flips one spin
    assert "conserve S_z" in msg and "x mask 0x1 " in msg, msg
    msg = _refused(ctx, 6, 3, heis + [(0b110000, 0, 0.25)], dtype)    # a lone XX term: no YY to cancel it on aligned spins
    assert "conserve S_z" in msg and "x mask 0x30 " in msg, msg
    m = 0b11
    msg = _refused(ctx, 6, 3, [(m << 2, 0, 0.25), (m << 2, m << 2, 0.25), (m, 0, 0.25), (m, m, 0.2)], dtype)   # J_x != J_y on bond 0
    assert "conserve S_z" in msg and "x mask 0x3 " in msg, msg
    for n_down in (-1, 7):
        assert "n_down" in _refused(ctx, 6, n_down, heis, dtype)
    assert "n_sites" in _refused(ctx, 31, 15, heis, dtype)
    msg = _refused(ctx, 6, 3, [(0b11, 0b01, 1.0)], dtype)             # X1 Y0 alone: one Y, and not conserving
    assert ("odd number of Y" in msg) if not _cplx(dtype) else ("conserve S_z" in msg), msg
    wide = (1 << 21) - 1                                              # XX + YY on one bond under a Z string over 21 sites
    msg = _refused(ctx, 24, 12, [(0b11, wide & ~0b11, 0.25), (0b11, wide, 0.25)], dtype)
    assert "21 sites" in msg and "cannot be made" in msg and "x mask 0x3 " in msg, msg
    ok = L.PauliSectorOperator(ctx, 24, 1, [(0b11, (wide >> 1) & ~0b11, 0.25), (0b11, wide >> 1, 0.25)], dtype)   # 20 sites: checked
    assert ok.n == 24
    with pytest.raises(capi.LanczosHipError):
        L.CsrOperator.select_spmv(ok, capi.SPMV_CSR_STREAM)           # not a CSR operator, like the lattice operator
    with pytest.raises(capi.LanczosHipError):
        L.CsrOperator.set_accuracy(ok, capi.ACCURACY_NORMWISE)
    assert L.CsrOperator.accuracy(ok) == capi.ACCURACY_COMPONENTWISE
    ok.close()


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_zero_and_diagonal_operators(ctx, dtype):
    n_sites, n_down = 7, 3
    n = math.comb(n_sites, n_down)
    x = K.start_x(n, dtype)
    xd, yd = ctx.to_device(x), ctx.empty(n, dtype)
    op = L.PauliSectorOperator(ctx, n_sites, n_down, [], dtype)                       # no term: the zero operator
    assert op.info() == (n, n, 0) and op.inf_norm() == 0.0
    L.spmv(op, xd, yd, offset=0.0)
    assert np.all(yd.get() == 0)
    op.close()
    op = L.PauliSectorOperator(ctx, n_sites, n_down, [(0, 0, 0.5)] + G.zfield_terms(n_sites, 0.25), dtype)
    L.spmv(op, xd, yd, offset=0.0)                                                    # 0.5 - 0.25 (L - 2 n_down): exact in every T
    want = (0.5 - 0.25 * (n_sites - 2 * n_down)) * x.astype(WIDE[TYPE_IDS[TYPES.index(dtype)]])
    assert np.array_equal(yd.get(), want.astype(dtype))
    op.close()
    xd.free()
    yd.free()


def test_refused_on_a_sharded_context(tmp_path):
    """Two ranks on the box's GPU over the test transport: the operator is single-GPU."""
    from conftest import SHM_TRANSPORT

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name = "/ll_shm_psec_" + uuid.uuid4().hex[:12]
    env = dict(os.environ, LL_COMM_PLUGIN=SHM_TRANSPORT, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(root, "tests", "shm_pauli_refused_worker.py"), str(r), "2", name,
                               str(tmp_path), "sector"], env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-4000:]
    for r in range(2):
        res = json.load(open(os.path.join(tmp_path, "rank%d.json" % r)))
        assert res["code"] == capi.LL_ERR_INVALID and "sharded" in res["msg"], res
