"""ll_pauli_block_expand and ll_pauli_block_project on rings of 20 to 30 sites (the cases, their pinned dimensions, the forced block
sizes and the tabulated (units, grid) of tests/pauli_block_embed_large_cases.py; tests/test_pauli_block_embed_plan_host.py holds
the trip counts without a GPU): every kernel takes two or more trips of its grid-stride loop, indices and rank tables are those of
30 sites, and a sector block is expanded into the full space.

The instrument is the INTEGER state of pauli_measure_large_cases (parts from +-{1 .. 7}):
  expand, real character    got == (wide(c[col]) * val).astype(T), the numpy product — tolerance zero, as the small file derives it.
  project, real character   the |G| terms +-psi[g a] are integers and so is every partial sum S (|S| <= 7 * 120 < 2^53): exact in
                            any order, so got == (float64(S) * (sqrt(float64(R_a)) / float64(|G|))).astype(T) bit for bit.
  complex momenta           the bounds of tests/test_gpu_pauli_block_embed.py: 16 eps_d |val c| + eps_T |ref| per element of expand,
                            (2 (|G| + 8) + 8) eps_d sum |val psi| + eps_T |want| per coefficient of project.
Empty rows of B come back exactly +0.0 in a NaN-prefilled output; the default block sizes give the same bits as the forced ones.
The host references are the sparse embeddings over sector_states (a search, no 2^30 numbers); for 2^20 / 2^21 the dense index.

All eight cases run at their 30-, 22-, 21- and 20-site sizes: creation and the references take a few seconds at most (printed per
case with the GPU time)."""
import math
import time

import numpy as np
import pytest

import exact_ref as E
import lambda_lanczos_amd as L
import pauli_block_embed_large_cases as C
import pauli_large_cases as PL
import pauli_measure_large_cases as M
from guarded import pattern
from pauli_cases import _eps
from test_gpu_pauli_expect import NAN_FILL

pytestmark = pytest.mark.gpu

_EMBED = {}


def _embedding(case):
    key = C.case_id(case)
    if key not in _EMBED:
        t0 = time.perf_counter()
        _EMBED[key] = C.embedding(case[0], case[1], case[2]) + (time.perf_counter() - t0,)
        for a in _EMBED[key][:3]:
            a.setflags(write=False)
    return _EMBED[key]


def _operators(ctx, case, dtype):
    kind, shape, target = case[:3]
    terms = PL.model_terms(C.block_model(kind, shape), shape[0])
    if kind == "momentum":
        block = L.PauliMomentumOperator(ctx, *shape, terms, dtype)
    elif kind == "momentum_full":
        block = L.PauliMomentumFullOperator(ctx, *shape, terms, dtype)
    else:
        block = L.PauliSymmetricOperator(ctx, shape[0], shape[1], terms, dtype, parity=shape[2], inversion=shape[3], n_down=shape[4])
    zz = [(0, 3, 1.0)]
    top = L.PauliOperator(ctx, target[1], zz, dtype) if target[0] == "full" else L.PauliSectorOperator(ctx, target[1], target[2], zz, dtype)
    return block, top


def _device_call(ctx, fn, vec, n_out):
    """fn(in, out) on device buffers, the output prefilled with NaN; the result on the host."""
    din = ctx.to_device(vec)
    dout = ctx.to_device(pattern(n_out, vec.dtype, NAN_FILL))
    try:
        fn(din, dout)
        got = dout.get()
        assert np.array_equal(din.get(), vec), "the call changed its input"
    finally:
        din.free()
        dout.free()
    return got


CASES = [(case, t) for case in C.CASES for t in C.tids(case[0], case[1])]


@pytest.mark.parametrize("case,tid", CASES, ids=["%s-%s" % (C.case_id(c), t) for c, t in CASES])
def test_expand_and_project_on_large_rings(ctx, case, tid):
    kind, shape, target, ebits, pbits, e_launch, p_launch = case
    dtype = M.TYPES[tid]
    real = C.real_character(kind, shape)
    gsize = C.group_size(kind, shape)
    n, dim = C.target_dim(target), C.block_dim(kind, shape)
    assert C.expand_launch(n, ebits) == e_launch and C.project_launch(dim, pbits) == p_launch
    assert e_launch[0] > e_launch[1] and p_launch[0] > p_launch[1]                     # two or more trips of both loops
    t0 = time.perf_counter()
    block, top = _operators(ctx, case, dtype)
    t_create = time.perf_counter() - t0
    try:
        assert block.n_local == dim and top.n_local == n
        col, val, R, t_embed = _embedding(case)
        c = M.integer_state(dim, dtype, 21)
        psi = M.integer_state(n, dtype, 22)
        t0 = time.perf_counter()
        ref_e = C.expand_np(col, val, c, dtype)
        if real:
            ref_p = C.project_integer_np(col, val, R, psi, dim, kind, shape, dtype)
        else:
            want, mag = C.project_np(col, val, psi, dim)
        t_host = time.perf_counter() - t0 + t_embed
        t0 = time.perf_counter()
        ctx.set_tuning("pauli_block_expand_block_bits", str(ebits))
        ctx.set_tuning("pauli_block_project_block_bits", str(pbits))
        got_e = _device_call(ctx, lambda i, o: block.expand(i, top, out=o), c, n)
        got_p = _device_call(ctx, lambda i, o: block.project(i, top, out=o), psi, dim)
        ctx.set_tuning("pauli_block_expand_block_bits", None)
        ctx.set_tuning("pauli_block_project_block_bits", None)
        dflt_e = _device_call(ctx, lambda i, o: block.expand(i, top, out=o), c, n)
        dflt_p = _device_call(ctx, lambda i, o: block.project(i, top, out=o), psi, dim)
        t_gpu = time.perf_counter() - t0
        assert not np.any(np.isnan(got_e)) and not np.any(np.isnan(got_p)), "an element of an output was not written"
        assert np.array_equal(got_e.view(np.uint8), dflt_e.view(np.uint8)) and np.array_equal(got_p.view(np.uint8), dflt_p.view(np.uint8))
        empty = col < 0
        assert np.array_equal(got_e[empty].view(np.uint8), np.zeros(int(empty.sum()), got_e.dtype).view(np.uint8))
        if target[0] == "full" and kind != "momentum_full" and shape[-1] is not None:
            assert int(empty.sum()) >= n - math.comb(shape[0], shape[-1])                  # every state outside the sector
        if real:
            assert np.array_equal(got_e, ref_e), "expand: not the numpy product bit for bit"
            assert np.array_equal(got_p, ref_p), "project: not float64(S) * (sqrt(R) / |G|) bit for bit"
            worst = (0.0, 0.0)
        else:
            scale = np.abs(val) * np.abs(c.astype(np.complex128)[np.maximum(col, 0)])
            be = 16.0 * E.EPS_D * scale + _eps(dtype) * np.abs(ref_e.astype(np.complex128)) + 1e-300
            ee = np.abs(got_e.astype(np.complex128) - ref_e.astype(np.complex128))
            assert np.all(ee <= be), ("expand", int(np.argmax(ee - be)))
            bp = (2 * (gsize + 8) + 8) * E.EPS_D * mag + _eps(dtype) * np.abs(want) + 1e-300
            ep = np.abs(got_p.astype(np.complex128) - want)
            assert np.all(ep <= bp), ("project", int(np.argmax(ep - bp)))
            worst = (float(np.max(ee / be)), float(np.max(ep / bp)))
        assert np.count_nonzero(got_e) == int((~empty).sum()) and np.count_nonzero(got_p) > dim // 2
    finally:
        ctx.set_tuning("pauli_block_expand_block_bits", None)
        ctx.set_tuning("pauli_block_project_block_bits", None)
        block.close()
        top.close()
    print("%s %s: expand %s project %s (units, grid); creation %.2f s, GPU calls %.2f s, host reference %.2f s; worst error / bound %s"
          % (C.case_id(case), tid, e_launch, p_launch, t_create, t_gpu, t_host, worst))
