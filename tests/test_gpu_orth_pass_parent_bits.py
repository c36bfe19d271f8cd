"""Every way a two-sweep Gram-Schmidt pass can end (Engine::orth_pass: folded and published, folded and not published, partial sums
pending, derived norm pending) and the complete call (Engine::orth: the primitive ll_orth_block_*, a restart pass's start vector)
against what the commit BEFORE Engine::orth was split returned: tests/golden/orth_pass_parent_bits.json holds, per case, the
iteration counts, the eigenvalues and alpha / beta arrays as hex floats, the SHA-256 of every output vector's bytes and the
ll_run_stats counters n_passes, total_iterations, second_passes, lagged_iterations, pair_iterations; per ll_orth_block call the
norm and the coefficients as hex floats and the SHA-256 of w; per two-rank job and rank the SHA-256 of the fields that
test_gpu_multirank.test_overlapped_exchange_is_bit_identical_to_the_serial_issue_order compares.  Everything is compared for
equality: no tolerance anywhere.  Fixed start vectors and operators without creation-time kernel timing only.  The fixture was
recorded twice, in two processes, from the parent commit's library, and the two recordings agreed in every field of every case
(record(): what wrote it)."""
import hashlib
import json
import os

import numpy as np
import pytest

import lambda_lanczos_amd as L
from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G
from test_gpu_multirank import run_ranks

pytestmark = pytest.mark.gpu

TYPES = {"d": np.float64, "z": np.complex128, "s": np.float32, "c": np.complex64}
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "orth_pass_parent_bits.json")
COUNTERS = ("n_passes", "total_iterations", "second_passes", "lagged_iterations", "pair_iterations")
N = 4096


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _hex(values):
    return [float(x).hex() for x in values]


def _start(n, dtype, seed=1):
    return G.start_vector(n, seed, np.complex128 if np.dtype(dtype).kind == "c" else np.float64).astype(dtype)


def _chain(ctx, dtype, n=N):
    """The open chain 2 u_i - u_{i-1} - u_{i+1}: a deferring operator (ScaleIn), no Ritz value converges in the windows used here."""
    return L.StencilOperator(ctx, [n], diag=2.0, hop=-1.0, dtype=dtype)


def _pb(ctx, dtype, n=N):
    """The 64 x 64 Laplacian through the propagation-blocked kernel: it takes ||w||^2 itself and cannot defer."""
    assert n == N and np.dtype(dtype) == np.float64
    return L.CsrOperator(ctx, *G.laplace2d(64, 0, N), kernel=capi.SPMV_PB)


def _callback(ctx, dtype, n=N):
    """The chain as user code on numpy arrays: the unspeculated loop."""

    def mv_mul(x, y):
        y += 2.0 * x
        y[1:] -= x[:-1]
        y[:-1] -= x[1:]

    return L.HostOperator(ctx, mv_mul, n, dtype)


class _Keys:
    """Tuning keys of the session's context for one case, removed again afterwards."""

    def __init__(self, ctx, keys):
        self.ctx, self.keys = ctx, keys

    def __enter__(self):
        for k, v in self.keys.items():
            self.ctx.set_tuning(k, v)

    def __exit__(self, *exc):
        for k in self.keys:
            self.ctx.set_tuning(k, None)
        if "slab_bytes" in self.keys:
            self.ctx.release_cache()   # (the slabs of four vectors serve no other run)


def _eigen(ctx, make, tid, max_it, keys=None, n=N, num_eigs=1, orth_mode=capi.ORTH_CGS_DGKS):
    dtype = TYPES[tid]
    init = _start(n, dtype)
    with _Keys(ctx, keys or {}):
        op = make(ctx, dtype, n)
        try:
            eng = L.LambdaLanczos(op, n, False, num_eigs)
            eng.init_vector = lambda v, *_: v.__setitem__(slice(None), init)
            eng.max_iteration = max_it
            eng.orth_mode = orth_mode
            vals, vecs = eng.run()
        finally:
            op.close()
    rec = {"iterations": eng.getIterationCounts(), "eigenvalues": _hex(vals), "alpha": _hex(eng.last_alpha),
           "beta": _hex(eng.last_beta), "sha": [_sha(v) for v in vecs]}
    rec.update({k: int(eng.last_stats[k]) for k in COUNTERS})
    return rec


def _expo(ctx, tid, keys=None, full=False):
    dtype = TYPES[tid]
    inp = _start(N, dtype)
    with _Keys(ctx, keys or {}):
        op = _chain(ctx, dtype)
        try:
            ex = L.Exponentiator(op, N)
            ex.max_iteration = 40   # (a real `a` never meets the stop test, |1 - |overlap|| < eps: exp(a T) is not unitary)
            ex.full_orthogonalize = full
            out, m = ex.run(-0.3j if tid == "z" else -0.3, inp)
        finally:
            op.close()
    rec = {"iterations": [int(m)], "sha": [_sha(out)]}
    rec.update({k: int(ex.last_stats[k]) for k in COUNTERS})
    return rec


def _orth_block(ctx, tid, nb, mode):
    """ll_orth_block_* on n = 1000 (ld = 1024) against nb start vectors of other seeds (not orthonormal: the bits are what counts)."""
    dtype, n, ld = TYPES[tid], 1000, 1024
    slab = np.zeros((max(nb, 1), ld), dtype=dtype)
    for j in range(nb):
        slab[j, :n] = _start(n, dtype, seed=3 + j) / np.sqrt(n / 3.0)
    bd, wd = ctx.to_device(slab), ctx.to_device(_start(n, dtype))
    try:
        nrm, h = L.orth_block(ctx, bd if nb else None, nb, ld, wd, n, mode=mode, want_h=True)
        w = wd.get()
    finally:
        bd.free()
        wd.free()
    return {"norm": float(nrm).hex(), "h": _hex(np.asarray(h).view(np.float64)), "sha": [_sha(w)]}


def _rank_fields(r):
    """What test_overlapped_exchange_is_bit_identical_to_the_serial_issue_order compares bit for bit, of one rank."""
    kept = {key: {f: r[key][f] for f in ("alpha", "vals", "vecs")} for key in ("randsym_csr", "randsym_pb")}
    kept.update({key: r[key] for key in ("spmv_pb", "spmv_csr", "laplace", "tiled")})
    return hashlib.sha256(json.dumps(kept, sort_keys=True).encode()).hexdigest()


def _sharded(tmp_path, extra):
    ranks = run_ranks(tmp_path, 2, LL_SPMV_KERNEL="pb", **extra)
    return {"sha": [_rank_fields(r) for r in ranks], "iterations": [r["randsym_pb"]["iters"] for r in ranks],
            "lagged_iterations": [r[k]["lagged"] for r in ranks for k in ("randsym_csr", "randsym_pb")],
            "pair_iterations": [r[k]["pair"] for r in ranks for k in ("randsym_csr", "randsym_pb")]}


CASES = {}
for _t in "dzsc":
    CASES["chain-dgks-%s" % _t] = lambda ctx, t=_t: _eigen(ctx, _chain, t, 40)
for _t in "dz":
    CASES["chain-dgks-unfused-%s" % _t] = lambda ctx, t=_t: _eigen(ctx, _chain, t, 40, {"fuse_launches": 0})
    CASES["chain-mgs-%s" % _t] = lambda ctx, t=_t: _eigen(ctx, _chain, t, 40, orth_mode=capi.ORTH_MGS)
    CASES["chain-cgs2-%s" % _t] = lambda ctx, t=_t: _eigen(ctx, _chain, t, 40, orth_mode=capi.ORTH_CGS2)
    CASES["expo-%s" % _t] = lambda ctx, t=_t: _expo(ctx, t)
    CASES["expo-unfused-%s" % _t] = lambda ctx, t=_t: _expo(ctx, t, {"fuse_launches": 0})
    CASES["expo-full-%s" % _t] = lambda ctx, t=_t: _expo(ctx, t, full=True)
CASES["chain-streaming-d"] = lambda ctx: _eigen(ctx, _chain, "d", 30, {"fuse_launches": 1}, n=131072)
CASES["pb-dgks-d"] = lambda ctx: _eigen(ctx, _pb, "d", 40)
CASES["chain-second-pass-d"] = lambda ctx: _eigen(ctx, _chain, "d", 30, {"dgks_threshold": 2.0})
CASES["chain-two-groups-d"] = lambda ctx: _eigen(ctx, _chain, "d", 130, {"slab_bytes": 1})
CASES["callback-dgks-d"] = lambda ctx: _eigen(ctx, _callback, "d", 30)
CASES["chain-three-eigs-d"] = lambda ctx: _eigen(ctx, _chain, "d", 60, num_eigs=3)
for _t in "dzsc":
    for _nb in (7, 0):
        for _m, _label in ((capi.ORTH_CGS_DGKS, "dgks"), (capi.ORTH_CGS2, "cgs2"), (capi.ORTH_MGS, "mgs")):
            CASES["block-%s-%s-nb%d" % (_label, _t, _nb)] = lambda ctx, t=_t, nb=_nb, m=_m: _orth_block(ctx, t, nb, m)
TWO_SWEEP = sorted(name for name in CASES if not name.startswith("block-"))

SHARDED = {"derived": {}, "unfused": {"LL_FUSE_LAUNCHES": "0"}, "measured": {"LL_SHARDED_NORM": "measured"}}


def record(ctx, tmp_path):
    """What tests/golden/orth_pass_parent_bits.json holds: run with the parent commit's library (LL_LIB_PATH), twice, in two
    processes; the two recordings agreed in every field."""
    return {"cases": {name: CASES[name](ctx) for name in sorted(CASES)},
            "sharded": {name: _sharded(os.path.join(tmp_path, name), SHARDED[name]) for name in sorted(SHARDED)}}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_PATH) as f:
        return json.load(f)


def test_the_fixture_holds_every_case(golden):
    assert sorted(golden["cases"]) == sorted(CASES)
    assert sorted(golden["sharded"]) == sorted(SHARDED)
    # every two-sweep row took the code under test, on the parent too
    for name in TWO_SWEEP:
        assert golden["cases"][name]["lagged_iterations"] == 0 and golden["cases"][name]["pair_iterations"] == 0, name
    for name in SHARDED:
        assert not any(golden["sharded"][name]["lagged_iterations"]), name
    assert golden["cases"]["chain-second-pass-d"]["second_passes"] == 30
    assert golden["cases"]["chain-two-groups-d"]["total_iterations"] == 130
    assert golden["cases"]["chain-three-eigs-d"]["n_passes"] > 1


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_returns_the_parent_commit_s_bits(ctx, golden, name):
    got = CASES[name](ctx)
    want = golden["cases"][name]
    print(name, {k: got[k] for k in ("iterations",) + COUNTERS if k in got})
    if name in TWO_SWEEP:
        assert got["lagged_iterations"] == 0
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], (name, key)


@pytest.mark.parametrize("name", sorted(SHARDED))
def test_two_ranks_return_the_parent_commit_s_bits(tmp_path, golden, name):
    got = _sharded(tmp_path, SHARDED[name])
    print(name, got["iterations"], got["lagged_iterations"])
    assert not any(got["lagged_iterations"])
    assert got == golden["sharded"][name]
