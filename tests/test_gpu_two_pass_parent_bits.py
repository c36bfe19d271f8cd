"""The three basis-free entry points (ll_lanczos_two_pass_*, ll_expo_two_pass, ll_expo_two_pass_multi) and the two primitives
(ll_recur_accum_scaled, ll_recur_accum_multi) against what the commit BEFORE their drivers were put on one skeleton returned:
tests/golden/two_pass_parent_bits.json holds, per case, the iteration counts, workspace_vectors, replay_mismatches, the SHA-256 of
every output's bytes and, for the eigen-solver, the eigenvalue, the residual and the alpha / beta arrays as hex floats; and, per
refused call, the return code and the text of ll_last_error.  Everything is compared for equality.  Fixed start vectors and
matrix-free operators only, so no random draw and no creation-time kernel timing enters.  The fixture was recorded twice, in two
processes, and a case is in it only where the two recordings agreed in every field (record(): what wrote it)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import lambda_lanczos_amd as L
from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G

pytestmark = pytest.mark.gpu

TYPES = {"d": np.float64, "z": np.complex128, "s": np.float32, "c": np.complex64}
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "two_pass_parent_bits.json")
TFIM_TIMES = [-0.5j, 0j, -1.5j, -0.1j]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _start(n, dtype):
    return G.start_vector(n, 1, np.complex128 if np.dtype(dtype).kind == "c" else np.float64).astype(dtype)


def _chain(ctx, dtype):
    """The open transverse-field Ising chain of 10 sites (no Y term: every type takes it), n = 1024."""
    return L.PauliOperator(ctx, 10, G.tfim_terms(10, 1.0, 1.5), dtype), 1024, _start(1024, dtype)


def _sector(ctx, dtype):
    """The Heisenberg ring of 14 sites at n_down = 7: n = 3432, several strips with a ragged last one."""
    return L.PauliSectorOperator(ctx, 14, 7, G.heisenberg_terms(14), dtype), 3432, _start(3432, dtype)


def _diagonal(ctx, dtype):
    """Z terms only: every basis state is an eigenvector, so the recurrence breaks down after one iteration (no replay)."""
    v = np.zeros(64, dtype=dtype)
    v[7] = -2j if np.dtype(dtype).kind == "c" else 2.0
    return L.PauliOperator(ctx, 6, [(0, 1 << j, float(j + 1)) for j in range(6)], dtype), 64, v


def _expo_record(ms, outs, stats):
    return {"m": [int(m) for m in ms], "workspace_vectors": int(stats["workspace_vectors"]),
            "replay_mismatches": int(stats["replay_mismatches"]), "sha": [_sha(o) for o in outs]}


def _expo(ctx, make, tid, a, where="host", max_it=None):
    """ll_expo_two_pass; where: 'host', 'device', 'inplace' (the output is the input's device buffer) or 'same_host' (input and
    output are one host array)."""
    dtype = TYPES[tid]
    op, n, inp = make(ctx, dtype)
    try:
        ex = L.Exponentiator(op, n)
        if max_it is not None:
            ex.max_iteration = max_it
        if where == "host":
            out, m = ex.run_two_pass(a, inp)
            stats = ex.last_stats
        elif where == "same_host":
            out, p, it, st = inp.copy(), ex._params(), C.c_int64(), capi.RunStats()
            capi.check(capi.lib().ll_expo_two_pass(ctx.handle, op.handle, C.byref(p), float(np.real(a)), float(np.imag(a)),
                                                   capi.ptr(out), capi.ptr(out), C.byref(it), C.byref(st)))
            m, stats = it.value, st.as_dict()
        else:
            d_in = ctx.to_device(inp)
            d_out = d_in if where == "inplace" else ctx.empty(n, dtype)
            got, m = ex.run_two_pass(a, d_in, out=d_out)
            assert got is d_out
            out, stats = d_out.get(), ex.last_stats
            d_out.free()
            d_in.free()
    finally:
        op.close()
    return _expo_record([m], [out], stats)


def _expo_multi(ctx, make, tid, times, where="host", max_it=None):
    """ll_expo_two_pass_multi; where: 'host', 'mixed' (outputs 0 and 2 on the device) or 'inplace' (all on the device, output 2 is
    the input's buffer)."""
    dtype = TYPES[tid]
    op, n, inp = make(ctx, dtype)
    try:
        ex = L.Exponentiator(op, n)
        if max_it is not None:
            ex.max_iteration = max_it
        if where == "host":
            outs, ms = ex.run_two_pass_multi(times, inp)
        else:
            d_in = ctx.to_device(inp)
            on_device = (0, 2) if where == "mixed" else tuple(range(len(times)))
            bufs = [ctx.empty(n, dtype) if j in on_device else None for j in range(len(times))]
            if where == "inplace":
                bufs[2].free()
                bufs[2] = d_in
            got, ms = ex.run_two_pass_multi(times, d_in, out=bufs)
            outs = [g.get() if isinstance(g, L.DeviceArray) else g for g in got]
            for b in bufs + [d_in]:
                if b is not None:
                    b.free()
    finally:
        op.close()
    return _expo_record(ms, outs, ex.last_stats)


def _eigen(ctx, make, tid, vec="host", find_maximum=False, max_it=None, start="hook"):
    """ll_lanczos_two_pass_*; vec: 'host', 'device' or 'none'; start: 'hook' or 'device' (init_vector_dev)."""
    dtype = TYPES[tid]
    op, n, init = make(ctx, dtype)
    d_init = d_out = None
    try:
        eng = L.LambdaLanczos(op, n, find_maximum, 1)
        if start == "device":
            d_init = eng.init_vector = ctx.to_device(init)
        else:
            eng.init_vector = lambda v, *_: v.__setitem__(slice(None), init)
        if max_it is not None:
            eng.max_iteration = max_it
        if vec == "device":
            d_out = eng.eigenvectors_out = ctx.empty(n, dtype)
        val, v, info = eng.run_two_pass(want_vector=vec != "none")
        outs = [] if vec == "none" else [d_out.get() if vec == "device" else v]
        if d_init is not None:
            assert np.array_equal(d_init.get().view(np.uint8), init.view(np.uint8))   # init_vector_dev is never modified
    finally:
        op.close()
        for b in (d_init, d_out):
            if b is not None:
                b.free()
    rec = _expo_record([info["iterations"]], outs, info["stats"])
    rec.update(eigenvalue=float(val).hex(), residual="none" if info["residual"] is None else float(info["residual"]).hex(),
               alpha=[float(x).hex() for x in eng.last_alpha], beta=[float(x).hex() for x in eng.last_beta])
    return rec


CASES = {}
for _t in "zc":
    for _w in ("host", "device", "inplace"):
        CASES["expo-chain-%s-%s" % (_t, _w)] = lambda ctx, t=_t, w=_w: _expo(ctx, _chain, t, -0.5j, w)
        CASES["multi-chain-%s-%s" % (_t, "mixed" if _w == "device" else _w)] = (
            lambda ctx, t=_t, w=_w: _expo_multi(ctx, _chain, t, TFIM_TIMES, "mixed" if w == "device" else w))
for _t in "ds":
    CASES["expo-chain-%s-max40" % _t] = lambda ctx, t=_t: _expo(ctx, _chain, t, -0.5, max_it=40)
CASES["expo-sector-z"] = lambda ctx: _expo(ctx, _sector, "z", -0.5j)
CASES["expo-eigenvector-z"] = lambda ctx: _expo(ctx, _diagonal, "z", -0.25j)
CASES["expo-same-host-array-z"] = lambda ctx: _expo(ctx, _chain, "z", -0.5j, "same_host")
CASES["multi-chain-d-two-times-max40"] = lambda ctx: _expo_multi(ctx, _chain, "d", [-0.5, -0.1], max_it=40)
CASES["multi-chain-z-one-time"] = lambda ctx: _expo_multi(ctx, _chain, "z", [-0.5j])
CASES["multi-chain-z-sixteen-equal-times"] = lambda ctx: _expo_multi(ctx, _chain, "z", [-0.5j] * 16)
for _t in "dzsc":
    for _v in ("host", "device", "none"):
        CASES["eigen-chain-%s-%s" % (_t, _v)] = lambda ctx, t=_t, v=_v: _eigen(ctx, _chain, t, v)
CASES["eigen-chain-d-maximum"] = lambda ctx: _eigen(ctx, _chain, "d", find_maximum=True)
CASES["eigen-chain-z-maximum"] = lambda ctx: _eigen(ctx, _chain, "z", find_maximum=True)
CASES["eigen-chain-d-max12"] = lambda ctx: _eigen(ctx, _chain, "d", max_it=12)
CASES["eigen-eigenvector-start-d"] = lambda ctx: _eigen(ctx, _diagonal, "d")
CASES["eigen-eigenvector-start-z"] = lambda ctx: _eigen(ctx, _diagonal, "z")
CASES["eigen-chain-z-init-vector-dev"] = lambda ctx: _eigen(ctx, _chain, "z", start="device")
CASES["eigen-chain-s-init-vector-dev-device"] = lambda ctx: _eigen(ctx, _chain, "s", vec="device", start="device")


def refusals(ctx):
    """[name, return code, ll_last_error text] of every refused call, in a fixed order.  No call reaches a kernel: each is
    refused by an argument check (the buffers are nevertheless valid and large enough for their n)."""
    lib = capi.lib()
    n = 1024
    zop, _, zin = _chain(ctx, np.complex128)
    dop, _, din = _chain(ctx, np.float64)
    other = L.Context(0)
    oop = L.PauliOperator(other, 10, G.tfim_terms(10, 1.0, 1.5), np.complex128)
    dev = [ctx.empty(n, np.complex128) for _ in range(4)]
    zero_dev = ctx.to_device(np.zeros(n, dtype=np.complex128))
    big = np.zeros(2 * n, dtype=np.complex128)
    big[:n] = zin
    zeros = np.zeros(n, dtype=np.complex128)
    rows = []

    def call(name, fn, *args):
        rc = fn(*args)
        rows.append([name, int(rc), lib.ll_last_error().decode("utf-8", "replace") if rc != capi.LL_OK else ""])

    def ep(op=zop, **kw):
        p = L.Exponentiator(op, n)._params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def lp(op=zop, **kw):
        p = L.LambdaLanczos(op, n, False, 1)._params(kw.pop("num_eigs", 1))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def vps(*ptrs):
        return (C.c_void_p * len(ptrs))(*ptrs)

    def reim(*a):
        return (C.c_double * (2 * len(a)))(*[x for v in a for x in (complex(v).real, complex(v).imag)])

    h, o = ctx.handle, zop.handle
    it, st, its = C.c_int64(), capi.RunStats(), (C.c_int64 * 17)()
    hout, hout2 = np.zeros(n, dtype=np.complex128), np.zeros(n, dtype=np.complex128)
    dout = np.zeros(n)
    try:
        # ---- ll_expo_two_pass
        E = lib.ll_expo_two_pass
        good = [h, o, C.byref(ep()), 0.0, -0.5, capi.ptr(zin), capi.ptr(hout), C.byref(it), C.byref(st)]
        for k, what in ((0, "ctx"), (1, "op"), (2, "params"), (5, "input"), (6, "output"), (7, "itern")):
            args = list(good)
            args[k] = None
            call("expo: null " + what, E, *args)
        call("expo: operator of another context", E, h, oop.handle, *good[2:])
        call("expo: matrix_size mismatch", E, h, o, C.byref(ep(matrix_size=n + 1)), *good[3:])
        call("expo: full_orthogonalize", E, h, o, C.byref(ep(full_orthogonalize=1)), *good[3:])
        call("expo: a_im on a real operator", E, h, dop.handle, C.byref(ep(dop)), -0.5, 0.25, capi.ptr(din), capi.ptr(dout),
             C.byref(it), C.byref(st))
        call("expo: a_im on a real operator with full_orthogonalize", E, h, dop.handle, C.byref(ep(dop, full_orthogonalize=1)),
             -0.5, 0.25, capi.ptr(din), capi.ptr(dout), C.byref(it), C.byref(st))
        call("expo: a_im on a real operator with a matrix_size mismatch", E, h, dop.handle,
             C.byref(ep(dop, matrix_size=n + 1)), -0.5, 0.25, capi.ptr(din), capi.ptr(dout), C.byref(it), C.byref(st))
        call("expo: full_orthogonalize with a matrix_size mismatch", E, h, o, C.byref(ep(full_orthogonalize=1, matrix_size=n + 1)),
             *good[3:])
        call("expo: zero input", E, *good[:5], capi.ptr(zeros), *good[6:])
        call("expo: zero input with full_orthogonalize", E, h, o, C.byref(ep(full_orthogonalize=1)), 0.0, -0.5, capi.ptr(zeros),
             *good[6:])
        # ---- ll_expo_two_pass_multi
        M = lib.ll_expo_two_pass_multi
        two = reim(-0.5j, -0.1j)
        good = [h, o, C.byref(ep()), 2, two, capi.ptr(zin), vps(hout.ctypes.data, hout2.ctypes.data), its, C.byref(st)]
        for k, what in ((0, "ctx"), (1, "op"), (2, "params"), (4, "times"), (5, "input"), (6, "outputs")):
            args = list(good)
            args[k] = None
            call("multi: null " + what, M, *args)
        call("multi: operator of another context", M, h, oop.handle, *good[2:])
        call("multi: matrix_size mismatch", M, h, o, C.byref(ep(matrix_size=n + 1)), *good[3:])
        call("multi: full_orthogonalize", M, h, o, C.byref(ep(full_orthogonalize=1)), *good[3:])
        call("multi: a_im on a real operator", M, h, dop.handle, C.byref(ep(dop)), 2, reim(-0.5, -0.5j), capi.ptr(din),
             vps(hout.ctypes.data, hout2.ctypes.data), its, C.byref(st))
        call("multi: a_im on a real operator with full_orthogonalize", M, h, dop.handle, C.byref(ep(dop, full_orthogonalize=1)), 2,
             reim(-0.5, -0.5j), capi.ptr(din), vps(hout.ctypes.data, hout2.ctypes.data), its, C.byref(st))
        seventeen = reim(*([-0.1j] * 17))
        many = vps(*([hout.ctypes.data] * 17))
        call("multi: n_times 0", M, *good[:3], 0, *good[4:])
        call("multi: n_times 17", M, *good[:3], 17, seventeen, good[5], many, its, C.byref(st))
        call("multi: n_times 17 with a null output", M, *good[:3], 17, seventeen, good[5], vps(*([None] * 17)), its, C.byref(st))
        call("multi: n_times 17 with full_orthogonalize", M, h, o, C.byref(ep(full_orthogonalize=1)), 17, seventeen, good[5], many,
             its, C.byref(st))
        call("multi: null output in the list", M, *good[:6], vps(hout.ctypes.data, None), its, C.byref(st))
        call("multi: null output in the list with full_orthogonalize", M, h, o, C.byref(ep(full_orthogonalize=1)), *good[3:6],
             vps(hout.ctypes.data, None), its, C.byref(st))
        call("multi: two overlapping outputs", M, *good[:5], capi.ptr(zin),
             vps(big.ctypes.data, big.ctypes.data + (n // 2) * 16), its, C.byref(st))
        call("multi: the same device output twice", M, *good[:5], dev[0].ptr, vps(dev[1].ptr, dev[1].ptr), its, C.byref(st))
        call("multi: output partly overlapping the input", M, *good[:5], capi.ptr(big),
             vps(hout.ctypes.data, big.ctypes.data + (n // 2) * 16), its, C.byref(st))
        call("multi: output partly overlapping the input and a null output", M, *good[:5], capi.ptr(big),
             vps(big.ctypes.data + (n // 2) * 16, None), its, C.byref(st))
        call("multi: zero input", M, *good[:5], capi.ptr(zeros), *good[6:])
        # ---- ll_lanczos_two_pass_z
        T = lib.ll_lanczos_two_pass_z
        val, res = C.c_double(), C.c_double()
        p = lp()
        p.init_vector_dev = dev[0].ptr
        good = [h, o, C.byref(p), C.byref(val), capi.ptr(hout), C.byref(it), C.byref(res), None, None, C.byref(st)]
        for k, what in ((0, "ctx"), (1, "op"), (2, "params"), (3, "eigenvalue")):
            args = list(good)
            args[k] = None
            call("eigen: null " + what, T, *args)
        call("eigen: operator of another context", T, h, oop.handle, *good[2:])
        call("eigen: operator of another scalar type", lib.ll_lanczos_two_pass_d, *good)
        call("eigen: operator of another width", lib.ll_lanczos_two_pass_c, *good)

        def with_start(**kw):
            q = lp(**kw)
            q.init_vector_dev = dev[0].ptr
            return q

        call("eigen: matrix_size mismatch", T, h, o, C.byref(with_start(matrix_size=n + 1)), *good[3:])
        call("eigen: num_eigs 2", T, h, o, C.byref(with_start(num_eigs=2)), *good[3:])
        call("eigen: num_eigs 2 with a matrix_size mismatch", T, h, o, C.byref(with_start(num_eigs=2, matrix_size=n + 1)), *good[3:])
        call("eigen: eigvec is init_vector_dev", T, *good[:4], dev[0].ptr, *good[5:])
        call("eigen: eigvec is init_vector_dev with num_eigs 2", T, h, o, C.byref(with_start(num_eigs=2)), good[3], dev[0].ptr,
             *good[5:])
        q = lp()
        q.init_vector_dev = zero_dev.ptr
        call("eigen: zero start vector", T, h, o, C.byref(q), *good[3:])
        call("eigen: zero start vector without an eigenvector", T, h, o, C.byref(q), good[3], None, *good[5:])
        # ---- ll_recur_accum_scaled
        S = lib.ll_recur_accum_scaled
        good = [h, ord("z"), 8, dev[0].ptr, dev[1].ptr, None, 0.5, 0.25, 0.5, 0.0, dev[2].ptr]
        for k, what in ((0, "ctx"), (3, "y"), (4, "x"), (10, "psi")):
            args = list(good)
            args[k] = None
            call("scaled: null " + what, S, *args)
        call("scaled: negative n", S, h, ord("z"), -1, *good[3:])
        for s in "ds":
            call("scaled: g_im on '%s'" % s, S, h, ord(s), *good[2:9], 0.125, good[10])
        call("scaled: g_im on 'd' with null y", S, h, ord("d"), 8, None, *good[4:9], 0.125, good[10])
        call("scaled: storage 'x'", S, h, ord("x"), *good[2:])
        call("scaled: storage 'x' with null y", S, h, ord("x"), 8, None, *good[4:])
        call("scaled: storage 'x' with null ctx", S, None, ord("x"), *good[2:])
        # ---- ll_recur_accum_multi
        R = lib.ll_recur_accum_multi
        good = [h, ord("z"), 8, dev[0].ptr, dev[1].ptr, None, 0.5, 0.25, 2, reim(0.5, 0.25j), vps(dev[2].ptr, dev[3].ptr)]
        for k, what in ((0, "ctx"), (3, "y"), (4, "x"), (9, "coefficients"), (10, "accumulators")):
            args = list(good)
            args[k] = None
            call("accum-multi: null " + what, R, *args)
        call("accum-multi: null accumulator in the list", R, *good[:10], vps(dev[2].ptr, None))
        call("accum-multi: n_acc 0", R, *good[:8], 0, *good[9:])
        call("accum-multi: n_acc 17", R, *good[:8], 17, reim(*([0.5] * 17)), vps(*([dev[2].ptr] * 17)))
        call("accum-multi: n_acc 17 with storage 'x'", R, h, ord("x"), *good[2:8], 17, reim(*([0.5] * 17)), vps(*([dev[2].ptr] * 17)))
        call("accum-multi: n_acc 17 with null ctx", R, None, *good[1:8], 17, reim(*([0.5] * 17)), vps(*([dev[2].ptr] * 17)))
        for s in "ds":
            call("accum-multi: g_im on '%s'" % s, R, h, ord(s), *good[2:])
        call("accum-multi: g_im on 'd' with a null accumulator before it", R, h, ord("d"), *good[2:10], vps(None, dev[3].ptr))
        call("accum-multi: g_im on 'd' with a null accumulator after it", R, h, ord("d"), *good[2:9], reim(0.25j, 0.5),
             vps(dev[2].ptr, None))
        call("accum-multi: storage 'x'", R, h, ord("x"), *good[2:])
    finally:
        for b in dev + [zero_dev]:
            b.free()
        for op in (zop, dop, oop):
            op.close()
        other.close()
    return rows


def record(ctx):
    """What tests/golden/two_pass_parent_bits.json holds: run at the parent commit, twice, and kept where both runs agree."""
    return {"cases": {name: CASES[name](ctx) for name in sorted(CASES)}, "refusals": refusals(ctx)}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_PATH) as f:
        return json.load(f)


def test_the_fixture_holds_every_case(golden):
    assert sorted(golden["cases"]) == sorted(CASES)
    families = {name.split("-")[0] for name in golden["cases"]}
    assert families == {"expo", "multi", "eigen"}


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_returns_the_parent_commit_s_bits(ctx, golden, name):
    got = CASES[name](ctx)
    want = golden["cases"][name]
    print(name, "m", got["m"], "workspace", got["workspace_vectors"], "mismatches", got["replay_mismatches"])
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], (name, key)


def test_refusals_are_the_parent_commit_s(ctx, golden):
    got = refusals(ctx)
    assert len(got) == len(golden["refusals"])
    for g, w in zip(got, golden["refusals"]):
        print(g)
        assert g == w
        assert g[1] != capi.LL_OK
