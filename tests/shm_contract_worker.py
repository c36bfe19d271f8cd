"""One rank of tests/test_gpu_sharded_contracts.py: `world` of these processes share the single GPU of the test box and talk through
the host-staged test transport (LL_COMM_PLUGIN), like tests/shm_rank_worker.py.  Every operator form of a sharded context is
created with an explicit kernel / accuracy (no timing decides anything, so every rank walks the same sequence of collectives)
and applied to the rank's shard of x at three offsets, x and y in guarded buffers at pointer shift 0 and 1.  The shards of
every y, every alpha and what the operator reports about itself go into rank<r>.npz; the parent checks them against the exact
host reference.  argv: rank world shm_name out_dir

plan(world) and the input builders are imported by the parent too: both sides must name the same cases and build the same
matrices."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import contract_cases as K  # noqa: E402
import lambda_lanczos_amd as L  # noqa: E402
from lambda_lanczos_amd import _capi as capi  # noqa: E402

TYPES = {"d": np.float64, "z": np.complex128, "s": np.float32, "c": np.complex64}
OFFSETS = [0.0, -2.5, 0.1]
SHIFTS = (0, 1)
# the switches and hooks a case may set; everything a case does not name is unset for it
MANAGED = ["LL_PB_PHASE2", "LL_TL_FORCE", "LL_FORCE_RP64", "LL_STENCIL_VEC", "LL_CSR_SPLIT", "LL_GATHER_CHUNKS", "LL_PB_BLOCK",
           "LL_PB_ROW_BLOCK"]
CSR_N = 5003          # shards of 2502 / 2501 rows on two ranks, 1668 / 1668 / 1667 on three
TINY = [1, 2, 3]      # empty shards, n_local < n_shard, the pad branch of the all-gather


def _single(dtype):
    return np.dtype(dtype) in (np.float32, np.complex64)


def csr_forms():
    """name -> (kernel, accuracy, settings, fixed-point sums?, column-split image?)"""
    forms = {}
    for split in (True, False):
        for rp64 in (False, True):
            env = {}
            if not split:
                env["LL_CSR_SPLIT"] = "0"
            if rp64:
                env["LL_FORCE_RP64"] = "1"
            forms["csr_%s%s" % ("split" if split else "gather", "_rp64" if rp64 else "")] = \
                (capi.SPMV_CSR_STREAM, None, env, False, split)
    for phase2, acc in (("fixed", capi.ACCURACY_NORMWISE), ("ordered", None), ("atomic", None)):
        for chunks in ("1", "3"):
            for block in (None, "37"):
                env = {"LL_GATHER_CHUNKS": chunks}
                if phase2 != "fixed":
                    env["LL_PB_PHASE2"] = phase2
                if block:
                    env["LL_PB_BLOCK"] = block
                forms["pb_%s_g%s%s" % (phase2, chunks, "_b37" if block else "")] = (capi.SPMV_PB, acc, env, phase2 == "fixed", False)
    for label, acc in (("fixed", capi.ACCURACY_NORMWISE), ("ordered", capi.ACCURACY_COMPONENTWISE)):
        for block in (None, "37"):
            env = {"LL_TL_FORCE": "1"}
            if block:
                env["LL_PB_ROW_BLOCK"] = block
            forms["tiled_%s%s" % (label, "_b37" if block else "")] = (capi.SPMV_TILED, acc, env, label == "fixed", False)
    return forms


LATTICES = {   # name -> (dims, periodic per dimension)
    "37x64_periodic": ((37, 64), (True, True)),          # the cuts fall inside a lattice row
    "37x64_open": ((37, 64), (False, False)),
    "5x8x8_mixed": ((5, 8, 8), (True, False, True)),
    "2x8x8_periodic": ((2, 8, 8), (True, True, True)),   # two ranks: one hyperplane each, the lower and the upper neighbour are the same rank
    "4x8x8_periodic": ((4, 8, 8), (True, True, True)),   # four ranks: one hyperplane each
}


def plan(world):
    """The cases of one launch, in the order every rank runs them: (key, kind, form / lattice name, size, settings)."""
    cases = []
    sizes = ([CSR_N] if world in (2, 3) else []) + TINY
    for name, form in csr_forms().items():
        for n in sizes:
            cases.append(("csr:%s:%d" % (name, n), "csr", name, n, form[2]))
    dense = {2: [1027, 1040], 3: [1027, 1040, 3]}.get(world, [])
    for n in dense:
        for split in (True, False):
            cases.append(("dense:%s:%d" % ("split" if split else "gather", n), "dense", "split" if split else "gather", n,
                          {} if split else {"LL_CSR_SPLIT": "0"}))
    lat = {2: ["37x64_periodic", "37x64_open", "5x8x8_mixed", "2x8x8_periodic"], 3: ["37x64_periodic", "37x64_open", "5x8x8_mixed"],
           4: ["4x8x8_periodic"]}.get(world, [])
    for name in lat:
        for vec in ("1", "0"):
            cases.append(("lattice:%s:vec%s" % (name, vec), "lattice", name, LATTICES[name][0], {"LL_STENCIL_VEC": vec}))
    return cases


_INPUTS = {}


def inputs(kind, name, size, t):
    """The whole (unsharded) problem of a case in storage type t: dict with x, the reference csr and what the operator is built
    from.  Cached; the parent and every rank build the same."""
    key = (kind, name if kind == "lattice" else None, size, t)
    if key in _INPUTS:
        return _INPUTS[key]
    dtype = TYPES[t]
    if kind == "csr":
        csr, x, special = K.sharded_edge_matrix(size, dtype)
        out = {"csr": csr, "x": x, "special": special}
    elif kind == "dense":
        a, csr, x = K.dense_matrix(size, dtype)
        out = {"a": a, "csr": csr, "x": x}
    else:
        dims, periodic = LATTICES[name]
        n = int(np.prod(dims))
        rng = np.random.default_rng(n)
        onsite = rng.uniform(-1, 1, n)
        hop = [-1.0] * len(dims) if np.dtype(dtype).kind != "c" else [-1.0 + 0.5j, -0.5 - 0.25j, 0.75 + 0.0j][: len(dims)]
        # the on-site terms are kept in the real type of T (float for s / c); the kernel adds them to diag in double
        os_ref = onsite.astype(np.float32).astype(np.float64) if _single(dtype) else onsite
        csr = K.open_boundaries(K.stencil_csr(dims, hop, 0.25, os_ref, dtype), dims, periodic)
        out = {"csr": csr, "x": K.start_x(n, dtype), "dims": list(dims), "periodic": list(periodic), "hop": hop, "onsite": onsite}
    _INPUTS[key] = out
    return out


def _set_env(ctx, settings):
    """The way conftest._LLEnv does it: os.environ, then the library's switches re-read and the hooks applied to the context."""
    from util import sync_hooks

    for name in MANAGED:
        if name in settings:
            os.environ[name] = settings[name]
        else:
            os.environ.pop(name, None)
    ctx.reload_env()
    sync_hooks(ctx)


def _create(ctx, kind, name, size, t, rb, nl):
    inp = inputs(kind, name, size, t)
    if kind == "csr":
        kernel, accuracy = csr_forms()[name][:2]
        return L.CsrOperator(ctx, *K.shard_rows(inp["csr"], rb, nl), n_cols=size, row_begin=rb, accuracy=accuracy, kernel=kernel)
    if kind == "dense":
        return L.DenseOperator(ctx, inp["a"][rb:rb + nl], row_begin=rb)
    return L.StencilOperator(ctx, inp["dims"], diag=0.25, hop=inp["hop"], periodic=inp["periodic"], onsite=inp["onsite"][rb:rb + nl],
                             dtype=TYPES[t], row_begin=rb, n_local=nl)


def _applies(ctx, op, x_local, dtype):
    """y (shift, offset, n_local) and alpha (shift, offset); the guard zones of x and y are checked after every apply."""
    from test_gpu_accuracy_contracts import _guarded, _unguard

    nl = x_local.shape[0]
    ys = np.zeros((len(SHIFTS), len(OFFSETS), nl), dtype=dtype)
    alphas = np.zeros((len(SHIFTS), len(OFFSETS)))
    for si, shift in enumerate(SHIFTS):
        xb, xv = _guarded(ctx, x_local, shift)
        yb, yv = _guarded(ctx, np.zeros(nl, dtype), shift)
        for oi, offset in enumerate(OFFSETS):
            alphas[si, oi] = L.spmv(op, xv, yv, offset=offset, want_dot=True)
            ys[si, oi] = _unguard(yb, nl, shift)
            assert np.array_equal(_unguard(xb, nl, shift), x_local), "the SpMV changed its input"
        xb.free()
        yb.free()
    return ys, alphas


def main():
    from util import install_hook_sync

    rank, world, name, out_dir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    install_hook_sync()   # the harness's hook settings (util.HOOK_KEYS in os.environ) -> every context of this process
    os.environ["LL_SPMV_KEEP_BOTH"] = "1"
    ctx = L.Context(0)
    ctx.init_comm(name.encode() + b"\0" * (128 - len(name)), rank, world)
    arrays, meta = {}, {}
    t0 = time.time()
    for key, kind, form, size, settings in plan(world):
        _set_env(ctx, settings)
        n = int(np.prod(size))
        rb, nl = ctx.partition(n)
        for t, dtype in TYPES.items():
            rec = {"n_local": nl, "row_begin": rb}
            try:
                op = _create(ctx, kind, form, size, t, rb, nl)
            except capi.LanczosHipError as e:
                # a kernel asked for by name that cannot be built is refused on EVERY rank (the decision is collective)
                rec["refused"] = str(e)
                meta[key + ":" + t] = rec
                continue
            if kind == "csr":
                rec["selected"] = op.selected_spmv()
                rec["layout"] = list(op.tiled_layout())
                rec["accuracy"] = op.accuracy()
            rec["device_bytes"] = op.device_bytes()
            x_local = np.ascontiguousarray(inputs(kind, form, size, t)["x"][rb:rb + nl])
            arrays[key + ":" + t + ":y"], arrays[key + ":" + t + ":alpha"] = _applies(ctx, op, x_local, dtype)
            op.close()
            meta[key + ":" + t] = rec
    _set_env(ctx, {})
    meta["seconds"] = time.time() - t0
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), meta=np.array(json.dumps(meta)), **arrays)
    ctx.close()


if __name__ == "__main__":
    main()
