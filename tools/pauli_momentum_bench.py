#!/usr/bin/env python3
"""Apply time of the momentum-block sum-of-Pauli-strings operator against (a) the S_z-sector operator on the same number of
sites and flipped spins (vectors n_sites times longer: the operator a user without momentum sectors runs) and (b) the CSR
operator of the block's own matrix.

Heisenberg ring and XXZ (Delta = 0.8) + Dzyaloshinskii-Moriya (D = 0.35) ring, sector n_down = L / 2; momentum 0 in fp64 (the
Heisenberg ring only: the other H is complex) and complex double, momentum 1 in complex double.  The CSR operator is created
from generators.pauli_momentum_csr(...) with the creation-time timing (it keeps the fastest of its kernels): it and the sector
operator are the baselines, not the code under test.  HIP events on the library stream; the three operators ALTERNATE in one
process: after a warm-up, 12 rounds of (10 applies of each in turn); median and spread (min, max) over the rounds of each.
Creation times on the host clock; device bytes; the two ends of the byte model of DESIGN.md section 3.1 as GB/s.
    python tools/pauli_momentum_bench.py [out.json] [--sizes 24] [--block-bits default]
(run under rocprofv3 --kernel-trace --stats for kernel times)"""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lambda_lanczos_amd as L  # noqa: E402
from lambda_lanczos_amd import generators as G  # noqa: E402

ctx = L.Context(0)
KINDS = {0: "csr_stream", 1: "pb", 2: "tiled", 3: "sym"}
ROUNDS, APPLIES = 12, 10


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def timed(op, xd, yd):
    ctx.timer_start()
    for _ in range(APPLIES):
        L.spmv(op, xd, yd, want_dot=True)
    return ctx.timer_stop() / APPLIES


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def one(label, n_sites, n_down, m, terms, dtype, block_bits):
    D = math.comb(n_sites, n_down)
    isz = np.dtype(dtype).itemsize
    wide = np.complex128 if np.dtype(dtype).kind == "c" else np.float64
    r = {"n_sites": n_sites, "n_down": n_down, "momentum": m, "n_sector": D, "terms": len(terms), "dtype": np.dtype(dtype).name}
    t0 = time.perf_counter()
    mop = L.PauliMomentumOperator(ctx, n_sites, n_down, m, terms, dtype)
    r["create_momentum_s"] = time.perf_counter() - t0
    n = r["n"] = mop.n
    t0 = time.perf_counter()
    sop = L.PauliSectorOperator(ctx, n_sites, n_down, terms, dtype)
    r["create_sector_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    csr = G.pauli_momentum_csr(n_sites, n_down, m, terms, dtype)
    r["expand_csr_host_s"] = time.perf_counter() - t0
    r["nnz_csr"] = int(csr[0][-1])
    t0 = time.perf_counter()
    cop = L.CsrOperator(ctx, *csr)
    r["create_csr_s"] = time.perf_counter() - t0
    del csr
    r["csr_kernel"] = KINDS[cop.selected_spmv()]
    r["device_bytes_momentum"], r["device_bytes_csr"], r["device_bytes_sector"] = mop.device_bytes(), cop.device_bytes(), sop.device_bytes()
    xd, yd = ctx.to_device(G.start_vector_fast(n, 1, wide).astype(dtype)), ctx.empty(n, dtype)
    xs, ys = ctx.to_device(G.start_vector_fast(D, 1, wide).astype(dtype)), ctx.empty(D, dtype)
    ops = (("momentum", mop, xd, yd), ("csr", cop, xd, yd), ("sector", sop, xs, ys))
    groups = len({t[0] for t in terms if t[0]})
    for bits in block_bits:
        ctx.set_tuning("pauli_momentum_block_bits", None if bits == "default" else bits)
        for _, op, a, b in ops:   # warm-up of all
            for _ in range(3):
                L.spmv(op, a, b, want_dot=True)
        ctx.synchronize()
        ms = {name: [] for name, _, _, _ in ops}
        for _ in range(ROUNDS):
            for name, op, a, b in ops:
                ms[name].append(timed(op, a, b))
        e = {"block_bits": bits, "groups_flipping": groups}
        for name in ms:
            e[name] = stats(ms[name])
        e["momentum_over_sector"] = e["momentum"]["median_ms"] / e["sector"]["median_ms"]
        e["momentum_over_csr"] = e["momentum"]["median_ms"] / e["csr"]["median_ms"]
        lo = (2 * isz + 5) * n                       # x, y, representatives, periods: every gather found in cache
        hi = lo + groups * (isz + 4) * n             # no gather found in cache: one orbit entry and one element per group
        e["model_bytes"] = [lo, hi]
        e["model_gbs"] = [lo / e["momentum"]["median_ms"] / 1e6, hi / e["momentum"]["median_ms"] / 1e6]
        e["csr_gbs"] = ((isz + 4) * r["nnz_csr"] + (2 * isz + 4) * n) / e["csr"]["median_ms"] / 1e6
        r["block_%s" % bits] = e
    ctx.set_tuning("pauli_momentum_block_bits", None)
    for d in (xd, yd, xs, ys):
        d.free()
    for op in (mop, cop, sop):
        op.close()
    ctx.release_cache()
    print(label, json.dumps(r), flush=True)
    return r


out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
sizes = [int(s) for s in arg("--sizes", "24").split(",")]
block_bits = arg("--block-bits", "default").split(",")
out = {}
for n_sites in sizes:
    models = (("heisenberg_ring", G.heisenberg_terms(n_sites), True),
              ("xxz_dm_ring", G.heisenberg_terms(n_sites, 1.0, 0.8) + G.dm_terms(n_sites, 0.35), False))
    for model, terms, real_h in models:
        for m, dtype in ((0, np.float64), (0, np.complex128), (1, np.complex128)):
            if np.dtype(dtype).kind != "c" and not real_h:
                continue   # the Dzyaloshinskii-Moriya terms carry one Y each: complex types only
            label = "%s_L%d_n%d_m%d_%s" % (model, n_sites, n_sites // 2, m, np.dtype(dtype).name)
            out[label] = one(label, n_sites, n_sites // 2, m, terms, dtype, block_bits)
            if out_path:
                with open(out_path, "w") as f:
                    json.dump(out, f, indent=1)
