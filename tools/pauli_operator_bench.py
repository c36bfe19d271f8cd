#!/usr/bin/env python3
"""Apply time of the matrix-free sum-of-Pauli-strings operator against the CSR operator of the same matrix.

Heisenberg ring and open transverse-field Ising chain, fp64 and complex double.  The CSR operator is created from
generators.pauli_csr(...) with the creation-time timing (it keeps the fastest of CSR-stream / PB / tiled): those kernels are
the baseline, not the code under test.  HIP events on the library stream; the two operators ALTERNATE in one process: after a
warm-up, 12 rounds of (10 applies of one, 10 applies of the other); median and spread (min, max) over the rounds of each.
Creation times on the host clock; device bytes of both; the two ends of the byte model of DESIGN.md section 3 as GB/s.
    python tools/pauli_operator_bench.py [out.json] [--sizes 22,24] [--tile-bits default,13]
(run under rocprofv3 --kernel-trace --stats for kernel times)"""
import json
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


def one(label, n_sites, terms, dtype, tile_bits):
    n = 1 << n_sites
    isz = np.dtype(dtype).itemsize
    r = {"n_sites": n_sites, "n": n, "terms": len(terms), "dtype": np.dtype(dtype).name}
    t0 = time.perf_counter()
    pop = L.PauliOperator(ctx, n_sites, terms, dtype)
    r["create_pauli_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    csr = G.pauli_csr(n_sites, terms, dtype)
    r["expand_csr_host_s"] = time.perf_counter() - t0
    r["nnz_csr"] = int(csr[0][-1])
    t0 = time.perf_counter()
    cop = L.CsrOperator(ctx, *csr)
    r["create_csr_s"] = time.perf_counter() - t0
    del csr
    r["csr_kernel"] = KINDS[cop.selected_spmv()]
    r["device_bytes_pauli"], r["device_bytes_csr"] = pop.device_bytes(), cop.device_bytes()
    x = G.start_vector_fast(n, 1, np.complex128 if np.dtype(dtype).kind == "c" else np.float64).astype(dtype)
    xd, yd = ctx.to_device(x), ctx.empty(n, dtype)
    masks = sorted({t[0] for t in terms})
    for bits in tile_bits:
        ctx.set_tuning("pauli_tile_bits", None if bits == "default" else bits)
        b = min(n_sites, int(bits) if bits != "default" else int(np.log2((32 << 10) // isz)))
        g_remote = sum(1 for m in masks if m >> b)
        for op in (pop, cop):   # warm-up of both
            for _ in range(3):
                L.spmv(op, xd, yd, want_dot=True)
        ctx.synchronize()
        pm, cm = [], []
        for _ in range(ROUNDS):
            pm.append(timed(pop, xd, yd))
            cm.append(timed(cop, xd, yd))
        e = {"tile_bits": b, "groups": len(masks), "groups_remote": g_remote, "pauli": stats(pm), "csr": stats(cm)}
        e["pauli_over_csr"] = e["pauli"]["median_ms"] / e["csr"]["median_ms"]
        lo, hi = 2 * isz * n, (g_remote + 2) * isz * n
        e["model_bytes"] = [lo, hi]
        e["model_gbs"] = [lo / e["pauli"]["median_ms"] / 1e6, hi / e["pauli"]["median_ms"] / 1e6]
        e["csr_gbs"] = ((isz + 4) * r["nnz_csr"] + (2 * isz + 4) * n) / e["csr"]["median_ms"] / 1e6
        r["tile_%s" % bits] = e
    ctx.set_tuning("pauli_tile_bits", None)
    xd.free()
    yd.free()
    pop.close()
    cop.close()
    ctx.release_cache()
    print(label, json.dumps(r), flush=True)
    return r


out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
sizes = [int(s) for s in arg("--sizes", "22,24").split(",")]
tile_bits = arg("--tile-bits", "default").split(",")
out = {}
for n_sites in sizes:
    for dtype in (np.float64, np.complex128):
        for model, terms in (("heisenberg_ring", G.heisenberg_terms(n_sites)), ("tfim_open", G.tfim_terms(n_sites, 1.0, 1.5))):
            label = "%s_L%d_%s" % (model, n_sites, np.dtype(dtype).name)
            out[label] = one(label, n_sites, terms, dtype, tile_bits)
            if out_path:
                with open(out_path, "w") as f:
                    json.dump(out, f, indent=1)
