#!/usr/bin/env python3
"""Apply time of the S_z-sector sum-of-Pauli-strings operator against (a) the CSR operator of the sector's matrix and (b) the
full-space matrix-free operator on the same number of sites.

Heisenberg ring and open J1-J2 chain (J2 = 0.4, Delta = 0.7), sector n_down = L / 2, fp64 and complex double.  The CSR operator
is created from generators.pauli_sector_csr(...) with the creation-time timing (it keeps the fastest of its kernels): it and
the full-space operator are the baselines, not the code under test.  HIP events on the library stream; the three operators
ALTERNATE in one process: after a warm-up, 12 rounds of (10 applies of each in turn); median and spread (min, max) over the
rounds of each.  Creation times on the host clock; device bytes; the two ends of the byte model of DESIGN.md section 3.1 as GB/s.
    python tools/pauli_sector_bench.py [out.json] [--sizes 24] [--block-bits default,12]
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


def j1j2_terms(n_sites, j1=1.0, j2=0.4, delta=0.7):
    terms = G.heisenberg_terms(n_sites, j1, delta, periodic=False)
    for j in range(n_sites - 2):
        m = (1 << j) | (1 << (j + 2))
        terms += [(m, 0, 0.25 * j2), (m, m, 0.25 * j2), (0, m, 0.25 * j2)]
    return terms


def timed(op, xd, yd):
    ctx.timer_start()
    for _ in range(APPLIES):
        L.spmv(op, xd, yd, want_dot=True)
    return ctx.timer_stop() / APPLIES


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def one(label, n_sites, n_down, terms, dtype, block_bits):
    n, nf = math.comb(n_sites, n_down), 1 << n_sites
    isz = np.dtype(dtype).itemsize
    wide = np.complex128 if np.dtype(dtype).kind == "c" else np.float64
    r = {"n_sites": n_sites, "n_down": n_down, "n": n, "n_full": nf, "terms": len(terms), "dtype": np.dtype(dtype).name}
    t0 = time.perf_counter()
    sop = L.PauliSectorOperator(ctx, n_sites, n_down, terms, dtype)
    r["create_sector_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    fop = L.PauliOperator(ctx, n_sites, terms, dtype)
    r["create_full_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    csr = G.pauli_sector_csr(n_sites, n_down, terms, dtype)
    r["expand_csr_host_s"] = time.perf_counter() - t0
    r["nnz_csr"] = int(csr[0][-1])
    t0 = time.perf_counter()
    cop = L.CsrOperator(ctx, *csr)
    r["create_csr_s"] = time.perf_counter() - t0
    del csr
    r["csr_kernel"] = KINDS[cop.selected_spmv()]
    r["device_bytes_sector"], r["device_bytes_csr"], r["device_bytes_full"] = sop.device_bytes(), cop.device_bytes(), fop.device_bytes()
    xd, yd = ctx.to_device(G.start_vector_fast(n, 1, wide).astype(dtype)), ctx.empty(n, dtype)
    xf, yf = ctx.to_device(G.start_vector_fast(nf, 1, wide).astype(dtype)), ctx.empty(nf, dtype)
    ops = (("sector", sop, xd, yd), ("csr", cop, xd, yd), ("full", fop, xf, yf))
    groups = len({t[0] for t in terms if t[0]})
    for bits in block_bits:
        ctx.set_tuning("pauli_sector_block_bits", None if bits == "default" else bits)
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
        e["sector_over_csr"] = e["sector"]["median_ms"] / e["csr"]["median_ms"]
        e["sector_over_full"] = e["sector"]["median_ms"] / e["full"]["median_ms"]
        lo, hi = (2 * isz + 4) * n, ((groups + 2) * isz + 4) * n
        e["model_bytes"] = [lo, hi]
        e["model_gbs"] = [lo / e["sector"]["median_ms"] / 1e6, hi / e["sector"]["median_ms"] / 1e6]
        e["csr_gbs"] = ((isz + 4) * r["nnz_csr"] + (2 * isz + 4) * n) / e["csr"]["median_ms"] / 1e6
        r["block_%s" % bits] = e
    ctx.set_tuning("pauli_sector_block_bits", None)
    for d in (xd, yd, xf, yf):
        d.free()
    for op in (sop, cop, fop):
        op.close()
    ctx.release_cache()
    print(label, json.dumps(r), flush=True)
    return r


out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
sizes = [int(s) for s in arg("--sizes", "24").split(",")]
block_bits = arg("--block-bits", "default").split(",")
out = {}
for n_sites in sizes:
    for dtype in (np.float64, np.complex128):
        for model, terms in (("heisenberg_ring", G.heisenberg_terms(n_sites)), ("j1j2_open", j1j2_terms(n_sites))):
            label = "%s_L%d_m%d_%s" % (model, n_sites, n_sites // 2, np.dtype(dtype).name)
            out[label] = one(label, n_sites, n_sites // 2, terms, dtype, block_bits)
            if out_path:
                with open(out_path, "w") as f:
                    json.dump(out, f, indent=1)
