#!/usr/bin/env python3
"""Apply time of the one-triangle operator (LL_SPMV_SYM) against the best full-storage kernel on the same matrix.

For each matrix the triangle is taken from the generator's full matrix (col >= row), the full operator is created with the
creation-time timing (it keeps the fastest of CSR-stream / PB / tiled) and the triangle through ll_op_create_csr_sym_d/_z.
HIP events on the library stream, median of 5 rounds of 10 applies; creation times on the host clock; device bytes of both.
    python tools/sym_operator_bench.py [out.json]          (run under rocprofv3 --kernel-trace --stats for kernel times)"""
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


def upper(csr):
    rp, ci, va = csr
    n = rp.shape[0] - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    keep = ci >= rows
    trp = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=n), out=trp[1:])
    return trp, np.ascontiguousarray(ci[keep]), np.ascontiguousarray(va[keep])


def apply_ms(op, n, dtype):
    x = G.start_vector(n, 1, np.complex128 if np.dtype(dtype).kind == "c" else np.float64).astype(dtype)
    xd, yd = ctx.to_device(x), ctx.empty(n, dtype)
    ms = []
    for _ in range(6):
        L.spmv(op, xd, yd, want_dot=True)
        ctx.synchronize()
        ctx.timer_start()
        for _ in range(10):
            L.spmv(op, xd, yd, want_dot=True)
        ms.append(ctx.timer_stop() / 10)
    xd.free()
    yd.free()
    return sorted(ms[1:])[2]


def one(label, full):
    n = full[0].shape[0] - 1
    tri = upper(full)
    t0 = time.perf_counter()
    fop = L.CsrOperator(ctx, *full)
    t1 = time.perf_counter()
    sop = L.CsrOperator.from_triangle(ctx, *tri, uplo="U")
    t2 = time.perf_counter()
    kinds = {0: "csr_stream", 1: "pb", 2: "tiled", 3: "sym"}
    r = {"n": n, "nnz_full": int(full[0][-1]), "nnz_triangle": int(tri[0][-1]),
         "full_kernel": kinds[fop.selected_spmv()], "sym_kernel": kinds[sop.selected_spmv()],
         "create_full_s": t1 - t0, "create_sym_s": t2 - t1,
         "device_bytes_full": fop.device_bytes(), "device_bytes_sym": sop.device_bytes()}
    r["full_ms"] = apply_ms(fop, n, full[2].dtype)
    r["sym_ms"] = apply_ms(sop, n, full[2].dtype)
    r["sym_over_full"] = r["sym_ms"] / r["full_ms"]
    r["bytes_ratio"] = r["device_bytes_sym"] / r["device_bytes_full"]
    fop.close()
    sop.close()
    print(label, json.dumps(r), flush=True)
    return r


out = {}
out["laplace_1000x1000"] = one("laplace_1000x1000", G.laplace2d(1000))
out["torus_1000x1000_c128"] = one("torus_1000x1000_c128", G.torus(1000))
out["randsym_1e7_band1000"] = one("randsym_1e7_band1000", G.randsym(10_000_000, band=1000))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
