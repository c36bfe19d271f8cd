#!/usr/bin/env python3
"""Apply time of the sum-of-Pauli-strings operator on one momentum block of the FULL 2^L space of a ring
(PauliMomentumFullOperator) against (a) PauliOperator on all 2^L states (vectors about L times longer: what a user whose H does
not conserve S_z runs without it) and (b) the CSR operator of the block's own matrix; on the Heisenberg ring also against (c) the
SUM over n_down of the applies of the S_z-sector momentum operators (PauliMomentumOperator), which cover the same block.

Transverse-field Ising ring (J = 1, h = 0.7), XYZ ring (1, 0.6, 0.8) and Heisenberg ring; momentum 0 in fp64 and complex double,
momentum 1 in complex double.  The CSR operator is created from generators.pauli_momentum_full_csr(...) with the creation-time
timing (it keeps the fastest of its kernels): it and the other operators are the baselines, not the code under test.  HIP events
on the library stream; the operators ALTERNATE in one process: after a warm-up, 12 rounds of (10 applies of each in turn); median
and spread (min, max) over the rounds of each.  Creation times on the host clock (also at --create-sizes, where nothing is
applied); device bytes; the largest bucket and the trip count of the index search, RECOMPUTED here by creation's rule (keys *_recomputed: the
library has no query that reads them back from the image); the two
ends of the byte model of DESIGN.md section 3.1 as GB/s.
    python tools/pauli_momentum_full_bench.py [out.json] [--sizes 24] [--create-sizes 24,28] [--block-bits default] [--cases 0:float64,1:complex128]
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


def timed(ops):
    """ops: a list of (operator, x, y) applied one after the other — one entry, or the sectors of a direct sum"""
    ctx.timer_start()
    for _ in range(APPLIES):
        for op, xd, yd in ops:
            L.spmv(op, xd, yd, want_dot=True)
    return ctx.timer_stop() / APPLIES


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def search_shape(reps, n_sites):
    """(buckets, largest bucket, halvings of the search) by the rule of create_pauli_momentum_full"""
    dim, pb = reps.shape[0], 0
    while pb < n_sites and (2 << pb) <= dim // 8:
        pb += 1
    largest = int(np.bincount((reps >> np.uint32(n_sites - pb)).astype(np.int64), minlength=1 << pb).max())
    trips, n = 0, largest
    while n > 1:
        n -= n // 2
        trips += 1
    return 1 << pb, largest, trips


def one(label, n_sites, m, terms, dtype, block_bits, sectors):
    isz = np.dtype(dtype).itemsize
    wide = np.complex128 if np.dtype(dtype).kind == "c" else np.float64
    r = {"n_sites": n_sites, "momentum": m, "n_full": 1 << n_sites, "terms": len(terms), "dtype": np.dtype(dtype).name}
    t0 = time.perf_counter()
    mop = L.PauliMomentumFullOperator(ctx, n_sites, m, terms, dtype)
    r["create_block_s"] = time.perf_counter() - t0
    n = r["n"] = mop.n
    t0 = time.perf_counter()
    fop = L.PauliOperator(ctx, n_sites, terms, dtype)
    r["create_full_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    csr = G.pauli_momentum_full_csr(n_sites, m, terms, dtype)
    r["expand_csr_host_s"] = time.perf_counter() - t0
    r["nnz_csr"] = int(csr[0][-1])
    t0 = time.perf_counter()
    cop = L.CsrOperator(ctx, *csr)
    r["create_csr_s"] = time.perf_counter() - t0
    del csr
    r["csr_kernel"] = KINDS[cop.selected_spmv()]
    r["device_bytes_block"], r["device_bytes_csr"], r["device_bytes_full"] = mop.device_bytes(), cop.device_bytes(), fop.device_bytes()
    # RECOMPUTED here by creation's rule (the library has no query for them): not read back from the image
    r["buckets_recomputed"], r["largest_bucket_recomputed"], r["search_trips_recomputed"] = search_shape(
        G.full_momentum_basis(n_sites, m)[0], n_sites)
    xd, yd = ctx.to_device(G.start_vector_fast(n, 1, wide).astype(dtype)), ctx.empty(n, dtype)
    xf, yf = ctx.to_device(G.start_vector_fast(1 << n_sites, 1, wide).astype(dtype)), ctx.empty(1 << n_sites, dtype)
    ops = [("block", [(mop, xd, yd)]), ("csr", [(cop, xd, yd)]), ("full", [(fop, xf, yf)])]
    held = [mop, cop, fop]
    if sectors:   # the same block as the direct sum of the S_z sectors' blocks
        parts, t0 = [], time.perf_counter()
        for nd in range(n_sites + 1):
            if G.momentum_basis(n_sites, nd, m)[0].shape[0] == 0:
                continue
            parts.append(L.PauliMomentumOperator(ctx, n_sites, nd, m, terms, dtype))
        r["create_sector_blocks_s"] = time.perf_counter() - t0
        r["device_bytes_sector_blocks"] = sum(p.device_bytes() for p in parts)
        assert sum(p.n for p in parts) == n
        ops.append(("sector_blocks", [(p, ctx.to_device(G.start_vector_fast(p.n, 1, wide).astype(dtype)), ctx.empty(p.n, dtype))
                                      for p in parts]))
        held += parts
    groups = len({t[0] for t in terms if t[0]})
    for bits in block_bits:
        ctx.set_tuning("pauli_momentum_full_block_bits", None if bits == "default" else bits)
        for _, lst in ops:   # warm-up of all
            for _ in range(3):
                for op, a, b in lst:
                    L.spmv(op, a, b, want_dot=True)
        ctx.synchronize()
        ms = {name: [] for name, _ in ops}
        for _ in range(ROUNDS):
            for name, lst in ops:
                ms[name].append(timed(lst))
        e = {"block_bits": bits, "groups_flipping": groups}
        for name in ms:
            e[name] = stats(ms[name])
        for name in ms:
            if name != "block":
                e["block_over_" + name] = e["block"]["median_ms"] / e[name]["median_ms"]
        lo = (2 * isz + 5) * n                                         # x, y, representatives, periods: every gather found in cache
        hi = lo + groups * (isz + 8 + 4 * r["search_trips_recomputed"]) * n      # none found: an element, two bucket bounds, the search's loads
        e["model_bytes"] = [lo, hi]
        e["model_gbs"] = [lo / e["block"]["median_ms"] / 1e6, hi / e["block"]["median_ms"] / 1e6]
        e["partners_per_s"] = groups * n / e["block"]["median_ms"] * 1e3
        e["csr_gbs"] = ((isz + 4) * r["nnz_csr"] + (2 * isz + 4) * n) / e["csr"]["median_ms"] / 1e6
        r["block_%s" % bits] = e
    ctx.set_tuning("pauli_momentum_full_block_bits", None)
    for _, lst in ops:
        for _, a, b in lst:
            a.free()
            b.free()
    for op in held:
        op.close()
    ctx.release_cache()
    print(label, json.dumps(r), flush=True)
    return r


def models(n_sites):
    return (("tfim_ring", G.tfim_terms(n_sites, 1.0, 0.7, periodic=True), False),
            ("xyz_ring", G.xyz_terms(n_sites, 1.0, 0.6, 0.8), False),
            ("heisenberg_ring", G.heisenberg_terms(n_sites), True))


out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
sizes = [int(s) for s in arg("--sizes", "24").split(",") if s]
create_sizes = [int(s) for s in arg("--create-sizes", "24,28").split(",") if s]
block_bits = arg("--block-bits", "default").split(",")
# (momentum, dtype) pairs, e.g. --cases 0:float64,1:complex128
cases = [(int(c.split(":")[0]), np.dtype(c.split(":")[1]).type) for c in arg("--cases", "0:float64,1:complex128,0:complex128").split(",")]
out = {}


def save():
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


for n_sites in create_sizes:   # creation alone: the necklace enumeration, the bucket table, the uploads
    terms = G.tfim_terms(n_sites, 1.0, 0.7, periodic=True)
    for m, dtype in ((0, np.float64), (1, np.complex128)):
        t0 = time.perf_counter()
        op = L.PauliMomentumFullOperator(ctx, n_sites, m, terms, dtype)
        dt = time.perf_counter() - t0
        label = "create_tfim_ring_L%d_m%d_%s" % (n_sites, m, np.dtype(dtype).name)
        out[label] = {"n_sites": n_sites, "momentum": m, "n": op.n, "create_block_s": dt, "device_bytes_block": op.device_bytes(),
                      "bytes_per_state": op.device_bytes() / op.n, "table_over_all_states_bytes": 4 << n_sites}
        op.close()
        print(label, json.dumps(out[label]), flush=True)
        save()
for n_sites in sizes:
    for m, dtype in cases:
        for model, terms, sectors in models(n_sites):
            label = "%s_L%d_m%d_%s" % (model, n_sites, m, np.dtype(dtype).name)
            out[label] = one(label, n_sites, m, terms, dtype, block_bits, sectors)
            save()
