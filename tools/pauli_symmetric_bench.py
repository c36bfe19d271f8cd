#!/usr/bin/env python3
"""Apply time of the sum-of-Pauli-strings operator on one momentum / reflection / spin-inversion block of a ring
(PauliSymmetricOperator) against (a) PauliMomentumFullOperator on the momentum block that contains it (vectors about 2 or 4 times
longer: what a user runs without the two symmetries) and (b) the CSR operator of the block's own matrix.

Transverse-field Ising ring (J = 1, h = 0.7), XYZ ring (1, 0.6, 0.8) and Heisenberg ring (also on the sector n_down = L / 2); the
blocks (m, parity, inversion) of --cases in fp64.  The CSR operator is created from generators.pauli_symmetric_csr(...) with the
creation-time timing (it keeps the fastest of its kernels): it and the momentum operator are the baselines, not the code under
test.  HIP events on the library stream; the operators ALTERNATE in one process: after a warm-up, 12 rounds of (10 applies of
each in turn); median and spread (min, max) over the rounds of each.  Creation times on the host clock (also at --create-sizes,
where nothing is applied); device bytes; the trip count of the index search, RECOMPUTED here by creation's rule (the library has
no query that reads it back from the image); the two ends of the byte model of DESIGN.md section 3.1 as GB/s.
    python tools/pauli_symmetric_bench.py [out.json] [--sizes 24] [--create-sizes 24,28] [--block-bits default] [--cases 0:1:1,0:1:0,12:-1:-1]
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


def search_trips(reps, n_sites):
    """(buckets, largest bucket, halvings of the search) by the rule of creation"""
    dim, pb = reps.shape[0], 0
    while pb < n_sites and (2 << pb) <= dim // 8:
        pb += 1
    largest = int(np.bincount((reps >> np.uint32(n_sites - pb)).astype(np.int64), minlength=1 << pb).max())
    trips, n = 0, largest
    while n > 1:
        n -= n // 2
        trips += 1
    return 1 << pb, largest, trips


def one(label, n_sites, case, terms, n_down, block_bits):
    m, p, z = case
    dtype = np.float64
    isz = np.dtype(dtype).itemsize
    r = {"n_sites": n_sites, "momentum": m, "parity": p, "inversion": z, "n_down": n_down, "terms": len(terms)}
    t0 = time.perf_counter()
    sop = L.PauliSymmetricOperator(ctx, n_sites, m, terms, dtype, parity=p, inversion=z, n_down=n_down)
    r["create_block_s"] = time.perf_counter() - t0
    n = r["n"] = sop.n
    t0 = time.perf_counter()
    mop = L.PauliMomentumFullOperator(ctx, n_sites, m, terms, dtype)
    r["create_momentum_s"] = time.perf_counter() - t0
    r["n_momentum"] = mop.n
    t0 = time.perf_counter()
    csr = G.pauli_symmetric_csr(n_sites, m, p, z, terms, dtype, n_down=n_down)
    r["expand_csr_host_s"] = time.perf_counter() - t0
    r["nnz_csr"] = int(csr[0][-1])
    t0 = time.perf_counter()
    cop = L.CsrOperator(ctx, *csr)
    r["create_csr_s"] = time.perf_counter() - t0
    del csr
    r["csr_kernel"] = KINDS[cop.selected_spmv()]
    r["device_bytes_block"], r["device_bytes_csr"], r["device_bytes_momentum"] = sop.device_bytes(), cop.device_bytes(), mop.device_bytes()
    r["buckets_recomputed"], r["largest_bucket_recomputed"], r["search_trips_recomputed"] = search_trips(
        G.symmetric_basis(n_sites, m, p, z, n_down)[0], n_sites)
    xd, yd = ctx.to_device(G.start_vector_fast(n, 1, dtype)), ctx.empty(n, dtype)
    xm, ym = ctx.to_device(G.start_vector_fast(mop.n, 1, dtype)), ctx.empty(mop.n, dtype)
    ops = [("block", sop, xd, yd), ("csr", cop, xd, yd), ("momentum", mop, xm, ym)]
    groups = len({t[0] for t in terms if t[0]})
    for bits in block_bits:
        ctx.set_tuning("pauli_symmetric_block_bits", None if bits == "default" else bits)
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
        for name in ms:
            if name != "block":
                e["block_over_" + name] = e["block"]["median_ms"] / e[name]["median_ms"]
        lo = (2 * isz + 5) * n                                          # x, y, representatives, orbit lengths: every gather in cache
        hi = lo + groups * (isz + 12 + 4 * r["search_trips_recomputed"]) * n      # none found: element, bucket bounds, the search, the compare
        e["model_bytes"] = [lo, hi]
        e["model_gbs"] = [lo / e["block"]["median_ms"] / 1e6, hi / e["block"]["median_ms"] / 1e6]
        e["partners_per_s"] = groups * n / e["block"]["median_ms"] * 1e3
        e["csr_gbs"] = ((isz + 4) * r["nnz_csr"] + (2 * isz + 4) * n) / e["csr"]["median_ms"] / 1e6
        r["block_%s" % bits] = e
    ctx.set_tuning("pauli_symmetric_block_bits", None)
    for a in (xd, yd, xm, ym):
        a.free()
    for op in (sop, cop, mop):
        op.close()
    ctx.release_cache()
    print(label, json.dumps(r), flush=True)
    return r


def models(n_sites):
    return (("tfim_ring", G.tfim_terms(n_sites, 1.0, 0.7, periodic=True), None),
            ("xyz_ring", G.xyz_terms(n_sites, 1.0, 0.6, 0.8), None),
            ("heisenberg_ring", G.heisenberg_terms(n_sites), None),
            ("heisenberg_ring_half", G.heisenberg_terms(n_sites), n_sites // 2))


out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
sizes = [int(s) for s in arg("--sizes", "24").split(",") if s]
create_sizes = [int(s) for s in arg("--create-sizes", "24,28").split(",") if s]
block_bits = arg("--block-bits", "default").split(",")
# (momentum, parity, inversion) triples, e.g. --cases 0:1:1,12:-1:-1
cases = [tuple(int(v) for v in c.split(":")) for c in arg("--cases", "0:1:1,0:1:0,0:0:1").split(",")]
out = {}


def save():
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


for n_sites in create_sizes:   # creation alone: the necklace enumeration with the O(L) walk per necklace, the buckets, the uploads
    terms = G.tfim_terms(n_sites, 1.0, 0.7, periodic=True)
    for p, z in ((1, 1), (0, 1), (1, 0)):
        t0 = time.perf_counter()
        op = L.PauliSymmetricOperator(ctx, n_sites, 0, terms, np.float64, parity=p, inversion=z)
        dt = time.perf_counter() - t0
        label = "create_tfim_ring_L%d_m0_p%d_z%d" % (n_sites, p, z)
        out[label] = {"n_sites": n_sites, "parity": p, "inversion": z, "n": op.n, "create_block_s": dt,
                      "device_bytes_block": op.device_bytes(), "bytes_per_state": op.device_bytes() / op.n}
        op.close()
        print(label, json.dumps(out[label]), flush=True)
        save()
for n_sites in sizes:
    for case in cases:
        for model, terms, n_down in models(n_sites):
            if n_down is not None and case[2] and 2 * n_down != n_sites:
                continue
            label = "%s_L%d_m%d_p%d_z%d" % ((model, n_sites) + case)
            out[label] = one(label, n_sites, case, terms, n_down, block_bits)
            save()
