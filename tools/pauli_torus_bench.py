#!/usr/bin/env python3
"""Apply time of the sum-of-Pauli-strings operator on one translation block of an Lx x Ly torus (PauliTorusOperator) against
PauliSymmetricOperator(parity = inversion = 0) on the m = 0 block of the RING of as many sites in the same S_z sector: the same
search form and the same number of images per partner, so the difference is the cost of the two-direction rotation (the
Hamiltonians differ: the Heisenberg torus has 2 n bonds, the ring n; the time per partner is the comparable number).

Heisenberg torus (J = 1) on 6 x 4, block (0, 0) at n_down = 12, in fp64 and complex double; and the 6 x 5 block (0, 0) at
n_down = 15 (fp64) with its creation time.  HIP events on the library stream; the operators ALTERNATE in one process: after a
warm-up, 12 rounds of (10 applies of each in turn); median and spread (min, max) over the rounds of each; no counters in the timed
run.  Creation times on the host clock; device bytes; the lower end of the byte model of DESIGN.md section 3.1 (every gather found
in cache) as GB/s, and the time per partner (state and group with X != 0).
    python tools/pauli_torus_bench.py [out.json] [--skip-30]"""
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
ROUNDS, APPLIES = 12, 10


def timed(op, xd, yd):
    ctx.timer_start()
    for _ in range(APPLIES):
        L.spmv(op, xd, yd, want_dot=True)
    return ctx.timer_stop() / APPLIES


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def model(e, name, n, groups, isz):
    lo = (2 * isz + 5) * n                                   # x, y, representatives, orbit lengths: every gather found in cache
    ms = e[name]["median_ms"]
    e[name + "_model_bytes_all_cached"] = lo
    e[name + "_model_gbs_all_cached"] = lo / ms / 1e6
    e[name + "_ns_per_partner"] = ms * 1e6 / (groups * n)


def compare(lx, ly, n_down, dtype):
    n_sites = lx * ly
    isz = np.dtype(dtype).itemsize
    tterms, rterms = G.heisenberg_torus_terms(lx, ly), G.heisenberg_terms(n_sites)
    r = {"lx": lx, "ly": ly, "n_down": n_down, "dtype": np.dtype(dtype).name}
    t0 = time.perf_counter()
    top = L.PauliTorusOperator(ctx, lx, ly, 0, 0, tterms, dtype, n_down=n_down)
    r["create_torus_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    rop = L.PauliSymmetricOperator(ctx, n_sites, 0, rterms, dtype, parity=0, inversion=0, n_down=n_down)
    r["create_ring_s"] = time.perf_counter() - t0
    r["n_torus"], r["n_ring"] = top.n, rop.n
    r["device_bytes_torus"], r["device_bytes_ring"] = top.device_bytes(), rop.device_bytes()
    r["groups_torus"], r["groups_ring"] = len({t[0] for t in tterms if t[0]}), len({t[0] for t in rterms if t[0]})
    xt, yt = ctx.to_device(G.start_vector_fast(top.n, 1, dtype)), ctx.empty(top.n, dtype)
    xr, yr = ctx.to_device(G.start_vector_fast(rop.n, 1, dtype)), ctx.empty(rop.n, dtype)
    ops = [("torus", top, xt, yt), ("ring", rop, xr, yr)]
    for _, op, a, b in ops:   # warm-up of both
        for _ in range(3):
            L.spmv(op, a, b, want_dot=True)
    ctx.synchronize()
    ms = {name: [] for name, _, _, _ in ops}
    for _ in range(ROUNDS):
        for name, op, a, b in ops:
            ms[name].append(timed(op, a, b))
    for name in ms:
        r[name] = stats(ms[name])
    model(r, "torus", top.n, r["groups_torus"], isz)
    model(r, "ring", rop.n, r["groups_ring"], isz)
    r["torus_over_ring_per_partner"] = r["torus_ns_per_partner"] / r["ring_ns_per_partner"]
    for a in (xt, yt, xr, yr):
        a.free()
    top.close()
    rop.close()
    ctx.release_cache()
    return r


out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
out = {}


def save():
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


for dtype in (np.float64, np.complex128):
    label = "heisenberg_6x4_nd12_%s" % np.dtype(dtype).char
    out[label] = compare(6, 4, 12, dtype)
    print(label, json.dumps(out[label]), flush=True)
    save()
if "--skip-30" not in sys.argv:
    label = "heisenberg_6x5_nd15_d"
    out[label] = compare(6, 5, 15, np.float64)
    print(label, json.dumps(out[label]), flush=True)
    save()
