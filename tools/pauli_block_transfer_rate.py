#!/usr/bin/env python3
"""Seconds per call of ll_pauli_block_transfer (out = B_t^H P B_s c, every buffer in device memory) beside the composed path it
replaces — expand into the full space, ll_spmv of the PauliOperator of the same strings, project — on the same device in
ALTERNATING runs: momentum blocks of the full space of rings of 24 and 26 sites and momentum blocks of the sector n_down = 14 of
a ring of 28 sites, complex double, with the strings Z_0 and X_0 X_1.  Beside the seconds: the device memory of the vectors of
each path (fused: c and out, sizeof(T) (D_s + D_t); composed: c, out and two vectors of the full space), and the largest
difference of the two results.

Host clock around whole calls (each ends in a device synchronisation).  After one warm-up of each, ROUNDS rounds of (fused,
composed); median and spread (min, max) over the rounds.  There is no threshold.
    python tools/pauli_block_transfer_rate.py [out.json] [--cases 24,26,28s] [--rounds 5]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lambda_lanczos_amd as L  # noqa: E402
from lambda_lanczos_amd import generators as G  # noqa: E402

STRINGS = {"Z_0": [(0, 1, 1.0)], "X_0 X_1": [(3, 0, 1.0)]}
M_S, M_T = 0, 3


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    cases, rounds = arg("--cases", "24,26,28s").split(","), int(arg("--rounds", "5"))
    dtype = np.complex128
    ctx = L.Context(0)

    def timed(call):
        ctx.synchronize()
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        return time.perf_counter() - t0

    res = {"rounds": rounds, "m_s": M_S, "m_t": M_T, "cases": {}}
    for case in cases:
        sector = case.endswith("s")
        n_sites = int(case.rstrip("s"))
        t0 = time.perf_counter()
        if sector:
            ham = G.heisenberg_terms(n_sites, 1.0, 1.0, periodic=True)
            src = L.PauliMomentumOperator(ctx, n_sites, n_sites // 2, M_S, ham, dtype)
            tgt = L.PauliMomentumOperator(ctx, n_sites, n_sites // 2, M_T, ham, dtype)
        else:
            ham = G.tfim_terms(n_sites, 1.0, 1.5, periodic=True)
            src = L.PauliMomentumFullOperator(ctx, n_sites, M_S, ham, dtype)
            tgt = L.PauliMomentumFullOperator(ctx, n_sites, M_T, ham, dtype)
        create_s = time.perf_counter() - t0
        c = ctx.to_device(G.start_vector_fast(src.n_local, 1).astype(dtype))
        fused, composed = ctx.empty(tgt.n_local, dtype), ctx.empty(tgt.n_local, dtype)
        n = 1 << n_sites
        psi, phi = ctx.empty(n, dtype), ctx.empty(n, dtype)
        isz = np.dtype(dtype).itemsize
        for name, terms in STRINGS.items():
            full = L.PauliOperator(ctx, n_sites, terms, dtype)

            def run_composed():
                src.expand(c, full, out=psi)
                L.spmv(full, psi, phi)
                tgt.project(phi, full, out=composed)

            calls = {"fused": lambda: src.transfer(terms, c, tgt, out=fused), "composed": run_composed}
            for call in calls.values():
                timed(call)
            times = {k: [] for k in calls}
            for _ in range(rounds):
                for k, call in calls.items():
                    times[k].append(timed(call))
            a, b = fused.get(), composed.get()
            entry = {"D_s": src.n_local, "D_t": tgt.n_local, "N": n, "create_s": create_s,
                     "fused_vector_bytes": isz * (src.n_local + tgt.n_local), "composed_vector_bytes": isz * (src.n_local + tgt.n_local + 2 * n),
                     "operator_device_bytes": [src.device_bytes(), tgt.device_bytes()],
                     "max_difference": float(np.max(np.abs(a - b))), "norm": float(np.linalg.norm(a))}
            for k, v in times.items():
                entry[k] = stats(v)
            res["cases"]["%s %s" % (case, name)] = entry
            print(case, name, json.dumps(entry), flush=True)
            full.close()
        for buf in (c, fused, composed, psi, phi):
            buf.free()
        src.close()
        tgt.close()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
