#!/usr/bin/env python3
"""Iterations per second of the two-pass Exponentiator (Exponentiator.run_two_pass) against the stored-basis one
(Exponentiator.run) on the open transverse-field Ising chain of tools/two_pass_rate.py (L = 24, J = 1, h = 1.5) in complex double
(256 MiB per vector), a = -0.05i, default eps, same operator, same input.

The stored-basis run is the baseline, not the code under test.  Host clock around whole calls (each ends in a device
synchronisation); input and output stay in device memory.  The two calls ALTERNATE in one process: after one warm-up of each,
ROUNDS rounds of (stored basis, two-pass); median and spread (min, max) over the rounds.
  stored basis      run(): iterations / seconds of the call (includes the GEMV over the basis)
  two-pass          run_two_pass(): iterations / seconds of the call, i.e. of BOTH passes — 2 m - 1 operator applications for
                    m iterations; "operator applications per second" counts those
and the n-sized device vectors each needs beside the caller's two: workspace_vectors against iterations + 1.  There is no
threshold: the number answers whether the two-pass form runs at about the stored-basis rate, as the eigen-solver's does.
    python tools/expo_two_pass_rate.py [out.json] [--sites 24] [--rounds 5]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lambda_lanczos_amd as L  # noqa: E402
from lambda_lanczos_amd import generators as G  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    n_sites, rounds = int(arg("--sites", "24")), int(arg("--rounds", "5"))
    n = 1 << n_sites
    a = -0.05j
    ctx = L.Context(0)
    op = L.PauliOperator(ctx, n_sites, G.tfim_terms(n_sites, 1.0, 1.5), np.complex128)
    start = G.start_vector_fast(n, 1).astype(np.complex128)
    start /= np.linalg.norm(start)
    psi = ctx.to_device(start)
    out = {"stored": ctx.empty(n, np.complex128), "two_pass": ctx.empty(n, np.complex128)}
    ex = L.Exponentiator(op, n)

    def timed(call):
        ctx.synchronize()
        t0 = time.perf_counter()
        r = call()
        ctx.synchronize()
        return time.perf_counter() - t0, r

    def stored():
        dt, (_, it) = timed(lambda: ex.run(a, psi, out=out["stored"]))
        return dt, int(it), int(it) + 1, None

    def two_pass():
        dt, (_, it) = timed(lambda: ex.run_two_pass(a, psi, out=out["two_pass"]))
        return dt, int(it), ex.last_stats["workspace_vectors"], dict(ex.last_stats)

    calls = (("stored", stored), ("two_pass", two_pass))
    for _, f in calls:   # warm-up of both
        f()
    sec = {k: [] for k, _ in calls}
    last = {}
    for _ in range(rounds):
        for k, f in calls:
            r = f()
            sec[k].append(r[0])
            last[k] = r
    ms, m2 = last["stored"][1], last["two_pass"][1]
    # the two results, compared in slices (a whole vector is 256 MiB on the host)
    diff = 0.0
    piece = 1 << 20
    o_s, o_t = out["stored"].get(), out["two_pass"].get()
    for i in range(0, n, piece):
        diff = max(diff, float(np.max(np.abs(o_s[i:i + piece] - o_t[i:i + piece]))))
    res = {
        "n_sites": n_sites, "n": n, "vector_bytes": 16 * n, "rounds": rounds, "a": [a.real, a.imag],
        "iterations_two_pass": m2, "iterations_stored": ms,
        "max_abs_difference_of_the_outputs": diff,
        "seconds": {k: stats(v) for k, v in sec.items()},
        "iterations_per_second": {
            "stored_basis": stats([ms / t for t in sec["stored"]]),
            "two_pass_whole_call": stats([m2 / t for t in sec["two_pass"]]),
        },
        "operator_applications_per_second": {
            "stored_basis": stats([ms / t for t in sec["stored"]]),
            "two_pass": stats([(2 * m2 - 1) / t for t in sec["two_pass"]]),
        },
        "device_vectors": {"two_pass": last["two_pass"][2], "stored_basis_at_least": last["stored"][2]},
        "replay_mismatches": last["two_pass"][3]["replay_mismatches"],
    }
    print(json.dumps(res, indent=1), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    for v in (psi, out["stored"], out["two_pass"]):
        v.free()
    op.close()
    ctx.close()


if __name__ == "__main__":
    main()
