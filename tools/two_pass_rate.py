#!/usr/bin/env python3
"""Iterations per second of the two-pass eigen-solver (LambdaLanczos.run_two_pass) against the stored-basis solver
(LambdaLanczos.run) on the open transverse-field Ising chain of tests/test_gpu_pauli.py (L = 24, J = 1, h = 1.5, fp64, 128 MiB per
vector), same operator, same start vector, eigenvalue_offset = -sum |coef|, default eps, max_iteration 300.

The stored-basis solver is the baseline, not the code under test; it runs with one tracked root (num_eigs_per_iteration = 1), the
stop rule of the two-pass solver, so that both do the same number of iterations.  Host clock around whole calls (each ends in a
device synchronisation); all n-sized inputs and outputs stay in device memory.  The three calls ALTERNATE in one process: after
one warm-up of each, ROUNDS rounds of (pass 1 alone, both passes, stored basis); median and spread (min, max) over the rounds.
  pass 1            run_two_pass(want_vector=False): iterations / seconds of the call
  pass 2            (seconds of run_two_pass() - seconds of pass 1 alone) for iterations - 1 replayed steps; includes the
                    normalisation of psi and the residual's operator application
  stored basis      run(): iterations / seconds of the call (includes the Ritz GEMV over the basis)
and the n-sized device vectors each needs: workspace_vectors against iterations + 1 basis vectors.
    python tools/two_pass_rate.py [out.json] [--sites 24] [--rounds 5]"""
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
    ctx = L.Context(0)
    op = L.PauliOperator(ctx, n_sites, G.tfim_terms(n_sites, 1.0, 1.5))
    start = ctx.to_device(G.start_vector_fast(n, 1))
    out = ctx.empty(n)

    def engine():
        eng = L.LambdaLanczos(op, n, False, 1)
        eng.eigenvalue_offset = -op.inf_norm()
        eng.max_iteration = 300
        eng.num_eigs_per_iteration = 1
        eng.init_vector = start
        eng.eigenvectors_out = out
        return eng

    def timed(call):
        ctx.synchronize()
        t0 = time.perf_counter()
        r = call()
        ctx.synchronize()
        return time.perf_counter() - t0, r

    def pass1():
        eng = engine()
        dt, (val, _, info) = timed(lambda: eng.run_two_pass(want_vector=False))
        return dt, val, info["iterations"], info["stats"]["workspace_vectors"], None

    def both():
        eng = engine()
        dt, (val, _, info) = timed(eng.run_two_pass)
        return dt, val, info["iterations"], info["stats"]["workspace_vectors"], info

    def stored():
        eng = engine()
        dt, (vals, _) = timed(eng.run)
        return dt, vals[0], eng.getIterationCounts()[0], eng.getIterationCounts()[0] + 1, None

    calls = (("pass1", pass1), ("both", both), ("stored", stored))
    for _, f in calls:   # warm-up of all
        f()
    sec = {k: [] for k, _ in calls}
    last = {}
    for _ in range(rounds):
        for k, f in calls:
            r = f()
            sec[k].append(r[0])
            last[k] = r
    m1, m2, ms = last["pass1"][2], last["both"][2], last["stored"][2]
    pass2 = [b - a for a, b in zip(sec["pass1"], sec["both"])]
    res = {
        "n_sites": n_sites, "n": n, "vector_bytes": 8 * n, "rounds": rounds,
        "eigenvalue_two_pass": last["both"][1], "eigenvalue_stored": last["stored"][1],
        "iterations_two_pass": m2, "iterations_stored": ms,
        "seconds": {k: stats(v) for k, v in sec.items()}, "seconds_pass2": stats(pass2),
        "iterations_per_second": {
            "pass1": stats([m1 / t for t in sec["pass1"]]),
            "pass2": stats([(m2 - 1) / t for t in pass2]),
            "two_pass_whole_call": stats([m2 / t for t in sec["both"]]),
            "stored_basis": stats([ms / t for t in sec["stored"]]),
        },
        "device_vectors": {"two_pass_no_vector": last["pass1"][3], "two_pass_device_vector": last["both"][3],
                           "stored_basis_at_least": last["stored"][3]},
        "replay_mismatches": last["both"][4]["stats"]["replay_mismatches"], "residual": last["both"][4]["residual"],
    }
    print(json.dumps(res, indent=1), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    op.close()
    ctx.close()


if __name__ == "__main__":
    main()
