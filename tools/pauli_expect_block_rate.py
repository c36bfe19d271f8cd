#!/usr/bin/env python3
"""Seconds per sweep of PauliSymmetricOperator.expectation (ll_pauli_expect_block: observables measured on the coefficients of a
symmetry block, up to 32 per sweep, scalars out) on the (m = 0, p = +1, z = +1) blocks of rings of 24 and 28 sites, double, for two
observable sets — the diagonal <Z_0 Z_r> and the off-diagonal <X_0 X_r>, r = 1 .. L/2 (one sweep each) — against the only route a
user had before it: per observable, create a PauliSymmetricOperator from the symmetrised strings
(generators.symmetrised_strings), apply it with the fused dot <c, Pbar c> into a scratch vector, close it.

The old route is the baseline, not the code under test; it is timed with the creation (what a user pays per observable) and the
applies alone.  Host clock around whole calls (each ends in a device synchronisation).  The two routes ALTERNATE in one process:
after one warm-up of each, ROUNDS rounds of (old, new) per set; median and spread (min, max) over the rounds.  Beside the seconds:
the sweeps, the gathers the sweep makes (states x groups with X != 0, summed over the slots), seconds per gather, and the largest
difference between the routes.  There is no threshold.
    python tools/pauli_expect_block_rate.py [out.json] [--sites 24,28] [--rounds 5]"""
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


def observable_sets(n_sites):
    pairs = [1 | (1 << r) for r in range(1, n_sites // 2 + 1)]
    return {"z0_zr": [(0, m, 1.0) for m in pairs], "x0_xr": [(m, 0, 1.0) for m in pairs]}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    sites, rounds = [int(s) for s in arg("--sites", "24,28").split(",")], int(arg("--rounds", "5"))
    dtype, m, parity, inversion = np.float64, 0, 1, 1
    ctx = L.Context(0)

    def timed(call):
        ctx.synchronize()
        t0 = time.perf_counter()
        r = call()
        ctx.synchronize()
        return time.perf_counter() - t0, r

    res = {"dtype": np.dtype(dtype).name, "block": {"momentum": m, "parity": parity, "inversion": inversion}, "rounds": rounds, "rings": {}}
    for n_sites in sites:
        t0 = time.perf_counter()
        basis_op = L.PauliSymmetricOperator(ctx, n_sites, m, G.tfim_terms(n_sites, 1.0, 1.5, periodic=True), dtype, parity=parity,
                                            inversion=inversion)
        create_s = time.perf_counter() - t0
        n = basis_op.n_local
        start = G.start_vector_fast(n, 1).astype(dtype)
        start /= np.linalg.norm(start)
        c, scratch = ctx.to_device(start), ctx.empty(n, dtype)
        del start
        per_set = {}
        for name, obs in observable_sets(n_sites).items():
            sym = [[(x, z, w * t[2]) for x, z, w in G.symmetrised_strings(n_sites, t, parity, inversion)] for t in obs]
            apply_s = []

            def old():
                out, inner = [], 0.0
                for terms in sym:
                    o = L.PauliSymmetricOperator(ctx, n_sites, m, terms, dtype, parity=parity, inversion=inversion)
                    ctx.synchronize()
                    t1 = time.perf_counter()
                    out.append(L.spmv(o, c, scratch, want_dot=True))
                    ctx.synchronize()
                    inner += time.perf_counter() - t1
                    o.close()
                apply_s.append(inner)
                return np.array(out)

            def new():
                return basis_op.expectation(c, obs, return_sweeps=True)

            old(), new()   # warm-up of both
            apply_s.clear()
            sec = {"old": [], "new": []}
            for _ in range(rounds):
                dt, v_old = timed(old)
                sec["old"].append(dt)
                dt, (v_new, sweeps) = timed(new)
                sec["new"].append(dt)
            sec["old_applies_alone"] = list(apply_s)
            gathers = n * sum(sum(1 for x in {x for x, _, _ in terms} if x) for terms in sym)
            strings = sum(len(terms) for terms in sym)
            t_new, t_old, t_app = (float(np.median(sec[k])) for k in ("new", "old", "old_applies_alone"))
            per_set[name] = {
                "observables": len(obs), "sweeps": sweeps, "symmetrised_strings": strings, "gathers": gathers,
                "seconds": {k: stats(v) for k, v in sec.items()},
                "seconds_per_sweep": t_new / max(sweeps, 1),
                "nanoseconds_per_gather": (t_new / gathers * 1e9) if gathers else None,
                "nanoseconds_per_state_and_string": t_new / (n * strings) * 1e9,
                "old_over_new": t_old / t_new, "old_applies_alone_over_new": t_app / t_new,
                "largest_difference_between_the_routes": float(np.max(np.abs(v_old - v_new))),
            }
            print(n_sites, name, json.dumps(per_set[name]), flush=True)
        res["rings"][str(n_sites)] = {"n_local": n, "vector_bytes": n * np.dtype(dtype).itemsize, "create_block_s": create_s,
                                      "device_bytes": basis_op.device_bytes(), "sets": per_set}
        basis_op.close()
        c.free()
        scratch.free()
    print(json.dumps(res, indent=1), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
