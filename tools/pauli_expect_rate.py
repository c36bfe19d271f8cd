#!/usr/bin/env python3
"""Seconds for a set of expectation values by ONE PauliOperator.expectation call (ll_pauli_expect: many observables per sweep over
psi, scalars out) against the route a user had before it: one single-term PauliOperator per observable and ll_spmv_* with the fused
dot <psi, P psi> into a scratch vector.  Open chain of L = 24 spins, double (128 MiB per vector) and complex double (256 MiB); psi
stays in device memory.  Observable sets: all 276 Z_i Z_j (one group: diagonal), all 276 X_i X_j (every observable its own group),
and the 24 + 24 single-site X and Z.

The old route is the baseline, not the code under test.  Host clock around whole calls (each ends in a device synchronisation:
ll_pauli_expect returns with its values, ll_spmv_* with its dot).  The two routes ALTERNATE in one process: after one warm-up of
each, ROUNDS rounds of (old, new) per set; median and spread (min, max) over the rounds.  Beside the seconds: the sweeps, the byte
model of the sweep — between sweeps * sizeof(T) n and sum over the batches of (1 + G_remote) sizeof(T) n, G_remote = the batch's x
masks that touch a bit at or above the tile — and the bytes per second either end of the model gives the measured time; for the
old route 2 sizeof(T) n per observable (3 when the partner tile is remote).  There is no threshold.
    python tools/pauli_expect_rate.py [out.json] [--sites 24] [--rounds 5]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lambda_lanczos_amd as L  # noqa: E402
from lambda_lanczos_amd import generators as G  # noqa: E402

BATCH = 32          # accumulators per sweep (csrc/pauli_expect.hip)
TILE_BYTES = 32768  # LDS tile of the full-space kernels (csrc/ll_internal.hpp kPauliTileBytes)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def observable_sets(n_sites):
    pairs = [(1 << i) | (1 << j) for i in range(n_sites) for j in range(i + 1, n_sites)]
    return {
        "zz_pairs": [(0, m, 1.0) for m in pairs],
        "xx_pairs": [(m, 0, 1.0) for m in pairs],
        "single_x_and_z": [(1 << j, 0, 1.0) for j in range(n_sites)] + [(0, 1 << j, 1.0) for j in range(n_sites)],
    }


def remote_groups(obs, tile_bits):
    """Per batch of the plan (sorted by x mask, cut every BATCH): the distinct x masks that touch a bit at or above the tile."""
    xs = sorted(x for x, _, _ in obs)
    return [len({x for x in xs[i:i + BATCH] if x >> tile_bits}) for i in range(0, len(xs), BATCH)]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    n_sites, rounds = int(arg("--sites", "24")), int(arg("--rounds", "5"))
    n = 1 << n_sites
    ctx = L.Context(0)

    def timed(call):
        ctx.synchronize()
        t0 = time.perf_counter()
        r = call()
        ctx.synchronize()
        return time.perf_counter() - t0, r

    res = {"n_sites": n_sites, "n": n, "rounds": rounds, "batch": BATCH, "types": {}}
    for dtype in (np.float64, np.complex128):
        elem = np.dtype(dtype).itemsize
        tile_bits = min(n_sites, (TILE_BYTES // elem).bit_length() - 1)
        start = G.start_vector_fast(n, 1).astype(dtype)
        if np.dtype(dtype).kind == "c":
            start = start + 1j * np.roll(start.real, 1)
        start /= np.linalg.norm(start)
        psi, scratch = ctx.to_device(start), ctx.empty(n, dtype)
        del start
        basis_op = L.PauliOperator(ctx, n_sites, G.tfim_terms(n_sites, 1.0, 1.5), dtype)
        per_set = {}
        for name, obs in observable_sets(n_sites).items():
            singles = [L.PauliOperator(ctx, n_sites, [t], dtype) for t in obs]

            def old():
                return np.array([L.spmv(o, psi, scratch, want_dot=True) for o in singles])

            def new():
                return basis_op.expectation(psi, obs, return_sweeps=True)

            old(), new()   # warm-up of both
            sec = {"old": [], "new": []}
            for _ in range(rounds):
                dt, v_old = timed(old)
                sec["old"].append(dt)
                dt, (v_new, sweeps) = timed(new)
                sec["new"].append(dt)
            for o in singles:
                o.close()
            g_remote = remote_groups(obs, tile_bits)
            lo, hi = sweeps * elem * n, sum((1 + g) * elem * n for g in g_remote)
            t_new, t_old = float(np.median(sec["new"])), float(np.median(sec["old"]))
            old_bytes = sum((3 if x >> tile_bits else 2) * elem * n for x, _, _ in obs)
            per_set[name] = {
                "observables": len(obs), "sweeps": sweeps, "remote_groups_per_sweep": g_remote,
                "seconds": {k: stats(v) for k, v in sec.items()},
                "seconds_per_observable": {"old": t_old / len(obs), "new": t_new / len(obs)},
                "old_over_new": t_old / t_new,
                "model_bytes": {"low": lo, "high": hi, "old_route": old_bytes},
                "model_terabytes_per_second": {"low": lo / t_new / 1e12, "high": hi / t_new / 1e12, "old_route": old_bytes / t_old / 1e12},
                "largest_difference_between_the_routes": float(np.max(np.abs(v_old - v_new))),
            }
            print(np.dtype(dtype).name, name, json.dumps(per_set[name]), flush=True)
        res["types"][np.dtype(dtype).name] = {"vector_bytes": elem * n, "tile_bits": tile_bits, "sets": per_set}
        basis_op.close()
        psi.free()
        scratch.free()
    print(json.dumps(res, indent=1), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
