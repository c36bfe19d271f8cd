#!/usr/bin/env python3
"""Seconds per call of ll_pauli_block_expand (Psi = B c) and ll_pauli_block_project (c = B^H Psi) with every buffer in device
memory, on the (m = 0, p = +1, z = +1) blocks of the full space and the momentum-full block m = 1 of rings of 24 and 26 sites,
in double and complex double, against the byte model of DESIGN.md 3.7:
    expand   writes sizeof(T) N, reads c through a cached gather;      project   reads sizeof(T) N gathered, writes sizeof(T) D,
so the figure beside the seconds is sizeof(T) N / seconds, a LOWER bound of the traffic.  Beside them: ll_scal on N elements (a
kernel that reads and writes the vector once: the streaming rate an expand can be held against) and, on rings of at most 22 sites
(--sites), the route a user had before: the host's numpy product through generators.symmetric_embedding.

Host clock around whole calls (each ends in a device synchronisation).  scal, expand and project ALTERNATE in one process:
after one warm-up of each, ROUNDS rounds of (scal, expand, project); median and spread (min, max) over the rounds.  There is no
threshold.
    python tools/pauli_block_embed_rate.py [out.json] [--sites 24,26] [--rounds 5]"""
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
    sites, rounds = [int(s) for s in arg("--sites", "24,26").split(",")], int(arg("--rounds", "5"))
    ctx = L.Context(0)

    def timed(call):
        ctx.synchronize()
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        return time.perf_counter() - t0

    res = {"rounds": rounds, "rings": {}}
    for n_sites in sites:
        terms = G.tfim_terms(n_sites, 1.0, 1.5, periodic=True)
        for tid, dtype in (("d", np.float64), ("z", np.complex128)):
            blocks = {"symmetric_0_+_+": lambda: L.PauliSymmetricOperator(ctx, n_sites, 0, terms, dtype, parity=1, inversion=1)}
            if tid == "z":
                blocks["momentum_full_1"] = lambda: L.PauliMomentumFullOperator(ctx, n_sites, 1, terms, dtype)
            target = L.PauliOperator(ctx, n_sites, [(0, 3, 1.0)], dtype)
            n = target.n_local
            psi, other = ctx.empty(n, dtype), ctx.empty(n, dtype)
            nbytes = n * np.dtype(dtype).itemsize
            for name, make in blocks.items():
                t0 = time.perf_counter()
                block = make()
                create_s = time.perf_counter() - t0
                dim = block.n_local
                c = ctx.to_device(G.start_vector_fast(dim, 1).astype(dtype))
                back = ctx.empty(dim, dtype)
                block.expand(c, target, out=other)      # finite numbers for the streaming kernel
                calls = {"scal": lambda: L.scal(ctx, 0.5, other, n),
                         "expand": lambda: block.expand(c, target, out=psi),
                         "project": lambda: block.project(psi, target, out=back)}
                for call in calls.values():
                    timed(call)
                times = {k: [] for k in calls}
                for _ in range(rounds):
                    for k, call in calls.items():
                        times[k].append(timed(call))
                err = float(np.max(np.abs(back.get() - c.get())))
                entry = {"D": dim, "N": n, "vector_bytes": nbytes, "create_s": create_s, "round_trip_max_error": err}
                for k, v in times.items():
                    entry[k] = dict(stats(v), bytes_per_s_lower_bound=nbytes / float(np.median(v)))
                if n_sites <= 22 and name.startswith("symmetric"):
                    col, val = G.symmetric_embedding(n_sites, 0, 1, 1, None, dense=False)
                    ch = c.get()
                    t0 = time.perf_counter()
                    _ = np.where(col >= 0, val * ch[np.maximum(col, 0)], 0.0).astype(dtype)
                    entry["host_numpy_product_s"] = time.perf_counter() - t0      # (without forming the embedding itself)
                res["rings"]["%d-%s-%s" % (n_sites, tid, name)] = entry
                print(n_sites, tid, name, json.dumps(entry))
                c.free()
                back.free()
                block.close()
            psi.free()
            other.free()
            target.close()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
