#!/usr/bin/env python3
"""Seconds for the reduced density matrix of m sites by ONE PauliOperator.reduced_density_matrix call (ll_pauli_rdm: one sweep over
psi, 4^m numbers out) against the route a user had before it: tomography through PauliOperator.expectation (ll_pauli_expect) with
all 4^m Pauli strings on the sites, ceil(4^m / 32) sweeps (fewer where strings are identically zero on a real type), and
rho = 2^-m sum_P <P> P on the host.  Full space of L = 26 spins, double (512 MiB) and complex double (1 GiB); psi stays in device
memory.  m = 1, 2, 4, 6 with the sites low (0 .. m - 1), high (L - m .. L - 1) and scattered.

The tomography route is the baseline, not the code under test.  Host clock around whole calls (each returns with its values, after
a device synchronisation).  The two routes ALTERNATE in one process: after one warm-up of each, ROUNDS rounds of (tomography,
direct) per case; median and spread (min, max) over the rounds.  Beside the seconds: the bytes the direct kernel reads,
sizeof(T) n, per second of its median time against the read ceiling that ll_bandwidth_probe reports in the same process, the
flops of the rank-k update (8 per complex product, 2 per real one, over the upper triangle in blocks), and the largest difference
between the two matrices.  There is no threshold.
    python tools/pauli_rdm_rate.py [out.json] [--sites 26] [--rounds 5]"""
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lambda_lanczos_amd as L  # noqa: E402
from lambda_lanczos_amd import generators as G  # noqa: E402

PAULI = {"I": np.eye(2, dtype=np.complex128), "X": np.array([[0, 1], [1, 0]], np.complex128),
         "Y": np.array([[0, -1j], [1j, 0]], np.complex128), "Z": np.array([[1, 0], [0, -1]], np.complex128)}
BLOCK_EDGE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 4, 6: 4}   # csrc/pauli_rdm_plan.hpp pauli_rdm_block_edge


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def site_lists(n_sites, m):
    step = (n_sites - 1) // max(m - 1, 1)
    return {"low": list(range(m)), "high": list(range(n_sites - m, n_sites)),
            "scattered": [n_sites // 2] if m == 1 else [k * step for k in range(m)]}


def strings_on(sites):
    """All 4^m strings on the sites with the matrix of each (bit k of a is sites[k])."""
    out = []
    for letters in itertools.product("IXYZ", repeat=len(sites)):
        x = sum(1 << s for s, c in zip(sites, letters) if c in "XY")
        z = sum(1 << s for s, c in zip(sites, letters) if c in "YZ")
        mat = np.eye(1, dtype=np.complex128)
        for c in reversed(letters):
            mat = np.kron(mat, PAULI[c])
        out.append(((x, z, 1.0), mat))
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    n_sites, rounds = int(arg("--sites", "26")), int(arg("--rounds", "5"))
    n = 1 << n_sites
    ctx = L.Context(0)
    read_gbs, copy_gbs = ctx.bandwidth_probe()

    res = {"n_sites": n_sites, "n": n, "rounds": rounds, "read_ceiling_gigabytes_per_second": read_gbs,
           "copy_gigabytes_per_second": copy_gbs, "types": {}}
    for dtype in (np.float64, np.complex128):
        elem = np.dtype(dtype).itemsize
        cplx = np.dtype(dtype).kind == "c"
        start = G.start_vector_fast(n, 1).astype(dtype)
        if cplx:
            start = start + 1j * np.roll(start.real, 1)
        start /= np.linalg.norm(start)
        psi = ctx.to_device(start)
        del start
        op = L.PauliOperator(ctx, n_sites, G.tfim_terms(n_sites, 1.0, 1.5), dtype)
        cases = {}
        for m in (1, 2, 4, 6):
            edge = BLOCK_EDGE[m]
            nb = (1 << m) // edge
            products = nb * (nb + 1) // 2 * edge * edge          # per row, upper triangle in blocks
            flops = (8 if cplx else 2) * products * (n >> m)
            for where, sites in site_lists(n_sites, m).items():
                strings = strings_on(sites)
                obs = [t for t, _ in strings]

                def tomography():
                    vals, sweeps = op.expectation(psi, obs, return_sweeps=True)
                    return sum(v * mat for v, (_, mat) in zip(vals, strings)) / (1 << m), sweeps

                def direct():
                    return op.reduced_density_matrix(psi, sites, return_sweeps=True)

                tomography(), direct()   # warm-up of both
                sec = {"tomography": [], "direct": []}
                for _ in range(rounds):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    rho_t, sweeps_t = tomography()
                    sec["tomography"].append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    rho_d, sweeps_d = direct()
                    sec["direct"].append(time.perf_counter() - t0)
                t_d, t_t = float(np.median(sec["direct"])), float(np.median(sec["tomography"]))
                cases["m%d_%s" % (m, where)] = {
                    "m": m, "sites": sites, "sweeps": {"tomography": sweeps_t, "direct": sweeps_d},
                    "seconds": {k: stats(v) for k, v in sec.items()},
                    "tomography_over_direct": t_t / t_d,
                    "direct_bytes": elem * n, "direct_gigabytes_per_second": elem * n / t_d / 1e9,
                    "direct_fraction_of_read_ceiling": elem * n / t_d / 1e9 / read_gbs,
                    "direct_flops": flops, "direct_teraflops_per_second": flops / t_d / 1e12,
                    "largest_difference_between_the_routes": float(np.max(np.abs(rho_t - rho_d))),
                }
                print(np.dtype(dtype).name, "m%d_%s" % (m, where), json.dumps(cases["m%d_%s" % (m, where)]), flush=True)
        res["types"][np.dtype(dtype).name] = {"vector_bytes": elem * n, "cases": cases}
        op.close()
        psi.free()
    print(json.dumps(res, indent=1), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
