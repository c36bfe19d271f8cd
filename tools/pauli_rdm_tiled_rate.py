#!/usr/bin/env python3
"""Seconds for the reduced density matrix of m = 8, 10, 12 sites by ONE PauliOperator.reduced_density_matrix_tiled call
(ll_pauli_rdm_tiled: the rank-K update rho = F F^H on the f64 matrix cores, out in device memory) against the only other route
on the device: a torch gather of the fibres, F = psi.view((2,) * n).permute(...).reshape(2^m, -1) — with neighbouring sites merged
into one dimension, torch permutes at most 16 — made contiguous, a second copy of psi, and F @ F.conj().T through the BLAS
library, which computes the full square.  Full space of 24 and 26 spins, double and complex double, the sites low (0 .. m - 1),
high (n - m .. n - 1) and scattered (pairs of neighbours spread over the chain); psi stays in device memory.

The torch route is the yardstick, not the code under test.  Host clock around whole calls, each ending in a device synchronisation.
The two routes ALTERNATE in one process: after one warm-up of each, ROUNDS rounds of (torch, tiled) per case; median and spread
(min, max) over the rounds.  Beside the seconds: Tflop/s as the kernel forms the update (2 flops per real product, 8 per complex
one, over the quadrants of the macro-tiles of the upper triangle that it multiplies), the bytes of psi over the time against the
read ceiling that ll_bandwidth_probe reports in the same process, the ratio to the torch route and the largest difference between
the two matrices.  Also: m = 6 by the new kernel beside the one-sweep kernel of ll_pauli_rdm.  There is no threshold.
    python tools/pauli_rdm_tiled_rate.py [out.json] [--sites 24,26] [--m 8,10,12] [--rounds 5]"""
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lambda_lanczos_amd as L  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def site_lists(n_sites, m):
    """Ascending; scattered: m / 2 pairs of neighbours spread over the chain (torch permutes at most 16 dimensions: see gather_plan)."""
    step = (n_sites - 2) // (m // 2 - 1)
    return {"low": list(range(m)), "high": list(range(n_sites - m, n_sites)),
            "scattered": [j * step + k for j in range(m // 2) for k in (0, 1)]}


def gather_plan(n_sites, sites):
    """(shape, perm) with psi.view(shape).permute(perm).reshape(2^m, -1) = F for ASCENDING sites: the view of (2,) * n_sites with
    every run of neighbouring sites that are all inside or all outside the subsystem merged into one dimension (the most
    significant site first), the subsystem's runs moved to the front."""
    assert sites == sorted(sites)
    runs = []   # (inside, number of sites), from site n_sites - 1 down
    for s in range(n_sites - 1, -1, -1):
        inside = s in sites
        if runs and runs[-1][0] == inside:
            runs[-1][1] += 1
        else:
            runs.append([inside, 1])
    shape = [1 << r[1] for r in runs]
    perm = [d for d, r in enumerate(runs) if r[0]] + [d for d, r in enumerate(runs) if not r[0]]
    assert len(shape) <= 16
    return shape, perm


def kernel_flops(n_sites, m, cplx):
    """What pauli_rdm_tiled_kernel multiplies: per macro-tile of the upper triangle four quadrants of 32 x 32, three on the diagonal."""
    nb = 1 << max(0, m - 6)
    quadrants = 4 * (nb * (nb + 1) // 2) - nb
    return (8 if cplx else 2) * quadrants * 32 * 32 * (1 << (n_sites - m))


def device_view(t, np_dtype):
    return types.SimpleNamespace(ptr=t.data_ptr(), dtype=np.dtype(np_dtype), shape=(t.numel(),))


def main():
    import torch

    out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    sizes = [int(s) for s in arg("--sites", "24,26").split(",")]
    rounds = int(arg("--rounds", "5"))
    ms = [int(s) for s in arg("--m", "8,10,12").split(",")]
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    ctx = L.Context(0)
    read_gbs, copy_gbs = ctx.bandwidth_probe()
    res = {"rounds": rounds, "read_ceiling_gigabytes_per_second": read_gbs, "copy_gigabytes_per_second": copy_gbs, "cases": {}}
    gen = torch.Generator(device="cuda").manual_seed(20261021)
    for n_sites in sizes:
        n = 1 << n_sites
        for np_dtype, t_dtype in ((np.float64, torch.float64), (np.complex128, torch.complex128)):
            cplx = np.dtype(np_dtype).kind == "c"
            elem = np.dtype(np_dtype).itemsize
            psi = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
            if cplx:
                psi = torch.complex(psi, torch.randn(n, dtype=torch.float64, device="cuda", generator=gen))
            psi /= torch.linalg.vector_norm(psi)
            view = device_view(psi, np_dtype)
            op = L.PauliOperator(ctx, n_sites, [(0, 1, 1.0)], np_dtype)
            for m in [6] + ms:
                dim = 1 << m
                out = torch.empty((dim, dim), dtype=torch.complex128, device="cuda")
                out_view = device_view(out, np.complex128)
                for where, sites in site_lists(n_sites, m).items():
                    shape, perm = gather_plan(n_sites, sites)

                    def torch_route():
                        f = psi.view(shape).permute(perm).reshape(dim, -1)
                        rho = f @ f.conj().T
                        torch.cuda.synchronize()
                        return rho

                    def tiled():
                        op.reduced_density_matrix_tiled(view, sites, out=out_view)   # returns after the stream's synchronisation

                    def one_sweep():
                        return op.reduced_density_matrix(view, sites)

                    other, other_name = (one_sweep, "ll_pauli_rdm") if m == 6 else (torch_route, "torch")
                    torch.cuda.synchronize()
                    ref = other()
                    tiled()
                    torch.cuda.synchronize()
                    ref = torch.as_tensor(ref, device="cuda").to(torch.complex128)
                    diff = float((out - ref).abs().max() / ref.abs().max())
                    del ref
                    sec = {other_name: [], "tiled": []}
                    for _ in range(rounds):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        other()
                        sec[other_name].append(time.perf_counter() - t0)
                        t0 = time.perf_counter()
                        tiled()
                        sec["tiled"].append(time.perf_counter() - t0)
                    t_new, t_old = float(np.median(sec["tiled"])), float(np.median(sec[other_name]))
                    flops = kernel_flops(n_sites, m, cplx)
                    key = "n%d_%s_m%d_%s" % (n_sites, np.dtype(np_dtype).char, m, where)
                    res["cases"][key] = {
                        "n_sites": n_sites, "dtype": np.dtype(np_dtype).name, "m": m, "sites": sites,
                        "seconds": {k: stats(v) for k, v in sec.items()},
                        other_name + "_over_tiled": t_old / t_new,
                        "tiled_flops": flops, "tiled_teraflops_per_second": flops / t_new / 1e12,
                        "psi_bytes": elem * n, "psi_gigabytes_per_second": elem * n / t_new / 1e9,
                        "psi_fraction_of_read_ceiling": elem * n / t_new / 1e9 / read_gbs,
                        "largest_relative_difference_between_the_routes": diff,
                    }
                    print(key, json.dumps(res["cases"][key]), flush=True)
                del out
            op.close()
            del psi
            torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
