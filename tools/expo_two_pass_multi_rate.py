#!/usr/bin/env python3
"""Seconds for s separate Exponentiator.run_two_pass calls against ONE Exponentiator.run_two_pass_multi call with the same s times,
s = 1, 2, 4, 8, on the open transverse-field Ising chain of tools/expo_two_pass_rate.py (L = 24, J = 1, h = 1.5) in complex double
(256 MiB per vector), default eps, same operator, same input.  The times are a_j = -0.05i (j + 1): their iteration counts m_j differ,
so accumulators retire early in the multi call.

The s separate calls are the baseline (the only way before the multi call existed), not the code under test.  Host clock around
whole calls (each ends in a device synchronisation); input and outputs stay in device memory.  The two forms ALTERNATE in one
process: after one warm-up of each, ROUNDS rounds of (separate, multi) per s; median and spread (min, max) over the rounds.  Beside
the seconds, the two models they are to be read against:
  operator applications   2 max_j m_j - 1            against  sum_j (2 m_j - 1)
  pass-2 bytes            sum_k (4 + 2 s'_k) 16 n    against  sum_j 6 * 16 n (m_j - 1)      s'_k = |{j : k + 1 < m_j}|, k + 1 < max m_j
and whether the outputs of the two forms are the same bytes.

Then the replayed step alone (the primitives recur_accum / recur_accum_multi on the same vectors, LAUNCHES launches between two
synchronisations, alternating): seconds per launch of the single kernel and of the multi kernel with 1, 2, 4 and 8 accumulators,
and the bytes per second the byte model gives them.  There is no threshold.
    python tools/expo_two_pass_multi_rate.py [out.json] [--sites 24] [--rounds 5] [--launches 20]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lambda_lanczos_amd as L  # noqa: E402
from lambda_lanczos_amd import generators as G  # noqa: E402

COUNTS = (1, 2, 4, 8)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def same_bytes(x, y, n, piece=1 << 20):
    """Two device vectors compared in slices (a whole vector is 256 MiB on the host)."""
    hx, hy = x.get(), y.get()
    return all(np.array_equal(hx[i:i + piece].view(np.uint8), hy[i:i + piece].view(np.uint8)) for i in range(0, n, piece))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    n_sites, rounds, launches = int(arg("--sites", "24")), int(arg("--rounds", "5")), int(arg("--launches", "20"))
    n = 1 << n_sites
    times = [-0.05j * (j + 1) for j in range(max(COUNTS))]
    ctx = L.Context(0)
    op = L.PauliOperator(ctx, n_sites, G.tfim_terms(n_sites, 1.0, 1.5), np.complex128)
    start = G.start_vector_fast(n, 1).astype(np.complex128)
    start /= np.linalg.norm(start)
    psi = ctx.to_device(start)
    out_sep = [ctx.empty(n, np.complex128) for _ in times]
    out_multi = [ctx.empty(n, np.complex128) for _ in times]
    ex = L.Exponentiator(op, n)

    def timed(call):
        ctx.synchronize()
        t0 = time.perf_counter()
        r = call()
        ctx.synchronize()
        return time.perf_counter() - t0, r

    def separate(s):
        return timed(lambda: [int(ex.run_two_pass(times[j], psi, out=out_sep[j])[1]) for j in range(s)])

    def multi(s):
        dt, (_, ms) = timed(lambda: ex.run_two_pass_multi(times[:s], psi, out=out_multi[:s]))
        return dt, ms

    per_s = []
    for s in COUNTS:
        separate(s), multi(s)   # warm-up of both
        sec = {"separate": [], "multi": []}
        for _ in range(rounds):
            dt, m_sep = separate(s)
            sec["separate"].append(dt)
            dt, m_multi = multi(s)
            sec["multi"].append(dt)
        mismatches = ex.last_stats["replay_mismatches"]
        active = [sum(1 for m in m_multi if k + 1 < m) for k in range(max(m_multi) - 1)]
        per_s.append({
            "s": s, "times_im": [t.imag for t in times[:s]], "m_j": m_multi, "m_j_separate": m_sep,
            "seconds": {k: stats(v) for k, v in sec.items()},
            "separate_over_multi": float(np.median(sec["separate"]) / np.median(sec["multi"])),
            "operator_applications": {"multi": 2 * max(m_multi) - 1, "separate": sum(2 * m - 1 for m in m_sep)},
            "pass2_bytes": {"multi": sum((4 + 2 * c) * 16 * n for c in active), "separate": sum(6 * 16 * n * (m - 1) for m in m_sep)},
            "outputs_are_the_same_bytes": all(same_bytes(out_sep[j], out_multi[j], n) for j in range(s)),
            "replay_mismatches": mismatches,
            "workspace_vectors": ex.last_stats["workspace_vectors"],
        })
        print(json.dumps(per_s[-1]), flush=True)

    # ---- the replayed step alone: y -= a x + b p, psi_j += g_j y (a = b = 0 keeps the values where they are over many launches)
    y, x, p = out_sep[0], out_sep[1], out_sep[2]
    g = 0.0 + 0.0j

    def step_single():
        for _ in range(launches):
            L.recur_accum(ctx, y, x, p, 0.0, 0.0, g, out_multi[0], n)

    def step_multi(c):
        def run():
            for _ in range(launches):
                L.recur_accum_multi(ctx, y, x, p, 0.0, 0.0, [g] * c, out_multi[:c], n)
        return run

    kernels = [("single", 1, step_single)] + [("multi_%d" % c, c, step_multi(c)) for c in COUNTS]
    for _, _, f in kernels:
        timed(f)
    ksec = {k: [] for k, _, _ in kernels}
    for _ in range(rounds):
        for k, _, f in kernels:
            ksec[k].append(timed(f)[0] / launches)
    step = {}
    for k, c, _ in kernels:
        nbytes = (4 + 2 * c) * 16 * n
        step[k] = {"accumulators": c, "model_bytes": nbytes, "seconds_per_launch": stats(ksec[k]),
                   "model_terabytes_per_second": nbytes / float(np.median(ksec[k])) / 1e12}
    res = {"n_sites": n_sites, "n": n, "vector_bytes": 16 * n, "rounds": rounds, "launches": launches, "calls": per_s,
           "replayed_step": step}
    print(json.dumps(res, indent=1), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    for v in [psi] + out_sep + out_multi:
        v.free()
    op.close()
    ctx.close()


if __name__ == "__main__":
    main()
