"""One rank of the sharded-context checks of tests/test_gpu_pauli_sector.py, _momentum.py, _momentum_full.py and _symmetric.py: two
of these processes share the test box's GPU through the host-staged test transport (LL_COMM_PLUGIN) and ask for a
sum-of-Pauli-strings operator of the given kind on a ring of 10 sites, which a sharded context refuses.
argv: rank world shm_name out_dir kind (sector | momentum | momentum_full | symmetric)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import lambda_lanczos_amd as L  # noqa: E402
from util import install_hook_sync  # noqa: E402
from lambda_lanczos_amd import generators as G  # noqa: E402

install_hook_sync()

CREATE = {
    "sector": lambda ctx: L.PauliSectorOperator(ctx, 10, 5, G.heisenberg_terms(10)),
    "momentum": lambda ctx: L.PauliMomentumOperator(ctx, 10, 5, 0, G.heisenberg_terms(10)),
    "momentum_full": lambda ctx: L.PauliMomentumFullOperator(ctx, 10, 0, G.tfim_terms(10, 1.0, 0.7, periodic=True)),
    "symmetric": lambda ctx: L.PauliSymmetricOperator(ctx, 10, 0, G.tfim_terms(10, 1.0, 0.7, periodic=True), parity=1, inversion=1),
}


def main():
    rank, world, name, out_dir, kind = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
    ctx = L.Context(0)
    ctx.init_comm(name.encode() + b"\0" * (128 - len(name)), rank, world)
    res = {}
    try:
        CREATE[kind](ctx)
        res["code"] = 0
    except L.capi.LanczosHipError as e:
        res["code"] = e.code
        res["msg"] = str(e)
    ctx.close()
    with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main()
