"""One rank of the sharded-context check of tests/test_gpu_expo_two_pass.py: two of these processes share the test box's GPU
through the host-staged test transport (LL_COMM_PLUGIN), each holds its shard of the 2-D Laplacian as a CSR operator — which a
sharded context accepts — and asks for the two-pass Exponentiator, which it refuses.
argv: rank world shm_name out_dir"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import lambda_lanczos_amd as L  # noqa: E402
from util import install_hook_sync  # noqa: E402
from lambda_lanczos_amd import generators as G  # noqa: E402

install_hook_sync()


def main():
    rank, world, name, out_dir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    ctx = L.Context(0)
    ctx.init_comm(name.encode() + b"\0" * (128 - len(name)), rank, world)
    side = 24
    n = side * side
    rb, nl = ctx.partition(n)
    op = L.CsrOperator(ctx, *G.laplace2d(side, rb, nl), n_cols=n, row_begin=rb)
    ex = L.Exponentiator(op, n)
    res = {}
    try:
        ex.run_two_pass(-0.5, G.start_vector(nl, 1, np.float64, rb))
        res["code"] = 0
    except L.capi.LanczosHipError as e:
        res["code"] = e.code
        res["msg"] = str(e)
    op.close()
    ctx.close()
    with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main()
