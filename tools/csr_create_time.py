"""Creation time of the CSR operator for config 3's matrix (random symmetric, n = 1e7): host clock around ll_op_create_csr_*,
twice per process (the first creation carries the process's one-off costs)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import lambda_lanczos_amd as L  # noqa: E402
from lambda_lanczos_amd import generators as G  # noqa: E402

n = 10_000_000
ctx = L.Context(0)
csr = G.randsym(n)
times = []
for _ in range(2):
    ctx.synchronize()
    t0 = time.perf_counter()
    op = L.CsrOperator(ctx, *csr)
    ctx.synchronize()
    times.append(time.perf_counter() - t0)
    kind = op.selected_spmv()
    op.close()
print(json.dumps({"lib": L.LIB_PATH, "create_s": times, "selected_spmv": kind}))
ctx.close()
