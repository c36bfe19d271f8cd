"""ll_pauli_block_transfer on rings of 16 and 20 sites (test_gpu_pauli_block_transfer.py holds the contract and its constant):
one 16-site pair of the full space (D about 4.1 k: several chunks of 1024 states per workgroup at large block bits, several
blocks at the default), one 16-site pair of the sector n_down = 8, and one 20-site pair of the full space (D about 52 k) checked
on 256 sampled rows against the gather form evaluated on the CPU (generators.pauli_block_transfer_rows_np), as
test_gpu_pauli_large.py samples its rows.  Every case at the default block bits, at the smallest the tuning key admits (0: one
index per workgroup block, so block and grid-stride boundaries are crossed: 52 k blocks over a grid of 2048) and at 12 (one
block, four chunks at 16 sites): the same bits of the output at every setting; norm2 is a sum per workgroup, so its order
follows the setting and it is held to its bound each time."""
import numpy as np
import pytest

import contract_cases as K
import exact_ref as E
from lambda_lanczos_amd import generators as G
from pauli_expect_block_cases import Block
from test_gpu_pauli_block_transfer import TYPES, TWO, X0X2, Y0Z1, Z0, block_op, check_result, kind_shape, transfer_bound

pytestmark = pytest.mark.gpu

KEYS = {"momentum_full": "pauli_momentum_full_block_bits", "momentum": "pauli_momentum_block_bits"}
SETTINGS = (None, "0", "12")


def _at_every_setting(ctx, kind, call):
    """call() -> (out, norm2) at each block-bits setting: [(out, norm2)], the outputs bit for bit equal."""
    res = []
    try:
        for bits in SETTINGS:
            ctx.set_tuning(KEYS[kind], bits)
            res.append(call())
            assert np.array_equal(res[0][0].view(np.uint8), res[-1][0].view(np.uint8)), ("the bits depend on the block size", bits)
    finally:
        ctx.set_tuning(KEYS[kind], None)
    return res


PAIRS_16 = [(Block("momentum_full", 16, 3), Block("momentum_full", 16, 11), "z"), (Block("momentum_full", 16, 0), Block("momentum_full", 16, 8), "d"),
            (Block("momentum_full", 16, 8), Block("momentum_full", 16, 8), "s"), (Block("momentum", 16, 5, n_down=8), Block("momentum", 16, 14, n_down=8), "z"),
            (Block("momentum", 16, 8, n_down=8), Block("momentum", 16, 0, n_down=8), "d"), (Block("momentum", 16, 2, n_down=8), Block("momentum", 16, 6, n_down=8), "c")]


@pytest.mark.parametrize("bs,bt,tid", PAIRS_16, ids=["%s-to-m%d-%s" % (a.id, b.m, t) for a, b, t in PAIRS_16])
def test_sixteen_sites(ctx, bs, bt, tid):
    dtype = TYPES[tid]
    kind = bs.kind
    src, tgt = block_op(ctx, bs, dtype), block_op(ctx, bt, dtype)
    assert (4000 <= src.n_local <= 4200) if kind == "momentum_full" else (780 <= src.n_local <= 830), src.n_local
    c = K.start_x(src.n_local, dtype, seed=11)
    for terms in [Z0, X0X2, TWO] + ([Y0Z1] if tid in "zc" and not bs.sector else []):   # (in a sector Y_0 Z_1 gives +0.0: the small rings)
        want, mag = G.pauli_block_transfer_np(kind, kind_shape(bs)[1], kind_shape(bt)[1], terms, c, return_magnitude=True)
        for got, norm2 in _at_every_setting(ctx, kind, lambda: src.transfer(terms, c, tgt, return_norm2=True)):
            r = check_result(got, norm2, want, mag, 16, len(terms), dtype, (bs.id, bt.id, tid, terms))
        assert np.any(got != 0)
        print("worst error / bound", bs.id, bt.m, tid, terms, r)


def test_twenty_sites_sampled_rows(ctx):
    """D about 52 k in z.  The sampled rows come from the gather form over the strings of Pbar_q — Z_0, X_0 X_2 and Y_0 Z_1 have
    the full period 20, so no string is dropped and the kernel's terms are the reference's: N = 20 n_terms strings, the
    magnitudes are those of the strings."""
    dtype = np.complex128
    n_sites = 20
    bs, bt = Block("momentum_full", n_sites, 7), Block("momentum_full", n_sites, 16)
    src, tgt = block_op(ctx, bs, dtype), block_op(ctx, bt, dtype)
    assert 52000 <= src.n_local <= 53000 and 52000 <= tgt.n_local <= 53000
    c = K.start_x(src.n_local, dtype, seed=11)
    rng = np.random.default_rng(20)
    rows = np.unique(np.concatenate([[0, 1, 255, 256, 1023, 1024, 2047, 2048, tgt.n_local - 2, tgt.n_local - 1],
                                     rng.integers(0, tgt.n_local, 246)]))
    for terms in (Z0, X0X2, Y0Z1):
        want, mag = G.pauli_block_transfer_rows_np("momentum_full", (n_sites, bs.m), (n_sites, bt.m), terms, c, rows=rows)
        for got, norm2 in _at_every_setting(ctx, "momentum_full", lambda: src.transfer(terms, c, tgt, return_norm2=True)):
            err = np.abs(got[rows] - want)
            bound = transfer_bound(n_sites, len(terms), mag, want, dtype)
            assert np.all(err <= bound), (terms, int(np.argmax(err - bound)))
            sq = float(np.sum(np.abs(got) ** 2))
            assert abs(norm2 - sq) <= 2.0 * (got.shape[0] + 8) * E.EPS_D * sq
        assert np.count_nonzero(want) >= rows.shape[0] // 2   # (a row all of whose partners the source block excludes is 0)
        print("20 sites: worst error / bound", terms, float(np.max(err / bound)))
