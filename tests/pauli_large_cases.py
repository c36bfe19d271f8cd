"""The cases of tests/test_gpu_pauli_large.py and tests/test_pauli_large_host.py: rings of 20 to 30 sites for the five
matrix-free spin-1/2 kernels, their term lists and the pinned block dimensions.  No GPU, no test.

Every D below comes from the host generator (generators.momentum_basis, full_momentum_basis, symmetric_basis) and is tied by
sum rules that the generator does not use (test_pauli_large_host)."""
import numpy as np

import exact_ref as E
from lambda_lanczos_amd import generators as G

MAX_GRID = 2048      # kMaxGrid = 8 * kCUs (csrc/ll_internal.hpp): the grid of the kernels' grid-stride loops
WRAPS = 3 * MAX_GRID + 1   # blocks from which some workgroups take three trips of the loop, others four (or more), the last ragged


def dm_heisenberg(n_sites):
    """The complex model of test_gpu_pauli_sector ("dm")."""
    return G.dm_terms(n_sites, 0.35, periodic=True) + G.heisenberg_terms(n_sites, 1.0, 0.8, periodic=True)


def model_terms(model, n_sites):
    if model == "heisenberg":
        return G.heisenberg_terms(n_sites, 1.0, 1.0, periodic=True)
    if model == "dm":
        return dm_heisenberg(n_sites)
    if model == "tfim":
        return G.tfim_terms(n_sites, 1.0, 0.7, periodic=True)
    if model == "xyz":
        return G.xyz_terms(n_sites, 1.0, 0.6, 0.8)
    raise KeyError(model)


# (n_sites, n_down) -> model.  (30, 4): both rank tables at h = 15 (2^15 entries each); (20, 10): 11 548 blocks at 16 indices per
# block; (29, 3), (30, 3): h = 15 and 14 / 15 other bits, D = 3654 and 4060 — below 3 * 2048 + 1: one index per block there, two
# trips of the loop, the third is (30, 4)'s and (20, 10)'s.
SECTOR = [((30, 4), "heisenberg"), ((20, 10), "heisenberg"), ((29, 3), "heisenberg"), ((30, 3), "dm")]

# (n_sites, n_down, momentum) -> D_m, Heisenberg ring.  (30, 5, 7): complex phases, every orbit of length 30; (30, 4, 0): orbits of
# length 15 inside the block (norm ratios), (30, 4, 15): excluded from it; (20, 10, 10): orbits of length 2, 4, 10, 20 and
# 9252 >= 3 * 2048 + 1 blocks at one index per block; (27, 4, 9): odd ring.  The others stay below 3 * 2048 + 1 states: one index
# per block there ((30, 5, 7): three trips for some workgroups, two for the rest).
MOMENTUM = {(30, 5, 7): 4750, (30, 4, 0): 917, (30, 4, 15): 910, (20, 10, 10): 9252, (27, 4, 9): 650}

# (n_sites, momentum) -> (model, D_m): the full 2^n_sites space.  All wrap: 6560, 6548 and 6242 blocks at 8 / 8 / 16 indices.
MOMENTUM_FULL = {(20, 10): ("tfim", 52480), (20, 3): ("xyz", 52377), (21, 7): ("xyz", 99860)}

# (n_sites, momentum, parity, inversion, n_down) -> (model, D).  The dilute sectors of 27 to 30 sites put (nearly) the whole basis
# into bucket 0 of the search: (30, 0, +, 0, 4) prefix_shift 25, largest bucket 511 of 511, 9 halvings; (30, 15, -, 0, 5) shift
# 22, 2319 of 2421, 12 halvings; (28, 14, -, 0, 5) shift 21, 1757 of 1794, 11; (27, 9, 0, 0, 4) shift 21, 650 of 650, 10 (complex
# phases).  (20, 10, -, -, 10): all four streams, orbit lengths 2 .. 80.  Below 3 * 2048 + 1 states these run one index per
# block; the third trip is (22, 0, +, +, 11)'s (8359 blocks) and the full-space blocks' (6824 and 6682 at two indices).
SYMMETRIC = {(30, 0, 1, 0, 4): ("heisenberg", 511), (30, 15, -1, 0, 5): ("heisenberg", 2421),
             (28, 14, -1, 0, 5): ("heisenberg", 1794), (27, 9, 0, 0, 4): ("heisenberg", 650),
             (20, 10, -1, -1, 10): ("heisenberg", 2429), (22, 0, 1, 1, 11): ("heisenberg", 8359),
             (20, 0, 1, 1, None): ("xyz", 13648), (20, 10, -1, -1, None): ("xyz", 13364)}

# the cases whose D lies below 3 * 2048 + 1: they run at one index per block and leave the third trip to the others of their kernel
BELOW_WRAP = {("sector", (29, 3)), ("sector", (30, 3)),
              ("momentum", (30, 5, 7)), ("momentum", (30, 4, 0)), ("momentum", (30, 4, 15)), ("momentum", (27, 4, 9)),
              ("symmetric", (30, 0, 1, 0, 4)), ("symmetric", (30, 15, -1, 0, 5)), ("symmetric", (28, 14, -1, 0, 5)),
              ("symmetric", (27, 9, 0, 0, 4)), ("symmetric", (20, 10, -1, -1, 10))}

_POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], np.int64)


def sector_abs_rows(n_sites, n_down, terms, X):
    """What the class bound takes from exact_ref.rows_exact(generators.pauli_sector_csr(..., merge=False), X) — the entries per row
    and sum_j |a_ij| |X_j|, one entry per term whose partner stays in the sector — term by term, without the matrix (C(22, 11)
    rows of 66 entries would take 1 GB) and without the exact sums, which the bound never reads."""
    s = G.sector_states(n_sites, n_down).astype(np.int64)
    h = (n_sites + 1) // 2
    lo, hi = G.sector_rank_tables(n_sites, n_down, h)
    ax = E.abs1(X)
    absrow, rowsum, nnz = np.zeros(s.shape[0]), np.zeros(s.shape[0]), np.zeros(s.shape[0], np.int64)
    for xm, _, c in terms:
        p = s ^ int(xm)
        inside = _POP16[p & 0xFFFF] + _POP16[p >> 16] == n_down
        q = np.where(inside, p, s[0])
        k = lo[q & ((1 << h) - 1)].astype(np.int64) + hi[q >> h]
        absrow += np.where(inside, abs(float(c)) * ax[k], 0.0)
        rowsum += np.where(inside, abs(float(c)), 0.0)
        nnz += inside
    return E.Rows(None, absrow, rowsum, nnz)


# ------------------------------------------------------------------ PauliOperator on all 2^20 states
PAULI_SITES = 20
PAULI_SAMPLE = 8192


def _bits(*sites):
    return sum(1 << j for j in sites)


def pauli_terms(cplx):
    """The TFIM ring plus six strings on sites 14 to 19 — above every tile: the tile's share of a term's parity and the remote
    tiles' addresses come from these bits alone.  The last two carry an odd number of Y (complex types only)."""
    terms = G.tfim_terms(PAULI_SITES, 1.0, 0.7, periodic=True)
    terms += [(_bits(14, 15, 19), _bits(15, 17, 19), 0.31),      # X14 Y15 Z17 Y19
              (_bits(16, 18), _bits(19), -0.27),                  # X16 X18 Z19
              (_bits(14, 16), _bits(14, 16), 0.23),               # Y14 Y16
              (_bits(19), _bits(14), 0.19)]                       # Z14 X19: shares its x mask with the field term of site 19
    if cplx:
        terms += [(_bits(15, 18), _bits(18), 0.17),               # X15 Y18
                  (_bits(14, 17, 19), _bits(14, 16, 17, 19), -0.13)]   # Y14 Z16 Y17 Y19
    return terms


def pauli_sample():
    """8192 of the 2^20 states, ascending: the first and the last 64, the two on either side of every multiple of 2^12, the rest
    drawn with a fixed seed."""
    n = 1 << PAULI_SITES
    fixed = set(range(64)) | set(range(n - 64, n))
    for k in range(1 << 12, n, 1 << 12):
        fixed |= {k - 2, k - 1, k, k + 1}
    rest = np.setdiff1d(np.arange(n), np.fromiter(fixed, np.int64), assume_unique=False)
    drawn = np.random.default_rng(20).choice(rest, PAULI_SAMPLE - len(fixed), replace=False)
    out = np.sort(np.concatenate([np.fromiter(fixed, np.int64), drawn]))
    assert out.shape[0] == PAULI_SAMPLE and np.all(np.diff(out) > 0)
    return out


def small_bits(dim):
    """The largest b with ceil(dim / 2^b) >= 3 * 2048 + 1, or 0 where dim is too small for that: the block bits at which the
    grid-stride loop of a 2048-workgroup grid takes at least three trips with a ragged last one."""
    b = 0
    while -(-dim // (2 << b)) >= WRAPS:
        b += 1
    return b
