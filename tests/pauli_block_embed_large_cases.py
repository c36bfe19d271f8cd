"""The cases of tests/test_gpu_pauli_block_embed_large.py and tests/test_pauli_block_embed_plan_host.py: ll_pauli_block_expand and
ll_pauli_block_project on rings of 20 to 30 sites, with the pinned block dimensions of pauli_large_cases.  No GPU, no test.

Also here: a Python restatement of the launch rule of csrc/pauli_block_embed_plan.hpp (units of work and grid), the tabulated
(units, grid) of every case, and host references that never build 2^30 numbers: for a sector target the embedding's rows are
those of generators.*_embedding over sector_states; for the sector block in the full space of 2^20 states the sector's rows are
scattered to their states."""
import math

import numpy as np

import pauli_large_cases as PL
from lambda_lanczos_amd import generators as G

MAX_GRID = PL.MAX_GRID
EXPAND_BITS = 10      # kPauliBlockExpandBlockBits (csrc/pauli_block_embed_plan.hpp)
PROJECT_BITS = 8      # kPauliBlockProjectBlockBits


def launch(count, forced, default):
    """pauli_block_embed_launch: (units, grid)."""
    bits = default if forced is None else min(forced, 30)
    units = -(-count // (1 << bits))
    return units, min(units, MAX_GRID)


def expand_launch(n_target, forced=None):
    return launch(n_target, forced, EXPAND_BITS)


def project_launch(dim, forced=None):
    return launch(dim, forced, PROJECT_BITS)


# (block kind, block shape, target: ("sector", n_sites, n_down) or ("full", n_sites), forced expand bits, forced project bits,
#  expand (units, grid), project (units, grid)).  The forced bits give every kernel two or more trips of the grid-stride loop;
# with a sector target the last trip is ragged (units is no multiple of the grid).  A full-space target holds 2^n_sites states:
# its units are a power of two, so its trips are whole — the ragged last trip of the full-space forms is project's, whose units
# count representatives.
CASES = [
    ("momentum", (30, 5, 7), ("sector", 30, 5), 6, 1, (2227, 2048), (2375, 2048)),
    ("momentum", (20, 10, 10), ("sector", 20, 10), 6, 2, (2887, 2048), (2313, 2048)),
    ("momentum_full", (20, 3), ("full", 20), 8, 4, (4096, 2048), (3274, 2048)),
    ("momentum_full", (21, 7), ("full", 21), 9, 5, (4096, 2048), (3121, 2048)),
    ("symmetric", (30, 15, -1, 0, 5), ("sector", 30, 5), 6, 0, (2227, 2048), (2421, 2048)),
    ("symmetric", (22, 0, 1, 1, 11), ("sector", 22, 11), 8, 1, (2756, 2048), (4180, 2048)),
    ("symmetric", (20, 0, 1, 1, None), ("full", 20), 7, 2, (8192, 2048), (3412, 2048)),
    ("symmetric", (20, 10, -1, -1, 10), ("full", 20), 8, 0, (4096, 2048), (2429, 2048)),
]


def block_dim(kind, shape):
    if kind == "momentum":
        return PL.MOMENTUM[shape]
    return (PL.MOMENTUM_FULL if kind == "momentum_full" else PL.SYMMETRIC)[shape][1]


def block_model(kind, shape):
    if kind == "momentum":
        return "heisenberg"
    return (PL.MOMENTUM_FULL if kind == "momentum_full" else PL.SYMMETRIC)[shape][0]


def target_dim(target):
    return math.comb(target[1], target[2]) if target[0] == "sector" else 1 << target[1]


def momentum_of(kind, shape):
    return shape[2] if kind == "momentum" else shape[1]


def real_character(kind, shape):
    return (2 * momentum_of(kind, shape)) % shape[0] == 0


def group_size(kind, shape):
    if kind != "symmetric":
        return shape[0]
    return shape[0] * (2 if shape[2] else 1) * (2 if shape[3] else 1)


def tids(kind, shape):
    """The `_tids` rule of test_gpu_pauli_large.py: d, z, s, c where the block is real, else z and c."""
    return ("d", "z", "s", "c") if real_character(kind, shape) else ("z", "c")


def case_id(case):
    return "-".join([case[0]] + ["x" if v is None else str(v) for v in case[1]] + [str(v) for v in case[2]])


def embedding(kind, shape, target):
    """(col, val, R) over the target's basis: col -1 and val 0 where the row of B is empty; R the orbit length of the row's column
    (0 where empty).  The generators' sparse form; a sector block in the full space is scattered to its states."""
    if kind == "momentum":
        col, val = G.momentum_embedding(*shape, dense=False)
        periods = G.momentum_basis(*shape)[1]
        n_down = shape[1]
    elif kind == "momentum_full":
        col, val = G.full_momentum_embedding(*shape, dense=False)
        periods = G.full_momentum_basis(*shape)[1]
        n_down = None
    else:
        n_sites, m, p, z, n_down = shape
        col, val = G.symmetric_embedding(n_sites, m, p, z, n_down, dense=False)
        periods = G.symmetric_basis(n_sites, m, p, z, n_down)[1]
    if target[0] == "full" and n_down is not None:
        st = G.sector_states(shape[0], n_down).astype(np.int64)
        fcol, fval = np.full(1 << shape[0], -1, np.int64), np.zeros(1 << shape[0], np.complex128)
        fcol[st], fval[st] = col, val
        col, val = fcol, fval
    assert col.shape[0] == target_dim(target)
    R = np.where(col >= 0, periods[np.maximum(col, 0)], 0)
    return col, val, R


def expand_np(col, val, c, dtype):
    """(wide(c[col]) * val).astype(T): the contract of expand; empty rows +0.0."""
    cplx = np.dtype(dtype).kind == "c"
    wide = np.asarray(c).astype(np.complex128 if cplx else np.float64)
    v = val if cplx else val.real
    out = np.where(col >= 0, wide[np.maximum(col, 0)] * v, 0.0)
    return out.astype(dtype)


def project_integer_np(col, val, R, psi, dim, kind, shape, dtype):
    """The contract of project on an integer state with a real character: float64(S) * (sqrt(R) / |G|), S the exact integer
    sum_g conj(chi(g)) Psi[g a] over ALL |G| elements = (|G| / R) * sum over the orbit of sign(val) Psi."""
    assert real_character(kind, shape)
    Gs = group_size(kind, shape)
    cplx = np.dtype(dtype).kind == "c"
    wide = np.asarray(psi).astype(np.complex128 if cplx else np.float64)
    rows = np.flatnonzero(col >= 0)
    sign = np.sign(val.real[rows])
    assert np.all(np.abs(sign) == 1.0)
    mult = Gs // R[rows]
    assert np.all(mult * R[rows] == Gs)
    Ra = np.zeros(dim, np.int64)
    Ra[col[rows]] = R[rows]
    factor = np.sqrt(Ra.astype(np.float64)) / float(Gs)
    parts = [wide.real, wide.imag] if cplx else [wide]
    sums = []
    for p in parts:
        s = np.bincount(col[rows], weights=sign * mult * p[rows], minlength=dim)   # integers below 2^53: exact in any order
        assert np.array_equal(s, np.rint(s)) and np.all(np.abs(s) < 2.0 ** 53)
        sums.append(s * factor)
    out = sums[0] + 1j * sums[1] if cplx else sums[0]
    return out.astype(dtype)


def project_np(col, val, psi, dim):
    """B^H Psi in double (complex128) for any Psi, with sum |terms| per representative (for the bound)."""
    rows = np.flatnonzero(col >= 0)
    wide = np.asarray(psi).astype(np.complex128)
    terms = np.conj(val[rows]) * wide[rows]
    out = np.bincount(col[rows], weights=terms.real, minlength=dim) + 1j * np.bincount(col[rows], weights=terms.imag, minlength=dim)
    mag = np.bincount(col[rows], weights=np.abs(terms), minlength=dim)
    return out, mag
