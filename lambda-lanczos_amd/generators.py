"""Synthetic inputs of SURVEY.md section 8(d): deterministic functions of (index, seed) through splitmix64.

Two implementations that must agree bit for bit: numpy (this file; any size that fits numpy, used for the small
parity cases) and C++ (csrc/generators.cpp -> lib/libllgen.so; used at BASELINE sizes, n = 1e7 in a few seconds).
This is workload synthesis for bench.py / tests — neither the hot path nor the oracle.
"""
import ctypes as C
import math
import os

# the generator library's OpenMP workers must go to sleep right after a parallel region: workers that keep spinning
# (libomp: 200 ms) disturb launch-bound GPU runs that follow immediately (tools/stall_probe.py: one ~85 ms stall per
# process).  Read by the OpenMP runtimes when they start, so it is set before the library is loaded.
os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import numpy as np  # noqa: E402

from . import _capi as capi

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
K_OUT = 7


def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def u01(x):
    return (splitmix64(x) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def start_vector(n_local, seed=1, dtype=np.float64, row_begin=0):
    """v_i = 2*u01(seed*2^40 + i) - 1 (complex: re from 2i, im from 2i+1), i = global index."""
    base = np.uint64(seed) << np.uint64(40)
    g = np.arange(row_begin, row_begin + n_local, dtype=np.uint64)
    if np.dtype(dtype) == np.complex128:
        re = 2.0 * u01(base + np.uint64(2) * g) - 1.0
        im = 2.0 * u01(base + np.uint64(2) * g + np.uint64(1)) - 1.0
        return re + 1j * im
    return 2.0 * u01(base + g) - 1.0


# ------------------------------------------------------------------ numpy versions (small n)
def laplace2d_np(N, row_begin=0, n_local=None):
    n = N * N
    n_local = n - row_begin if n_local is None else n_local
    r = np.arange(row_begin, row_begin + n_local, dtype=np.int64)
    y, x = r // N, r % N
    cols = np.stack([r - N, r - 1, r, r + 1, r + N], axis=1)
    vals = np.tile(np.array([-1.0, -1.0, 4.0, -1.0, -1.0]), (n_local, 1))
    mask = np.stack([y > 0, x > 0, np.ones_like(r, bool), x + 1 < N, y + 1 < N], axis=1)
    rp = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
    return rp, cols[mask].astype(np.int32), vals[mask]


def _b_cols_np(n, band):
    i = np.arange(n, dtype=np.int64)[:, None]
    j = np.arange(K_OUT, dtype=np.int64)[None, :]
    h = splitmix64((64 * i + j).astype(np.uint64))
    if band <= 0:
        c = (h % np.uint64(n - 1)).astype(np.int64)
        c = c + (c >= i)
    else:
        off = (h % np.uint64(2 * band)).astype(np.int64)
        d = off - band
        d = d + (d >= 0)
        c = (i + d) % n
    v = 2.0 * u01((64 * i + j + 32).astype(np.uint64)) - 1.0
    return c, v


def randsym_np(n, band=0, row_begin=0, n_local=None):
    """A = B + B^T + 7I, 7 random out-entries per row of B, duplicates kept; rows sorted by column (stable)."""
    n_local = n - row_begin if n_local is None else n_local
    c, v = _b_cols_np(n, band)
    i = np.repeat(np.arange(n, dtype=np.int64), K_OUT)
    cf, vf = c.reshape(-1), v.reshape(-1)
    # (row, col, val, order-key): own entries first (by j), then diagonal, then transposed entries (by source row, j)
    rows = np.concatenate([i, np.arange(n, dtype=np.int64), cf])
    cols = np.concatenate([cf, np.arange(n, dtype=np.int64), i])
    vals = np.concatenate([vf, np.full(n, 7.0), vf])
    keep = (rows >= row_begin) & (rows < row_begin + n_local)
    rows, cols, vals = rows[keep], cols[keep], vals[keep]
    order = np.lexsort((np.arange(rows.shape[0]), cols, rows))  # stable within equal (row, col)
    rows, cols, vals = rows[order], cols[order], vals[order]
    rp = np.zeros(n_local + 1, dtype=np.int64)
    np.add.at(rp, rows - row_begin + 1, 1)
    return np.cumsum(rp), cols.astype(np.int32), vals


def torus_np(N, row_begin=0, n_local=None):
    n = N * N
    n_local = n - row_begin if n_local is None else n_local
    phi = 2.0 * math.pi * 3.0 / N
    r = np.arange(row_begin, row_begin + n_local, dtype=np.int64)
    y, x = r // N, r % N
    cols = np.stack([y * N + (x + 1) % N, y * N + (x + N - 1) % N, ((y + 1) % N) * N + x, ((y + N - 1) % N) * N + x, r],
                    axis=1)
    ph = phi * y.astype(np.float64)
    vals = np.stack([-np.cos(ph) - 1j * np.sin(ph), -np.cos(ph) + 1j * np.sin(ph), np.full(n_local, -1.0 + 0j),
                     np.full(n_local, -1.0 + 0j), (u01(r.astype(np.uint64)) - 0.5) + 0j], axis=1)
    order = np.argsort(cols, axis=1, kind="stable")
    cols = np.take_along_axis(cols, order, axis=1)
    vals = np.take_along_axis(vals, order, axis=1)
    rp = (5 * np.arange(n_local + 1)).astype(np.int64)
    return rp, cols.reshape(-1).astype(np.int32), vals.reshape(-1)


def dense_to_csr(a):
    """All entries of a small dense matrix as CSR (zeros included, like the reference's dense test lambdas)."""
    a = np.asarray(a)
    n = a.shape[0]
    rp = (n * np.arange(n + 1)).astype(np.int64)
    ci = np.tile(np.arange(n, dtype=np.int32), n)
    return rp, ci, np.ascontiguousarray(a.reshape(-1))


def coo_to_csr(n, rows, cols, vals):
    """{r, c, value} triplets (sample2_sparse.cpp:14-47) to CSR, stable in input order within a row."""
    rows = np.asarray(rows, dtype=np.int64)
    order = np.argsort(rows, kind="stable")
    rp = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rp, rows + 1, 1)
    return np.cumsum(rp), np.asarray(cols, dtype=np.int32)[order], np.asarray(vals)[order]


def ring_csr(n, t=-1.0, dtype=np.float64):
    """Periodic 1-D chain with hopping t (T1:493-501, T2:113-121)."""
    r = np.arange(n)
    cols = np.stack([(r - 1) % n, (r + 1) % n], axis=1)
    cols.sort(axis=1)
    return (2 * np.arange(n + 1)).astype(np.int64), cols.reshape(-1).astype(np.int32), np.full(2 * n, t, dtype=dtype)


def chain_csr(n, t=-1.0):
    """Open 1-D chain (sample3_dynamic.cpp:17-22, T1:265-273)."""
    rows, cols = [], []
    for i in range(n - 1):
        rows += [i, i + 1]
        cols += [i + 1, i]
    return coo_to_csr(n, rows, cols, np.full(len(rows), t))


def lattice_csr(dims, diag=0.0, hop=-1.0, periodic=False, onsite=None, dtype=np.float64, row_begin=0, n_local=None,
                phase_grad=None):
    """CSR image of the matrix-free lattice operator (ll_op_create_stencil_*): rows [row_begin, row_begin+n_local),
    entries in the operator's own order (lower neighbours slowest dimension first, diagonal, upper neighbours fastest
    first); a neighbour reached twice (periodic dimension of length 1 or 2) appears twice."""
    dims = [int(d) for d in np.atleast_1d(dims)]
    nd = len(dims)
    hop = np.broadcast_to(np.asarray(hop, dtype=np.complex128), (nd,))
    periodic = np.broadcast_to(np.asarray(periodic, dtype=bool), (nd,))
    n = int(np.prod(dims))
    n_local = n - row_begin if n_local is None else n_local
    r = np.arange(row_begin, row_begin + n_local, dtype=np.int64)
    coords = list(np.unravel_index(r, dims))
    strides = [int(np.prod(dims[k + 1:])) for k in range(nd)]
    cols, vals, have = [], [], []

    pg = None if phase_grad is None else np.asarray(phase_grad, dtype=np.float64).reshape(nd, nd)

    def neighbour(k, sign):
        c = coords[k] + sign
        ok = (c >= 0) & (c < dims[k])
        if periodic[k]:
            c, ok = c % dims[k], np.ones_like(ok)
        cols.append(r + (c - coords[k]) * strides[k])
        t = np.full(n_local, hop[k])
        if pg is not None and np.any(pg[k] != 0):   # Peierls phase taken at the bond's LOWER site
            low = [cc.copy() for cc in coords]
            if sign < 0:
                low[k] = c
            t = t * np.exp(1j * sum(pg[k, e] * low[e] for e in range(nd)))
        vals.append(np.conj(t) if sign < 0 else t)
        have.append(ok)

    for k in range(nd):
        neighbour(k, -1)
    cols.append(r.copy())
    vals.append(np.full(n_local, diag, dtype=np.complex128) + (0 if onsite is None else np.asarray(onsite)))
    have.append(np.ones(n_local, dtype=bool))
    for k in range(nd - 1, -1, -1):
        neighbour(k, +1)
    cols, vals, have = np.stack(cols, 1), np.stack(vals, 1), np.stack(have, 1)
    rp = np.concatenate([[0], np.cumsum(have.sum(1))]).astype(np.int64)
    va = vals[have]
    if not np.issubdtype(np.dtype(dtype), np.complexfloating):
        va = va.real
    return rp, cols[have].astype(np.int32), np.ascontiguousarray(va.astype(dtype))


# ------------------------------------------------------------------ spin-1/2 Hamiltonians as sums of Pauli strings
# A term is (x_mask, z_mask, coef): site j carries X (x bit only), Z (z bit only), Y (both); bit j of a basis state is site j
# (include/lanczos_hip.h, ll_op_create_pauli_*).
def heisenberg_terms(L, J=1.0, delta=1.0, periodic=True):
    """XXZ chain J sum_j (Sx Sx + Sy Sy + delta Sz Sz)_{j, j+1} on L spins 1/2 (S = sigma / 2): three terms per bond."""
    terms = []
    for j in range(L if periodic and L > 2 else L - 1):
        m = (1 << j) | (1 << ((j + 1) % L))
        terms += [(m, 0, 0.25 * J), (m, m, 0.25 * J), (0, m, 0.25 * J * delta)]
    return terms


def tfim_terms(L, J, h, periodic=False):
    """Transverse-field Ising chain -J sum_j Z_j Z_{j+1} - h sum_j X_j (Pauli matrices)."""
    terms = [(0, (1 << j) | (1 << ((j + 1) % L)), -float(J)) for j in range(L if periodic and L > 2 else L - 1)]
    return terms + [(1 << j, 0, -float(h)) for j in range(L)]


def xyz_terms(L, jx, jy, jz, periodic=True):
    """XYZ chain sum_j (jx X_j X_{j+1} + jy Y_j Y_{j+1} + jz Z_j Z_{j+1}) (Pauli matrices): three terms per bond; real symmetric;
    conserves S_z only where jx = jy."""
    terms = []
    for j in range(L if periodic and L > 2 else L - 1):
        a = (1 << j) | (1 << ((j + 1) % L))
        terms += [(a, 0, float(jx)), (a, a, float(jy)), (0, a, float(jz))]
    return terms


def tfim_ground_energy(L, J, h):
    """Exact ground-state energy of the OPEN transverse-field Ising chain: minus the sum of the singular values of the
    L x L matrix with h on the diagonal and J on the superdiagonal (free fermions)."""
    return -float(np.sum(np.linalg.svd(np.diag(np.full(L, float(h))) + np.diag(np.full(L - 1, float(J)), 1), compute_uv=False)))


def tfim_ring_ground_energy(L, J, h):
    """Exact ground-state energy of the transverse-field Ising RING -J sum Z_j Z_{j+1} - h sum X_j (J, h > 0, L even): the vacuum
    of the even fermion-parity sector, minus the sum over k = (2 n + 1) pi / L of sqrt(J^2 + h^2 + 2 J h cos k)."""
    k = (2 * np.arange(int(L)) + 1) * np.pi / int(L)
    return -float(np.sum(np.sqrt(float(J) ** 2 + float(h) ** 2 + 2.0 * float(J) * float(h) * np.cos(k))))


def _parity(v):
    """popcount(v) mod 2, element-wise (uint64 arrays)."""
    v = v.copy()
    for sh in (32, 16, 8, 4, 2, 1):
        v ^= v >> np.uint64(sh)
    return (v & np.uint64(1)).astype(np.int64)


def _popcount(v):
    """popcount(v), element-wise (uint64 arrays below 2^32)."""
    v = v - ((v >> np.uint64(1)) & np.uint64(0x55555555))
    v = (v & np.uint64(0x33333333)) + ((v >> np.uint64(2)) & np.uint64(0x33333333))
    v = (v + (v >> np.uint64(4))) & np.uint64(0x0F0F0F0F)
    return ((v * np.uint64(0x01010101)) >> np.uint64(24)) & np.uint64(0xFF)


def pauli_csr(n_sites, terms, dtype=np.float64, merge=True, states=None):
    """The matrix of H = sum_t coef_t P_t as CSR, by the definition: row s holds coef_t i^nY_t (-1)^popcount((s ^ x_t) & z_t) in
    column s ^ x_t.  merge=True: one entry per row and distinct x mask (masks ascending; the coefficients summed in list
    order, exact zeros dropped).  merge=False: one entry per term and state, in list order, duplicate columns allowed — every
    term's own magnitude stays visible to an error bound.  states (None: all 2^n_sites): the rows of these states only, in the
    order given (row k of the result is the row of states[k]; the columns stay state numbers) — rings whose whole matrix does
    not fit."""
    if states is None:
        s = np.arange(1 << int(n_sites), dtype=np.uint64)
    else:
        s = np.ascontiguousarray(states).astype(np.uint64).reshape(-1)
        if s.size and int(s.max()) >> int(n_sites):
            raise ValueError("a state at or above 2^n_sites")
    return _pauli_rows(s, terms, dtype, merge, None)


def _pauli_rows(s, terms, dtype, merge, column_of):
    """pauli_csr for the rows of the states s (uint64).  column_of (None: the partner state itself) maps an array of partner
    states to (column numbers, entries to keep) or to (column numbers, entries to keep, a factor of each entry in double)."""
    n = s.shape[0]
    dtype = np.dtype(dtype)
    cplx = dtype.kind == "c"
    terms = [(int(x), int(z), float(c)) for x, z, c in terms]
    phase = (1.0, 1j, -1.0, -1j)

    def column(x, z, c):
        ny = bin(x & z).count("1")
        if not cplx and ny & 1:
            raise ValueError("a term with an odd number of Y needs a complex dtype")
        p = phase[ny & 3] * c
        sign = 1.0 - 2.0 * _parity((s ^ np.uint64(x)) & np.uint64(z))
        return (sign * p if cplx else sign * p.real).astype(dtype)

    def partners(masks):
        if not masks:
            return np.zeros((n, 0), np.int32), np.ones((n, 0), bool), None
        if column_of is None:
            return np.stack([(s ^ np.uint64(x)).astype(np.int32) for x in masks], 1), np.ones((n, len(masks)), bool), None
        both = [column_of(s ^ np.uint64(x)) for x in masks]
        factor = np.stack([b[2] for b in both], 1) if len(both[0]) > 2 else None
        return np.stack([b[0].astype(np.int32) for b in both], 1), np.stack([b[1] for b in both], 1), factor

    def scaled(vals, factor):
        if factor is None:
            return vals
        return vals * (factor if cplx else factor.real)

    if merge:
        groups = {}
        for x, z, c in terms:
            groups.setdefault(x, []).append((z, c))
        masks = sorted(groups)
        vals = np.zeros((n, len(masks)), dtype=np.complex128 if cplx else np.float64)
        for k, x in enumerate(masks):
            for z, c in groups[x]:
                vals[:, k] += column(x, z, c)
        cols, inside, factor = partners(masks)
        vals = scaled(vals, factor).astype(dtype)
        keep = (vals != 0) & inside
        rp = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64)
        return rp, np.ascontiguousarray(cols[keep]), np.ascontiguousarray(vals[keep])
    T = len(terms)
    vals = np.stack([column(*t) for t in terms], 1) if T else np.zeros((n, 0), dtype)
    cols, inside, factor = partners([x for x, _, _ in terms])
    vals = scaled(vals, factor).astype(dtype)
    if column_of is None:
        rp = (np.arange(n + 1, dtype=np.int64) * T)
        return rp, np.ascontiguousarray(cols.reshape(-1)), np.ascontiguousarray(vals.reshape(-1))
    rp = np.concatenate([[0], np.cumsum(inside.sum(1))]).astype(np.int64)
    return rp, np.ascontiguousarray(cols[inside]), np.ascontiguousarray(vals[inside])


def dm_terms(L, D=1.0, periodic=True):
    """Dzyaloshinskii-Moriya chain D sum_j (X_j Y_{j+1} - Y_j X_{j+1}) (Pauli matrices): complex Hermitian, conserves S_z."""
    terms = []
    for j in range(L if periodic and L > 2 else L - 1):
        a, b = 1 << j, 1 << ((j + 1) % L)
        terms += [(a | b, b, float(D)), (a | b, a, -float(D))]
    return terms


def zfield_terms(L, h):
    """Uniform field along z, -h sum_j Z_j (Pauli matrices): diagonal, shifts a sector by -h (L - 2 n_down)."""
    return [(0, 1 << j, -float(h)) for j in range(L)]


# ------------------------------------------------------------------ one magnetisation (S_z) sector
# The states with n_down set bits (a set bit is sigma_z = -1) in ascending integer order (ll_op_create_pauli_sector_*).
def sector_states(n_sites, n_down):
    """The comb(n_sites, n_down) states with n_down set bits, ascending, as uint32."""
    n_sites, n_down = int(n_sites), int(n_down)
    if not 0 <= n_down <= n_sites <= 32:
        raise ValueError("need 0 <= n_down <= n_sites <= 32")
    out = np.zeros(1, dtype=np.uint32)   # the states on the first p sites, by number of set bits
    by_count = [out] + [np.zeros(0, np.uint32)] * n_down
    for p in range(n_sites):
        bit = np.uint32(1 << p)
        for m in range(min(p + 1, n_down), 0, -1):   # states on p + 1 sites with m set bits: bit p clear first, then set
            keep = by_count[m] if n_sites - (p + 1) >= n_down - m else by_count[m][:0]
            by_count[m] = np.concatenate([keep, by_count[m - 1] | bit])
        if n_sites - (p + 1) < n_down:   # too few sites left to reach n_down from here
            by_count[0] = by_count[0][:0]
    return by_count[n_down]


def sector_rank_tables(n_sites, n_down, h):
    """(lo_rank, hi_rank), uint32 of 2^h and 2^(n_sites - h) entries: the index of a state s of the sector in sector_states is
    lo_rank[s & (2^h - 1)] + hi_rank[s >> h].  With the set bits of s at p_1 < ... < p_m the index is sum_k comb(p_k, k): the
    low bits count k from 1, the others from n_down - popcount(others) + 1.  Entries no state of the sector reaches are 0."""
    n_sites, n_down, h = int(n_sites), int(n_down), int(h)
    if not 0 <= h <= n_sites:
        raise ValueError("need 0 <= h <= n_sites")
    binom = np.array([[math.comb(p, k) for k in range(n_sites + 2)] for p in range(n_sites + 1)], dtype=np.uint64)

    def share(width, first_site, below):
        """sum over the set bits p of v < 2^width of comb(first_site + p, k), k counting on from below(popcount(v)); 0 where
        below is negative (no such state in the sector)."""
        v = np.arange(1 << width, dtype=np.int64)
        bits = [(v >> p) & 1 for p in range(width)]
        k = below(sum(bits) if bits else np.zeros_like(v))
        ok = (k >= 0) & (k <= n_down)
        k, r = np.where(ok, k, 0), np.zeros(1 << width, dtype=np.uint64)
        for p in range(width):
            k = k + bits[p]
            r += np.where((bits[p] == 1) & ok & (k <= n_down), binom[first_site + p, np.minimum(k, n_sites + 1)], np.uint64(0))
        return r.astype(np.uint32)

    lo = share(h, 0, lambda pc: np.where(pc <= n_down, 0, -1))
    hi = share(n_sites - h, h, lambda pc: np.where(n_down - pc <= h, n_down - pc, -1))
    return lo, hi


def pauli_sector_csr(n_sites, n_down, terms, dtype=np.float64, merge=True):
    """The block of pauli_csr(n_sites, terms, dtype, merge) on the rows and columns of the sector (n_sites, n_down), columns
    renumbered by position in sector_states; entries whose column leaves the sector are dropped (exact zeros for an H that
    conserves S_z once merged; with merge=False the single terms that cancel there).  Only the sector's rows are formed."""
    n_sites, n_down = int(n_sites), int(n_down)
    states = sector_states(n_sites, n_down).astype(np.uint64)
    h = (n_sites + 1) // 2
    lo, hi = sector_rank_tables(n_sites, n_down, h)

    def column_of(p):
        inside = _popcount(p) == n_down
        q = np.where(inside, p, states[0])
        return lo[q & np.uint64((1 << h) - 1)].astype(np.int64) + hi[q >> np.uint64(h)], inside

    return _pauli_rows(states, terms, dtype, merge, column_of)


def pauli_string_apply_np(n_sites, term, psi, states=None):
    """P psi for the Pauli string P of term = (x_mask, z_mask, coef), formed exactly — a permutation, a sign and i^nY; the
    coefficient plays no part: (P psi)(r) = i^nY (-1)^popcount((r ^ x) & z) psi(r ^ x).  states (None: psi on all 2^n_sites
    states): psi on these states, ascending and with one popcount (sector_states); a partner r ^ x outside them contributes 0.
    The result has psi's dtype for an even nY and the complex dtype of psi's precision for an odd one."""
    x, z = int(term[0]), int(term[1])
    psi = np.asarray(psi).reshape(-1)
    if states is None:
        r = np.arange(1 << int(n_sites), dtype=np.uint64)
    else:
        r = np.ascontiguousarray(states).astype(np.uint64).reshape(-1)
    if psi.shape[0] != r.shape[0]:
        raise ValueError("psi holds %d values for %d states" % (psi.shape[0], r.shape[0]))
    if (x | z) >> int(n_sites):
        raise ValueError("a mask bit at or above n_sites")
    p = r ^ np.uint64(x)
    if states is None:
        src, inside = p.astype(np.int64), None
    else:
        src = np.minimum(np.searchsorted(r, p), max(r.shape[0] - 1, 0))
        inside = r[src] == p if r.shape[0] else np.zeros(0, bool)
    q = psi[src] if r.shape[0] else psi.copy()
    q = np.where(_parity(p & np.uint64(z)) == 1, -q, q)
    if inside is not None:
        q = np.where(inside, q, np.zeros((), q.dtype))
    ny = bin(x & z).count("1") & 3
    if ny & 1:   # times i (nY = 1) or -i (nY = 3): the parts swap, exactly
        cq = q.astype(np.result_type(q.dtype, np.complex64))
        q = (-cq.imag + 1j * cq.real) if ny == 1 else (cq.imag - 1j * cq.real)
        q = q.astype(cq.dtype)
    elif ny == 2:
        q = -q
    return q


def reduced_density_matrix_np(n_sites, sites, psi, states=None):
    """(rho, fibres): rho[a][a'] = sum_e psi(a, e) conj psi(a', e) in complex128 — the plain host restatement of ll_pauli_rdm —
    and fibres, the array of shape (2^m, 2^(n_sites - m)) with fibres[a][e] = psi(a, e) in psi's dtype: bit k of a is site
    sites[k], the bits of e fill the other sites in ascending order.  states (None: psi on all 2^n_sites states): psi on these
    states, ascending and with one popcount (sector_states); an (a, e) outside them is 0.  rho = fibres @ fibres^H, its upper triangle mirrored."""
    sites = [int(s) for s in sites]
    m, n_sites = len(sites), int(n_sites)
    if not 1 <= m <= n_sites or len(set(sites)) != m or min(sites) < 0 or max(sites) >= n_sites:
        raise ValueError("sites must be 1 to n_sites distinct sites in [0, n_sites)")
    psi = np.asarray(psi).reshape(-1)
    full = psi
    if states is not None:
        st = np.ascontiguousarray(states).astype(np.int64).reshape(-1)
        if psi.shape[0] != st.shape[0]:
            raise ValueError("psi holds %d values for %d states" % (psi.shape[0], st.shape[0]))
        full = np.zeros(1 << n_sites, dtype=psi.dtype)
        full[st] = psi
    elif psi.shape[0] != 1 << n_sites:
        raise ValueError("psi holds %d values for %d states" % (psi.shape[0], 1 << n_sites))
    env = [s for s in range(n_sites) if s not in sites]
    a = np.arange(1 << m, dtype=np.int64)
    e = np.arange(1 << (n_sites - m), dtype=np.int64)
    sa = np.zeros_like(a)
    for k, s in enumerate(sites):
        sa |= ((a >> k) & 1) << s
    se = np.zeros_like(e)
    for k, s in enumerate(env):
        se |= ((e >> k) & 1) << s
    fibres = full[sa[:, None] | se[None, :]]
    wide = fibres.astype(np.complex128)
    rho = wide @ wide.conj().T
    rho = np.triu(rho, 1) + np.triu(rho, 1).conj().T + np.diag(rho.diagonal().real)   # Hermitian bit for bit
    return rho, fibres


# ------------------------------------------------------------------ one momentum block of an S_z sector of a ring
# T rotates a state left by one bit (site j -> j + 1 mod L); the representative of an orbit {T^j s} is its smallest integer; block
# m holds the representatives whose orbit length R satisfies m R = 0 (mod L), ascending (ll_op_create_pauli_momentum_*).
def _orbits(n_sites, n_down):
    """For every state s of sector_states(n_sites, n_down): (states, its representative b, l with s = T^l b and 0 <= l < R, R)."""
    return _orbits_of(int(n_sites), sector_states(int(n_sites), n_down).astype(np.uint64))


def _orbits_of(L, states):
    """_orbits for any array of states (uint64) that is closed under the rotation: L - 1 rotations of the whole array."""
    mask = np.uint64((1 << L) - 1)
    rep, first = states.copy(), np.zeros(states.shape[0], np.int64)    # min over the rotations, the first j with T^j s = min
    period = np.full(states.shape[0], L, np.int64)
    cur = states.copy()
    for j in range(1, L):
        cur = ((cur << np.uint64(1)) | (cur >> np.uint64(L - 1))) & mask
        period = np.where((cur == states) & (period == L), j, period)
        less = cur < rep
        rep, first = np.where(less, cur, rep), np.where(less, j, first)
    return states, rep, (period - first) % period, period


def _momentum_phases(n_sites, m):
    """e^(-2 pi i m l / n_sites) for l = 0 .. n_sites - 1 in double, exact where it lies on an axis."""
    L = int(n_sites)
    k = (int(m) * np.arange(L, dtype=np.int64)) % L
    ph = np.exp(-2j * np.pi * k / L)
    axis = (4 * k) % L == 0
    ph[axis] = np.array([1.0, -1j, -1.0, 1j])[(4 * k[axis]) // L]
    return ph


def _check_momentum(n_sites, n_down, m):
    n_sites, n_down, m = int(n_sites), int(n_down), int(m)
    if not (1 <= n_sites <= 30 and 0 <= n_down <= n_sites and 0 <= m < n_sites):
        raise ValueError("need 1 <= n_sites <= 30, 0 <= n_down <= n_sites, 0 <= m < n_sites")
    return n_sites, n_down, m


def momentum_basis(n_sites, n_down, m):
    """(representatives, periods) of block m of the sector: the representatives r (uint32, ascending) with m R_r = 0 (mod n_sites)
    and their orbit lengths R_r (int64)."""
    n_sites, n_down, m = _check_momentum(n_sites, n_down, m)
    states, rep, _, period = _orbits(n_sites, n_down)
    inb = (states == rep) & ((m * period) % n_sites == 0)
    return states[inb].astype(np.uint32), period[inb]


def momentum_embedding(n_sites, n_down, m, dense=True):
    """B: the basis vectors |r; m> = N_r^(-1/2) sum_j e^(-2 pi i m j / L) T^j |r>, N_r = L^2 / R_r, as the columns of a
    comb(n_sites, n_down) x D_m matrix in the sector_states basis (an isometry).  A row holds at most one entry,
    e^(-2 pi i m l / L) / sqrt(R) for the state T^l r: dense=False returns (column of each row or -1, its value)."""
    n_sites, n_down, m = _check_momentum(n_sites, n_down, m)
    states, rep, l, period = _orbits(n_sites, n_down)
    inb = (m * period) % n_sites == 0
    reps = states[(states == rep) & inb]
    col = np.where(inb, np.searchsorted(reps, rep), -1).astype(np.int64)
    val = np.where(inb, _momentum_phases(n_sites, m)[l] / np.sqrt(period.astype(np.float64)), 0.0)
    if not dense:
        return col, val
    B = np.zeros((states.shape[0], reps.shape[0]), np.complex128)
    B[np.flatnonzero(inb), col[inb]] = val[inb]
    return B


def translation_fault(n_sites, terms):
    """None when H = sum of `terms` commutes with the one-site translation of the ring by the rule of
    ll_op_create_pauli_momentum_* (coefficients of equal masks merged in list order; the masks rotated by one site meet exactly
    the same coefficient, a missing term counting as 0); else the number of the first term at fault."""
    L = int(n_sites)
    full = (1 << L) - 1

    def rot(v):
        return ((v << 1) | (v >> (L - 1))) & full

    merged = {}
    for x, z, c in terms:
        merged[(int(x), int(z))] = merged.get((int(x), int(z)), 0.0) + float(c)
    for t, (x, z, _) in enumerate(terms):
        if merged.get((rot(int(x)), rot(int(z))), 0.0) != merged[(int(x), int(z))]:
            return t
    return None


def pauli_momentum_csr(n_sites, n_down, m, terms, dtype=np.float64, merge=True):
    """The block B^H H_sector B (B = momentum_embedding, H_sector = pauli_sector_csr) as CSR over momentum_basis, from the gather
    form, in double: row a holds, per x mask X whose partner a ^ X = T^l b stays in the sector with b in the block,
    w(a) sqrt(R_a / R_b) e^(-2 pi i m l / L) in the column of b, w as in pauli_csr.  merge as in pauli_sector_csr (merge=False:
    one entry per term and state).  A real dtype needs 2 m = 0 (mod n_sites); H must commute with the translation."""
    n_sites, n_down, m = _check_momentum(n_sites, n_down, m)
    terms = list(terms)
    if np.dtype(dtype).kind != "c" and (2 * m) % n_sites:
        raise ValueError("a real dtype takes m = 0 and m = n_sites / 2 only")
    t = translation_fault(n_sites, terms)
    if t is not None:
        raise ValueError("term %d (x_mask 0x%x, z_mask 0x%x) does not commute with the one-site translation"
                         % (t, terms[t][0], terms[t][1]))
    states, rep, l, period = _orbits(n_sites, n_down)
    inb = (m * period) % n_sites == 0
    isrep = (states == rep) & inb
    reps = states[isrep]
    col = np.where(inb, np.searchsorted(reps, rep), 0).astype(np.int64)
    phases = _momentum_phases(n_sites, m)
    h = (n_sites + 1) // 2
    lo, hi = sector_rank_tables(n_sites, n_down, h)
    ra = period[isrep].astype(np.float64)

    def column_of(p):
        inside = _popcount(p) == n_down
        q = np.where(inside, p, states[0])
        k = lo[q & np.uint64((1 << h) - 1)].astype(np.int64) + hi[q >> np.uint64(h)]
        return col[k], inside & inb[k], np.sqrt(ra / period[k]) * phases[l[k]]

    return _pauli_rows(reps, terms, dtype, merge, column_of)


# ------------------------------------------------------------------ one momentum block of the full 2^n_sites space of a ring
# The conventions above without the sector: block m holds the representatives of ALL states whose orbit length R satisfies
# m R = 0 (mod L), ascending (ll_op_create_pauli_momentum_full_*); H need not conserve S_z.
def _check_full_momentum(n_sites, m):
    n_sites, m = int(n_sites), int(m)
    if not (1 <= n_sites <= 30 and 0 <= m < n_sites):
        raise ValueError("need 1 <= n_sites <= 30, 0 <= m < n_sites")
    return n_sites, m


def _orbits_full(n_sites):
    return _orbits_of(n_sites, np.arange(1 << n_sites, dtype=np.uint64))


def full_momentum_basis(n_sites, m):
    """(representatives, periods) of block m of the full space: the representatives r (uint32, ascending) of all 2^n_sites states
    with m R_r = 0 (mod n_sites) and their orbit lengths R_r (int64)."""
    n_sites, m = _check_full_momentum(n_sites, m)
    states, rep, _, period = _orbits_full(n_sites)
    inb = (states == rep) & ((m * period) % n_sites == 0)
    return states[inb].astype(np.uint32), period[inb]


def full_momentum_embedding(n_sites, m, dense=True):
    """B: the basis vectors |r; m> = N_r^(-1/2) sum_j e^(-2 pi i m j / L) T^j |r>, N_r = L^2 / R_r, as the columns of a
    2^n_sites x D_m matrix (an isometry).  A row holds at most one entry, e^(-2 pi i m l / L) / sqrt(R) for the state T^l r:
    dense=False returns (column of each row or -1, its value)."""
    n_sites, m = _check_full_momentum(n_sites, m)
    states, rep, l, period = _orbits_full(n_sites)
    inb = (m * period) % n_sites == 0
    reps = states[(states == rep) & inb]
    col = np.where(inb, np.searchsorted(reps, rep), -1).astype(np.int64)
    val = np.where(inb, _momentum_phases(n_sites, m)[l] / np.sqrt(period.astype(np.float64)), 0.0)
    if not dense:
        return col, val
    B = np.zeros((states.shape[0], reps.shape[0]), np.complex128)
    B[np.flatnonzero(inb), col[inb]] = val[inb]
    return B


def pauli_momentum_full_csr(n_sites, m, terms, dtype=np.float64, merge=True):
    """The block B^H H B (B = full_momentum_embedding, H = pauli_csr) as CSR over full_momentum_basis, from the gather form, in
    double: row a holds, per x mask X whose partner a ^ X = T^l b has b in the block, w(a) sqrt(R_a / R_b) e^(-2 pi i m l / L) in
    the column of b, w as in pauli_csr.  merge as in pauli_csr (merge=False: one entry per term and state).  A real dtype needs
    2 m = 0 (mod n_sites); H must commute with the translation (it need not conserve S_z)."""
    n_sites, m = _check_full_momentum(n_sites, m)
    terms = list(terms)
    if np.dtype(dtype).kind != "c" and (2 * m) % n_sites:
        raise ValueError("a real dtype takes m = 0 and m = n_sites / 2 only")
    t = translation_fault(n_sites, terms)
    if t is not None:
        raise ValueError("term %d (x_mask 0x%x, z_mask 0x%x) does not commute with the one-site translation"
                         % (t, terms[t][0], terms[t][1]))
    states, rep, l, period = _orbits_full(n_sites)
    inb = (m * period) % n_sites == 0
    isrep = (states == rep) & inb
    reps = states[isrep]
    col = np.where(inb, np.searchsorted(reps, rep), 0).astype(np.int64)
    phases = _momentum_phases(n_sites, m)
    ra = period[isrep].astype(np.float64)

    def column_of(p):
        k = p.astype(np.int64)   # the state is its own number: no sector to leave
        return col[k], inb[k], np.sqrt(ra / period[k]) * phases[l[k]]

    return _pauli_rows(reps, terms, dtype, merge, column_of)


# ------------------------------------------------------------------ momentum + reflection + spin-inversion blocks of a ring
# The conventions above with two more symmetries of the ring: P reverses the n_sites bits (site j -> L - 1 - j), Z flips every
# spin (s -> ~s & (2^L - 1)).  The group G is generated by T, by P if parity != 0 and by Z if inversion != 0 (|G| = L, 2 L or
# 4 L elements T^j P^rho Z^zeta); its character is e^(-2 pi i m j / L) parity^rho inversion^zeta.  The representative of a G-orbit
# is its smallest integer; it is in the block iff the character is 1 on its stabiliser (ll_op_create_pauli_symmetric_*).
def _check_symmetric(n_sites, m, parity, inversion, n_down):
    n_sites, m, parity, inversion = int(n_sites), int(m), int(parity), int(inversion)
    n_down = None if n_down is None or int(n_down) < 0 else int(n_down)
    if not (1 <= n_sites <= 30 and 0 <= m < n_sites):
        raise ValueError("need 1 <= n_sites <= 30, 0 <= m < n_sites")
    if parity not in (0, 1, -1) or inversion not in (0, 1, -1):
        raise ValueError("parity and inversion must be 0, +1 or -1")
    if parity and (2 * m) % n_sites:
        raise ValueError("a reflection block needs m = 0 or m = n_sites / 2")
    if n_down is not None and not 0 <= n_down <= n_sites:
        raise ValueError("need 0 <= n_down <= n_sites")
    if n_down is not None and inversion and 2 * n_down != n_sites:
        raise ValueError("spin inversion maps the sector n_down onto n_sites - n_down: it needs 2 n_down = n_sites")
    return n_sites, m, parity, inversion, n_down


def _bit_reverse(L, v):
    """The L low bits of v (uint64 array) in reverse order."""
    out = np.zeros_like(v)
    for j in range(L):
        out |= ((v >> np.uint64(j)) & np.uint64(1)) << np.uint64(L - 1 - j)
    return out


def _orbits_symmetric(L, states, m, parity, inversion):
    """For every state s of `states` (uint64, closed under G): (its representative b, l and sign with s = g b and
    chi(g) = e^(-2 pi i m l / L) sign, the orbit length R = |G| / |stabiliser|, whether chi = 1 on the stabiliser).  4 L passes
    over the array at most."""
    mask = np.uint64((1 << L) - 1)
    n = states.shape[0]
    rep = np.full(n, mask + np.uint64(1), np.uint64)
    first, sign = np.zeros(n, np.int64), np.ones(n, np.float64)
    stab = np.zeros(n, np.int64)
    admitted = np.ones(n, bool)
    order = 0
    for rho in ((0, 1) if parity else (0,)):
        for zeta in ((0, 1) if inversion else (0,)):
            cur = _bit_reverse(L, states) if rho else states.copy()
            if zeta:
                cur ^= mask
            sg = (parity if rho else 1) * (inversion if zeta else 1)
            for j in range(L):                       # cur = T^j P^rho Z^zeta s
                if j:
                    cur = ((cur << np.uint64(1)) | (cur >> np.uint64(L - 1))) & mask
                # the character of this element in units of pi / L: 2 m j, plus L for a factor -1
                angle = (2 * m * j + (L if sg < 0 else 0)) % (2 * L)
                fixed = cur == states
                stab += fixed
                if angle:
                    admitted &= ~fixed
                less = cur < rep
                rep = np.where(less, cur, rep)
                first = np.where(less, j, first)
                sign = np.where(less, float(sg), sign)
                order += 1
    # s = h^-1 b with h = T^first P^rho Z^zeta the first minimiser: chi(h^-1) = e^(-2 pi i m (L - first) / L) sign
    return rep, (L - first) % L, sign, order // stab, admitted


def _symmetric_states(n_sites, n_down):
    if n_down is None:
        return np.arange(1 << n_sites, dtype=np.uint64)
    return sector_states(n_sites, n_down).astype(np.uint64)


def _symmetric_orbits(n_sites, m, parity, inversion, n_down):
    """(states, rep, l, sign, R, in the block) over the full space or the sector; admission is a property of the orbit."""
    states = _symmetric_states(n_sites, n_down)
    rep, l, sign, R, adm = _orbits_symmetric(n_sites, states, m, parity, inversion)
    return states, rep, l, sign, R, adm


def symmetric_basis(n_sites, m, parity, inversion, n_down=None):
    """(representatives, orbit lengths) of the block (m, parity, inversion) of the full space (n_down None) or of the sector
    n_down: the representatives r (uint32, ascending) of the G-orbits on whose stabiliser the character is 1, and R_r (int64).
    With parity = inversion = 0 and n_down None this is full_momentum_basis."""
    n_sites, m, parity, inversion, n_down = _check_symmetric(n_sites, m, parity, inversion, n_down)
    states, rep, _, _, R, adm = _symmetric_orbits(n_sites, m, parity, inversion, n_down)
    inb = (states == rep) & adm
    return states[inb].astype(np.uint32), R[inb]


def _symmetric_columns(n_sites, m, parity, inversion, n_down):
    """(states, in the block, column of each state's representative, chi(g) / sqrt(R) for s = g b, reps, R of the reps)."""
    states, rep, l, sign, R, adm = _symmetric_orbits(n_sites, m, parity, inversion, n_down)
    isrep = (states == rep) & adm
    reps = states[isrep]
    col = np.where(adm, np.searchsorted(reps, rep), 0).astype(np.int64)
    col = np.minimum(col, max(reps.shape[0] - 1, 0))
    chi = _momentum_phases(n_sites, m)[l] * sign
    return states, adm, col, chi, R, reps, R[isrep]


def symmetric_embedding(n_sites, m, parity, inversion, n_down=None, dense=True):
    """B: the basis vectors |r; chi> = N_r^(-1/2) sum_{g in G} chi(g) g |r> as the columns of a matrix over all 2^n_sites states
    (n_down None) or over sector_states(n_sites, n_down) — an isometry.  A row holds at most one entry, chi(g) / sqrt(R_b) for the
    state g b: dense=False returns (column of each row or -1, its value)."""
    n_sites, m, parity, inversion, n_down = _check_symmetric(n_sites, m, parity, inversion, n_down)
    states, adm, col, chi, R, reps, _ = _symmetric_columns(n_sites, m, parity, inversion, n_down)
    col = np.where(adm, col, -1)
    val = np.where(adm, chi / np.sqrt(R.astype(np.float64)), 0.0)
    if not dense:
        return col, val
    B = np.zeros((states.shape[0], reps.shape[0]), np.complex128)
    B[np.flatnonzero(adm), col[adm]] = val[adm]
    return B


def reflection_fault(n_sites, terms):
    """None when H = sum of `terms` commutes with the reflection j -> n_sites - 1 - j by the rule of
    ll_op_create_pauli_symmetric_* (coefficients of equal masks merged in list order; the bit-reversed masks meet exactly the same
    coefficient, a missing term counting as 0); else the number of the first term at fault."""
    L = int(n_sites)

    def rev(v):
        return int(format(v, "0%db" % L)[::-1], 2)

    merged = {}
    for x, z, c in terms:
        merged[(int(x), int(z))] = merged.get((int(x), int(z)), 0.0) + float(c)
    for t, (x, z, _) in enumerate(terms):
        if merged.get((rev(int(x)), rev(int(z))), 0.0) != merged[(int(x), int(z))]:
            return t
    return None


def inversion_fault(n_sites, terms):
    """None when H = sum of `terms` commutes with the global spin flip prod_j X_j: after merging equal masks no term with an odd
    popcount(z_mask) (an odd number of Y and Z factors) keeps a non-zero coefficient; else the number of the first term at fault."""
    merged = {}
    for x, z, c in terms:
        merged[(int(x), int(z))] = merged.get((int(x), int(z)), 0.0) + float(c)
    for t, (x, z, _) in enumerate(terms):
        if bin(int(z)).count("1") & 1 and merged[(int(x), int(z))] != 0.0:
            return t
    return None


def symmetrised_strings(n_sites, term, parity=0, inversion=0):
    """The average of the string `term` = (x_mask, z_mask[, coef]) over the group G of a ring's symmetry block — the one-site shift
    always, the reflection iff parity != 0, the global flip iff inversion != 0 — as a list of (x_mask, z_mask, weight): the numpy
    mirror of csrc/pauli_expect_block_plan.hpp.  The |G| images (both masks rotated left / bit-reversed; the flip keeps the masks
    and gives the sign (-1)^popcount(z)) are merged by (x, z) with their signed multiplicities added as integers, cancelled
    strings dropped, the others weighted multiplicity / |G| and sorted by x mask, then z mask.  The coefficient of `term` is
    not in the weights; an empty list means the observable is identically zero on every state of such a block.  For a state
    Psi = B c of the block, <Psi| P |Psi> = c^H M c with M = pauli_symmetric_csr(..., symmetrised_strings(...), ...)."""
    L, x, z = int(n_sites), int(term[0]), int(term[1])
    mask = (1 << L) - 1
    if not 1 <= L <= 30 or (x | z) & ~mask:
        raise ValueError("need 1 <= n_sites <= 30 and masks below 2^n_sites")

    def rev(v):
        return int(format(v, "0%db" % L)[::-1], 2)

    def rot(v, j):
        return ((v << j) | (v >> (L - j))) & mask

    flip_sign = -1 if bin(z).count("1") & 1 else 1
    mult, order = {}, 0
    for bx, bz in (((x, z), (rev(x), rev(z))) if parity else ((x, z),)):
        for j in range(L):
            key = (rot(bx, j), rot(bz, j))
            mult[key] = mult.get(key, 0) + 1 + (flip_sign if inversion else 0)
            order += 2 if inversion else 1
    return [(kx, kz, mult[(kx, kz)] / order) for kx, kz in sorted(mult) if mult[(kx, kz)] != 0]


def pauli_symmetric_csr(n_sites, m, parity, inversion, terms, dtype=np.float64, n_down=None, merge=True):
    """The block B^H H B (B = symmetric_embedding; H = pauli_csr, or pauli_sector_csr with n_down) as CSR over symmetric_basis,
    from the gather form, in double: row a holds, per x mask X whose partner a ^ X = g b has b in the block,
    w(a) sqrt(R_a / R_b) chi(g) in the column of b, w as in pauli_csr.  merge as in pauli_csr (merge=False: one entry per term and
    state).  A real dtype and parity != 0 need 2 m = 0 (mod n_sites); H must commute with the symmetries in use."""
    n_sites, m, parity, inversion, n_down = _check_symmetric(n_sites, m, parity, inversion, n_down)
    terms = list(terms)
    if np.dtype(dtype).kind != "c" and (2 * m) % n_sites:
        raise ValueError("a real dtype takes m = 0 and m = n_sites / 2 only")
    for fault, what in ((translation_fault, "the one-site translation"), (reflection_fault if parity else None, "the reflection"),
                        (inversion_fault if inversion else None, "the global spin flip")):
        t = fault(n_sites, terms) if fault else None
        if t is not None:
            raise ValueError("term %d (x_mask 0x%x, z_mask 0x%x) does not commute with %s" % (t, terms[t][0], terms[t][1], what))
    states, adm, col, chi, R, reps, ra = _symmetric_columns(n_sites, m, parity, inversion, n_down)
    if reps.shape[0] == 0:
        raise ValueError("the block is empty")
    ra = ra.astype(np.float64)
    if n_down is not None:
        h = (n_sites + 1) // 2
        lo, hi = sector_rank_tables(n_sites, n_down, h)

    def column_of(p):
        if n_down is None:
            k = p.astype(np.int64)   # the state is its own number
            return col[k], adm[k], np.sqrt(ra / R[k]) * chi[k]
        inside = _popcount(p) == n_down
        q = np.where(inside, p, states[0])
        k = lo[q & np.uint64((1 << h) - 1)].astype(np.int64) + hi[q >> np.uint64(h)]
        return col[k], inside & adm[k], np.sqrt(ra / R[k]) * chi[k]

    return _pauli_rows(reps, terms, dtype, merge, column_of)


# ------------------------------------------------------------------ translation blocks of an Lx x Ly torus
# Site (x, y) is bit x + Lx y, n = Lx Ly <= 30.  T_x rotates each of the Ly fields of Lx bits left by one (site (x, y) ->
# (x + 1 mod Lx, y)), T_y rotates the n-bit word left by Lx bits (site (x, y) -> (x, y + 1 mod Ly)).  G = {T_x^a T_y^b}, the code of
# an element is a + Lx b, its character e^(-2 pi i (m_x a / Lx + m_y b / Ly)).  The representative of a G-orbit is its smallest
# integer; it is in the block iff the character is 1 on its stabiliser (ll_op_create_pauli_torus).
def _check_torus(lx, ly, mx, my, n_down):
    lx, ly, mx, my = int(lx), int(ly), int(mx), int(my)
    n_down = None if n_down is None or int(n_down) < 0 else int(n_down)
    if not (lx >= 1 and ly >= 1 and lx * ly <= 30):
        raise ValueError("need lx, ly >= 1 and lx * ly <= 30")
    if not (0 <= mx < lx and 0 <= my < ly):
        raise ValueError("need 0 <= mx < lx and 0 <= my < ly")
    if n_down is not None and not 0 <= n_down <= lx * ly:
        raise ValueError("need 0 <= n_down <= lx * ly")
    return lx, ly, mx, my, n_down


def _torus_tx(lx, ly, v):
    """T_x on a state or a mask: a Python int or a uint64 array."""
    col0 = sum(1 << (lx * y) for y in range(ly))
    keep = ((1 << (lx * ly)) - 1) & ~col0
    if isinstance(v, np.ndarray):
        return ((v << np.uint64(1)) & np.uint64(keep)) | ((v >> np.uint64(lx - 1)) & np.uint64(col0))
    return ((v << 1) & keep) | ((v >> (lx - 1)) & col0)


def _torus_ty(lx, ly, v):
    """T_y on a state or a mask: a Python int or a uint64 array."""
    n = lx * ly
    if isinstance(v, np.ndarray):
        return ((v << np.uint64(lx)) | (v >> np.uint64(n - lx))) & np.uint64((1 << n) - 1)
    return ((v << lx) | (v >> (n - lx))) & ((1 << n) - 1)


def torus_bonds(lx, ly, dx, dy):
    """The distinct unordered pairs {(x, y), (x + dx mod lx, y + dy mod ly)} of two different sites of the lx x ly torus, as
    sorted (site, site) tuples in ascending order, site (x, y) = x + lx y.  Deduplicated: lx = 2, dx = 1 gives one bond per
    pair, and a displacement that maps every site onto itself gives none."""
    lx, ly = int(lx), int(ly)
    pairs = set()
    for y in range(ly):
        for x in range(lx):
            a, b = x + lx * y, (x + int(dx)) % lx + lx * ((y + int(dy)) % ly)
            if a != b:
                pairs.add((min(a, b), max(a, b)))
    return sorted(pairs)


def heisenberg_torus_terms(lx, ly, j1=1.0, j2=0.0):
    """The J1-J2 Heisenberg model on the lx x ly torus, j1 sum S_i . S_j over the nearest-neighbour bonds (displacements (1, 0) and
    (0, 1)) + j2 sum over the diagonal ones ((1, 1) and (1, -1)), S = sigma / 2: three strings of 0.25 J per distinct bond, as
    heisenberg_terms; no j2 strings where j2 = 0.  Conserves S_z and commutes with both translations."""
    terms = []
    for J, steps in ((float(j1), ((1, 0), (0, 1))), (float(j2), ((1, 1), (1, -1)))):
        if J == 0.0 and steps[0] == (1, 1):
            continue
        for a, b in sorted(set(torus_bonds(lx, ly, *steps[0])) | set(torus_bonds(lx, ly, *steps[1]))):
            m = (1 << a) | (1 << b)
            terms += [(m, 0, 0.25 * J), (m, m, 0.25 * J), (0, m, 0.25 * J)]
    return terms


def tfim_torus_terms(lx, ly, J, h):
    """Transverse-field Ising model on the lx x ly torus, -J sum Z_i Z_j over the distinct nearest-neighbour bonds - h sum X_i
    (Pauli matrices)."""
    bonds = sorted(set(torus_bonds(lx, ly, 1, 0)) | set(torus_bonds(lx, ly, 0, 1)))
    return [(0, (1 << a) | (1 << b), -float(J)) for a, b in bonds] + [(1 << j, 0, -float(h)) for j in range(int(lx) * int(ly))]


def _torus_phases(lx, ly, mx, my):
    """chi(T_x^a T_y^b) = e^(-2 pi i (mx a ly + my b lx) / (lx ly)) by the code a + lx b, exact where it lies on an axis; with ly = 1
    (or lx = 1) _momentum_phases of the ring."""
    n = lx * ly
    code = np.arange(n, dtype=np.int64)
    k = (mx * (code % lx) * ly + my * (code // lx) * lx) % n
    ph = np.exp(-2j * np.pi * k / n)
    axis = (4 * k) % n == 0
    ph[axis] = np.array([1.0, -1j, -1.0, 1j])[(4 * k[axis]) // n]
    return ph


def _orbits_torus(lx, ly, states, mx, my):
    """For every state s of `states` (uint64, closed under G): (its representative b, the code l of g with s = g b, the orbit
    length R = |G| / |stabiliser|, whether the character is 1 on the stabiliser).  lx ly passes over the array, b outer, a inner."""
    n = lx * ly
    cnt = states.shape[0]
    rep = np.full(cnt, np.uint64(1 << n), np.uint64)
    first = np.zeros(cnt, np.int64)
    stab = np.zeros(cnt, np.int64)
    admitted = np.ones(cnt, bool)
    cur = states.copy()
    for b in range(ly):
        for a in range(lx):   # cur = T_x^a T_y^b s
            fixed = cur == states
            stab += fixed
            if (mx * a * ly + my * b * lx) % n:
                admitted &= ~fixed
            less = cur < rep
            rep = np.where(less, cur, rep)
            first = np.where(less, a + lx * b, first)
            cur = _torus_tx(lx, ly, cur)
        cur = _torus_ty(lx, ly, cur)
    # s = h^-1 b with h = T_x^a T_y^b the first minimiser: the code of h^-1
    fa, fb = first % lx, first // lx
    return rep, (lx - fa) % lx + lx * ((ly - fb) % ly), n // stab, admitted


def _torus_columns(lx, ly, mx, my, n_down):
    """(states, in the block, column of each state's representative, chi(g) for s = g b, R, reps, R of the reps)."""
    states = _symmetric_states(lx * ly, n_down)
    rep, l, R, adm = _orbits_torus(lx, ly, states, mx, my)
    isrep = (states == rep) & adm
    reps = states[isrep]
    col = np.where(adm, np.searchsorted(reps, rep), 0).astype(np.int64)
    col = np.minimum(col, max(reps.shape[0] - 1, 0))
    return states, adm, col, _torus_phases(lx, ly, mx, my)[l], R, reps, R[isrep]


def torus_basis(lx, ly, mx, my, n_down=None):
    """(representatives, orbit lengths) of the block (mx, my) of the full space (n_down None) or of the sector n_down of the
    lx x ly torus: the representatives r (uint32, ascending) of the orbits on whose stabiliser the character is 1, and R_r (int64).
    With ly = 1 this is symmetric_basis(lx, mx, 0, 0, n_down)."""
    lx, ly, mx, my, n_down = _check_torus(lx, ly, mx, my, n_down)
    _, _, _, _, _, reps, ra = _torus_columns(lx, ly, mx, my, n_down)
    return reps.astype(np.uint32), ra


def torus_embedding(lx, ly, mx, my, n_down=None, dense=True):
    """B: the basis vectors |r; mx my> = N_r^(-1/2) sum_{g in G} chi(g) g |r> as the columns of a matrix over all 2^(lx ly) states
    (n_down None) or over sector_states(lx ly, n_down) — an isometry.  A row holds at most one entry, chi(g) / sqrt(R_b) for the
    state g b: dense=False returns (column of each row or -1, its value)."""
    lx, ly, mx, my, n_down = _check_torus(lx, ly, mx, my, n_down)
    states, adm, col, chi, R, reps, _ = _torus_columns(lx, ly, mx, my, n_down)
    col = np.where(adm, col, -1)
    val = np.where(adm, chi / np.sqrt(R.astype(np.float64)), 0.0)
    if not dense:
        return col, val
    B = np.zeros((states.shape[0], reps.shape[0]), np.complex128)
    B[np.flatnonzero(adm), col[adm]] = val[adm]
    return B


def torus_translation_fault(lx, ly, terms):
    """None when H = sum of `terms` commutes with T_x and with T_y of the lx x ly torus by the rule of ll_op_create_pauli_torus
    (coefficients of equal masks merged in list order; the masks moved by one site meet exactly the same coefficient, a missing
    term counting as 0); else (direction "x" or "y", the number of the first term at fault), T_x checked first."""
    lx, ly = int(lx), int(ly)
    merged = {}
    for x, z, c in terms:
        merged[(int(x), int(z))] = merged.get((int(x), int(z)), 0.0) + float(c)
    for name, move in (("x", _torus_tx), ("y", _torus_ty)):
        for t, (x, z, _) in enumerate(terms):
            if merged.get((move(lx, ly, int(x)), move(lx, ly, int(z))), 0.0) != merged[(int(x), int(z))]:
                return name, t
    return None


def torus_symmetrised_strings(lx, ly, term):
    """The average of the string `term` = (x_mask, z_mask[, coef]) over the lx ly translations of the torus, as a list of
    (x_mask, z_mask, weight) sorted by x mask, then z mask: symmetrised_strings for a torus block (both masks moved by the same
    element; no signs, so nothing cancels).  The coefficient of `term` is not in the weights."""
    lx, ly, x, z = int(lx), int(ly), int(term[0]), int(term[1])
    n = lx * ly
    if not (lx >= 1 and ly >= 1 and n <= 30) or (x | z) >> n:
        raise ValueError("need lx, ly >= 1, lx * ly <= 30 and masks below 2^(lx ly)")
    mult = {}
    for b in range(ly):
        for a in range(lx):
            mult[(x, z)] = mult.get((x, z), 0) + 1
            x, z = _torus_tx(lx, ly, x), _torus_tx(lx, ly, z)
        x, z = _torus_ty(lx, ly, x), _torus_ty(lx, ly, z)
    return [(kx, kz, mult[(kx, kz)] / n) for kx, kz in sorted(mult)]


def pauli_torus_csr(lx, ly, mx, my, terms, dtype=np.float64, n_down=None, merge=True):
    """The block B^H H B (B = torus_embedding; H = pauli_csr, or pauli_sector_csr with n_down) as CSR over torus_basis, from the
    gather form, in double: row a holds, per x mask X whose partner a ^ X = g b has b in the block, w(a) sqrt(R_a / R_b) chi(g) in
    the column of b, w as in pauli_csr.  merge as in pauli_symmetric_csr (merge=False: one entry per term and state).  A real
    dtype needs 2 mx = 0 (mod lx) and 2 my = 0 (mod ly); H must commute with both translations."""
    lx, ly, mx, my, n_down = _check_torus(lx, ly, mx, my, n_down)
    terms = list(terms)
    if np.dtype(dtype).kind != "c" and ((2 * mx) % lx or (2 * my) % ly):
        raise ValueError("a real dtype takes mx = 0 or lx / 2 and my = 0 or ly / 2 only")
    fault = torus_translation_fault(lx, ly, terms)
    if fault is not None:
        t = fault[1]
        raise ValueError("term %d (x_mask 0x%x, z_mask 0x%x) does not commute with T_%s" % (t, terms[t][0], terms[t][1], fault[0]))
    states, adm, col, chi, R, reps, ra = _torus_columns(lx, ly, mx, my, n_down)
    if reps.shape[0] == 0:
        raise ValueError("the block is empty")
    ra = ra.astype(np.float64)
    n_sites = lx * ly
    if n_down is not None:
        h = (n_sites + 1) // 2
        lo, hi = sector_rank_tables(n_sites, n_down, h)

    def column_of(p):
        if n_down is None:
            k = p.astype(np.int64)   # the state is its own number
            return col[k], adm[k], np.sqrt(ra / R[k]) * chi[k]
        inside = _popcount(p) == n_down
        q = np.where(inside, p, states[0])
        k = lo[q & np.uint64((1 << h) - 1)].astype(np.int64) + hi[q >> np.uint64(h)]
        return col[k], inside & adm[k], np.sqrt(ra / R[k]) * chi[k]

    return _pauli_rows(reps, terms, dtype, merge, column_of)


# ------------------------------------------------------------------ a sum of Pauli strings between two momentum blocks of a ring
# out = B_t^H (sum_j coef_j P_j) B_s c (ll_pauli_block_transfer): B_s, B_t the embeddings of two blocks of one kind,
#   kind "momentum"       shape = (n_sites, n_down, m)    momentum_embedding
#   kind "momentum_full"  shape = (n_sites, m)            full_momentum_embedding
def transferred_strings(n_sites, term, q):
    """The momentum-q component of the string `term` = (x_mask, z_mask[, coef]) on a ring,
        Pbar_q = (1 / L) sum_{j < L} e^(+2 pi i q j / L) [(x, z) both rotated RIGHT by j sites],
    as a list of (x_mask, z_mask, weight) with complex weights, sorted by x mask, then z mask: the numpy mirror of
    csrc/pauli_block_transfer_plan.hpp.  B_t^H P B_s = B_t^H Pbar_q B_s for q = m_t - m_s (mod L).  A string whose masks come
    back after r sites has r distinct images; they survive iff q r = 0 (mod L) — decided in integers — with the weight
    e^(2 pi i q j / L) / r, exact where the phase lies on an axis.  The coefficient of `term` is not in the weights; an empty
    list means the string has no momentum-q component."""
    L, x, z, q = int(n_sites), int(term[0]), int(term[1]), int(q)
    mask = (1 << L) - 1
    if not 1 <= L <= 30 or (x | z) & ~mask or not 0 <= q < L:
        raise ValueError("need 1 <= n_sites <= 30, masks below 2^n_sites and 0 <= q < n_sites")

    def rotr(v, j):
        return ((v >> j) | (v << (L - j))) & mask

    r = next(d for d in range(1, L + 1) if L % d == 0 and rotr(x, d) == x and rotr(z, d) == z)
    if (q * r) % L:
        return []
    ph = np.conj(_momentum_phases(L, q))   # e^(+2 pi i q j / L)
    return sorted((rotr(x, j), rotr(z, j), complex(ph[j]) / r) for j in range(r))


def _transfer_block(kind, shape):
    """(n_sites, n_down or None, m, states of the embedding's rows or None, (col, val) of the embedding, (reps, periods))."""
    if kind == "momentum":
        n_sites, n_down, m = (int(v) for v in shape)
        return (n_sites, n_down, m, sector_states(n_sites, n_down), momentum_embedding(n_sites, n_down, m, dense=False),
                momentum_basis(n_sites, n_down, m))
    if kind == "momentum_full":
        n_sites, m = (int(v) for v in shape)
        return n_sites, None, m, None, full_momentum_embedding(n_sites, m, dense=False), full_momentum_basis(n_sites, m)
    raise ValueError("kind must be 'momentum' or 'momentum_full'")


def pauli_block_transfer_np(kind, shape_s, shape_t, terms, c, return_magnitude=False):
    """out = B_t^H (sum_j coef_j P_j) B_s c in complex128 by its definition — expand with the source's one-entry-per-row
    embedding, pauli_string_apply_np per term, project with the target's — the plain host restatement of
    ll_pauli_block_transfer.  kind and the shapes as in the comment above; `terms` holds (x_mask, z_mask, coef); c holds the
    source block's coefficients.  In a sector a partner outside it contributes nothing.  With return_magnitude also
    |B_t|^T (sum_j |coef_j| |P_j|) |B_s| |c| per row: the sum of the absolute values of everything the row gathers, which bounds
    the same sum over the merged strings of the gather form (pauli_block_transfer_rows_np)."""
    L, nd, _, states, (col_s, val_s), _ = _transfer_block(kind, shape_s)
    L_t, nd_t, _, _, (col_t, val_t), (reps_t, _) = _transfer_block(kind, shape_t)
    if L != L_t or nd != nd_t:
        raise ValueError("the two blocks differ in n_sites or n_down")
    c = np.asarray(c, dtype=np.complex128).reshape(-1)
    psi = np.where(col_s >= 0, val_s * c[np.maximum(col_s, 0)], 0.0)
    phi = np.zeros_like(psi)
    for term in terms:
        phi = phi + float(term[2]) * pauli_string_apply_np(L, term, psi, states)
    out = np.zeros(reps_t.shape[0], np.complex128)
    rows = np.flatnonzero(col_t >= 0)
    np.add.at(out, col_t[rows], np.conj(val_t[rows]) * phi[rows])
    if not return_magnitude:
        return out
    apsi, aphi = np.abs(psi), np.zeros(psi.shape[0])
    for term in terms:
        aphi = aphi + abs(float(term[2])) * pauli_string_apply_np(L, (term[0], 0, 1.0), apsi, states)
    mag = np.bincount(col_t[rows], weights=np.abs(val_t[rows]) * aphi[rows], minlength=reps_t.shape[0])
    return out, mag


def pauli_block_transfer_rows_np(kind, shape_s, shape_t, terms, c, rows=None):
    """(values, magnitudes) of the rows `rows` (None: all) of pauli_block_transfer_np's result from the GATHER form that the kernel
    evaluates, in complex128 / float64:
        out(a) = sum over the strings (X', z', weight) of transferred_strings(term, m_t - m_s), over the terms
                 coef weight i^nY (-1)^popcount((a ^ X') & z') sqrt(R_a / R_b) e^(-2 pi i m_s l / L) c_b,     a ^ X' = T^l b
    with a, R_a of the target block and b, l, R_b of the source block; a partner outside the source block (or outside the sector)
    contributes nothing.  magnitudes[a] = the sum of the absolute values of those contributions: what an error bound of the row
    multiplies.  Cost O(rows x strings x n_sites): rows of a 20-site block stay cheap."""
    L, nd, m_s, (reps_s, _) = _transfer_reps(kind, shape_s)
    L_t, nd_t, m_t, (reps_t, per_t) = _transfer_reps(kind, shape_t)
    if L != L_t or nd != nd_t:
        raise ValueError("the two blocks differ in n_sites or n_down")
    c = np.asarray(c, dtype=np.complex128).reshape(-1)
    rows = np.arange(reps_t.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    a = reps_t[rows].astype(np.uint64)
    ra = per_t[rows].astype(np.float64)
    phases = _momentum_phases(L, m_s)
    val, mag = np.zeros(a.shape[0], np.complex128), np.zeros(a.shape[0], np.float64)
    q = (m_t - m_s) % L
    reps_s64 = reps_s.astype(np.uint64)
    for term in terms:
        for x, z, wt in transferred_strings(L, term, q):
            p = a ^ np.uint64(x)
            _, b, l, rb = _orbits_of(L, p)
            inb = (m_s * rb) % L == 0
            if nd is not None:
                inb &= _popcount(p) == nd
            j = np.minimum(np.searchsorted(reps_s64, b), reps_s64.shape[0] - 1)
            inb &= reps_s64[j] == b
            sign = np.where(_parity(p & np.uint64(z)) == 1, -1.0, 1.0)
            t = (float(term[2]) * wt * (1j ** (bin(x & z).count("1") & 3))) * sign * np.sqrt(ra / rb) * phases[l] * c[j]
            t = np.where(inb, t, 0.0)
            val += t
            mag += np.abs(t)
    return val, mag


def _transfer_reps(kind, shape):
    """(n_sites, n_down or None, m, (reps, periods)): _transfer_block without the embedding over all states."""
    if kind == "momentum":
        n_sites, n_down, m = (int(v) for v in shape)
        return n_sites, n_down, m, momentum_basis(n_sites, n_down, m)
    if kind == "momentum_full":
        n_sites, m = (int(v) for v in shape)
        return n_sites, None, m, full_momentum_basis(n_sites, m)
    raise ValueError("kind must be 'momentum' or 'momentum_full'")

# ------------------------------------------------------------------ C++ versions (BASELINE sizes)
_gen = None


def _lib():
    global _gen
    if _gen is None:
        if not os.path.exists(capi.GEN_PATH):
            raise RuntimeError("%s not built (run __graft_entry__.build())" % capi.GEN_PATH)
        g = C.CDLL(capi.GEN_PATH)
        i64, vp = C.c_int64, C.c_void_p
        g.llgen_splitmix64.restype, g.llgen_splitmix64.argtypes = C.c_uint64, [C.c_uint64]
        g.llgen_start_vector_d.argtypes = [C.c_uint64, i64, i64, vp]
        g.llgen_start_vector_z.argtypes = [C.c_uint64, i64, i64, vp]
        g.llgen_laplace2d_count.restype, g.llgen_laplace2d_count.argtypes = i64, [i64, i64, i64]
        g.llgen_laplace2d_fill.argtypes = [i64, i64, i64, vp, vp, vp]
        g.llgen_randsym_count.restype, g.llgen_randsym_count.argtypes = i64, [i64, i64, i64, i64]
        g.llgen_randsym_fill.argtypes = [i64, i64, i64, i64, vp, vp, vp]
        g.llgen_torus_fill.argtypes = [i64, i64, i64, vp, vp, vp]
        _gen = g
    return _gen


def start_vector_fast(n_local, seed=1, dtype=np.float64, row_begin=0):
    v = np.empty(n_local, dtype=dtype)
    fn = _lib().llgen_start_vector_z if np.dtype(dtype) == np.complex128 else _lib().llgen_start_vector_d
    fn(seed, row_begin, n_local, capi.ptr(v))
    return v


def laplace2d(N, row_begin=0, n_local=None):
    n_local = N * N - row_begin if n_local is None else n_local
    nnz = _lib().llgen_laplace2d_count(N, row_begin, n_local)
    rp, ci, va = np.empty(n_local + 1, np.int64), np.empty(nnz, np.int32), np.empty(nnz, np.float64)
    _lib().llgen_laplace2d_fill(N, row_begin, n_local, capi.ptr(rp), capi.ptr(ci), capi.ptr(va))
    return rp, ci, va


def randsym(n, band=0, row_begin=0, n_local=None):
    n_local = n - row_begin if n_local is None else n_local
    nnz = _lib().llgen_randsym_count(n, band, row_begin, n_local)
    rp, ci, va = np.empty(n_local + 1, np.int64), np.empty(nnz, np.int32), np.empty(nnz, np.float64)
    _lib().llgen_randsym_fill(n, band, row_begin, n_local, capi.ptr(rp), capi.ptr(ci), capi.ptr(va))
    return rp, ci, va


def torus(N, row_begin=0, n_local=None):
    n_local = N * N - row_begin if n_local is None else n_local
    rp, ci, va = np.empty(n_local + 1, np.int64), np.empty(5 * n_local, np.int32), np.empty(5 * n_local, np.complex128)
    _lib().llgen_torus_fill(N, row_begin, n_local, capi.ptr(rp), capi.ptr(ci), capi.ptr(va))
    return rp, ci, va


def laplace2d_lambda_min(N):
    """Analytic smallest eigenvalue of the N x N Dirichlet 5-point Laplacian."""
    return 4.0 - 4.0 * math.cos(math.pi / (N + 1))
