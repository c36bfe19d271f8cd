"""The cases of tests/test_gpu_pauli_measure_large.py and tests/test_pauli_measure_large_host.py: the four measuring kernels
(pauli_expect_kernel, pauli_expect_sector_kernel, pauli_rdm_kernel, pauli_rdm_sector_kernel) on 20 to 30 sites, where a
workgroup takes more than one trip of its grid-stride loop.  No GPU, no test.

The instrument is an INTEGER state: re and im from +-{1 .. 7}.  Every product conj(psi(s')) psi(s) is then an integer of magnitude
at most 2 * 7 * 7 = 98 and every partial sum an integer below 98 n < 2^53: exact in double in ANY summation order, so the
kernels must return the host's integer bit for bit — tolerance zero, derived (exact_condition), not measured.

Also here: a Python restatement of the four launch rules (units of work and grid), the observables, and host references that never
embed a sector in 2^n_sites numbers."""
import math

import numpy as np

import pauli_large_cases as PL
from lambda_lanczos_amd import generators as G

TYPES = {"d": np.float64, "z": np.complex128, "s": np.float32, "c": np.complex64}

MAX_GRID = PL.MAX_GRID          # kMaxGrid = 8 * kCUs (csrc/ll_internal.hpp): the grid of the kernels' grid-stride loops
TILE_BYTES = 32 << 10           # kPauliTileBytes (csrc/ll_internal.hpp): the LDS tile, super-tile or batch of one workgroup
MAX_TILE_BYTES = 64 << 10       # kPauliMaxTileBytes (csrc/ll_internal.hpp): the largest tile pauli_tile_bits may ask for
SECTOR_BLOCK_BITS = 10          # kPauliSectorBlockBits (csrc/ll_internal.hpp): 2^10 indices per block of the sector kernels
EXPECT_BATCH = 32               # kPauliExpectBatch (csrc/pauli_expect.hip): slots per sweep
RDM_PARTIAL_DOUBLES = 1 << 20   # kPauliRdmPartialBytes / sizeof(double) (csrc/pauli_rdm.hip): the partials of one call at most
RDM_THREADS = 256               # kPauliRdmThreads (csrc/pauli_rdm_plan.hpp)
AMP = 7                         # |re|, |im| of an integer state: 1 .. AMP


def _cplx(dtype):
    return np.dtype(dtype).kind == "c"


def _bits(*sites):
    return sum(1 << j for j in sites)


def _parity(w):
    """popcount(w) mod 2 of an int64 array below 2^32."""
    return (PL._POP16[w & 0xFFFF] + PL._POP16[w >> 16]) & 1


# ------------------------------------------------------------------ the instrument
def integer_state(n, dtype, seed):
    """n amplitudes whose parts are drawn from +-{1 .. AMP}: none is zero, all are exact in float, double and their complex types."""
    rng = np.random.default_rng(seed)
    x = rng.integers(1, AMP + 1, n).astype(np.float64) * rng.choice([-1.0, 1.0], n)
    if _cplx(dtype):
        x = x + 1j * (rng.integers(1, AMP + 1, n).astype(np.float64) * rng.choice([-1.0, 1.0], n))
    return x.astype(dtype)


def exact_condition(n):
    """Every sum of n products of two amplitudes (complex: two real products each) is an integer below 2^53."""
    return 2 * AMP * AMP * n < 2 ** 53


# ------------------------------------------------------------------ the launch rules, restated: (units of work, grid)
def expect_tile_bits(n_sites, itemsize, forced=None):
    """launch_pauli_expect: pauli_tile_bits, else the largest tile within TILE_BYTES; at most MAX_TILE_BYTES and the vector."""
    b = forced
    if b is None:
        b = 0
        while (itemsize << (b + 1)) <= TILE_BYTES:
            b += 1
    while b > 0 and (itemsize << b) > MAX_TILE_BYTES:
        b -= 1
    return min(b, n_sites)


def expect_full_launch(n_sites, itemsize, forced=None):
    units = 1 << (n_sites - expect_tile_bits(n_sites, itemsize, forced))
    return units, min(units, MAX_GRID)


def expect_sector_launch(dim, forced=None):
    """launch_pauli_expect_sector: blocks of 2^b indices, b = pauli_sector_block_bits (at most 30) or SECTOR_BLOCK_BITS."""
    b = SECTOR_BLOCK_BITS if forced is None else min(forced, 30)
    units = -(-dim // (1 << b))
    return units, min(units, MAX_GRID)


def rdm_block_edge(m):
    return 1 if m <= 2 else (2 if m == 3 else 4)


def rdm_blocks(m):
    """The R x R blocks of the upper triangle of rho."""
    nb = (1 << m) // rdm_block_edge(m)
    return nb * (nb + 1) // 2


def rdm_partials(m, complex_storage):
    """Doubles of one workgroup's partials."""
    return rdm_blocks(m) * rdm_block_edge(m) ** 2 * (2 if complex_storage else 1)


def rdm_grid(units, m, complex_storage):
    return min(units, MAX_GRID, max(1, RDM_PARTIAL_DOUBLES // rdm_partials(m, complex_storage)))


def rdm_tile_bits(n_sites, sites, itemsize, forced=None):
    """pauli_rdm_tile_bits: (t, h) — forced or n_sites, lowered until the super-tile of 2^(t + h(t)) elements fits TILE_BYTES."""
    def high(t):
        return sum(1 for s in sites if s >= t)

    t = forced if forced is not None and 0 <= forced < n_sites else n_sites
    while t > 0 and (itemsize << (t + high(t))) > TILE_BYTES:
        t -= 1
    return t, high(t)


def rdm_full_launch(n_sites, sites, dtype, forced=None):
    dtype = np.dtype(dtype)
    t, h = rdm_tile_bits(n_sites, sites, dtype.itemsize, forced)
    units = 1 << (n_sites - t - h)
    return units, rdm_grid(units, len(sites), _cplx(dtype))


def rdm_block_bits(n_sites, m, itemsize, forced=None):
    """pauli_rdm_block_bits: forced or all n_sites - m environment bits, lowered until 2^(b + m) elements fit TILE_BYTES."""
    b = forced if forced is not None and 0 <= forced < n_sites - m else n_sites - m
    while b > 0 and (itemsize << (b + m)) > TILE_BYTES:
        b -= 1
    return b


def rdm_sector_launch(n_sites, m, dtype, forced=None):
    dtype = np.dtype(dtype)
    b = rdm_block_bits(n_sites, m, dtype.itemsize, forced)
    units = -(-(1 << (n_sites - m)) // (1 << b))
    return units, rdm_grid(units, m, _cplx(dtype))


# ------------------------------------------------------------------ the cases
ALL = ("d", "z", "s", "c")

# (storage, n_sites, forced pauli_tile_bits).  20 sites at 64 states per tile: 16384 tiles, 8 trips; at 512: 2048 tiles, one trip
# with partner tiles up to 11 bits away (in BELOW_WRAP); the default tile with two trips: z at 23 sites, d at 24 (4096 tiles).
EXPECT_FULL = [(t, 20, b) for t in ALL for b in (6, 9)] + [("z", 23, None), ("d", 24, None)]

# (storage, (n_sites, n_down), block bits: None — the default — or "small" — pauli_large_cases.small_bits(D)).
# (20, 10): 11548 blocks of 16, ragged; (30, 4): 6852 blocks of 4, h = 15; both run at the default too (one trip: BELOW_WRAP);
# (24, 12): 2641 default blocks, two trips, the second ragged — d and z (the host reference of 2.7e6 states costs seconds).
EXPECT_SECTOR = ([(t, s, b) for t in ALL for s in ((20, 10), (30, 4)) for b in (None, "small")] +
                 [("d", (24, 12), None), ("z", (24, 12), None)])

SIX_20 = [13, 1, 19, 5, 3, 9]   # {1, 3, 5, 9, 13, 19}, unsorted
SIX_22 = [21, 1, 13, 3, 9, 5]   # {1, 3, 5, 9, 13, 21}, unsorted
FIVE_20 = [19, 3, 0, 4, 2]      # {0, 2, 3, 4, 19}, unsorted
# (storage, n_sites, sites, forced pauli_rdm_tile_bits, super-tiles, grid): the last two are pinned and re-derived by the host test
RDM_FULL = ([(t, 20, SIX_20, 6, 2048, 481) for t in ("d", "s")] + [(t, 20, SIX_20, 7, 1024, 240) for t in ("z", "c")] +
            [(t, 20, FIVE_20, 6, 8192, 1820) for t in ("d", "s")] + [(t, 20, FIVE_20, 6, 8192, 910) for t in ("z", "c")] +
            [(t, 20, [0, 2, 4, 19], 6, 8192, 2048) for t in ALL] + [(t, 20, [19], 6, 8192, 2048) for t in ALL] +
            [("z", 20, [1, 3, 5, 9, 13, 19], None, 512, 240), ("c", 20, [1, 3, 5, 9, 13, 19], None, 256, 240),
             ("d", 22, SIX_22, None, 1024, 481), ("s", 22, SIX_22, None, 512, 481),
             ("z", 23, [0, 22], None, 4096, 2048), ("d", 24, [23, 0], None, 4096, 2048)])

SIX_30 = [29, 2, 15, 7, 14, 22]
# (storage, (n_sites, n_down), sites, forced pauli_rdm_block_bits).  (20, 10) at 16 configurations per batch: m = 1 32768 batches,
# 16 trips; m = 6 1024 batches against 481 or 240 workgroups; default bits, m = 6 in z: 512 against 240.  (30, 4) at the default:
# 131072 to 524288 batches, 64 to more than 2000 trips over all 2^30 (a, e) pairs, of which 27405 are loaded.  (24, 12), m = 2.
RDM_SECTOR = ([(t, (20, 10), [19], 4) for t in ALL] + [(t, (20, 10), SIX_20, 4) for t in ALL] +
              [("z", (20, 10), [1, 3, 5, 9, 13, 19], None)] +
              [(t, (30, 4), s, None) for t in ALL for s in ([29], [0, 15, 14], SIX_30)] +
              [("d", (24, 12), [0, 23], None), ("z", (24, 12), [23, 0], None)])

# the cases that are in a table for another reason than the second trip: remote partners 11 bits away; the default block beside
# the small one
BELOW_WRAP = ({("expect_full", t, 20, 9) for t in ALL} |
              {("expect_sector", t, s, None) for t in ALL for s in ((20, 10), (30, 4))})


def sector_block_bits(dim, bits):
    return PL.small_bits(dim) if bits == "small" else bits


def launch_of(kernel, case):
    """(units, grid) of a case of the table of `kernel`."""
    dtype = np.dtype(TYPES[case[0]])
    if kernel == "expect_full":
        return expect_full_launch(case[1], dtype.itemsize, case[2])
    if kernel == "expect_sector":
        dim = math.comb(*case[1])
        return expect_sector_launch(dim, sector_block_bits(dim, case[2]))
    if kernel == "rdm_full":
        return rdm_full_launch(case[1], case[2], dtype, case[3])
    if kernel == "rdm_sector":
        return rdm_sector_launch(case[1][0], len(case[2]), dtype, case[3])
    raise KeyError(kernel)


TABLES = {"expect_full": EXPECT_FULL, "expect_sector": EXPECT_SECTOR, "rdm_full": RDM_FULL, "rdm_sector": RDM_SECTOR}


def case_key(kernel, case):
    """What BELOW_WRAP lists."""
    return (kernel,) + tuple(tuple(v) if isinstance(v, list) else v for v in case[:4 if kernel.startswith("rdm") else 3])


def case_id(case):
    return "-".join("x" if v is None else ".".join(map(str, v)) if isinstance(v, (list, tuple)) else str(v) for v in case)


# ------------------------------------------------------------------ the observables
def is_zero(term, complex_storage, sector):
    """The two rules that answer +0.0 without a sweep (csrc/pauli_expect_plan.hpp)."""
    x, z, _ = term
    return (not complex_storage and bin(x & z).count("1") % 2 == 1) or (sector and bin(x).count("1") % 2 == 1)


def slots_of(obs, complex_storage, sector):
    return sum(not is_zero(t, complex_storage, sector) for t in obs)


def observables(n_sites, k, complex_storage, sector):
    """About 40 strings around the boundary k — the tile bits of the full space, the rank split h of a sector — and the top site:
    more than one batch of slots and the last one ragged.  X and Y on the top site are the two odd x masks of a sector."""
    top = n_sites - 1
    assert 1 <= k - 1 and k + 1 < top
    full = (1 << n_sites) - 1
    obs = [(0, 0, 1.37),                                                          # the identity
           (_bits(top), 0, 0.61), (_bits(top), _bits(top), -1.21), (0, _bits(top), 2.3),    # X, Y, Z on the top site
           (_bits(0, top), 0, 0.37),                                              # X_0 X_top
           (_bits(k - 1, k), 0, -0.77), (_bits(k - 1, k), _bits(k - 1, k), 0.43), (0, _bits(k - 1, k), 1.9),   # XX, YY, ZZ across k
           (0, _bits(k - 1), -0.33), (0, _bits(k), 0.57),
           (_bits(k - 1, k), _bits(top), 0.29),                                   # X X Z_top: the x mask of the pair across k
           (_bits(k + 1, top), 0, 0.53), (0, _bits(k + 1, top), -0.91), (_bits(k + 1, top), _bits(k + 1, top), 0.83),   # above k
           (_bits(k, top), _bits(0, k - 1), -0.47),                               # X_k X_top Z_0 Z_(k-1)
           (_bits(0, 1, k, top), 0, 0.71),                                        # four flips on both sides
           (full, 0, 1.1), (0, full, -0.9),                                       # X...X, Z...Z
           (_bits(0, top), _bits(0, top), 0.67)]                                  # Y_0 Y_top: nY = 2
    if complex_storage:
        obs += [(_bits(0, top), _bits(top), 0.59),                                # X_0 Y_top: nY = 1
                (_bits(0, k - 1, k, top), _bits(0, k, top), -0.41)]               # Y_0 X_(k-1) Y_k Y_top: nY = 3
    rng = np.random.default_rng(1000 * n_sites + k)
    for _ in range(16):
        if sector:   # 0, 2 or 4 flips: the x masks of a sector have an even popcount (and few bits, or no partner stays inside)
            x = _bits(*rng.choice(n_sites, size=int(rng.choice([0, 2, 2, 4])), replace=False).tolist())
        else:
            x = int(rng.integers(0, full + 1))
        z = int(rng.integers(0, full + 1))
        if not complex_storage and bin(x & z).count("1") % 2 == 1:
            z ^= (x & z) & -(x & z)   # one Y less: even nY
        obs.append((x, z, float(rng.uniform(-2.0, 2.0))))
    obs += [(obs[5][0], obs[5][1], -0.19), (obs[-1][0], obs[-1][1], 0.23)]        # two strings twice, other coefficients
    slots = slots_of(obs, complex_storage, sector)
    assert EXPECT_BATCH < slots < 2 * EXPECT_BATCH, slots
    return obs


def _part_and_sign(x, z):
    """Re[i^nY v] = Re v, -Im v, -Re v, Im v for nY mod 4 = 0, 1, 2, 3: (take the imaginary part, sign)."""
    ny = bin(x & z).count("1") & 3
    return bool(ny & 1), (-1.0 if ny in (1, 2) else 1.0)


def expect_values(sums, obs, complex_storage, sector):
    """coef * float(S): one IEEE product, what the host side of ll_pauli_expect forms; +0.0 by the zero rules."""
    return np.array([0.0 if is_zero(t, complex_storage, sector) else t[2] * float(s) for t, s in zip(obs, sums)])


def expect_sums_full(n_sites, psi, obs):
    """S = sum_s Re[ conj(psi(s ^ x)) i^nY (-1)^popcount(s & z) psi(s) ] per observable, as Python ints, for an integer state on
    all 2^n_sites states: the gather as two takes on psi as a matrix [high bits][low bits], the signs as two +-1 vectors."""
    lo_bits = n_sites // 2
    nlo, nhi = 1 << lo_bits, 1 << (n_sites - lo_bits)
    psi = np.asarray(psi).reshape(nhi, nlo)
    cplx = np.iscomplexobj(psi)
    wr = np.ascontiguousarray(psi.real, dtype=np.float64)
    wi = np.ascontiguousarray(psi.imag, dtype=np.float64) if cplx else None
    ilo, ihi = np.arange(nlo, dtype=np.int64), np.arange(nhi, dtype=np.int64)

    def partner(w, x):
        xhi, xlo = x >> lo_bits, x & (nlo - 1)
        w = w.take(ihi ^ xhi, axis=0) if xhi else w
        return w.take(ilo ^ xlo, axis=1) if xlo else w

    out, have = [0] * len(obs), {}
    for j in sorted(range(len(obs)), key=lambda j: obs[j][0]):
        x, z = int(obs[j][0]), int(obs[j][1])
        if have.get("x") != x:   # one x mask at a time: the partner's parts, and Re v, Im v once an observable asks
            have = {"x": x, "pr": partner(wr, x), "pi": partner(wi, x) if cplx else None}
        imag, sign = _part_and_sign(x, z)
        if imag and not cplx:
            continue   # Im v = 0
        if imag not in have:   # v = conj(p) psi: Re v = pr wr + pi wi, Im v = pr wi - pi wr
            if imag:
                have[imag] = have["pr"] * wi - have["pi"] * wr
            else:
                have[imag] = have["pr"] * wr + have["pi"] * wi if cplx else have["pr"] * wr
        s = (1.0 - 2.0 * _parity(ihi & (z >> lo_bits))) @ (have[imag] @ (1.0 - 2.0 * _parity(ilo & (z & (nlo - 1)))))
        assert s == np.rint(s) and abs(s) < 2.0 ** 53
        out[j] = int(sign * s)
    return out


def expect_sums_sector(n_sites, n_down, psi, obs):
    """The same on the states of one S_z sector (psi on generators.sector_states); a partner outside the sector contributes
    nothing.  The partner's index: a look-up table over all states up to 24 sites, a binary search above."""
    st = G.sector_states(n_sites, n_down).astype(np.int64)
    dim = st.shape[0]
    wide = np.asarray(psi).astype(np.complex128 if np.iscomplexobj(psi) else np.float64)
    table = None
    if n_sites <= 24:
        table = np.full(1 << n_sites, -1, np.int32)
        table[st] = np.arange(dim, dtype=np.int32)
    out, v_of = [0] * len(obs), {}
    for j in sorted(range(len(obs)), key=lambda j: obs[j][0]):
        x, z = int(obs[j][0]), int(obs[j][1])
        if x not in v_of:
            v_of.clear()
            p = st ^ x
            if table is not None:
                idx = table[p].astype(np.int64)
                inside = idx >= 0
            else:
                idx = np.minimum(np.searchsorted(st, p), dim - 1)
                inside = st[idx] == p
            v_of[x] = np.where(inside, np.conj(wide[np.where(inside, idx, 0)]) * wide, 0.0)
        imag, sign = _part_and_sign(x, z)
        if imag and not np.iscomplexobj(wide):
            continue
        part = v_of[x].imag if imag else v_of[x].real
        s = float((1.0 - 2.0 * _parity(st & z)) @ part)
        assert s == np.rint(s) and abs(s) < 2.0 ** 53
        out[j] = int(sign * s)
    return out


# ------------------------------------------------------------------ fibres and rho
def _wide(a):
    return a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)


def gram(fibres):
    """rho[a][a'] = sum_e f_a(e) conj f_a'(e), complex128: exact for an integer state (a float64 product of the fibres)."""
    f = _wide(fibres)
    return (f @ f.conj().T).astype(np.complex128)


def full_fibres(n_sites, sites, psi):
    """fibres[a][e] = psi(a, e) on all 2^n_sites states: bit k of a is sites[k], the bits of e fill the other sites ascending."""
    m = len(sites)
    env = [s for s in range(n_sites) if s not in sites]
    a, e = np.arange(1 << m, dtype=np.int64), np.arange(1 << (n_sites - m), dtype=np.int64)
    sa, se = np.zeros_like(a), np.zeros_like(e)
    for k, s in enumerate(sites):
        sa |= ((a >> k) & 1) << s
    for k, s in enumerate(env):
        se |= ((e >> k) & 1) << s
    return np.asarray(psi)[sa[:, None] | se[None, :]]


def sector_fibres(n_sites, n_down, sites, psi):
    """The fibres of a state on generators.sector_states(n_sites, n_down) without the 2^n_sites numbers of the full space: every
    state splits into (a, e), and e is numbered by its rank among the e that occur.  Shape (2^m, n_e), n_e <= D; an (a, e) that
    is no state of the sector is 0.  The columns are a subset of those of generators.reduced_density_matrix_np(..., states=...),
    the others being zero: the same Gram matrix."""
    st = G.sector_states(n_sites, n_down).astype(np.int64)
    psi = np.asarray(psi).reshape(-1)
    assert psi.shape[0] == st.shape[0]
    a, e = np.zeros_like(st), np.zeros_like(st)
    for k, s in enumerate(sites):
        a |= ((st >> s) & 1) << k
    for k, s in enumerate(s for s in range(n_sites) if s not in sites):
        e |= ((st >> s) & 1) << k
    vals, col = np.unique(e, return_inverse=True)
    fibres = np.zeros((1 << len(sites), vals.shape[0]), psi.dtype)
    fibres[a, col.reshape(-1)] = psi
    return fibres
