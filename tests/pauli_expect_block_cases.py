"""What the tests of ll_pauli_expect_block share (tests/test_pauli_expect_block_host.py on the CPU,
tests/test_gpu_pauli_expect_block.py on the GPU): the blocks, the observables, the state Psi = B c through the embeddings of
generators.py, and the expected values with their bounds — computed once per block and storage type and left unchanged."""
import numpy as np

import contract_cases as K
import exact_ref as E
from lambda_lanczos_amd import generators as G

BATCH = 32   # slots per sweep (csrc/pauli_expect_block.hip kPauliExpectBlockBatch)


class Block:
    """kind: "momentum_full" (n_sites, m), "momentum" (n_sites, n_down, m) or "symmetric" (n_sites, m, parity, inversion, n_down)."""

    def __init__(self, kind, n_sites, m, parity=0, inversion=0, n_down=None):
        self.kind, self.n_sites, self.m = kind, n_sites, m
        self.parity, self.inversion, self.n_down = parity, inversion, n_down
        assert kind in ("momentum_full", "momentum", "symmetric") and (kind != "momentum" or n_down is not None)
        assert kind == "symmetric" or (parity == 0 and inversion == 0)

    @property
    def sector(self):
        return self.n_down is not None

    @property
    def id(self):
        return "%s-L%d-m%d-p%d-z%d-nd%s" % (self.kind, self.n_sites, self.m, self.parity, self.inversion, self.n_down)

    def real_ok(self):
        return (2 * self.m) % self.n_sites == 0

    def embedding(self):
        """(column of each state or -1, its value): the rows of B over all states or over the sector's."""
        if self.kind == "momentum_full":
            return G.full_momentum_embedding(self.n_sites, self.m, dense=False)
        if self.kind == "momentum":
            return G.momentum_embedding(self.n_sites, self.n_down, self.m, dense=False)
        return G.symmetric_embedding(self.n_sites, self.m, self.parity, self.inversion, self.n_down, dense=False)

    def states(self):
        return None if self.n_down is None else G.sector_states(self.n_sites, self.n_down)

    def create(self, L, ctx, dtype, terms):
        if self.kind == "momentum_full":
            return L.PauliMomentumFullOperator(ctx, self.n_sites, self.m, terms, dtype)
        if self.kind == "momentum":
            return L.PauliMomentumOperator(ctx, self.n_sites, self.n_down, self.m, terms, dtype)
        return L.PauliSymmetricOperator(ctx, self.n_sites, self.m, terms, dtype, parity=self.parity, inversion=self.inversion,
                                        n_down=self.n_down)

    def hamiltonian(self):
        """Terms every symmetry in use commutes with (they play no part in a measurement)."""
        if self.sector or self.kind == "momentum":
            return G.heisenberg_terms(self.n_sites, 1.0, 0.8, periodic=True)
        return G.tfim_terms(self.n_sites, 1.0, 0.7, periodic=True)


def expand(block, c):
    """Psi = B c in double (complex128), from the values of c as they are stored."""
    col, val = block.embedding()
    cw = np.asarray(c).astype(np.complex128)
    return np.where(col >= 0, val * cw[np.maximum(col, 0)], 0.0).astype(np.complex128)


def _site(*js):
    m = 0
    for j in js:
        m |= 1 << j
    return m


def observable_set(n_sites, parity, seed):
    """The identity; Z_0, X_0, Y_0; Z_0 Z_r, X_0 X_r, Y_0 Y_r and X_0 Y_r for r = 1 .. L/2; X_0 Y_1, X_0 Z_1 X_2, Y_0 Y_1 Z_2 Z_5;
    Z_3 Z_5 (the orbit of Z_0 Z_2: coefficients 1 and -1/2, so that dividing them out is exact); under parity X_0 Z_1 and Z_0 X_1;
    twelve random strings.  Returns (observables, index of Z_0 Z_2, index of Z_3 Z_5, index of X_0 Z_1 or None)."""
    L = n_sites
    rng = np.random.default_rng(seed)
    obs = [(0, 0, 1.0), (0, 1, 2.0), (1, 0, 0.5), (1, 1, -1.25)]
    zz = {}
    for r in range(1, L // 2 + 1):
        m = _site(0, r)
        zz[r] = len(obs)
        obs += [(0, m, 1.0), (m, 0, 0.25 + 0.01 * r), (m, m, -0.75), (m, 1 << r, 1.5)]
    obs += [(_site(0, 1), _site(1), 0.3), (_site(0, 2), _site(1), -2.0), (_site(0, 1), _site(0, 1, 2, 5), 0.7)]
    i35 = len(obs)
    obs += [(0, _site(3, 5), -0.5)]
    ixz = None
    if parity:
        ixz = len(obs)
        obs += [(_site(0), _site(1), 1.0), (_site(1), _site(0), 1.0)]
    full = (1 << L) - 1
    obs += [(int(rng.integers(0, full + 1)), int(rng.integers(0, full + 1)), float(rng.uniform(-2, 2))) for _ in range(12)]
    return obs, zz[2], i35, ixz


def strings_of(block, term):
    return G.symmetrised_strings(block.n_sites, term, block.parity, block.inversion)


def is_zero(block, term, dtype):
    """The rules that answer +0.0 without a slot."""
    x, z = int(term[0]), int(term[1])
    real = np.dtype(dtype).kind != "c"
    return (len(strings_of(block, term)) == 0 or (real and bin(x & z).count("1") % 2 == 1) or
            (block.sector and bin(x).count("1") % 2 == 1))


def sweeps_of(block, obs, dtype):
    return -(-sum(not is_zero(block, t, dtype) for t in obs) // BATCH)


_REF = {}


def reference(block, dtype, n_local):
    """(c, observables, expected values, bounds, indices): want_k = coef_k Re <Psi, P_k Psi> correctly rounded, with
    bound_k = (2 (D S_k + 8) + 32) eps_d scale_k + eps_d |want_k|, scale_k = |coef_k| sum |Psi||P_k Psi|, S_k the distinct
    symmetrised strings, D = n_local."""
    key = (block.id, np.dtype(dtype).char)
    if key not in _REF:
        c = K.start_x(n_local, dtype, seed=11)
        obs, i02, i35, ixz = observable_set(block.n_sites, block.parity, 1000 * block.n_sites + block.m)
        psi = expand(block, c)
        states = block.states()
        want, bound = np.zeros(len(obs)), np.zeros(len(obs))
        for k, t in enumerate(obs):
            q = G.pauli_string_apply_np(block.n_sites, t, psi, states=states)
            want[k] = t[2] * E.dot_exact(psi, q).real
            s_k = len(strings_of(block, t))
            bound[k] = (2 * (n_local * s_k + 8) + 32) * E.EPS_D * abs(t[2]) * E.dot_abs(psi, q) + E.EPS_D * abs(want[k])
        c.setflags(write=False)
        _REF[key] = (c, obs, want, bound, (i02, i35, ixz))
    return _REF[key]
