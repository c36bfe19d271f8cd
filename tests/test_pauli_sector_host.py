"""Host side of the S_z-sector operator (ll_op_create_pauli_sector_*): the generators that define the sector's basis, its rank
tables and the sector block of the expanded matrix (lambda_lanczos_amd.generators), checked against their definitions.  No GPU."""
import math

import numpy as np
import pytest

from lambda_lanczos_amd import generators as G


def _popcount(v):
    v = np.asarray(v, dtype=np.uint64)
    return sum(((v >> np.uint64(p)) & np.uint64(1)).astype(np.int64) for p in range(32))


def j1j2_terms(n_sites, j1=1.0, j2=0.4, delta=0.7):
    terms = G.heisenberg_terms(n_sites, j1, delta, periodic=False)
    for j in range(n_sites - 2):
        m = (1 << j) | (1 << (j + 2))
        terms += [(m, 0, 0.25 * j2), (m, m, 0.25 * j2), (0, m, 0.25 * j2)]
    return terms


MODELS = {
    "heisenberg": lambda L: G.heisenberg_terms(L, 1.0, 1.0, periodic=True),
    "j1j2": j1j2_terms,
    "dm": lambda L: G.dm_terms(L, 0.3, periodic=True) + G.heisenberg_terms(L, 1.0, 0.8),
    "zfield": lambda L: G.zfield_terms(L, 0.37) + G.heisenberg_terms(L, 1.0, 1.0, periodic=False),
}


def test_sector_states_are_the_ascending_states_of_the_sector():
    for L in range(0, 13):
        for m in range(L + 1):
            s = G.sector_states(L, m)
            assert s.dtype == np.uint32 and s.shape == (math.comb(L, m),)
            assert np.all(_popcount(s) == m) and np.all(s < (1 << L) if L else s == 0)
            assert np.all(np.diff(s.astype(np.int64)) > 0)
    s = G.sector_states(30, 15)
    assert s.shape == (math.comb(30, 15),)
    assert s[0] == (1 << 15) - 1 and s[-1] == ((1 << 15) - 1) << 15
    with pytest.raises(ValueError):
        G.sector_states(4, 5)


def test_rank_tables_give_every_state_its_index():
    for L in range(0, 15):
        for m in range(L + 1):
            s = G.sector_states(L, m).astype(np.int64)
            for h in sorted({0, 1 % (L + 1), L // 2, (L + 1) // 2, max(L - 1, 0), L}):
                lo, hi = G.sector_rank_tables(L, m, h)
                assert lo.dtype == np.uint32 and hi.dtype == np.uint32
                assert lo.shape == (1 << h,) and hi.shape == (1 << (L - h),)
                idx = lo[s & ((1 << h) - 1)].astype(np.int64) + hi[s >> h]
                assert np.array_equal(idx, np.arange(s.shape[0])), (L, m, h)
    s = G.sector_states(30, 15)
    pick = np.random.default_rng(11).integers(0, s.shape[0], 10_000)
    pick[:2] = 0, s.shape[0] - 1
    for h in (14, 15, 16):
        lo, hi = G.sector_rank_tables(30, 15, h)
        sv = s[pick].astype(np.int64)
        assert np.array_equal(lo[sv & ((1 << h) - 1)].astype(np.int64) + hi[sv >> h], pick), h


def _dense(csr, n_cols):
    rp, ci, va = csr
    a = np.zeros((rp.shape[0] - 1, n_cols), dtype=np.complex128)
    np.add.at(a, (np.repeat(np.arange(rp.shape[0] - 1), np.diff(rp)), ci), va)
    return a


@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("merge", [True, False], ids=["merged", "per_term"])
def test_sector_csr_is_the_block_of_the_full_matrix(model, merge):
    for L in (1, 2, 3, 4, 7, 10):
        if model == "j1j2" and L < 3:
            continue
        terms = MODELS[model](L)
        dtype = np.complex128 if model == "dm" else np.float64
        full = G.pauli_csr(L, terms, dtype, merge)
        fd = _dense(full, 1 << L)
        for m in sorted({0, 1, L // 2, L - 1, L} & set(range(L + 1))):
            st = G.sector_states(L, m).astype(np.int64)
            rp, ci, va = G.pauli_sector_csr(L, m, terms, dtype, merge)
            assert rp.dtype == np.int64 and ci.dtype == np.int32 and va.dtype == np.dtype(dtype)
            assert rp.shape == (st.shape[0] + 1,) and rp[-1] == ci.shape[0] == va.shape[0]
            assert np.all((ci >= 0) & (ci < st.shape[0]))
            assert np.array_equal(_dense((rp, ci, va), st.shape[0]), fd[np.ix_(st, st)]), (L, m)
            if merge:   # same entries in the same order as the full matrix's rows, columns renumbered
                frp, fci, fva = full
                rank = {int(v): k for k, v in enumerate(st)}
                for i in (0, st.shape[0] // 2, st.shape[0] - 1):
                    ent = [(rank[int(c)], v) for c, v in zip(fci[frp[st[i]]:frp[st[i] + 1]], fva[frp[st[i]]:frp[st[i] + 1]])
                           if int(c) in rank]
                    assert [e[0] for e in ent] == list(ci[rp[i]:rp[i + 1]])
                    assert [e[1] for e in ent] == list(va[rp[i]:rp[i + 1]])


@pytest.mark.parametrize("model", sorted(MODELS))
def test_sector_rows_have_no_weight_outside_the_sector(model):
    """The rows of a sector of an S_z-conserving H: every merged entry that leaves the sector is exactly zero (pauli_csr drops
    exact zeros, so none is stored), which is what the sector operator's creation demands of its input."""
    for L in (3, 6, 10):
        terms = MODELS[model](L)
        dtype = np.complex128 if model == "dm" else np.float64
        rp, ci, va = G.pauli_csr(L, terms, dtype, merge=True)
        rows = np.repeat(np.arange(1 << L), np.diff(rp))
        assert np.array_equal(_popcount(rows), _popcount(ci)), (model, L)
        for m in range(L + 1):
            srp = G.pauli_sector_csr(L, m, terms, dtype, merge=True)[0]
            st = G.sector_states(L, m).astype(np.int64)
            assert np.array_equal(np.diff(srp), rp[st + 1] - rp[st])     # nothing was discarded


def test_the_transverse_field_chain_leaves_every_sector():
    """What the conservation check has to catch: the block pauli_sector_csr discards is not zero for a field along x."""
    L = 6
    terms = G.tfim_terms(L, 1.0, 1.5)
    rp, ci, va = G.pauli_csr(L, terms, np.float64, merge=True)
    for m in range(L + 1):
        st = G.sector_states(L, m).astype(np.int64)
        srp, sci, sva = G.pauli_sector_csr(L, m, terms, np.float64, merge=True)
        dropped = int(np.sum(rp[st + 1] - rp[st])) - int(srp[-1])
        assert dropped == L * st.shape[0]            # every state's L single-spin flips
        inside = np.isin(ci, st)
        rows = np.repeat(np.arange(1 << L), np.diff(rp))
        out = np.isin(rows, st) & ~inside
        assert np.all(np.abs(va[out]) == 1.5) and out.sum() == dropped


def test_model_term_lists():
    assert G.dm_terms(3, 0.5, periodic=False) == [(0b011, 0b010, 0.5), (0b011, 0b001, -0.5), (0b110, 0b100, 0.5), (0b110, 0b010, -0.5)]
    assert len(G.dm_terms(4, 1.0, periodic=True)) == 8 and len(G.dm_terms(2, 1.0, periodic=True)) == 2
    assert G.zfield_terms(3, 0.25) == [(0, 1, -0.25), (0, 2, -0.25), (0, 4, -0.25)]
    a = _dense(G.pauli_csr(4, G.dm_terms(4, 0.7), np.complex128), 16)
    assert np.array_equal(a, a.conj().T) and np.any(a.imag != 0)
    with pytest.raises(ValueError):
        G.pauli_csr(4, G.dm_terms(4, 0.7), np.float64)     # odd numbers of Y: complex
