"""generators.pauli_block_transfer_np, pauli_block_transfer_rows_np and transferred_strings — the CPU restatements of
ll_pauli_block_transfer — against the dense B_t^H P B_s c on rings of 4, 6 and 7 sites: every pair of non-empty blocks of both
kinds, strings with X, Y and Z that do NOT commute with the translation, and a two-term sum.  numpy only."""
import numpy as np
import pytest

from lambda_lanczos_amd import generators as G

TERM_LISTS = [[(0, 1, 1.0)],                    # Z_0
              [(1, 0, 1.0)],                    # X_0
              [(5, 0, 0.7)],                    # X_0 X_2
              [(1, 3, 1.3)],                    # Y_0 Z_1
              [(3, 3, -0.9)],                   # Y_0 Y_1
              [(1, 1, 1.0)],                    # Y_0
              [(3, 4, -0.5), (0, 3, 2.0)]]      # X_0 X_1 Z_2 + 2 Z_0 Z_1


def _dense_string(n_sites, term):
    """P as a dense 2^n x 2^n matrix from the definition P|s> = i^nY (-1)^popcount(s & z) |s ^ x>."""
    x, z = term[0], term[1]
    n = 1 << n_sites
    P = np.zeros((n, n), np.complex128)
    for s in range(n):
        P[s ^ x, s] = (1j ** (bin(x & z).count("1") & 3)) * (-1.0) ** bin(s & z).count("1")
    return P


def _blocks(kind, n_sites):
    out = []
    for nd in ([None] if kind == "momentum_full" else range(n_sites + 1)):
        for m in range(n_sites):
            shape = (n_sites, m) if nd is None else (n_sites, nd, m)
            B = G.full_momentum_embedding(n_sites, m) if nd is None else G.momentum_embedding(n_sites, nd, m)
            if B.shape[1]:
                out.append((nd, shape, B))
    return out


@pytest.mark.parametrize("kind", ["momentum_full", "momentum"])
@pytest.mark.parametrize("n_sites", [4, 6, 7])
def test_transfer_np_is_the_dense_product(kind, n_sites):
    rng = np.random.default_rng(n_sites)
    dense = [sum(t[2] * _dense_string(n_sites, t) for t in terms) for terms in TERM_LISTS]
    blocks = _blocks(kind, n_sites)
    pairs, worst = 0, 0.0
    for nd_s, shape_s, Bs in blocks:
        c = rng.standard_normal(Bs.shape[1]) + 1j * rng.standard_normal(Bs.shape[1])
        sel = slice(None) if nd_s is None else G.sector_states(n_sites, nd_s).astype(np.int64)
        for nd_t, shape_t, Bt in blocks:
            if nd_t != nd_s:
                continue
            for terms, P in zip(TERM_LISTS, dense):
                want = Bt.conj().T @ (P[sel][:, sel] @ (Bs @ c))
                scale = np.linalg.norm(c) * sum(abs(t[2]) for t in terms)
                got = G.pauli_block_transfer_np(kind, shape_s, shape_t, terms, c)
                rows, mag = G.pauli_block_transfer_rows_np(kind, shape_s, shape_t, terms, c)
                assert got.shape == want.shape == rows.shape == mag.shape
                worst = max(worst, float(np.max(np.abs(got - want))) / scale, float(np.max(np.abs(rows - want))) / scale)
                assert np.max(np.abs(got - want)) <= 64 * 2.0 ** -52 * scale, (shape_s, shape_t, terms)
                assert np.max(np.abs(rows - want)) <= 64 * 2.0 ** -52 * scale, (shape_s, shape_t, terms)
                assert np.all(np.abs(rows) <= mag * (1 + 1e-12))
                some = np.arange(0, want.shape[0], 2)
                r2, m2 = G.pauli_block_transfer_rows_np(kind, shape_s, shape_t, terms, c, rows=some)
                assert np.array_equal(r2, rows[some]) and np.array_equal(m2, mag[some])
            pairs += 1
    assert pairs >= n_sites * n_sites
    print("pairs", pairs, "worst error / (||c|| sum |coef|)", worst)


def test_transferred_strings_are_the_momentum_component():
    """sum over q of Pbar_q = P; Pbar_q is a sum of rotations with exact phases on the axes; the strings that are dropped are
    those whose period r has q r != 0 (mod L)."""
    L = 6
    for term in [(0, 1, 1.0), (9, 0, 1.0), (0b010101, 0b101010, 1.0), (3, 6, 1.0)]:
        total = {}
        for q in range(L):
            strings = G.transferred_strings(L, term, q)
            assert strings == sorted(strings)
            for x, z, w in strings:
                total[(x, z)] = total.get((x, z), 0.0) + w
        for key, w in total.items():
            assert abs(w - (1.0 if key == (term[0], term[1]) else 0.0)) <= 8 * 2.0 ** -52, (term, key, w)
    assert G.transferred_strings(6, (0b010101, 0, 1.0), 1) == [] and len(G.transferred_strings(6, (0b010101, 0, 1.0), 3)) == 2
    assert G.transferred_strings(4, (0, 1, 1.0), 1) == [(0, 1, 0.25), (0, 2, -0.25j), (0, 4, -0.25), (0, 8, 0.25j)]
    with pytest.raises(ValueError):
        G.transferred_strings(4, (16, 0, 1.0), 0)
    with pytest.raises(ValueError):
        G.pauli_block_transfer_np("symmetric", (4, 0), (4, 1), [(0, 1, 1.0)], np.ones(6))
    with pytest.raises(ValueError):
        G.pauli_block_transfer_np("momentum", (4, 2, 0), (4, 1, 0), [(0, 1, 1.0)], np.ones(2))
