"""CPU-side checks of the torus generators behind ll_op_create_pauli_torus (generators.torus_basis, torus_embedding,
pauli_torus_csr, heisenberg_torus_terms, ...): the dimensions of the blocks against a table computed by direct orbit
enumeration (with its sum rules), B^H B = 1 and the block B^H H B against the gather form, the ground energy of the 4 x 4
Heisenberg torus, the ring limit, the bond lists, and the C entry point's declaration (one untyped name, in the header and in the
Python prototypes alike)."""
import math
import re

import numpy as np
import pytest

from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G
from util import csr_matvec

E0_4X4 = -11.228483208428853     # numpy eigvalsh of the (0, 0) block of heisenberg_torus_terms(4, 4) at n_down = 8: 32 bonds


def _dims(lx, ly, n_down=None):
    return {(mx, my): G.torus_basis(lx, ly, mx, my, n_down)[0].shape[0] for mx in range(lx) for my in range(ly)}


def _table(lx, ly, special, rest):
    return {(mx, my): special.get((mx, my), rest) for mx in range(lx) for my in range(ly)}


DIMS = [
    (2, 2, None, _table(2, 2, {(0, 0): 7}, 3), 16),
    (3, 2, None, {(0, 0): 14, (0, 1): 10, (1, 0): 11, (2, 0): 11, (1, 1): 9, (2, 1): 9}, 64),
    (3, 3, None, _table(3, 3, {(0, 0): 64}, 56), 512),
    (3, 4, None, _table(3, 4, {(0, 0): 352, (0, 2): 348, (0, 1): 338, (0, 3): 338, (1, 0): 346, (2, 0): 346, (1, 2): 344, (2, 2): 344},
                        335), 4096),
    (4, 2, 4, _table(4, 2, {(0, 0): 12, (2, 0): 10}, 8), 70),
    (4, 3, 6, _table(4, 3, {(0, 0): 80, (2, 0): 80, (0, 1): 78, (0, 2): 78, (2, 1): 78, (2, 2): 78, (1, 0): 76, (3, 0): 76}, 75), 924),
    (4, 4, 8, _table(4, 4, {(0, 0): 822, (0, 2): 816, (2, 0): 816, (2, 2): 816}, 800), 12870),
    (4, 4, None, _table(4, 4, {(0, 0): 4156, (0, 2): 4140, (2, 0): 4140, (2, 2): 4140}, 4080), 65536),
]


@pytest.mark.parametrize("lx,ly,n_down,want,total", DIMS, ids=["%dx%d-nd%s" % d[:3] for d in DIMS])
def test_block_dimensions_against_the_table(lx, ly, n_down, want, total):
    got = _dims(lx, ly, n_down)
    assert got == want
    assert sum(got.values()) == total == (1 << (lx * ly) if n_down is None else math.comb(lx * ly, n_down))


def test_block_dimensions_of_the_5_by_4_torus_at_half_filling():
    for (mx, my), D in {(0, 0): 9252, (0, 2): 9252, (1, 2): 9250}.items():
        reps, R = G.torus_basis(5, 4, mx, my, 10)
        assert reps.shape[0] == D and np.all(np.diff(reps.astype(np.int64)) > 0) and np.all(20 % R == 0)


def test_bonds_are_distinct_pairs():
    assert G.torus_bonds(2, 2, 1, 0) == [(0, 1), (2, 3)]                     # lx = 2: one bond per pair, not two
    assert G.torus_bonds(2, 2, 0, 1) == [(0, 2), (1, 3)]
    assert G.torus_bonds(2, 2, 1, 1) == G.torus_bonds(2, 2, 1, -1) == [(0, 3), (1, 2)]
    assert G.torus_bonds(4, 1, 0, 1) == [] and len(G.torus_bonds(4, 1, 1, 0)) == 4
    assert len(G.torus_bonds(4, 4, 1, 0)) == len(G.torus_bonds(4, 4, 0, 1)) == 16
    assert len(G.heisenberg_torus_terms(4, 4)) == 3 * 32 and len(G.heisenberg_torus_terms(4, 4, 1.0, 0.5)) == 3 * 64
    assert len(G.heisenberg_torus_terms(2, 2, 1.0, 0.5)) == 3 * 6
    assert all(c == 0.25 for _, _, c in G.heisenberg_torus_terms(3, 3))
    assert sorted(G.heisenberg_torus_terms(6, 1)) == sorted(G.heisenberg_terms(6, 1.0, 1.0, periodic=True))
    assert sorted(G.tfim_torus_terms(6, 1, 1.0, 0.7)) == sorted(G.tfim_terms(6, 1.0, 0.7, periodic=True))
    assert len(G.tfim_torus_terms(4, 3, 1.0, 0.7)) == 24 + 12


SHAPES = [(2, 2, None), (3, 2, None), (2, 3, None), (3, 3, None), (4, 2, None), (4, 2, 4), (4, 3, 6), (3, 4, 5)]


@pytest.mark.parametrize("lx,ly,n_down", SHAPES, ids=["%dx%d-nd%s" % s for s in SHAPES])
def test_embedding_is_an_isometry_and_the_block_is_the_gather_form(lx, ly, n_down):
    n = lx * ly
    terms = G.heisenberg_torus_terms(lx, ly, 1.0, 0.5)
    if n_down is None:
        terms = terms + G.tfim_torus_terms(lx, ly, 0.3, 0.45)        # breaks S_z, keeps both translations
        H = G.pauli_csr(n, terms, np.complex128)
    else:
        H = G.pauli_sector_csr(n, n_down, terms, np.complex128)
    assert G.torus_translation_fault(lx, ly, terms) is None
    rows = H[0].shape[0] - 1
    total = 0
    for mx in range(lx):
        for my in range(ly):
            B = G.torus_embedding(lx, ly, mx, my, n_down)
            reps, R = G.torus_basis(lx, ly, mx, my, n_down)
            D = reps.shape[0]
            total += D
            assert B.shape == (rows, D)
            if D == 0:
                continue
            assert np.max(np.abs(B.conj().T @ B - np.eye(D))) <= 1e-14
            HB = np.stack([csr_matvec(H, np.ascontiguousarray(B[:, k])) for k in range(D)], 1)
            blk = B.conj().T @ HB
            assert np.max(np.abs(blk - blk.conj().T)) <= 1e-13
            rp, ci, va = G.pauli_torus_csr(lx, ly, mx, my, terms, np.complex128, n_down=n_down)
            dense = np.zeros((D, D), np.complex128)
            np.add.at(dense, (np.repeat(np.arange(D), np.diff(rp)), ci), va)
            assert np.max(np.abs(dense - blk)) <= 1e-13, (mx, my)
            # H commutes with the group: it does not leave the block
            assert np.max(np.abs(HB - B @ blk)) <= 1e-12
            one = G.pauli_torus_csr(lx, ly, mx, my, terms, np.complex128, n_down=n_down, merge=False)
            x = np.cos(np.arange(D) * 0.37) + 1j * np.sin(np.arange(D) * 0.11)
            assert np.max(np.abs(csr_matvec(one, x) - dense @ x)) <= 1e-12
    assert total == rows


def test_ground_energy_of_the_4_by_4_heisenberg_torus():
    terms = G.heisenberg_torus_terms(4, 4)
    rp, ci, va = G.pauli_torus_csr(4, 4, 0, 0, terms, np.float64, n_down=8)
    D = rp.shape[0] - 1
    assert D == 822
    dense = np.zeros((D, D))
    np.add.at(dense, (np.repeat(np.arange(D), np.diff(rp)), ci), va)
    assert np.max(np.abs(dense - dense.T)) <= 1e-14
    assert abs(np.linalg.eigvalsh(dense)[0] - E0_4X4) <= 1e-12


@pytest.mark.parametrize("L,m,n_down", [(8, 5, None), (9, 3, None), (12, 5, 6), (6, 0, None)])
def test_a_torus_of_one_row_or_one_column_is_the_ring(L, m, n_down):
    terms = G.xyz_terms(L, 1.0, 0.6, 0.8) if n_down is None else G.heisenberg_terms(L, 1.0, 1.0, periodic=True)
    want = G.pauli_symmetric_csr(L, m, 0, 0, terms, np.complex128, n_down=n_down)
    for lx, ly, mx, my in ((L, 1, m, 0), (1, L, 0, m)):
        reps, R = G.torus_basis(lx, ly, mx, my, n_down)
        ring_reps, ring_R = G.symmetric_basis(L, m, 0, 0, n_down)
        assert np.array_equal(reps, ring_reps) and np.array_equal(R, ring_R)
        got = G.pauli_torus_csr(lx, ly, mx, my, terms, np.complex128, n_down=n_down)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))          # the same bits
        assert G.torus_symmetrised_strings(lx, ly, (3, 5, 1.0)) == G.symmetrised_strings(L, (3, 5, 1.0))


def test_translation_faults_and_argument_checks():
    cyl = [t for t in G.heisenberg_torus_terms(4, 3) if not (t[0] | t[1]) == (1 << 0) | (1 << 8)]   # the bond (0,0)-(0,2) cut
    assert G.torus_translation_fault(4, 3, G.heisenberg_torus_terms(4, 3)) is None
    d, t = G.torus_translation_fault(4, 3, cyl)
    assert d in ("x", "y")
    open_y = [t for t in G.heisenberg_torus_terms(4, 3) if not any((t[0] | t[1]) == (1 << x) | (1 << (x + 8)) for x in range(4))]
    assert G.torus_translation_fault(4, 3, open_y)[0] == "y"               # an open cylinder: T_x holds, T_y does not
    ring16 = G.heisenberg_terms(16, 1.0, 1.0, periodic=True)
    assert G.torus_translation_fault(4, 4, ring16)[0] == "x" and G.torus_translation_fault(16, 1, ring16) is None
    with pytest.raises(ValueError):
        G.pauli_torus_csr(4, 3, 0, 0, open_y)
    with pytest.raises(ValueError):
        G.pauli_torus_csr(4, 4, 1, 0, G.heisenberg_torus_terms(4, 4), np.float64)
    for bad in ((0, 4, 0, 0), (4, 8, 0, 0), (4, 4, 4, 0), (4, 4, 0, -1)):
        with pytest.raises(ValueError):
            G.torus_basis(*bad)
    with pytest.raises(ValueError):
        G.torus_basis(4, 4, 0, 0, 17)
    assert G.torus_symmetrised_strings(4, 4, (0, 1 | (1 << 5), 2.0)) == G.torus_symmetrised_strings(4, 4, (0, (1 << 6) | (1 << 11), 1.0))
    assert abs(sum(w for _, _, w in G.torus_symmetrised_strings(4, 3, (5, 3, 1.0))) - 1.0) <= 1e-15


def test_the_entry_point_is_declared_once_untyped_in_header_and_prototypes():
    name = "ll_op_create_pauli_torus"
    with open(capi.HEADER_PATH) as f:
        declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(ll_[a-z0-9_]+)\s*\(", f.read(), flags=re.M))
    assert name in declared and name in capi.PROTOTYPES
    for sfx in "dzsc":
        assert name + "_" + sfx not in declared and name + "_" + sfx not in capi.PROTOTYPES
    restype, argtypes = capi.PROTOTYPES[name]
    assert len(argtypes) == 10                                              # ctx, storage, lx, ly, n_down, mx, my, n_terms, terms, out
    lib = capi.lib()
    st = lib.ll_op_create_pauli_torus(None, ord("d"), 4, 4, -1, 0, 0, 0, None, None)
    assert st == capi.LL_ERR_INVALID                                        # refused before a device is touched
