"""CPU-side checks of ll_pauli_expect_block: generators.symmetrised_strings — the numpy mirror of csrc/pauli_expect_block_plan.hpp —
through the identity the feature rests on: for a state Psi = B c of a symmetry block,
    <Psi| P |Psi> = c^H M c,     M = pauli_symmetric_csr(the strings of P averaged over the block's group),
with B from the embeddings of generators.py; on rings of 6 to 9 sites (short orbits included), momentum 0, L/2 and general,
parity and inversion +-1, with and without an S_z sector.  And the all-null call, refused before a device is touched."""
import ctypes as C

import numpy as np
import pytest

import contract_cases as K
from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G
from pauli_expect_block_cases import Block, expand, observable_set, strings_of
from util import csr_matvec

#          n_sites, m, parity, inversion, n_down
BLOCKS = [(6, 0, 0, 0, None), (6, 3, 0, 0, None), (7, 2, 0, 0, None), (8, 0, 1, 1, None), (8, 4, -1, -1, None), (8, 0, -1, 0, None),
          (9, 3, 0, 1, None), (9, 0, 1, 0, None), (8, 0, 1, 1, 4), (8, 3, 0, 0, 4), (6, 3, 0, -1, 3), (9, 0, -1, 0, 4), (6, 0, 1, -1, None)]


@pytest.mark.parametrize("spec", BLOCKS, ids=["L%d-m%d-p%d-z%d-nd%s" % b for b in BLOCKS])
def test_block_quadratic_form_of_the_symmetrised_strings(spec):
    n_sites, m, parity, inversion, n_down = spec
    block = Block("symmetric", n_sites, m, parity, inversion, n_down)
    reps, _ = G.symmetric_basis(n_sites, m, parity, inversion, n_down)
    assert reps.shape[0] > 0
    c = K.start_x(reps.shape[0], np.complex128, seed=5)
    psi = expand(block, c)
    assert abs(np.vdot(psi, psi) - np.vdot(c, c)) <= 1e-12 * abs(np.vdot(c, c))   # B is an isometry
    obs, _, _, _ = observable_set(n_sites, parity, 77 * n_sites + m)
    cancelled, worst = 0, 0.0
    for t in obs:
        sym = strings_of(block, t)
        q = G.pauli_string_apply_np(n_sites, t, psi, states=block.states())
        want = np.vdot(psi, q)
        if sym:
            assert abs(sum(w for _, _, w in sym) - 1.0) <= 1e-15 * len(sym)
            assert sym == sorted(sym) and len({(x, z) for x, z, _ in sym}) == len(sym)
            got = np.vdot(c, csr_matvec(G.pauli_symmetric_csr(n_sites, m, parity, inversion, sym, np.complex128, n_down=n_down), c))
        else:   # every image cancelled: the flip is in use and popcount(z) is odd
            assert inversion and bin(t[1]).count("1") % 2 == 1
            cancelled += 1
            got = 0.0
        scale = np.sum(np.abs(psi) * np.abs(q)) + 1e-300
        worst = max(worst, abs(got - want) / scale)
        assert abs(got - want) <= 1e-12 * scale, (t, got, want)
    assert (cancelled > 0) == bool(inversion)
    print("worst |c^H M c - Psi^H P Psi| / sum |Psi||P Psi|", spec, worst)


def test_symmetrised_strings_by_hand():
    # Z_0 Z_2 on 6 sites under the shift alone: six images of weight 1/6; with the reflection the same six, each met twice
    want = sorted((0, ((5 << j) | (5 >> (6 - j))) & 63, 1.0 / 6.0) for j in range(6))
    assert G.symmetrised_strings(6, (0, 5, 3.0)) == want                      # the coefficient is not in the weights
    assert G.symmetrised_strings(6, (0, 5, 1.0), parity=1) == want
    assert G.symmetrised_strings(6, (0, 5, 1.0), parity=-1, inversion=1) == want
    assert G.symmetrised_strings(6, (0, 40, 1.0)) == want   # Z_3 Z_5: the same orbit, the same list
    # Z_0 Z_3: a short orbit — three distinct images of weight 2/6
    assert G.symmetrised_strings(6, (0, 9, 1.0)) == [(0, 9, 2.0 / 6.0), (0, 18, 2.0 / 6.0), (0, 36, 2.0 / 6.0)]
    # Z_0 under the flip: every image cancels; X_0 does not
    assert G.symmetrised_strings(6, (0, 1, 1.0), inversion=-1) == []
    assert len(G.symmetrised_strings(6, (1, 0, 1.0), inversion=-1)) == 6
    # X_0 Z_1 and Z_0 X_1 are mirror images: one list under the reflection, two without it
    assert G.symmetrised_strings(6, (1, 2, 1.0), parity=1) == G.symmetrised_strings(6, (2, 1, 1.0), parity=1)
    assert G.symmetrised_strings(6, (1, 2, 1.0)) != G.symmetrised_strings(6, (2, 1, 1.0))
    with pytest.raises(ValueError):
        G.symmetrised_strings(3, (8, 0, 1.0))


def test_all_null_call_is_refused_before_a_device_is_touched():
    lib = capi.lib()
    sweeps = C.c_int64(-7)
    st = lib.ll_pauli_expect_block(None, None, 0, None, None, None, C.byref(sweeps))
    assert st == capi.LL_ERR_INVALID and b"null argument" in lib.ll_last_error()
    assert sweeps.value == -7
    st = lib.ll_pauli_expect_block(None, None, 3, None, None, None, None)
    assert st == capi.LL_ERR_INVALID and b"null argument" in lib.ll_last_error()
