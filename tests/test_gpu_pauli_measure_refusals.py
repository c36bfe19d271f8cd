"""The refusal texts of the five measuring entry points (ll_pauli_expect, ll_pauli_expect_block, ll_pauli_rdm,
ll_pauli_block_expand, ll_pauli_block_project), pinned byte for byte: the status code and the whole ll_last_error() of every
case below.  EXPECTED was recorded from the library as it stood before the entry points were given one shared host driver
(csrc/pauli_measure.hpp); a change of the host code around the kernels must reproduce it.

The cases, per entry point, on a 4-site ring in float64: each of the five Pauli kinds and a 4 x 4 CSR operator; an operator of a
second context; a null psi; for the two expectation calls a mask bit at n_sites and a coefficient that is not finite (for
ll_pauli_rdm, which takes no observables, a site at n_sites and a repeated site in their place; the embeddings take neither).
The embeddings take the six operators once as the block (target: the full space) and once as the target (block: the
full-space momentum block).  Three more cases per call fail two checks at once: which one is reported is part of the text.
A call that succeeds is recorded as (LL_OK, ""): what ll_last_error() holds after a success is not a contract."""
import ctypes as C

import numpy as np
import pytest

import lambda_lanczos_amd as L
from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G

pytestmark = pytest.mark.gpu

N_SITES = 4
KINDS = ["full", "sector", "momentum", "momentum_full", "symmetric", "csr"]


def _operators(ctx):
    ring = G.heisenberg_terms(N_SITES, 1.0, 0.8, periodic=True)
    tf = G.tfim_terms(N_SITES, 1.0, 0.7, periodic=True)
    return {
        "full": L.PauliOperator(ctx, N_SITES, tf, np.float64),
        "sector": L.PauliSectorOperator(ctx, N_SITES, 2, ring, np.float64),
        "momentum": L.PauliMomentumOperator(ctx, N_SITES, 2, 0, ring, np.float64),
        "momentum_full": L.PauliMomentumFullOperator(ctx, N_SITES, 0, tf, np.float64),
        "symmetric": L.PauliSymmetricOperator(ctx, N_SITES, 0, tf, np.float64, parity=1),
        "csr": L.CsrOperator(ctx, *G.laplace2d_np(2)),
    }


def table(ctx):
    """case id -> (status, ll_last_error() if the call failed else "")"""
    lib = capi.lib()
    ctx2 = L.Context(0)
    ops, ops2 = _operators(ctx), _operators(ctx2)
    psi = np.linspace(0.25, 1.0, 16)      # every basis here holds at most 16 values
    vec = np.zeros(16)
    psi_p, vec_p = capi.ptr(psi), capi.ptr(vec)
    got = {}

    def record(name, status):
        assert name not in got, name
        got[name] = (int(status), lib.ll_last_error().decode("utf-8") if status != capi.LL_OK else "")

    def expect(entry, op, obs=((0, 1, 1.0),), p=psi_p):
        arr, n_obs = L.engine._term_array(obs)
        out, sweeps = np.zeros(max(n_obs, 1)), C.c_int64(0)
        return getattr(lib, entry)(ctx.handle, op.handle, n_obs, arr, p, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(sweeps))

    def rdm(op, sites=(0, 2), p=psi_p):
        arr = (C.c_int32 * len(sites))(*sites)
        out, sweeps = np.zeros(2 * 4 ** len(sites)), C.c_int64(0)
        return lib.ll_pauli_rdm(ctx.handle, op.handle, len(sites), arr, p, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(sweeps))

    try:
        for entry, good in (("ll_pauli_expect", "full"), ("ll_pauli_expect_block", "momentum_full")):
            for k in KINDS:
                record("%s/%s" % (entry, k), expect(entry, ops[k]))
            record(entry + "/second-context", expect(entry, ops2[good]))
            record(entry + "/null-psi", expect(entry, ops[good], p=None))
            record(entry + "/mask-out-of-range", expect(entry, ops[good], obs=((0, 1, 1.0), (1 << N_SITES, 0, 1.0))))
            record(entry + "/coef-not-finite", expect(entry, ops[good], obs=((0, 1, 1.0), (1, 0, 1.0), (0, 2, float("inf")))))
            record(entry + "/second-context+csr", expect(entry, ops2["csr"]))
            record(entry + "/null-psi+csr", expect(entry, ops["csr"], p=None))
            record(entry + "/mask+coef", expect(entry, ops[good], obs=((1 << N_SITES, 0, float("nan")),)))
        for k in KINDS:
            record("ll_pauli_rdm/" + k, rdm(ops[k]))
        record("ll_pauli_rdm/second-context", rdm(ops2["full"]))
        record("ll_pauli_rdm/null-psi", rdm(ops["full"], p=None))
        record("ll_pauli_rdm/site-out-of-range", rdm(ops["full"], sites=(0, N_SITES)))
        record("ll_pauli_rdm/site-repeated", rdm(ops["sector"], sites=(1, 3, 1)))
        record("ll_pauli_rdm/second-context+csr", rdm(ops2["csr"]))
        record("ll_pauli_rdm/null-psi+csr", rdm(ops["csr"], p=None))
        record("ll_pauli_rdm/csr+site-out-of-range", rdm(ops["csr"], sites=(0, N_SITES)))
        for entry in ("ll_pauli_block_expand", "ll_pauli_block_project"):
            fn = getattr(lib, entry)
            for k in KINDS:
                record("%s/block-%s" % (entry, k), fn(ctx.handle, ops[k].handle, ops["full"].handle, psi_p, vec_p))
            for k in KINDS:
                record("%s/target-%s" % (entry, k), fn(ctx.handle, ops["momentum_full"].handle, ops[k].handle, psi_p, vec_p))
            record(entry + "/second-context-block", fn(ctx.handle, ops2["momentum_full"].handle, ops["full"].handle, psi_p, vec_p))
            record(entry + "/second-context-target", fn(ctx.handle, ops["momentum_full"].handle, ops2["full"].handle, psi_p, vec_p))
            record(entry + "/null-psi", fn(ctx.handle, ops["momentum_full"].handle, ops["full"].handle, None, vec_p))
            record(entry + "/second-context-both+csr", fn(ctx.handle, ops2["csr"].handle, ops2["csr"].handle, psi_p, vec_p))
            record(entry + "/null-psi+csr", fn(ctx.handle, ops["csr"].handle, ops["full"].handle, None, vec_p))
            record(entry + "/csr-both", fn(ctx.handle, ops["csr"].handle, ops["csr"].handle, psi_p, vec_p))
    finally:
        for o in list(ops.values()) + list(ops2.values()):
            o.close()
        ctx2.close()
    return got


EXPECTED = {
    "ll_pauli_expect/full": (0, ""),
    "ll_pauli_expect/sector": (0, ""),
    "ll_pauli_expect/momentum": (1, "invalid argument: the operator is a momentum block of an S_z sector: symmetrised observables are not built (an observable must be summed over the block's group first); measure on a full-space or S_z-sector operator"),
    "ll_pauli_expect/momentum_full": (1, "invalid argument: the operator is a momentum block of the full space: symmetrised observables are not built (an observable must be summed over the block's group first); measure on a full-space or S_z-sector operator"),
    "ll_pauli_expect/symmetric": (1, "invalid argument: the operator is a momentum / reflection / spin-inversion block: symmetrised observables are not built (an observable must be summed over the block's group first); measure on a full-space or S_z-sector operator"),
    "ll_pauli_expect/csr": (1, "invalid argument: the operator is a CSR operator: expectation values of Pauli strings need an operator that defines a spin basis (full-space or S_z-sector sum of Pauli strings)"),
    "ll_pauli_expect/second-context": (1, "invalid argument: the operator belongs to another context"),
    "ll_pauli_expect/null-psi": (1, "invalid argument: null argument"),
    "ll_pauli_expect/mask-out-of-range": (1, "invalid argument: observable 1: a mask bit at or above n_sites"),
    "ll_pauli_expect/coef-not-finite": (1, "invalid argument: observable 2: the coefficient is not finite"),
    "ll_pauli_expect/second-context+csr": (1, "invalid argument: the operator belongs to another context"),
    "ll_pauli_expect/null-psi+csr": (1, "invalid argument: null argument"),
    "ll_pauli_expect/mask+coef": (1, "invalid argument: observable 0: a mask bit at or above n_sites"),
    "ll_pauli_expect_block/full": (1, "invalid argument: the operator is a full-space sum of Pauli strings: its basis is not a symmetry block; measure with ll_pauli_expect"),
    "ll_pauli_expect_block/sector": (1, "invalid argument: the operator is a sum of Pauli strings on an S_z sector: its basis is not a symmetry block; measure with ll_pauli_expect"),
    "ll_pauli_expect_block/momentum": (0, ""),
    "ll_pauli_expect_block/momentum_full": (0, ""),
    "ll_pauli_expect_block/symmetric": (0, ""),
    "ll_pauli_expect_block/csr": (1, "invalid argument: the operator is a CSR operator: expectation values on a symmetry block need a momentum, full-momentum or momentum / reflection / spin-inversion block of a sum of Pauli strings"),
    "ll_pauli_expect_block/second-context": (1, "invalid argument: the operator belongs to another context"),
    "ll_pauli_expect_block/null-psi": (1, "invalid argument: null argument"),
    "ll_pauli_expect_block/mask-out-of-range": (1, "invalid argument: observable 1: a mask bit at or above n_sites"),
    "ll_pauli_expect_block/coef-not-finite": (1, "invalid argument: observable 2: the coefficient is not finite"),
    "ll_pauli_expect_block/second-context+csr": (1, "invalid argument: the operator belongs to another context"),
    "ll_pauli_expect_block/null-psi+csr": (1, "invalid argument: null argument"),
    "ll_pauli_expect_block/mask+coef": (1, "invalid argument: observable 0: a mask bit at or above n_sites"),
    "ll_pauli_rdm/full": (0, ""),
    "ll_pauli_rdm/sector": (0, ""),
    "ll_pauli_rdm/momentum": (1, "invalid argument: the operator is a momentum block of an S_z sector: reduced density matrices of symmetry blocks are not built (a site is not a tensor factor of the block's basis); measure on a full-space or S_z-sector operator"),
    "ll_pauli_rdm/momentum_full": (1, "invalid argument: the operator is a momentum block of the full space: reduced density matrices of symmetry blocks are not built (a site is not a tensor factor of the block's basis); measure on a full-space or S_z-sector operator"),
    "ll_pauli_rdm/symmetric": (1, "invalid argument: the operator is a momentum / reflection / spin-inversion block: reduced density matrices of symmetry blocks are not built (a site is not a tensor factor of the block's basis); measure on a full-space or S_z-sector operator"),
    "ll_pauli_rdm/csr": (1, "invalid argument: the operator is a CSR operator: a reduced density matrix needs an operator that defines a spin basis (full-space or S_z-sector sum of Pauli strings)"),
    "ll_pauli_rdm/second-context": (1, "invalid argument: the operator belongs to another context"),
    "ll_pauli_rdm/null-psi": (1, "invalid argument: null argument"),
    "ll_pauli_rdm/site-out-of-range": (1, "invalid argument: site 1 of the list (4) is outside [0, n_sites = 4)"),
    "ll_pauli_rdm/site-repeated": (1, "invalid argument: site 2 of the list (1) is repeated"),
    "ll_pauli_rdm/second-context+csr": (1, "invalid argument: the operator belongs to another context"),
    "ll_pauli_rdm/null-psi+csr": (1, "invalid argument: null argument"),
    "ll_pauli_rdm/csr+site-out-of-range": (1, "invalid argument: the operator is a CSR operator: a reduced density matrix needs an operator that defines a spin basis (full-space or S_z-sector sum of Pauli strings)"),
    "ll_pauli_block_expand/block-full": (1, "invalid argument: the block operator is a full-space sum of Pauli strings: it must be a momentum, full-momentum or momentum / reflection / spin-inversion block of a sum of Pauli strings"),
    "ll_pauli_block_expand/block-sector": (1, "invalid argument: the block operator is a sum of Pauli strings on an S_z sector: it must be a momentum, full-momentum or momentum / reflection / spin-inversion block of a sum of Pauli strings"),
    "ll_pauli_block_expand/block-momentum": (0, ""),
    "ll_pauli_block_expand/block-momentum_full": (0, ""),
    "ll_pauli_block_expand/block-symmetric": (0, ""),
    "ll_pauli_block_expand/block-csr": (1, "invalid argument: the block operator is a CSR operator: it must be a momentum, full-momentum or momentum / reflection / spin-inversion block of a sum of Pauli strings"),
    "ll_pauli_block_expand/target-full": (0, ""),
    "ll_pauli_block_expand/target-sector": (1, "invalid argument: a full-space block does not fit an S_z-sector target: use a full-space target (block: a momentum block of the full space, n_sites 4, n_down -1; target: a sum of Pauli strings on an S_z sector, n_sites 4, n_down 2)"),
    "ll_pauli_block_expand/target-momentum": (1, "invalid argument: the target operator is a momentum block of an S_z sector: it must be a full-space or S_z-sector sum of Pauli strings, which names the basis of the expanded state"),
    "ll_pauli_block_expand/target-momentum_full": (1, "invalid argument: the target operator is a momentum block of the full space: it must be a full-space or S_z-sector sum of Pauli strings, which names the basis of the expanded state"),
    "ll_pauli_block_expand/target-symmetric": (1, "invalid argument: the target operator is a momentum / reflection / spin-inversion block: it must be a full-space or S_z-sector sum of Pauli strings, which names the basis of the expanded state"),
    "ll_pauli_block_expand/target-csr": (1, "invalid argument: the target operator is a CSR operator: it must be a full-space or S_z-sector sum of Pauli strings, which names the basis of the expanded state"),
    "ll_pauli_block_expand/second-context-block": (1, "invalid argument: the block operator belongs to another context"),
    "ll_pauli_block_expand/second-context-target": (1, "invalid argument: the target operator belongs to another context"),
    "ll_pauli_block_expand/null-psi": (1, "invalid argument: ll_pauli_block_expand: null argument"),
    "ll_pauli_block_expand/second-context-both+csr": (1, "invalid argument: the block operator belongs to another context"),
    "ll_pauli_block_expand/null-psi+csr": (1, "invalid argument: ll_pauli_block_expand: null argument"),
    "ll_pauli_block_expand/csr-both": (1, "invalid argument: the block operator is a CSR operator: it must be a momentum, full-momentum or momentum / reflection / spin-inversion block of a sum of Pauli strings"),
    "ll_pauli_block_project/block-full": (1, "invalid argument: the block operator is a full-space sum of Pauli strings: it must be a momentum, full-momentum or momentum / reflection / spin-inversion block of a sum of Pauli strings"),
    "ll_pauli_block_project/block-sector": (1, "invalid argument: the block operator is a sum of Pauli strings on an S_z sector: it must be a momentum, full-momentum or momentum / reflection / spin-inversion block of a sum of Pauli strings"),
    "ll_pauli_block_project/block-momentum": (0, ""),
    "ll_pauli_block_project/block-momentum_full": (0, ""),
    "ll_pauli_block_project/block-symmetric": (0, ""),
    "ll_pauli_block_project/block-csr": (1, "invalid argument: the block operator is a CSR operator: it must be a momentum, full-momentum or momentum / reflection / spin-inversion block of a sum of Pauli strings"),
    "ll_pauli_block_project/target-full": (0, ""),
    "ll_pauli_block_project/target-sector": (1, "invalid argument: a full-space block does not fit an S_z-sector target: use a full-space target (block: a momentum block of the full space, n_sites 4, n_down -1; target: a sum of Pauli strings on an S_z sector, n_sites 4, n_down 2)"),
    "ll_pauli_block_project/target-momentum": (1, "invalid argument: the target operator is a momentum block of an S_z sector: it must be a full-space or S_z-sector sum of Pauli strings, which names the basis of the expanded state"),
    "ll_pauli_block_project/target-momentum_full": (1, "invalid argument: the target operator is a momentum block of the full space: it must be a full-space or S_z-sector sum of Pauli strings, which names the basis of the expanded state"),
    "ll_pauli_block_project/target-symmetric": (1, "invalid argument: the target operator is a momentum / reflection / spin-inversion block: it must be a full-space or S_z-sector sum of Pauli strings, which names the basis of the expanded state"),
    "ll_pauli_block_project/target-csr": (1, "invalid argument: the target operator is a CSR operator: it must be a full-space or S_z-sector sum of Pauli strings, which names the basis of the expanded state"),
    "ll_pauli_block_project/second-context-block": (1, "invalid argument: the block operator belongs to another context"),
    "ll_pauli_block_project/second-context-target": (1, "invalid argument: the target operator belongs to another context"),
    "ll_pauli_block_project/null-psi": (1, "invalid argument: ll_pauli_block_project: null argument"),
    "ll_pauli_block_project/second-context-both+csr": (1, "invalid argument: the block operator belongs to another context"),
    "ll_pauli_block_project/null-psi+csr": (1, "invalid argument: ll_pauli_block_project: null argument"),
    "ll_pauli_block_project/csr-both": (1, "invalid argument: the block operator is a CSR operator: it must be a momentum, full-momentum or momentum / reflection / spin-inversion block of a sum of Pauli strings"),
}


def test_refusal_texts_are_unchanged(ctx):
    got = table(ctx)
    for name in sorted(set(got) | set(EXPECTED)):
        print(name, got.get(name))
    assert len(got) == 75
    assert got == EXPECTED
