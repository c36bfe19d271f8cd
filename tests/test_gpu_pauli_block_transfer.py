"""A sum of Pauli strings between two momentum blocks of a ring (ll_pauli_block_transfer; csrc/pauli_block_transfer.hip, planned by
csrc/pauli_block_transfer_plan.hpp) on rings of 4, 6, 7, 8 and 12 sites: both kinds, every non-empty (source, target) pair —
q = 0 and q != 0 alike —, the terms Z_0, X_0, X_0 X_2, Y_0 Z_1 (complex only) and a two-term sum, all four storage types where
both blocks are real (the `_tids` rule of test_gpu_pauli_block_embed.py), z and c otherwise.  Reference:
generators.pauli_block_transfer_np (expand, apply, project, by the definition).

The contract, with eps_d = 2^-52, eps_T the storage type's epsilon, |.| the modulus, per row a of the target block:
    |got - want| <= K eps_d M(a) + eps_T |want|,     K = 2 (N + 8) + 24,  N = n_sites * n_terms,
M(a) = |B_t|^T (sum_j |coef_j| |P_j|) |B_s| |c| (a): the sum of the moduli of everything the row gathers — the R_a <= n_sites rows
of B_t times n_terms partners each, N terms at most; the kernel's merged strings are sums of these (at most N of them, the same
total modulus or less).  The constant, in the form of exact_ref.dot_bound (u = eps_d / 2):
    2 (N + 8)   a rounding per addition of either side's sum (the kernel: the weights of a group, then one fma per group; the
                reference: numpy's sums over the orbit) and per product, x 2 for the four-product complex terms, + 8 as there
    + 24        per gathered term the kernel carries the host's weight (phase table entry 2 u, coef / r and the product 2 u),
                sqrt(R_a / R_b) (2 u) and its product (u), the source's phase entry (2 u) and the complex product (2 u), the
                complex fma (2 u): 13 u per component, sqrt(2) times that for the modulus, 9.2 eps_d; the reference forms
                val c (phase / sqrt(R): 3 u, product 2 u), the exact string, conj(val) phi (5 u): 10 u, 7.1 eps_d.  16.3 < 24.
There is no n in it and nothing is measured.  eps_T |want| covers the storage rounding.
norm2: |norm2 - sum |got|^2| <= 2 (D_t + 8) eps_d sum |got|^2 (dot_bound over the D_t squares of the stored output).
Inputs and outputs in guarded NaN-padded device buffers at shifts 0 and 1 and on the host: the same bits, intact guards, the
input unchanged, an output prefilled with NaN fully written."""
import numpy as np
import pytest

import contract_cases as K
import exact_ref as E
import lambda_lanczos_amd as L
from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G
from pauli_cases import _cplx, _eps
from pauli_expect_block_cases import Block
from guarded import pattern
from test_gpu_accuracy_contracts import _guarded, _unguard
from test_gpu_pauli_expect import NAN_FILL, _refused

pytestmark = pytest.mark.gpu

RINGS = [4, 6, 7, 8, 12]
TYPES = {"d": np.float64, "z": np.complex128, "s": np.float32, "c": np.complex64}
Z0, X0, X0X2, Y0Z1 = [(0, 1, 1.0)], [(1, 0, 1.0)], [(5, 0, 0.7)], [(1, 3, 1.3)]
TWO = [(3, 0, -0.5), (0, 3, 2.0)]          # -X_0 X_1 / 2 + 2 Z_0 Z_1: a two-term sum
EXPAND_CONST = 16.0


def transfer_const(n_sites, n_terms):
    return 2.0 * (n_sites * n_terms + 8) + 24.0


def transfer_bound(n_sites, n_terms, mag, want, dtype):
    return transfer_const(n_sites, n_terms) * E.EPS_D * mag + _eps(dtype) * np.abs(want) + 1e-300


def _tids(bs, bt):
    return ("d", "z", "s", "c") if bs.real_ok() and bt.real_ok() else ("z", "c")


def _term_lists(tid):
    return [Z0, X0, X0X2, TWO] + ([Y0Z1] if tid in "zc" else [])


def kind_shape(block):
    if block.kind == "momentum":
        return "momentum", (block.n_sites, block.n_down, block.m)
    return "momentum_full", (block.n_sites, block.m)


def blocks_of(kind, n_sites, m):
    """Every non-empty block of the kind at this ring and momentum."""
    if kind == "momentum_full":
        return [Block("momentum_full", n_sites, m)]
    return [Block("momentum", n_sites, m, n_down=nd) for nd in range(n_sites + 1) if G.momentum_basis(n_sites, nd, m)[0].shape[0]]


_OPS = {}


def block_op(ctx, block, dtype):
    """One operator per block and storage type for the session (its Hamiltonian's terms play no part in a transfer)."""
    key = (id(ctx), block.id, np.dtype(dtype).char)
    if key not in _OPS:
        _OPS[key] = block.create(L, ctx, dtype, block.hamiltonian())
    return _OPS[key]


def everywhere(ctx, call, vec, n_out, what):
    """call(in, out) -> (out, norm2) with `vec` and the output in guarded device buffers at shifts 0 and 1 — the output prefilled
    with NaN — and on the host: the same bits of both results, the guards intact, the input unchanged.  Returns (out, norm2)."""
    first = None
    for shift in (0, 1):
        ib, iv = _guarded(ctx, vec, shift, NAN_FILL)
        ob, ov = _guarded(ctx, pattern(n_out, vec.dtype, NAN_FILL), shift, NAN_FILL)
        res, norm2 = call(iv, ov)
        assert res is ov
        got = _unguard(ob, n_out, shift, NAN_FILL).copy()
        assert np.array_equal(_unguard(ib, vec.shape[0], shift, NAN_FILL), vec), (what, "the call changed its input")
        ib.free()
        ob.free()
        assert not np.any(np.isnan(got)), (what, "an element of the output was not written")
        if first is None:
            first = (got, norm2)
        assert np.array_equal(first[0].view(np.uint8), got.view(np.uint8)) and norm2 == first[1], (what, "device", shift)
    host_in = vec.copy()
    got, norm2 = call(host_in, None)
    assert got.dtype == vec.dtype and got.shape == (n_out,) and np.array_equal(host_in, vec)
    assert np.array_equal(first[0].view(np.uint8), got.view(np.uint8)) and norm2 == first[1], (what, "host buffers")
    return first


def check_result(got, norm2, want, mag, n_sites, n_terms, dtype, what):
    if not _cplx(dtype):
        assert np.all(np.abs(want.imag) <= transfer_const(n_sites, n_terms) * E.EPS_D * mag), (what, "the reference of a real pair is not real")
    err = np.abs(got.astype(np.complex128) - want)
    bound = transfer_bound(n_sites, n_terms, mag, want, dtype)
    assert np.all(err <= bound), (what, int(np.argmax(err - bound)), float(np.max(err / bound)))
    sq = float(np.sum(np.abs(got.astype(np.complex128)) ** 2))
    assert abs(norm2 - sq) <= 2.0 * (got.shape[0] + 8) * E.EPS_D * sq, (what, "norm2", norm2, sq)
    return float(np.max(err / bound))


def _is_zero_bits(v):
    return not np.any(v.view(np.uint8))


CASES = [(kind, n, m) for n in RINGS for kind in ("momentum_full", "momentum") for m in range(n)]


@pytest.mark.parametrize("kind,n_sites,m_s", CASES, ids=["%s-L%d-ms%d" % c for c in CASES])
def test_every_pair_of_blocks(ctx, kind, n_sites, m_s):
    worst, pairs = 0.0, 0
    for bs in blocks_of(kind, n_sites, m_s):
        for m_t in range(n_sites):
            for bt in blocks_of(kind, n_sites, m_t):
                if bt.n_down != bs.n_down:
                    continue
                pairs += 1
                for tid in _tids(bs, bt):
                    dtype = TYPES[tid]
                    src, tgt = block_op(ctx, bs, dtype), block_op(ctx, bt, dtype)
                    c = K.start_x(src.n_local, dtype, seed=11)
                    for k, terms in enumerate(_term_lists(tid)):
                        what = (bs.id, bt.id, tid, terms)
                        want, mag = G.pauli_block_transfer_np(kind, kind_shape(bs)[1], kind_shape(bt)[1], terms, c, return_magnitude=True)
                        if k == 0:   # Z_0: every placement of the buffers
                            got, norm2 = everywhere(ctx, lambda i, o: src.transfer(terms, i, tgt, out=o, return_norm2=True), c, tgt.n_local, what)
                        else:
                            got, norm2 = src.transfer(terms, c, tgt, return_norm2=True)
                        worst = max(worst, check_result(got, norm2, want, mag, n_sites, len(terms), dtype, what))
                        if bs.sector and bin(terms[0][0]).count("1") % 2 == 1:   # X_0, Y_0 Z_1: no partner stays in the sector
                            assert _is_zero_bits(got) and norm2 == 0.0 and not np.signbit(norm2), (what, "not exactly +0.0")
    assert pairs >= n_sites
    print("worst error / bound", kind, n_sites, m_s, pairs, worst)


@pytest.mark.parametrize("kind", ["momentum_full", "momentum"])
@pytest.mark.parametrize("tid", ["z", "c"])
def test_a_single_string_is_unitary_over_the_target_blocks(ctx, kind, tid):
    """A Pauli string is unitary and the blocks of a ring (of a sector, for a string that keeps the sector: Z strings) resolve
    the identity: sum over all target blocks of ||transfer(c)||^2 = ||c||^2, within what the contract allows each coefficient
    (2 |want| e + e^2, e the bound of the row) plus the host's own sums."""
    dtype = TYPES[tid]
    n_sites = 8
    sources = [Block("momentum_full", n_sites, 3)] if kind == "momentum_full" else [Block("momentum", n_sites, 1, n_down=4),
                                                                                  Block("momentum", n_sites, 4, n_down=3)]
    strings = [Z0, X0, X0X2, Y0Z1] if kind == "momentum_full" else [Z0, [(0, 9, 1.0)]]
    for bs in sources:
        src = block_op(ctx, bs, dtype)
        c = K.start_x(src.n_local, dtype, seed=3)
        nn = float(np.sum(np.abs(c.astype(np.complex128)) ** 2))
        for terms in strings:
            unit = [(terms[0][0], terms[0][1], 1.0)]
            total, by_norm2, slack = 0.0, 0.0, 64.0 * n_sites * E.EPS_D * nn
            for m_t in range(n_sites):
                for bt in blocks_of(kind, n_sites, m_t):
                    if bt.n_down != bs.n_down:
                        continue
                    tgt = block_op(ctx, bt, dtype)
                    want, mag = G.pauli_block_transfer_np(kind, kind_shape(bs)[1], kind_shape(bt)[1], unit, c, return_magnitude=True)
                    got, norm2 = src.transfer(unit, c, tgt, return_norm2=True)
                    e = transfer_bound(n_sites, 1, mag, want, dtype)
                    total += float(np.sum(np.abs(got.astype(np.complex128)) ** 2))
                    by_norm2 += norm2
                    slack += float(np.sum(2.0 * np.abs(want) * e + e * e)) + 2.0 * (got.shape[0] + 8) * E.EPS_D * norm2
            assert abs(total - nn) <= slack and abs(by_norm2 - nn) <= slack, (bs.id, tid, unit, total, by_norm2, nn, slack)


@pytest.mark.parametrize("block", [Block("momentum_full", 12, 5), Block("momentum", 12, 4, n_down=6), Block("momentum_full", 8, 4),
                                   Block("momentum", 7, 0, n_down=3)], ids=lambda b: b.id)
def test_the_hamiltonian_from_a_block_to_itself_is_its_spmv(ctx, block):
    """transfer(H's terms, block, block) — q = 0, the plan gives back H's own merged terms — against spmv of the block operator:
    both within the bound of the reference, so their difference within twice that."""
    for tid in _tids(block, block):
        dtype = TYPES[tid]
        op = block_op(ctx, block, dtype)
        terms = block.hamiltonian()
        c = K.start_x(op.n_local, dtype, seed=11)
        want, mag = G.pauli_block_transfer_np(*kind_shape(block), kind_shape(block)[1], terms, c, return_magnitude=True)
        got, norm2 = op.transfer(terms, c, op, return_norm2=True)
        check_result(got, norm2, want, mag, block.n_sites, len(terms), dtype, (block.id, tid))
        xd, yd = ctx.to_device(c), ctx.empty(op.n_local, dtype)
        L.spmv(op, xd, yd)
        y = yd.get()
        xd.free()
        yd.free()
        bound = transfer_bound(block.n_sites, len(terms), mag, want, dtype)
        assert np.all(np.abs(y.astype(np.complex128) - got.astype(np.complex128)) <= 2.0 * bound), (block.id, tid)
        assert np.any(y != 0)


def test_the_composed_path_through_the_full_space_agrees(ctx):
    """project(P expand(c)) with P the PauliOperator of the same terms, on 12 sites in z: the fused result within its contract,
    the composed one within the sum of its three — expand ((16 eps_d + eps_T) per element, carried by |P| and |B_t|^T to M),
    the full-space apply (the component-wise class 8 (n_terms + 2) eps_T on its row sums, + eps_T for its narrowing, carried by
    |B_t|^T to M) and project ((2 (n_sites + 8) + 8) eps_d on sum |val||y| <= M, + eps_T |want|)."""
    dtype = np.complex128
    n_sites = 12
    bs, bt = Block("momentum_full", n_sites, 2), Block("momentum_full", n_sites, 7)
    src, tgt = block_op(ctx, bs, dtype), block_op(ctx, bt, dtype)
    c = K.start_x(src.n_local, dtype, seed=11)
    for terms in (Z0, Y0Z1, TWO):
        full = L.PauliOperator(ctx, n_sites, terms, dtype)
        try:
            want, mag = G.pauli_block_transfer_np("momentum_full", (n_sites, bs.m), (n_sites, bt.m), terms, c, return_magnitude=True)
            fused = src.transfer(terms, c, tgt)
            psi = ctx.empty(full.n_local, dtype)
            y = ctx.empty(full.n_local, dtype)
            src.expand(c, full, out=psi)
            L.spmv(full, psi, y)
            composed = tgt.project(y, full)
            psi.free()
            y.free()
        finally:
            full.close()
        eps = _eps(dtype)
        b_fused = transfer_bound(n_sites, len(terms), mag, want, dtype)
        b_comp = ((EXPAND_CONST + 2 * (n_sites + 8) + 8) * E.EPS_D + (8 * (len(terms) + 2) + 2) * eps) * mag + eps * np.abs(want)
        assert np.all(np.abs(fused - want) <= b_fused) and np.all(np.abs(composed - want) <= b_comp), terms
        assert np.all(np.abs(fused - composed) <= b_fused + b_comp) and np.any(fused != 0), terms


def test_no_terms_and_dropped_strings_give_exactly_zero(ctx):
    """n_terms == 0, and a string whose rotation period r has q r != 0 (mod L) — X_0 X_2 on four sites into an odd q —: the output
    is +0.0 in every byte, on the device and on the host, and norm2 is +0.0."""
    dtype = np.complex128
    src, tgt = block_op(ctx, Block("momentum_full", 4, 0), dtype), block_op(ctx, Block("momentum_full", 4, 1), dtype)
    c = K.start_x(src.n_local, dtype, seed=11)
    for terms in ([], X0X2):
        got, norm2 = everywhere(ctx, lambda i, o: src.transfer(terms, i, tgt, out=o, return_norm2=True), c, tgt.n_local, terms)
        assert _is_zero_bits(got) and norm2 == 0.0 and not np.signbit(norm2)
    assert G.transferred_strings(4, X0X2[0], 1) == [] and len(G.transferred_strings(4, X0X2[0], 2)) == 2


def test_refusals(ctx):
    n_sites = 6
    ring = G.heisenberg_terms(n_sites, 1.0, 0.8, periodic=True)
    tf = G.tfim_terms(n_sites, 1.0, 0.7, periodic=True)
    csr = L.CsrOperator(ctx, *G.laplace2d_np(4))
    full = L.PauliOperator(ctx, n_sites, Z0, np.float64)
    sect = L.PauliSectorOperator(ctx, n_sites, 3, ring, np.float64)
    mom = L.PauliMomentumOperator(ctx, n_sites, 3, 0, ring, np.float64)
    mom3 = L.PauliMomentumOperator(ctx, n_sites, 3, 3, ring, np.float64)
    mom2 = L.PauliMomentumOperator(ctx, n_sites, 2, 0, ring, np.float64)
    mf = L.PauliMomentumFullOperator(ctx, n_sites, 0, tf, np.float64)
    mf3 = L.PauliMomentumFullOperator(ctx, n_sites, 3, tf, np.float64)
    mf8 = L.PauliMomentumFullOperator(ctx, 8, 0, G.tfim_terms(8, 1.0, 0.7, periodic=True), np.float64)
    mfz = L.PauliMomentumFullOperator(ctx, n_sites, 1, tf, np.complex128)
    mfs = L.PauliMomentumFullOperator(ctx, n_sites, 0, tf, np.float32)
    symf = L.PauliSymmetricOperator(ctx, n_sites, 0, tf, np.float64, parity=1)
    ctx2 = L.Context(0)
    ctx2.init_comm(L.Context.unique_id(), 0, 1)
    shard = L.PauliMomentumFullOperator(ctx2, n_sites, 0, tf, np.float64)
    shard3 = L.PauliMomentumFullOperator(ctx2, n_sites, 3, tf, np.float64)
    lib = capi.lib()
    ops = (csr, full, sect, mom, mom3, mom2, mf, mf3, mf8, mfz, mfs, symf, shard, shard3)
    try:
        def no(source, target, terms, *needles):
            out = pattern(target.n_local, source.dtype, 0x5A)   # (the wrapper asks for the source's dtype; the library decides)
            keep = out.copy()
            _refused(lambda: L.pauli_block_transfer(source, target, terms, K.start_x(source.n_local, source.dtype), out=out), *needles)
            assert np.array_equal(out.view(np.uint8), keep.view(np.uint8)), "a refused call wrote its output"

        no(symf, mf, Z0, "momentum / reflection / spin-inversion block", "semi-momentum")
        no(mf, symf, Z0, "semi-momentum")
        _refused(lambda: symf.transfer(Z0, K.start_x(symf.n_local, np.float64), symf), "semi-momentum")
        no(full, mf, Z0, "must be momentum blocks", "a full-space sum of Pauli strings")
        no(mf, sect, Z0, "must be momentum blocks", "a sum of Pauli strings on an S_z sector")
        no(csr, mf, Z0, "must be momentum blocks", "a CSR operator")
        no(mf, mom, Z0, "different kinds")
        no(mom, mf, Z0, "different kinds")
        no(mf, mf8, Z0, "n_sites")
        no(mom, mom2, Z0, "n_down")
        no(mf, mfz, Z0, "storage type")
        no(mf, mfs, Z0, "storage type")
        no(mf, mf3, [(1, 1, 1.0)], "term 0", "odd number of Y")
        no(mf, mf3, [(0, 1, 1.0), (1 << n_sites, 0, 1.0)], "term 1", "a mask bit at or above n_sites")
        no(mf, mf3, [(0, 1, float("inf"))], "term 0", "not finite")
        no(shard, shard3, Z0, "a context with a communicator")
        no(mf, shard3, Z0, "the target operator belongs to another context")
        no(shard, mf3, Z0, "the target operator belongs to another context")
        # the C entry point: null arguments, a negative count, another context, overlapping buffers
        arr, _ = L.engine._term_array(Z0)
        c, out = K.start_x(mf.n_local, np.float64), np.zeros(mf3.n_local)
        good = [ctx.handle, mf.handle, mf3.handle, 1, arr, capi.ptr(c), capi.ptr(out), None]
        for k in (0, 1, 2, 4, 5, 6):
            args = list(good)
            args[k] = None
            assert lib.ll_pauli_block_transfer(*args) == capi.LL_ERR_INVALID and b"null argument" in lib.ll_last_error(), k
        args = list(good)
        args[3] = -1
        assert lib.ll_pauli_block_transfer(*args) == capi.LL_ERR_INVALID and b"n_terms is negative" in lib.ll_last_error()
        args = list(good)
        args[0] = ctx2.handle
        assert lib.ll_pauli_block_transfer(*args) == capi.LL_ERR_INVALID
        assert b"the source operator belongs to another context" in lib.ll_last_error()
        assert not np.any(out)
        both = np.zeros(mf.n_local + mf3.n_local)
        tail = both[mf.n_local - 1:]             # its first element is the last of the input's
        tail_out = both[mf3.n_local - 1:]       # its first element is the last of the output's
        for a, b in ((both, tail), (tail_out, both), (both, both)):
            args = list(good)
            args[5], args[6] = capi.ptr(a), capi.ptr(b)
            assert lib.ll_pauli_block_transfer(*args) == capi.LL_ERR_INVALID and b"input and output overlap" in lib.ll_last_error()
        # the wrapper's own checks, and the operators still work after the refusals; a null terms pointer with no terms is fine
        with pytest.raises(ValueError):
            mf.transfer(Z0, c[:-1], mf3)
        with pytest.raises(TypeError):
            mf.transfer(Z0, c, mf3, out=np.zeros(mf3.n_local, np.float32))
        args = list(good)
        args[3], args[4] = 0, None
        out[:] = 1.0
        assert lib.ll_pauli_block_transfer(*args) == capi.LL_OK and _is_zero_bits(out)
        want, mag = G.pauli_block_transfer_np("momentum_full", (n_sites, 0), (n_sites, 3), Z0, c, return_magnitude=True)
        got, norm2 = mf.transfer(Z0, c, mf3, return_norm2=True)
        check_result(got, norm2, want, mag, n_sites, 1, np.float64, "after the refusals")
        got = mom.transfer(Z0, K.start_x(mom.n_local, np.float64), mom3)
        assert got.shape == (mom3.n_local,) and np.any(got != 0)
    finally:
        for o in ops:
            o.close()
        ctx2.close()
